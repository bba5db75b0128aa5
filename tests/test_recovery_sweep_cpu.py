"""`morna recovery --results-sweep` without a GPU: the parser of the sweep, what argparse refuses, and that
the table of a prefix is the existing table arithmetic fed the prefix's histogram AND the prefix's length (min_count is
ceil(f * length of the list that was cut, not of the list that was searched)).  The yardsticks are test_recovery_cpu's
ref_recovery and ref_hist."""
import pytest

from test_recovery_cpu import FREQUENCIES, NOWHERE, generic_case, ref_hist, ref_recovery, result_list, rows_of_tables


def test_parse_results_sweep():
    from morna_amd.junctions import parse_results_sweep
    assert parse_results_sweep("20,5,5,10") == [5, 10, 20]
    assert parse_results_sweep("64") == [64] and parse_results_sweep("1") == [1]
    assert parse_results_sweep(",".join(str(p) for p in range(8, 0, -1))) == list(range(1, 9))      # eight are a sweep
    assert parse_results_sweep(",".join(["7"] * 20)) == [7]
    for bad in ("0", "65", "", "5,", "a", "1.5", "-3", "5,,6", ",".join(str(p) for p in range(1, 10))):
        with pytest.raises(ValueError):
            parse_results_sweep(bad)


def test_parser_flag_and_defaults():
    from morna_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["recovery", "-x", "idx", "-q", "7"])
    assert a.results_sweep is None
    assert (a.subparser_name, a.grid, a.truth_coverage, a.truth, a.junction_file, a.summary_only, a.results) == \
        ("recovery", None, 1, None, None, False, 20)
    s = p.parse_args(["search", "-x", "idx", "-q", "7"])
    for name, value in vars(s).items():                        # all of search's parameters, with search's defaults
        if name != "subparser_name":
            assert getattr(a, name) == value, name
    assert not hasattr(s, "results_sweep")
    a = p.parse_args(["recovery", "-x", "idx", "-q", "7", "-r", "64", "--results-sweep", "64,5"])
    assert (a.results, a.results_sweep) == (64, "64,5")


@pytest.mark.parametrize("argv, named", [
    (["recovery", "-q", "3", "-r", "10", "--results-sweep", "5,20"], ["20", "10"]),       # past -r: both numbers named
    (["recovery", "-q", "3", "--results-sweep", "21"], ["21", "20"]),                      # past the default -r
    (["recovery", "-q", "3", "-r", "64", "--results-sweep", "0"], ["--results-sweep"]),
    (["recovery", "-q", "3", "-r", "64", "--results-sweep", "65"], ["--results-sweep"]),
    (["recovery", "-q", "3", "-r", "64", "--results-sweep", "5,"], ["--results-sweep"]),
    (["recovery", "-q", "3", "-r", "64", "--results-sweep", "a"], ["--results-sweep"]),
    (["recovery", "-q", "3", "-r", "64", "--results-sweep", "1.5"], ["--results-sweep"]),
    (["recovery", "-q", "3", "-r", "64", "--results-sweep", ""], ["--results-sweep"]),
    (["recovery", "-q", "3", "-r", "64", "--results-sweep", "1,2,3,4,5,6,7,8,9"], ["--results-sweep"]),
    (["search", "-q", "3", "--results-sweep", "5"], ["--results-sweep"]),
    (["junctions", "-q", "3", "--junction-file", "j.gz", "-sf", "out", "--results-sweep", "5"], ["--results-sweep"]),
])
def test_parser_errors(argv, named, capsys):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv[:1] + ["-x", NOWHERE] + argv[1:])        # (an index that is not there: nothing got as far as reading it)
    assert e.value.code == 2
    err = capsys.readouterr().err
    for word in named:
        assert word in err, (word, err)


def test_a_prefix_table_uses_the_prefix_length(embedded):
    from morna_amd.junctions import min_count, recovery_rows
    lines, tables, coverages = generic_case(embedded)
    rows_by_sample = rows_of_tables(tables)
    samples = list(tables[0])
    results = result_list(samples, 7)
    truth = tables[0][samples[2]]
    differs = False                                            # some cell where the searched length would give another answer
    for p in (1, 4, 7):
        hist = ref_hist(rows_by_sample, len(lines), results[:p], truth, coverages)
        rows = recovery_rows(hist, p, FREQUENCIES, coverages)
        long_rows = recovery_rows(hist, 7, FREQUENCIES, coverages)
        at = 0
        for f in FREQUENCIES:
            for c in coverages:
                retrieved, tp, true = ref_recovery(lines, results[:p], truth, float(f), c, tables)
                row = rows[at]
                assert row["min_count"] == min_count(float(f), p)
                assert (row["retrieved"], row["true_positive"], row["false_positive"], row["false_negative"]) == \
                    (retrieved, tp, retrieved - tp, true - tp), (p, f, c)
                differs |= long_rows[at]["retrieved"] != retrieved
                at += 1
    assert differs
