"""`morna recovery` without a GPU: the tables derived from a histogram, the grid parser and the command line's refusals.

The yardstick is `ref_recovery` below: the retention step's restatement (test_junctions_cpu.ref_retain, morna.py:1539-1569)
on the text lines, intersected with a truth set -- the three counts junction_recovery_performance.py of the reference's
tests/ derives its precision / recall / fscore from.  `ref_hist` restates the histogram of DESIGN.md 8 (N6) in numpy;
the GPU tests (test_gpu_recovery.py) compare the library's histogram with it, entry for entry.
"""
import math

import numpy as np
import pytest

from test_junctions_cpu import ref_retain, sample_lists

INT32_MIN = -2**31


# ---- the restatement ---------------------------------------------------------------------------------------------------
def ref_recovery(lines, result_sample_ids, truth_set, f, c, tables=None):
    """(retrieved, true positives, true) of one result list under the filter (f, c): what the retention step keeps, and
    how much of `truth_set` (line numbers) is in it."""
    juncs, covrs = tables if tables is not None else sample_lists(lines)
    retained, _ = ref_retain([juncs[s] for s in result_sample_ids], [covrs[s] for s in result_sample_ids], f, c)
    return len(retained), len(retained & set(truth_set)), len(set(truth_set))


def rows_of_tables(tables):
    """{sample: (lines, coverages)} as int arrays, from sample_lists' tables."""
    juncs, covrs = tables
    return {s: (np.array(juncs[s], np.int64), np.array([int(c) for c in covrs[s]], np.int64)) for s in juncs}


def ref_hist(rows, n_lines, result_sample_ids, truth_lines, coverages):
    """hist[2][65][B + 1] of one result list: rows[s] = (lines, coverages) of sample s; an id at two ranks counts twice."""
    cnt = np.zeros(n_lines, np.int64)
    mx = np.full(n_lines, INT32_MIN, np.int64)
    for s in result_sample_ids:
        line, cov = rows[s]
        cnt[line] += 1
        mx[line] = np.maximum(mx[line], cov)
    b = np.where(cnt > 0, np.searchsorted(np.asarray(coverages, np.int64), mx, side="right"), 0)
    t = np.zeros(n_lines, np.int64)
    t[np.asarray(truth_lines, np.int64)] = 1
    counted = (cnt > 0) | (t > 0)
    hist = np.zeros((2, 65, len(coverages) + 1), np.int64)
    np.add.at(hist, (t[counted], cnt[counted], b[counted]), 1)
    return hist


FREQUENCIES = ["0", ".05", ".3", "1.0", "1.5"]


def generic_case(embedded):
    lines = embedded["generic"]
    tables = sample_lists(lines)
    all_cov = sorted(int(c) for v in tables[1].values() for c in v)
    # below every coverage, two that occur (the smallest and the median), one between, one above all
    coverages = sorted(set([all_cov[0] - 1, all_cov[0], all_cov[len(all_cov) // 2], all_cov[-1], all_cov[-1] + 1]))
    assert coverages[0] < all_cov[0] and coverages[-1] > all_cov[-1] and all_cov[len(all_cov) // 2] in coverages
    return lines, tables, coverages


def result_list(samples, m):
    """m results drawn from `samples` in a fixed scrambled order; more than len(samples): ids repeat."""
    order = [samples[(7 * i + 3) % len(samples)] for i in range(len(samples))]
    return [order[i % len(order)] for i in range(m)]


# ---- recovery_rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 7, 64])
def test_rows_of_ref_hist_equal_restatement(embedded, m):
    from morna_amd.junctions import RECOVERY_COLUMNS, min_count, recovery_rows
    lines, tables, coverages = generic_case(embedded)
    rows_by_sample = rows_of_tables(tables)
    samples = list(tables[0])
    results = result_list(samples, m)
    some_retrieved = False
    for truth in (tables[0][samples[2]], [], list(range(len(lines))), [0, len(lines) - 1]):
        hist = ref_hist(rows_by_sample, len(lines), results, truth, coverages)
        assert hist[0, 0].sum() == 0 and hist.sum() == len(set(truth) | set(j for s in results for j in tables[0][s]))
        rows = recovery_rows(hist, m, FREQUENCIES, coverages)
        assert len(rows) == len(FREQUENCIES) * len(coverages)
        at = 0
        for f in FREQUENCIES:                                  # frequency-major, in the order given
            for c in coverages:
                retrieved, tp, true = ref_recovery(lines, results, truth, float(f), c, tables)
                row = rows[at]
                at += 1
                assert tuple(row) == RECOVERY_COLUMNS
                assert (row["frequency_filter"], row["coverage_filter"], row["min_count"]) == (f, c, min_count(float(f), m))
                assert (row["retrieved"], row["true_positive"], row["false_positive"], row["false_negative"]) == \
                    (retrieved, tp, retrieved - tp, true - tp), (f, c, m)
                some_retrieved |= retrieved > 0
    assert some_retrieved == (m > 0)


def test_ratios_and_zero_denominators():
    from morna_amd.junctions import recovery_rows
    hist = np.zeros((2, 65, 3), np.int64)
    hist[1, 2, 1] = 6          # true, held by 2 results, largest coverage reaches the first threshold only
    hist[0, 2, 2] = 2          # not true, held by 2, reaches both
    hist[1, 0, 0] = 4          # true, held by nobody
    rows = recovery_rows(hist, 4, ["0", "1"], [5, 50])
    by = {(r["frequency_filter"], r["coverage_filter"]): r for r in rows}
    r = by[("0", 5)]
    assert (r["retrieved"], r["true_positive"], r["false_positive"], r["false_negative"]) == (8, 6, 2, 4)
    assert r["precision"] == 6 / 8 and r["recall"] == 6 / 10 and r["fscore"] == 2 * (6 / 8) * (6 / 10) / (6 / 8 + 6 / 10)
    r = by[("1", 50)]                                          # min_count 4 > 2: only the line whose coverage reaches 50
    assert (r["min_count"], r["retrieved"], r["true_positive"], r["false_negative"]) == (4, 2, 0, 10)
    assert r["precision"] == 0.0 and r["recall"] == 0.0 and math.isnan(r["fscore"])
    r = by[("1", 5)]
    assert (r["retrieved"], r["true_positive"]) == (8, 6)
    # nothing retrieved: precision nan; no truth at all: recall nan -- never an exception
    empty = recovery_rows(np.zeros((2, 65, 3), np.int64), 0, ["0.5"], [5, 50])
    assert all(math.isnan(e[k]) for e in empty for k in ("precision", "recall", "fscore"))
    assert all((e["retrieved"], e["true_positive"], e["false_negative"]) == (0, 0, 0) for e in empty)
    no_truth = hist.copy()
    no_truth[1] = 0
    r = recovery_rows(no_truth, 4, ["0"], [5, 50])[0]
    assert r["precision"] == 0.0 and math.isnan(r["recall"]) and math.isnan(r["fscore"])
    with pytest.raises(ValueError):
        recovery_rows(hist, 4, ["0"], [5])                     # a histogram of two thresholds, a grid of one


def test_extra_true_lowers_recall_only():
    from morna_amd.junctions import recovery_rows
    hist = np.zeros((2, 65, 2), np.int64)
    hist[1, 3, 1], hist[0, 1, 0], hist[1, 0, 0] = 5, 2, 1
    plain, more = recovery_rows(hist, 3, ["0"], [1])[0], recovery_rows(hist, 3, ["0"], [1], extra_true=4)[0]
    for key in ("retrieved", "true_positive", "false_positive", "precision", "min_count"):
        assert plain[key] == more[key]
    assert more["false_negative"] == plain["false_negative"] + 4 == 5
    assert plain["recall"] == 5 / 6 and more["recall"] == 5 / 10 and more["fscore"] < plain["fscore"]


def test_summary_is_the_sum_of_the_queries(embedded):
    from morna_amd.junctions import format_recovery_rows, recovery_rows, sum_recovery_rows
    lines, tables, coverages = generic_case(embedded)
    rows_by_sample = rows_of_tables(tables)
    samples = list(tables[0])
    per_query = []
    for q, m in enumerate((0, 1, 7, 64)):
        results = result_list(samples[q:] + samples[:q], m)
        hist = ref_hist(rows_by_sample, len(lines), results, tables[0][samples[q]], coverages)
        per_query.append(recovery_rows(hist, m, FREQUENCIES, coverages, extra_true=q))
    total = sum_recovery_rows(per_query)
    assert len(total) == len(per_query[0])
    for i, row in enumerate(total):
        for key in ("retrieved", "true_positive", "false_positive", "false_negative"):
            assert row[key] == sum(t[i][key] for t in per_query)
        assert (row["frequency_filter"], row["coverage_filter"], row["min_count"]) == \
            (per_query[0][i]["frequency_filter"], per_query[0][i]["coverage_filter"], "-")
        true = row["true_positive"] + row["false_negative"]
        assert row["recall"] == row["true_positive"] / true
        assert (row["precision"] == row["true_positive"] / row["retrieved"]) if row["retrieved"] else math.isnan(row["precision"])
    assert sum_recovery_rows([]) == []
    text = format_recovery_rows(total).split("\n")
    assert text[0].split("\t") == ["frequency_filter", "coverage_filter", "min_count", "retrieved", "true_positive", "false_positive",
                                   "false_negative", "precision", "recall", "fscore"]
    assert len(text) == len(total) + 2 and text[-1] == ""
    first = text[1].split("\t")
    assert first[:3] == ["0", str(coverages[0]), "-"] and first[8] == "%.12f" % total[0]["recall"]
    assert format_recovery_rows(recovery_rows(np.zeros((2, 65, 2), np.int64), 0, [".5"], [3])).split("\n")[1] == \
        ".5\t3\t0\t0\t0\t0\t0\tnan\tnan\tnan"


# ---- the grid ------------------------------------------------------------------------------------------------------------
def test_parse_recovery_grid():
    from morna_amd.junctions import DEFAULT_RECOVERY_GRID, parse_recovery_grid
    assert DEFAULT_RECOVERY_GRID == "0,.05,.1,.2,.3,.5,.75,1:1,2,3,5,10,20,50,1000"
    assert parse_recovery_grid() == parse_recovery_grid(None) == parse_recovery_grid(DEFAULT_RECOVERY_GRID) == \
        (["0", ".05", ".1", ".2", ".3", ".5", ".75", "1"], [1, 2, 3, 5, 10, 20, 50, 1000])
    assert parse_recovery_grid("1.5,0,.3,0:50,5,5,-2,1") == (["1.5", "0", ".3", "0"], [-2, 1, 5, 50])   # kept as given; sorted
    assert parse_recovery_grid(".5:" + ",".join(str(c) for c in range(15, 0, -1))) == ([".5"], list(range(1, 16)))
    assert parse_recovery_grid(".5:" + ",".join(["7"] * 20)) == ([".5"], [7])
    with pytest.raises(ValueError, match="15"):
        parse_recovery_grid(".5:" + ",".join(str(c) for c in range(16)))
    for bad in ("", ".05,5", ".05:5:1", "a:5", ".05:1.5", ".05:", ":5", ".05,:5", ".05:5,", "nan:5", "inf:5", ".05:x"):
        with pytest.raises(ValueError):
            parse_recovery_grid(bad)


# ---- the command line: what argparse refuses, before any index or library is touched -----------------------------------------
def test_recovery_parser_flags_and_defaults():
    from morna_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["recovery", "-x", "idx", "-q", "7"])
    assert (a.subparser_name, a.grid, a.truth_coverage, a.truth, a.junction_file, a.summary_only, a.results) == \
        ("recovery", None, 1, None, None, False, 20)
    s = p.parse_args(["search", "-x", "idx", "-q", "7"])
    for name, value in vars(s).items():                        # all of search's parameters, with search's defaults
        if name != "subparser_name":
            assert getattr(a, name) == value, name
    a = p.parse_args(["recovery", "-x", "idx", "--intropolis", "s.gz", "--truth", "d.gz", "--junction-file", "j.gz", "--grid", "0:1",
                      "--truth-coverage", "3", "--summary-only", "-e", "-r", "5", "--search-k", "9"])
    assert (a.intropolis, a.truth, a.junction_file, a.grid, a.truth_coverage, a.summary_only, a.exact, a.results, a.search_k) == \
        ("s.gz", "d.gz", "j.gz", "0:1", 3, True, True, 5, 9)


NOWHERE = "/nonexistent/recovery/idx"


@pytest.mark.parametrize("argv", [
    ["-q", "3", "-c", "10"],
    ["-q", "3", "-rl"],
    ["-q", "3", "-m"],
    ["-q", "3", "-d"],
    ["-q", "3", "--unhashed"],
    [],                                                                                        # a stream query
    ["-f", "raw"],
    ["--intropolis", "s.gz"],
    ["--intropolis", "s.gz", "--truth", "d.gz"],
    ["--intropolis", "s.gz", "--junction-file", "j.gz"],
    ["-q", "3", "--truth", "d.gz"],
    ["--query-ids", "1,2", "--truth", "d.gz", "--junction-file", "j.gz"],
    ["-q", "3", "--query-ids", "1,2"],
    ["--query-ids", "1,x"],
    ["--query-ids", "1,2", "--intropolis", "s.gz", "--truth", "d.gz", "--junction-file", "j.gz"],
    ["-q", "3", "--grid", ".05,5"],
    ["-q", "3", "--grid", ".05:" + ",".join(str(c) for c in range(16))],
    ["-q", "3", "--grid", "x:5"],
    ["-q", "3", "--truth-coverage", "1.5"],
])
def test_recovery_parser_errors(argv, capsys):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["recovery", "-x", NOWHERE] + argv)           # (an index that is not there: nothing got as far as reading it)
    assert e.value.code == 2
    capsys.readouterr()


def test_recovery_refusals_after_the_parser(tmp_path, monkeypatch):
    """junctions' wording: more than 64 results, no store next to the index, one process per shard."""
    from morna_amd import cli
    base = str(tmp_path / "idx")
    with pytest.raises(ValueError, match="at most 64 results"):
        cli.main(["recovery", "-x", base, "-q", "3", "-r", "65"])
    with pytest.raises(IOError, match="--junction-store"):
        cli.main(["recovery", "-x", base, "-q", "3"])
    with open(base + ".shards.mor", "w") as fh:
        fh.write("")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(RuntimeError, match="not available with one process per shard"):
        cli.main(["recovery", "-x", base, "-q", "3"])
