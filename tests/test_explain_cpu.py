"""`morna explain`, host side: the plain-Python restatement of the contract (explain_ref.py) against
cases computed by hand and against RefUnhashed's distances, the command line's refusals and the formatting helpers.  No GPU."""
import gzip
from math import sqrt

import numpy as np
import pytest

from explain_ref import bits, explain_pair
from test_unhashed_cpu import RefUnhashed


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restatement_by_hand():
    w = [2.0, 0.5, 0.0, 1.0, 4.0]
    # query: components 2, 1, 0 (weight 0), 0 (coverage 0); result: 6, 0 (weight 0), 2, 4
    got = explain_pair([0, 1, 2, 4], [1, 2, 5, 0], [0, 2, 3, 4], [3, 7, 2, 1], w, top=10)
    assert (got["qq"], got["n_q"]) == (5.0, 2)
    assert (got["pp"], got["n_r"]) == (56.0, 3)
    assert (got["pq"], got["shared"]) == (12.0, 1)
    assert (got["pp_shared"], got["qq_shared"]) == (36.0, 4.0)
    assert got["distance"] == sqrt(2.0 - 2.0 * 12.0 / sqrt(56.0 * 5.0))
    assert (got["lines"], got["terms"], got["cov_r"]) == ([0], [12.0], [3])
    # the same pair the other way round: the sums over the other row's entries
    back = explain_pair([0, 2, 3, 4], [3, 7, 2, 1], [0, 1, 2, 4], [1, 2, 5, 0], w, top=10)
    assert (back["pp"], back["qq"], back["pq"], back["pp_shared"], back["qq_shared"]) == (5.0, 56.0, 12.0, 4.0, 36.0)
    assert (back["shared"], back["n_q"], back["n_r"], back["cov_r"]) == (1, 3, 2, [1])


def test_restatement_ties_top_and_empty_sides():
    w = [1.0] * 6
    got = explain_pair(range(6), [1, 1, 2, 2, 1, 1], range(6), [2, 2, 1, 1, 2, 1], w, top=3)
    assert (got["lines"], got["terms"], got["cov_r"]) == ([0, 1, 2], [2.0, 2.0, 2.0], [2, 2, 1])       # equal terms: by line
    assert explain_pair(range(6), [1, 1, 2, 2, 1, 1], range(6), [2, 2, 1, 1, 2, 1], w, top=64)["lines"] == [0, 1, 2, 3, 4, 5]
    got = explain_pair(range(6), [1, 1, 2, 2, 1, 9], range(6), [2, 2, 1, 1, 2, 1], w, top=2)
    assert (got["lines"], got["terms"]) == ([5, 0], [9.0, 2.0])
    for q, r in (([], []), ([1], [2]), ([1], []), ([], [1])):
        got = explain_pair(q, [3] * len(q), r, [3] * len(r), w, top=5)
        assert got["distance"] == sqrt(2.0) and got["shared"] == 0 and got["lines"] == [] and got["pq"] == 0.0
    same = explain_pair([1, 4], [3, 5], [1, 4], [3, 5], w, top=5)
    assert same["distance"] == 0.0 and same["pp"] == same["qq"] == same["pq"] == same["pp_shared"] == same["qq_shared"] == 34.0


def test_distance_and_norms_are_ref_unhashed():
    rng = np.random.default_rng(29)
    n_lines = 700
    w = np.where(rng.random(n_lines) < 0.2, 0.0, rng.uniform(0.05, 6.0, n_lines))
    rows = []
    for n in (0, 1, 5, 64, 65, 200, 450, 700):
        l = np.sort(rng.choice(n_lines, size=n, replace=False))
        rows.append((l, np.ceil(rng.lognormal(1.0, 1.5, size=n)).astype(np.int64)))
    ref = RefUnhashed(rows, w)
    for q_lines, q_cov in rows:
        d = ref.distances(q_lines, q_cov)
        for i, (r_lines, r_cov) in enumerate(rows):
            got = explain_pair(q_lines, q_cov, r_lines, r_cov, w, top=4)
            assert bits(got["distance"]) == bits(d[i]) and bits(got["pp"]) == bits(ref.pp[i])
            assert got["terms"] == sorted(got["terms"], reverse=True) and len(got["lines"]) == min(4, got["shared"])
            assert 0.0 <= got["pp_shared"] <= got["pp"] and 0.0 <= got["qq_shared"] <= got["qq"]


# ---- the command line's refusals -----------------------------------------------------------------------------------------
def _refused(argv, capsys, text):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err, err


def test_argparse_errors_before_any_index_is_read(tmp_path, capsys):
    base = ["explain", "-x", "/nonexistent/index", "--junction-file", "j.gz"]      # never opened: every case fails in the parser
    ids = tmp_path / "ids.txt"
    ids.write_text("1\n2\n")
    _refused(["explain", "-x", "/nonexistent/index", "-q", "1"], capsys, "--junction-file")
    _refused(base + ["-q", "1", "--query-ids", "2,3"], capsys, "explain takes one query source")
    _refused(base + ["--intropolis", "q.gz", "--sample", "3"], capsys, "one query source")
    _refused(base + ["--query-ids", "1,x"], capsys, "--query-ids takes comma-separated integer sample ids")
    _refused(base + ["-q", "1", "--sample-seed", "3"], capsys, "--sample-seed cannot be used without --sample")
    _refused(base + ["--sample", "0"], capsys, "positive number of samples")
    _refused(base + ["-f", "bam"], capsys, "sam, bed, raw")
    for top in ("0", "65"):
        _refused(base + ["-q", "1", "--top", top], capsys, "--top takes 1 to 64")
    for r in ("0", "1025"):
        _refused(base + ["-q", "1", "-r", r], capsys, "-r takes 1 to 1024")
    _refused(base + ["-q", "1", "--against", "2,3", "-r", "5"], capsys, "--against cannot be used with -r/--results")
    _refused(base + ["-q", "1", "--against", "2,3", "-e"], capsys, "--against cannot be used with -e/--exact")
    _refused(base + ["-q", "1", "--against", "2,3", "--unhashed"], capsys, "--against cannot be used with --unhashed")
    _refused(base + ["-q", "1", "--against", "2,3", "--search-k", "7"], capsys, "--against cannot be used with --search-k")
    _refused(base + ["-q", "1", "--against", "2,3", "--within", str(ids)], capsys, "--against cannot be used with --within")
    _refused(base + ["-q", "1", "--against", "2,b"], capsys, "--against takes comma-separated integer sample ids")
    _refused(base + ["-q", "1", "--unhashed", "-e"], capsys, "--unhashed cannot be used with -e/--exact")
    _refused(base + ["-q", "1", "--unhashed", "--search-k", "7"], capsys, "--unhashed cannot be used with --search-k")
    _refused(base + ["-q", "1", "--within", str(ids), "--without", str(ids)], capsys, "--within and --without both name sample id 1")
    _refused(base + ["-q", "1", "--within", str(tmp_path / "missing.txt")], capsys, "missing.txt")
    for flag in (["--leave-out-groups", str(ids)], ["--downsample", "0.5"], ["--supersamples", str(ids)], ["-c", "5"]):
        _refused(base + ["-q", "1"] + flag, capsys, "unrecognized arguments")


def test_refused_without_store_or_weights_and_on_row_shards(tmp_path, capsys):
    idx = str(tmp_path / "idx")
    argv = ["explain", "-x", idx, "--junction-file", "j.gz", "-q", "1"]
    _refused(argv, capsys, "idx.junc.mor not found: this index has no junction store")
    (tmp_path / "idx.junc.mor").write_bytes(b"")
    _refused(argv, capsys, "idx.jw.mor not found: --unhashed needs the line weights")
    (tmp_path / "idx.jw.mor").write_bytes(b"")
    (tmp_path / "idx.shards.mor").write_bytes(b"")
    _refused(argv, capsys, "explain is not available on an index of row shards")


def test_flags_parse():
    from morna_amd import cli
    p = cli.build_parser()
    args = p.parse_args(["explain", "-x", "i", "--junction-file", "j.gz", "-q", "4"])
    assert (args.results, args.top, args.search_k, args.exact, args.unhashed, args.against, args.summary_only, args.metadata) == \
        (20, 10, 100, False, False, None, False, False)
    args = p.parse_args(["explain", "-x", "i", "--junction-file", "j.gz", "--query-ids", "4,5", "--against", "7,8", "--top", "3",
                         "--summary-only", "-m"])
    assert (args.query_ids, args.against, args.top, args.summary_only, args.metadata) == ("4,5", "7,8", 3, True, True)


# ---- the formatting helpers ------------------------------------------------------------------------------------------------
def _explained(d):
    from morna_amd.junctions import Explained
    return Explained([d[n] for n in Explained.SUMS], [d[n] for n in Explained.COUNTS], np.array(d["lines"], np.int32),
                     np.array(d["terms"], np.float64), np.array(d["cov_r"], np.int32))


def test_explain_rows_and_their_text():
    from morna_amd.junctions import explain_rows, format_explain_rows
    w = [2.0, 0.5, 0.0, 1.0, 4.0]
    q, r = ([0, 1, 3, 4], [1, 2, 5, 3]), ([0, 2, 3, 4], [3, 7, 2, 1])
    # components: query 2, 1, 5, 12; result 6, 0, 2, 4; terms 12 (line 0), 10 (line 3), 48 (line 4); pq 70
    pair = _explained(explain_pair(q[0], q[1], r[0], r[1], w, top=2))
    assert (pair.pq, pair.pp, pair.qq, pair.pp_shared, pair.qq_shared, pair.shared) == (70.0, 56.0, 174.0, 56.0, 173.0, 3)
    assert pair.result_outside == 0.0 and pair.query_outside == 1.0 - 173.0 / 174.0
    names = {4: "chr2 40 50", 0: "chr1 10 20"}
    summary, rows = explain_rows(pair, q[0], q[1], w, names)
    assert summary == (pair.distance, 3, 1.0 - 173.0 / 174.0, 0.0, 60.0 / 70.0)
    assert rows == [("chr2 40 50", 3, 1, 4.0, 48.0 / 70.0), ("chr1 10 20", 1, 3, 2.0, 12.0 / 70.0)]
    assert explain_rows(pair, q[0], q[1], w)[1][0][0] == 4                       # without names: the line number
    text = format_explain_rows(1, 7, 1049, 0.25, summary, rows)
    assert text == ("1.\t7\t1049\t0.25\t%s\t3\t0.005747\t0.000000\t0.857143\n"
                    "\tchr2 40 50\t3\t1\t4.0\t0.685714\n\tchr1 10 20\t1\t3\t2.0\t0.171429\n" % str(pair.distance))
    assert format_explain_rows(2, 7, 1049, 0.25, summary, (), meta=("liver\n",)) == \
        "2.\t7\t1049\t0.25\t%s\t3\t0.005747\t0.000000\t0.857143\t('liver\\n',)\n" % str(pair.distance)
    with pytest.raises(ValueError):
        explain_rows(pair, [1, 2], [1, 1], w)                                  # another query's row
    # nothing shared: the shares of pq are nan, an empty side's share is nan
    none = _explained(explain_pair([1], [2], [], [], w, top=2))
    summary, rows = explain_rows(none, [1], [2], w)
    assert rows == [] and summary[1] == 0 and summary[2] == 1.0 and summary[3] != summary[3] and summary[4] != summary[4]
    assert format_explain_rows(1, 0, 5, float("nan"), summary) == "1.\t0\t5\tnan\t%s\t0\t1.000000\tnan\tnan\n" % str(sqrt(2.0))


def test_line_names_reads_only_the_lines_asked_for(tmp_path):
    from morna_amd.junctions import line_names
    lines = ["chr%d\t%d\t%d\t+\tGT\tAG\t1,2\t3,4\n" % (1 + j % 3, 100 * j, 100 * j + 50) for j in range(40)]
    lines.append("broken\n")
    plain, packed = tmp_path / "j.tsv", tmp_path / "j.tsv.gz"
    plain.write_text("".join(lines))
    with gzip.open(str(packed), "wt") as fh:
        fh.write("".join(lines))
    for path in (str(plain), str(packed)):
        assert line_names(path, [39, 0, 7, 7]) == {0: "chr1 0 50", 7: "chr2 700 750", 39: "chr1 3900 3950"}
        assert line_names(path, []) == {}
        with pytest.raises(ValueError) as e:
            line_names(path, [3, 41])
        assert "ends before line 41" in str(e.value)
        with pytest.raises(ValueError) as e:
            line_names(path, [40])
        assert "line 40" in str(e.value) and "fields" in str(e.value)
        assert line_names(path, [5]) == {5: "chr3 500 550"}                     # the broken line is behind it: never looked at
