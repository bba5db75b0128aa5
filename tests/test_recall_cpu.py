"""Tree-prefix search and `morna recall`, host side: the list parser, the table arithmetic from a hits array (the -1 rows
included), the command line's argparse errors, the refusals, and the ctypes signatures of the four calls against the
header.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_list_parser():
    from morna_amd.search import parse_int_list
    assert parse_int_list("10,20,50", "--trees") == [10, 20, 50]
    assert parse_int_list(" 7 ", "--trees") == [7]
    assert parse_int_list("10,20,all", "--trees", all_value=200) == [10, 20, 200]
    assert parse_int_list("all", "--trees", all_value=8) == [8]
    assert parse_int_list(",".join(map(str, range(1, 65))), "--search-ks") == list(range(1, 65))
    for text, word in (("20,10", "ascend"), ("10,10", "ascend"), ("0,5", "positive"), ("-1,5", "positive"), ("", "integer"),
                       ("5,x", "integer"), ("1.5", "integer"), ("all", "integer"), ("10,200,all", "ascend"),
                       (",".join(map(str, range(1, 66))), "64")):
        with pytest.raises(ValueError, match=word):
            parse_int_list(text, "--trees", all_value=200 if text == "10,200,all" else None)


def test_table_arithmetic():
    from morna_amd.search import format_recall_rows, recall_rows, recall_summary
    trees, sks = [1, 4], [10, 100, 1000]
    exact = np.array([20, -1, 20, 5, 0], np.int32)                  # query 1: the exact search failed; query 4: no rows
    hits = np.zeros((2, 3, 5), np.int32)
    ncand = np.arange(30, dtype=np.int32).reshape(2, 3, 5) * 10
    ndots = np.arange(30, dtype=np.int32).reshape(2, 3, 5) + 1
    hits[:, :, 0] = [[5, 10, 20], [10, 20, 20]]
    hits[:, :, 1] = -1
    hits[:, :, 2] = [[0, 1, 2], [3, 4, 20]]
    hits[:, :, 3] = [[5, 5, 5], [1, 5, 5]]
    rows = recall_rows(trees, sks, hits, exact, ncand, ndots, 0)
    assert rows[0] == (1, 10, 5, 20, 0.25, 0, 1) and rows[5] == (4, 1000, 20, 20, 1.0, 250, 26) and len(rows) == 6
    assert recall_rows(trees, sks, hits, exact, ncand, ndots, 1)[2] == (1, 1000, -1, -1, None, 110, 12)
    assert recall_rows(trees, sks, hits, exact, ncand, ndots, 4)[0] == (1, 10, 0, 0, 0.0, 40, 5)
    summary, failed = recall_summary(trees, sks, hits, exact, ncand, ndots)
    assert failed == 1 and len(summary) == 6
    # cell (4 trees, search_k 1000): recalls 1, 1, 1 and 0 (the query without exact results) over the four counted queries
    t, s, mean, low, ones, cand, dots = summary[5]
    assert (t, s, mean, low, ones) == (4, 1000, 0.75, 0.0, 3)
    assert cand == (250 + 270 + 280 + 290) / 4.0 and dots == (26 + 28 + 29 + 30) / 4.0
    t, s, mean, low, ones, cand, dots = summary[0]
    assert (t, s, ones) == (1, 10, 1) and mean == (0.25 + 0.0 + 1.0 + 0.0) / 4 and low == 0.0
    text = format_recall_rows(rows[:1] + [recall_rows(trees, sks, hits, exact, ncand, ndots, 1)[2]])
    assert text == "1\t10\t5\t20\t0.250000\t0\t1\n1\t1000\t-1\t-1\tnan\t110\t12\n"
    assert format_recall_rows(summary[5:]) == "4\t1000\t0.750000\t0.000000\t3\t272.500000\t28.250000\n"
    # every exact search failed: no query is counted
    summary, failed = recall_summary([1], [10], np.full((1, 1, 2), -1), np.array([-1, -1]), np.zeros((1, 1, 2)), np.zeros((1, 1, 2)))
    assert failed == 2 and summary == [(1, 10, None, None, 0, None, None)]


def _refused(argv, capsys, text):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err, err


def test_argparse_errors_before_any_index_is_read(tmp_path, capsys):
    base = ["-x", "/nonexistent/index"]          # never opened: every case fails in the parser
    ids = tmp_path / "ids.txt"
    ids.write_text("1\n2\n")
    groups = tmp_path / "groups.tsv"
    groups.write_text("a\t1,2\n")
    t = ["--use-trees", "3"]
    _refused(["search"] + base + ["-q", "1", "-e"] + t, capsys, "--use-trees cannot be used with -e/--exact")
    _refused(["search"] + base + ["-q", "1", "--unhashed"] + t, capsys, "--use-trees cannot be used with --unhashed")
    _refused(["search"] + base + ["-q", "1", "--within", str(ids)] + t, capsys, "--use-trees cannot be used with --within")
    _refused(["search"] + base + ["-q", "1", "--without", str(ids)] + t, capsys, "--use-trees cannot be used with --without")
    _refused(["search"] + base + ["-q", "1", "--leave-out-groups", str(groups)] + t, capsys,
             "--use-trees cannot be used with --leave-out-groups")
    _refused(["search"] + base + ["-q", "1", "--use-trees", "0"], capsys, "positive tree count")
    _refused(["junctions"] + base + t + ["--junction-file", "j.gz", "-sf", "out"], capsys, "unrecognized arguments")
    _refused(["recovery"] + base + ["-q", "1"] + t, capsys, "unrecognized arguments")
    grid = ["--trees", "1,2", "--search-ks", "10,20"]
    _refused(["recall"] + base + grid, capsys, "exactly one query source")
    _refused(["recall"] + base + grid + ["-q", "1", "--sample", "5"], capsys, "exactly one query source")
    _refused(["recall"] + base + grid + ["--query-ids", "1,2", "--intropolis", "q.gz"], capsys, "exactly one query source")
    _refused(["recall"] + base + ["-q", "1", "--trees", "1,2"], capsys, "--search-ks")
    _refused(["recall"] + base + ["-q", "1", "--search-ks", "1,2"], capsys, "--trees")
    _refused(["recall"] + base + ["-q", "1", "--trees", "2,1", "--search-ks", "10"], capsys, "ascend")
    _refused(["recall"] + base + ["-q", "1", "--trees", "1", "--search-ks", "10,-1"], capsys, "positive")
    _refused(["recall"] + base + ["-q", "1", "--trees", "1", "--search-ks", "all"], capsys, "integer")
    _refused(["recall"] + base + ["-q", "1", "--trees", ",".join(map(str, range(1, 66))), "--search-ks", "10"], capsys, "64")
    _refused(["recall"] + base + grid + ["--query-ids", "1,x"], capsys, "--query-ids takes comma-separated integer sample ids")
    _refused(["recall"] + base + grid + ["-q", "1", "--sample-seed", "3"], capsys, "--sample-seed cannot be used without --sample")
    _refused(["recall"] + base + grid + ["--sample", "0"], capsys, "positive number of samples")
    _refused(["recall"] + base + grid + ["-q", "1", "-r", "257"], capsys, "1 to 256")
    _refused(["recall"] + base + grid + ["-q", "1", "-r", "0"], capsys, "1 to 256")
    for flag in (["-e"], ["--within", str(ids)], ["--without", str(ids)], ["--leave-out-groups", str(groups)], ["--unhashed"]):
        _refused(["recall"] + base + grid + ["-q", "1"] + flag, capsys, "unrecognized arguments")


def test_flags_parse_and_leave_today_s_command_lines_alone():
    from morna_amd import cli
    p = cli.build_parser()
    args = p.parse_args(["search", "-x", "i", "-q", "7"])
    assert args.use_trees is None and cli._use_trees(args) is None
    args = p.parse_args(["search", "-x", "i", "-q", "7", "--use-trees", "12"])
    assert cli._use_trees(args) == 12
    args = p.parse_args(["recovery", "-x", "i", "-q", "7"])
    assert cli._use_trees(args) is None
    args = p.parse_args(["recall", "-x", "i", "--sample", "9", "--trees", "1,all", "--search-ks", "5,50"])
    cli._check_recall_flags(p, args)
    assert (args.sample, args.sample_seed, args.results, args.search_k_list, args.summary_only) == (9, 0, 20, [5, 50], False)


def test_refusals_on_row_shards_and_under_torchrun(tmp_path, monkeypatch):
    """`recall` refuses an index of row shards and a torchrun launch before anything is loaded; the searcher's n_trees= and
    search_recall refuse a handle that is not one AnnoyIndex, and n_trees= with a restriction."""
    from morna_amd import cli
    from morna_amd.search import MornaSearch, TREES_SHARDS_REFUSAL
    base = str(tmp_path / "idx")
    open(base + ".shards.mor", "w").close()
    argv = ["recall", "-x", base, "-q", "1", "--trees", "1", "--search-ks", "10"]
    with pytest.raises(ValueError, match="row shards"):
        cli.main(argv)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one process per shard"):
        cli.main(argv)
    monkeypatch.delenv("WORLD_SIZE")
    s = MornaSearch.__new__(MornaSearch)
    s.annoy_index = object()                    # stands for shards.LocalShards: not one AnnoyIndex
    s._check_trees(None)
    with pytest.raises(ValueError) as e:
        s._check_trees(3)
    assert str(e.value) == TREES_SHARDS_REFUSAL
    with pytest.raises(ValueError, match="restriction"):
        s._check_trees(3, restriction=object())
    with pytest.raises(ValueError, match="row shards"):
        s.search_recall([0, 1], 20, [1], [10])
    with pytest.raises(ValueError, match="row shards"):
        s.search_member_n_batch([], 20, 100, n_trees=2)


# ---- the ctypes table against the header's prototypes ----------------------------------------------------------------------

_NEW = ("morna_get_nns_prefix", "morna_search_sweep", "morna_recall_sweep", "morna_search_sweep_stats")


def _ctype_of(decl):
    decl = re.sub(r"\bconst\b", "", decl).strip()
    stars = decl.count("*")
    base = decl.replace("*", " ").split()[0]
    if stars == 2:
        return C.POINTER(C.c_void_p)
    if stars == 1:
        return C.c_void_p
    return {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "int": C.c_int}[base]


def test_ctypes_signatures_match_the_header():
    from morna_amd import _lib
    with open(os.path.join(ROOT, "include", "morna_hip.h")) as fh:
        src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in _NEW:
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is _ctype_of(m.group(1)), name
        want = [_ctype_of(a) for a in m.group(2).split(",")]
        assert len(args) == len(want), name
        for i, (got, w) in enumerate(zip(args, want)):
            assert got is w, (name, i, got, w)
    # the argument order the issue's prototypes give
    m = re.search(r"morna_get_nns_prefix\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "q", "items", "nq", "k", "search_k", "n_trees_used", "ids", "dist", "count"]
    m = re.search(r"morna_search_sweep\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "q", "items", "nq", "k", "trees", "n_t", "search_ks", "n_s", "ids_out", "dist_out", "count_out", "ncand_out",
                     "ndots_out"]
    assert re.search(r"#define\s+MORNA_RECALL_MAX_K\s+256\b", src) and re.search(r"#define\s+MORNA_SWEEP_MAX_LIST\s+64\b", src)
