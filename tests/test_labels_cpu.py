"""`morna labels`, host side: the table arithmetic on hand-made sums and counts, the formatter, the
command line's argparse errors and refusals, a --labels file that names an id twice or an id outside the index, and the
ctypes signatures of the two calls against the header.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ONE = 2 ** 32


def fixed(x):
    return int(round(x * ONE))


def test_one_query_ties_self_skip_single_label_and_zero_distances():
    from morna_amd.search import label_means, label_query, label_rows
    names = ["liver", "brain", "heart"]
    # means 0.5, 0.5, 0.25: brain and liver tie, heart is nearest
    sums, counts = [fixed(0.5) * 4, fixed(0.5) * 2, fixed(0.25) * 8], [4, 2, 8]
    assert label_means(sums, counts) == [0.5, 0.5, 0.25]
    info = label_query(sums, counts, own=1)
    assert (info["predicted"], info["a"], info["other"], info["b"], info["agree"]) == (2, 0.5, 2, 0.25, False)
    assert info["silhouette"] == (0.25 - 0.5) / 0.5
    # a tie between labels goes to file order: predicted, the nearest other, and the ranking
    tie = label_query([fixed(0.5) * 3, fixed(0.5), fixed(0.75)], [3, 1, 1], own=2)
    assert (tie["predicted"], tie["other"], tie["b"], tie["a"], tie["agree"]) == (0, 0, 0.5, 0.75, False)
    assert label_query([fixed(0.5), fixed(0.5), 0], [1, 1, 0], own=1)["predicted"] == 0
    assert label_query([fixed(0.5), fixed(0.5), 0], [1, 1, 0], own=1)["agree"] is False
    assert label_query([fixed(0.5), fixed(0.5), 0], [1, 1, 0], own=0)["agree"] is True
    rows = label_rows(names, [fixed(0.5) * 3, fixed(0.5), fixed(0.75)], [3, 1, 1], own=2, top=2)
    assert rows == [("1.", "liver", 3, 0.5), ("2.", "brain", 1, 0.5), ("silhouette", "heart", 1, 0.75, "liver", 0.5, (0.5 - 0.75) / 0.75, 0)]
    # own count 0 after the self-skip (the query was its label's only sample): no silhouette, the label is not ranked
    alone = label_query([fixed(1.0) * 5, 0, fixed(1.5)], [5, 0, 1], own=1)
    assert alone["silhouette"] is None and alone["agree"] is None and alone["predicted"] == 0 and alone["means"][1] is None
    assert label_rows(names, [fixed(1.0) * 5, 0, fixed(1.5)], [5, 0, 1], own=1) == [("1.", "liver", 5, 1.0), ("2.", "heart", 1, 1.5)]
    # a single label: there is no "other"
    single = label_query([fixed(0.5) * 2], [2], own=0)
    assert single["silhouette"] is None and single["predicted"] == 0 and single["other"] is None
    assert label_query([fixed(0.5) * 2, 0, 0], [2, 0, 0], own=0)["silhouette"] is None
    # max(a, b) = 0: the silhouette is 0.0, and the tie goes to the lower label
    zero = label_query([0, 0], [3, 2], own=1)
    assert (zero["a"], zero["b"], zero["silhouette"], zero["predicted"], zero["agree"]) == (0.0, 0.0, 0.0, 0, False)
    # an unlabelled by-item query (own -1) and a query from outside the index (own None): ranked, no silhouette
    for own in (-1, None):
        info = label_query(sums, counts, own=own)
        assert info["own"] is None and info["silhouette"] is None and info["predicted"] == 2
    # nothing counted at all
    empty = label_query([0, 0], [0, 0], own=0)
    assert empty["predicted"] is None and empty["silhouette"] is None and label_rows(["a", "b"], [0, 0], [0, 0], own=0) == []
    # sums near 2^62 keep their integer meaning: 2^29 rows at distance 2 - 2^-32
    big = label_means([(2 ** 33 - 1) * 2 ** 29], [2 ** 29])
    assert big == [float((2 ** 33 - 1) * 2 ** 29) / ONE / 2 ** 29] and abs(big[0] - 2.0) < 1e-9


def test_summary_and_map():
    from morna_amd.search import label_map, label_summary
    names = ["liver", "brain", "heart"]
    #            liver        brain        heart
    sums = np.array([[fixed(0.25) * 2, fixed(0.75) * 2, 0],                 # q0 liver: a .25 b .75 s 2/3 agree
                     [fixed(0.5) * 3, fixed(1.0) * 2, fixed(0.25)],          # q1 liver: a .5 b .25 (heart) s -.5 disagree
                     [fixed(1.0) * 3, fixed(0.5), 0],                        # q2 brain: a .5 b 1 s .5 agree
                     [fixed(1.0) * 3, 0, 0],                                 # q3 brain, alone in its label: no silhouette
                     [fixed(1.25) * 3, fixed(1.5) * 2, 0]], np.uint64)       # q4 unlabelled
    counts = np.array([[2, 2, 0], [3, 2, 1], [3, 1, 0], [3, 0, 0], [3, 2, 0]], np.int32)
    own = np.array([0, 0, 1, 1, -1], np.int32)
    rows, without = label_summary(names, sums, counts, own)
    assert without == 2
    assert rows[0] == ("liver", 2, (0.25 + 0.5) / 2, (0.75 + 0.25) / 2, ((0.75 - 0.25) / 0.75 + (0.25 - 0.5) / 0.5) / 2, 1, 0.5)
    assert rows[1] == ("brain", 1, 0.5, 1.0, 0.5, 1, 1.0)
    assert rows[2][0] == "all" and rows[2][1] == 3 and rows[2][5:] == (2, 2.0 / 3) and len(rows) == 3   # heart has no query
    # external queries: the number predicted to every label, and the queries that count nothing
    rows, without = label_summary(names, sums, counts)
    assert rows == [("liver", 3), ("brain", 1), ("heart", 1)] and without == 0      # q0, q3, q4 | q2 | q1
    rows, without = label_summary(names, np.zeros((2, 3), np.uint64), np.zeros((2, 3), np.int32))
    assert rows == [("liver", 0), ("brain", 0), ("heart", 0)] and without == 2
    # no query has a silhouette: no rows at all
    assert label_summary(names, sums[3:4], counts[3:4], own[3:4]) == ([], 1)
    # the label map: cells with no query are None
    M = label_map(3, sums, counts, own)
    assert M[0] == [(0.25 + 0.5) / 2, (0.75 + 1.0) / 2, 0.25]
    assert M[1] == [1.0, 0.5, None]                       # q3 counts no brain sample, no brain query counts a heart sample
    assert M[2] == [None, None, None]                     # no query carries heart; the unlabelled query is in no row


def test_format_label_rows():
    from morna_amd.search import format_label_rows
    rows = [("1.", "liver", 3, 0.5), ("silhouette", "heart", 1, 0.75, "liver", 0.5, -1.0 / 3, 0), ("brain", None, 1.0, None)]
    assert format_label_rows(rows) == ("1.\tliver\t3\t0.500000\n"
                                       "silhouette\theart\t1\t0.750000\tliver\t0.500000\t-0.333333\t0\n"
                                       "brain\tnan\t1.000000\tnan\n")
    assert format_label_rows([]) == ""


def _refused(argv, capsys, text):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err, err


def test_argparse_errors_before_any_index_is_read(tmp_path, capsys):
    base = ["labels", "-x", "/nonexistent/index"]          # never opened: every case fails in the parser
    labels = tmp_path / "tissues.tsv"
    labels.write_text("liver\t1,2\nbrain\t3\n")
    ids = tmp_path / "ids.txt"
    ids.write_text("1\n2\n")
    L = ["--labels", str(labels)]
    _refused(base + ["-q", "1"], capsys, "--labels")
    _refused(base + L + ["-q", "1", "--all"], capsys, "one query source")
    _refused(base + L + ["--sample", "5", "--query-ids", "1,2"], capsys, "one query source")
    _refused(base + L + ["--intropolis", "q.gz", "--all"], capsys, "one query source")
    _refused(base + L + ["--query-ids", "1,x"], capsys, "--query-ids takes comma-separated integer sample ids")
    _refused(base + L + ["-q", "1", "--sample-seed", "3"], capsys, "--sample-seed cannot be used without --sample")
    _refused(base + L + ["--sample", "0"], capsys, "positive number of samples")
    _refused(base + L + ["-q", "1", "--top", "0"], capsys, "positive number of labels")
    _refused(base + L + ["-f", "bam"], capsys, "sam, bed, raw")
    # --matrix and --leave-out-groups need queries that are samples of the index
    _refused(base + L + ["--intropolis", "q.gz", "--matrix"], capsys, "--matrix cannot be used with --intropolis")
    _refused(base + L + ["-f", "raw", "--matrix"], capsys, "--matrix cannot be used with a query from a stream")
    _refused(base + L + ["--intropolis", "q.gz", "--leave-out-groups", str(labels)], capsys,
             "--leave-out-groups cannot be used with --intropolis")
    _refused(base + L + ["-f", "raw", "--leave-out-groups", str(labels)], capsys,
             "--leave-out-groups cannot be used with a query from a stream")
    _refused(base + L + ["-q", "1", "--within", str(ids), "--without", str(ids)], capsys, "--within and --without both name sample id 1")
    # the files are read in the parser
    _refused(base + ["--labels", str(tmp_path / "missing.tsv"), "-q", "1"], capsys, "missing.tsv")
    bad = tmp_path / "bad.tsv"
    bad.write_text("liver\t1,x\n")
    _refused(base + ["--labels", str(bad), "-q", "1"], capsys, "not an integer sample id")
    bad.write_text("liver\t1\nliver\t2\n")
    _refused(base + ["--labels", str(bad), "-q", "1"], capsys, "names a second group")
    bad.write_text("\n")
    _refused(base + ["--labels", str(bad), "-q", "1"], capsys, "names no label")
    # more than 4096 labels
    bad.write_text("".join("t%d\t%d\n" % (i, i) for i in range(4097)))
    _refused(base + ["--labels", str(bad), "-q", "1"], capsys, "names 4097 labels, at most 4096 are taken")
    # flags of `search` that `labels` does not take
    for flag in (["-e"], ["--unhashed"], ["-r", "5"], ["--search-k", "10"]):
        _refused(base + L + ["-q", "1"] + flag, capsys, "unrecognized arguments")


def test_flags_parse():
    from morna_amd import cli
    p = cli.build_parser()
    args = p.parse_args(["labels", "-x", "i", "--labels", "t.tsv", "--sample", "9"])
    assert (args.sample, args.sample_seed, args.top, args.matrix, args.summary_only, args.all_items, args.format) == \
        (9, 0, 3, False, False, False, "sam")
    args = p.parse_args(["labels", "-x", "i", "--labels", "t.tsv", "--all", "--matrix", "--top", "5", "--summary-only"])
    assert (args.all_items, args.matrix, args.top, args.summary_only) == (True, True, 5, True)
    # today's command lines are left alone
    args = p.parse_args(["search", "-x", "i", "-q", "7"])
    assert not hasattr(args, "labels") and not hasattr(args, "all_items")


def test_refusals_on_row_shards_under_torchrun_and_past_the_label_limit(tmp_path, monkeypatch):
    from morna_amd import cli
    from morna_amd.search import LABELS_SHARDS_REFUSAL, MornaSearch, labels_max_refusal
    base = str(tmp_path / "idx")
    open(base + ".shards.mor", "w").close()
    labels = tmp_path / "tissues.tsv"
    labels.write_text("liver\t1,2\nbrain\t3\n")
    argv = ["labels", "-x", base, "--labels", str(labels), "-q", "1"]
    with pytest.raises(ValueError) as e:
        cli.main(argv)
    assert str(e.value) == LABELS_SHARDS_REFUSAL and "row shards" in LABELS_SHARDS_REFUSAL
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one process per shard"):
        cli.main(argv)
    monkeypatch.delenv("WORLD_SIZE")
    s = MornaSearch.__new__(MornaSearch)
    s.annoy_index = object()                    # stands for shards.LocalShards: not one AnnoyIndex
    with pytest.raises(ValueError) as e:
        s.label_separation([0, 1], [("liver", [1])])
    assert str(e.value) == LABELS_SHARDS_REFUSAL

    class FakeIndex(object):                    # label_separation checks its arguments before the first library call
        def get_n_items(self):
            return 4
    from morna_amd import search
    monkeypatch.setattr(search, "AnnoyIndex", FakeIndex)
    s.annoy_index = FakeIndex()
    s.internal_id_map = {10: 0, 11: 1, 12: 2, 13: 3}
    with pytest.raises(ValueError) as e:
        s.label_separation([0], [("t%d" % i, []) for i in range(4097)])
    assert str(e.value) == labels_max_refusal(4097) and "4097" in str(e.value) and "4096" in str(e.value)
    with pytest.raises(ValueError, match="names 0 labels"):
        s.label_separation([0], [])
    # a --labels file naming an id twice, or an id outside the index
    with pytest.raises(ValueError, match="sample id 11 is in two groups, liver and brain"):
        s.label_separation([0], [("liver", [10, 11]), ("brain", [11])])
    with pytest.raises(ValueError, match="group brain names sample id 99, which is not in the index"):
        s.label_separation([0], [("liver", [10]), ("brain", [99])])
    s.internal_id_map[14] = 7
    with pytest.raises(ValueError, match="outside the index's 4 items"):
        s.label_separation([0], [("liver", [14])])


def test_labels_file_ids_become_item_labels():
    from morna_amd.search import restriction_arrays
    allow, item_label, n = restriction_arrays({10: 0, 11: 1, 12: 2, 13: 3}, 4, groups=[("liver", [12, 10]), ("empty", []), ("brain", [13])])
    assert allow is None and n == 3 and item_label.tolist() == [0, -1, 0, 2] and item_label.dtype == np.int32


# ---- the ctypes table against the header's prototypes ----------------------------------------------------------------------

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
    for name in ("morna_label_sums", "morna_label_sums_stats"):
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is _ctype_of(m.group(1)), name
        want = [_ctype_of(a) for a in m.group(2).split(",")]
        assert len(args) == len(want), name
        for i, (got, w) in enumerate(zip(args, want)):
            assert got is w, (name, i, got, w)
    m = re.search(r"morna_label_sums\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "r", "q", "items", "nq", "q_group", "item_label", "n_labels", "sums_out", "counts_out"]
    assert re.search(r"#define\s+MORNA_LABELS_MAX\s+4096\b", src)
    from morna_amd.search import LABELS_MAX
    assert LABELS_MAX == 4096
