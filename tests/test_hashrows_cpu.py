"""Hashed rows from store rows and `morna hashing`, host side: the restatement of the contract the GPU
tests compare with, pinned to the recorded feature matrices of the embedded fixtures; the table arithmetic, the --features
parser, the command line's argparse errors and refusals, and the ctypes signatures against the header.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_unhashed_cpu import ref_rows, ref_weights


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def ref_hash_rows(rows, w, line_hash, D):
    """The contract of morna_add_items_from_store in Python floats: rows[i] = (lines ascending, coverages); cell c of row i
    is S from +0.0, S = RN(S + sgn * RN(float(cov) * w[j])) over the entries with w[j] != 0 and hash[j] mod D == c (Python's
    floored modulo; sgn from the hash before the modulo) in line order, rounded once to fp32.  Sequential per cell."""
    D = int(D)
    out = np.zeros((len(rows), D), np.float32)
    for i, (lines, covs) in enumerate(rows):
        acc = [0.0] * D
        for j, cov in zip(np.asarray(lines).tolist(), np.asarray(covs).tolist()):
            wj = float(w[j])
            if wj == 0.0:
                continue
            h = int(line_hash[j])
            term = float(cov) * wj
            acc[h % D] = acc[h % D] + (-term if h < 0 else term)
        with np.errstate(over="ignore"):
            out[i] = np.array(acc, np.float64).astype(np.float32)
    return out


def host_hashes(lines):
    """int32 murmur3 of every line's "chrom start end" key through the library's host function."""
    from morna_amd._lib import lib
    out = []
    for text in lines:
        raw = " ".join(text.split("\t")[:3]).encode("ascii")
        out.append(int(lib().morna_hash32(raw, len(raw))))
    return np.array(out, np.int32)


@pytest.mark.parametrize("name", ["simple", "lossy", "lose_sample"])
@pytest.mark.parametrize("D", [40, 128, 3000])
def test_restatement_reproduces_the_recorded_matrices(embedded, embedded_mats, name, D):
    spec = embedded["expected"][name]
    lines = embedded[spec["input"]]
    assert len(set(" ".join(t.split("\t")[:3]) for t in lines)) == len(lines) == 20     # distinct keys: the line weights exist
    w = ref_weights(lines, spec["sample_count"], spec["sample_threshold"])
    rows = ref_rows(lines)
    ext = embedded_mats["%s_D%d_ext_ids" % (name, D)].tolist()
    assert len(ext) == spec["n_items"]
    got = ref_hash_rows([rows[s] for s in ext], w, host_hashes(lines), D)
    want = embedded_mats["%s_D%d_f32" % (name, D)]
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


def test_restatement_order_sign_and_modulo():
    # one cell, in line order: +2^60, +1, -2^60 gives 0.0; any other order gives 1.0
    w = np.array([2.0 ** 60, 1.0, 2.0 ** 60, 5.0, 0.0])
    h = np.array([7, 14, -7, -1, 3], np.int32)
    rows = [([0, 1, 2], [1, 1, 1]), ([3], [2]), ([4], [9]), ([], [])]
    out = ref_hash_rows(rows, w, h, 7)
    assert out[0].tolist() == [0.0] * 7
    assert out[1].tolist() == [0, 0, 0, 0, 0, 0, -10.0]                # -1 mod 7 == 6, the sign from the hash
    assert not out[2].any() and not out[3].any()                       # weight 0: no term; no entries: no row
    assert ref_hash_rows(rows[:1], w, np.array([7, 14, -8, 0, 0], np.int32), 7)[0].tolist() == [2.0 ** 60, 0, 0, 0, 0, 0, -2.0 ** 60]


# ---- the table arithmetic ----------------------------------------------------------------------------------------------------
def test_drop_query():
    from morna_amd.search import drop_query
    assert drop_query([5, 3, 9, -1], [0.0, 0.1, 0.2, np.inf], 5, 2) == ([3, 9], [0.1, 0.2])
    assert drop_query([3, 9, 4], [0.1, 0.2, 0.3], 5, 2) == ([3, 9], [0.1, 0.2])         # the query absent from its own list
    assert drop_query([3, 5, 9], [0.1, 0.1, 0.2], 5, 10) == ([3, 9], [0.1, 0.2])
    assert drop_query([5], [0.0], 5, 3) == ([], [])


def test_table_arithmetic():
    from morna_amd.search import format_hashing_rows, hashing_rows, hashing_summary, norm_ratio_stats
    truth = ([3, 9, 4, 7], [0.5, 0.625, 0.75, 0.875])                   # (dyadic distances: the arithmetic below is exact)
    exact = [([9, 1, 2, 8], [0.25, 0.3, 0.4, 0.5]),                     # one shared id: 9
             ([7, 3, 4, 9], [0.875, 0.5, 0.8125, 0.75]),                # all four
             ([1, 2, 6, 8], [0.1, 0.2, 0.3, 0.4])]                      # none
    approx = [([9, 3], [0.25, 0.5]), ([], []), ([4], [0.7])]
    rows = hashing_rows([16, 64, 300], truth, exact)
    assert rows[0] == (16, 4, 1, 0.25, 0.375)
    assert rows[1] == (64, 4, 4, 1.0, (0.0 + 0.125 + 0.0625 + 0.0) / 4)
    assert rows[2] == (300, 4, 0, 0.0, None)                            # no shared ids
    rows_a = hashing_rows([16, 64, 300], truth, exact, approx)
    assert [r[5:] for r in rows_a] == [(2, 0.5), (0, 0.0), (1, 0.25)] and [r[:5] for r in rows_a] == rows
    empty = hashing_rows([16], ([], []), [([1, 2], [0.1, 0.2])], [([1], [0.1])])
    assert empty == [(16, 0, 0, None, None, 0, None)]                   # truth 0
    assert format_hashing_rows(rows) == "16\t4\t1\t0.250000\t0.375000\n64\t4\t4\t1.000000\t0.046875\n300\t4\t0\t0.000000\t-\n"
    assert format_hashing_rows(empty) == "16\t0\t0\t-\t-\t0\t-\n"
    # the block over all queries, from the queries' own lines
    other = hashing_rows([16, 64, 300], ([1, 2], [0.125, 0.25]), [([1], [0.25]), ([2, 1], [0.25, 0.125]), ([5], [0.0])])
    none = hashing_rows([16, 64, 300], ([], []), [([1], [0.2])] * 3)
    summary = hashing_summary([rows, other, none], [(1.0, 0.0), (0.5, 0.25), (None, None)])
    assert summary[0] == (16, 6, 2, 2.0 / 6, (0.375 + 0.125) / 2, 1.0, 0.0)
    assert summary[1] == (64, 6, 6, 1.0, (0.046875 + 0.0) / 2, 0.5, 0.25)
    assert summary[2] == (300, 6, 0, 0.0, None, None, None)
    assert hashing_summary([none], [(1.0, 0.0)] * 3)[0] == (16, 0, 0, None, None, 1.0, 0.0)
    summary_a = hashing_summary([rows_a, rows_a], [(1.0, 0.0)] * 3)
    assert summary_a[0] == (16, 8, 2, 0.25, 0.375, 4, 0.5, 1.0, 0.0)
    # the norm columns: items without a norm left out, the variance of one item, nothing at all
    mean, var = norm_ratio_stats(np.array([4.0, 9.0, 7.0], np.float32), np.array([1.0, 36.0, 0.0]))
    assert mean == (2.0 + 0.5) / 2 and var == ((2.0 - 1.25) ** 2 + (0.5 - 1.25) ** 2) / 2
    assert norm_ratio_stats([2.25], [1.0]) == (1.5, 0.0)
    assert norm_ratio_stats([2.25, 1.0], [0.0, 0.0]) == (None, None)


def test_features_parser():
    from morna_amd.search import parse_features_list
    assert parse_features_list("500,1000,3000,8192,index", index_dim=32768) == [500, 1000, 3000, 8192, 32768]
    assert parse_features_list("index", index_dim=64) == [64]
    assert parse_features_list("16,index,300", index_dim=64) == [16, 64, 300]
    assert parse_features_list("1,32768") == [1, 32768]
    assert parse_features_list(",".join(map(str, range(1, 17)))) == list(range(1, 17))
    for text, dim, word in (("3000,500", None, "ascend"), ("64,index", 64, "ascend"), ("index,16", 64, "ascend"),
                            ("0,5", None, "positive"), ("5,32769", None, "32768"), (",".join(map(str, range(1, 18))), None, "16"),
                            ("index", None, "index"), ("5,x", None, "integer"), ("", None, "integer")):
        with pytest.raises(ValueError, match=word):
            parse_features_list(text, index_dim=dim)


# ---- the command line, before any index is read ------------------------------------------------------------------------------
def _refused(argv, capsys, text):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err, err


def test_argparse_errors_before_any_index_is_read(tmp_path, capsys):
    base = ["hashing", "-x", "/nonexistent/index", "--junction-file", "/nonexistent/j.gz"]
    f = ["--features", "16,64"]
    ids = tmp_path / "ids.txt"
    ids.write_text("1\n2\n")
    _refused(base + f, capsys, "exactly one query source")
    _refused(base + f + ["-q", "1", "--sample", "5"], capsys, "exactly one query source")
    _refused(base + ["-q", "1"], capsys, "--features")
    _refused(["hashing", "-x", "i", "-q", "1"] + f, capsys, "--junction-file")
    _refused(base + ["-q", "1", "--features", "64,16"], capsys, "ascend")
    _refused(base + ["-q", "1", "--features", "0,16"], capsys, "positive")
    _refused(base + ["-q", "1", "--features", "16,32769"], capsys, "32768")
    _refused(base + ["-q", "1", "--features", ",".join(map(str, range(1, 18)))], capsys, "at most 16")
    _refused(base + ["-q", "1", "--features", "index,index"], capsys, "twice")
    _refused(base + ["-q", "1", "--features", "16,all"], capsys, "integer")
    _refused(base + f + ["--query-ids", "1,x"], capsys, "--query-ids takes comma-separated integer sample ids")
    _refused(base + f + ["-q", "1", "--sample-seed", "3"], capsys, "--sample-seed cannot be used without --sample")
    _refused(base + f + ["--sample", "0"], capsys, "positive number of samples")
    _refused(base + f + ["-q", "1", "-r", "257"], capsys, "1 to 256")
    _refused(base + f + ["-q", "1", "--search-k", "50"], capsys, "--search-k cannot be used without --n-trees")
    _refused(base + f + ["-q", "1", "--n-trees", "0"], capsys, "positive tree count")
    for flag, word in ((["-e"], "-e/--exact"), (["--unhashed"], "--unhashed"), (["--within", str(ids)], "--within"),
                       (["--without", str(ids)], "--without"), (["--leave-out-groups", str(ids)], "--leave-out-groups"),
                       (["--intropolis", "q.gz"], "--intropolis")):
        _refused(base + f + ["-q", "1"] + flag, capsys, "hashing cannot be used with %s: " % word)


def test_flags_parse():
    from morna_amd import cli
    p = cli.build_parser()
    args = p.parse_args(["hashing", "-x", "i", "--junction-file", "j.gz", "--sample", "9", "--features", "500,index", "--n-trees", "4"])
    cli._check_hashing_flags(p, args)
    assert (args.sample, args.sample_seed, args.results, args.n_trees, args.search_k, args.summary_only) == (9, 0, 20, 4, 100, False)
    args = p.parse_args(["hashing", "-x", "i", "--junction-file", "j.gz", "--query-ids", "3,4", "--features", "index", "-r", "10",
                         "--summary-only"])
    cli._check_hashing_flags(p, args)
    assert args.query_ids == [3, 4] and args.n_trees is None and args.summary_only


def test_refusals_without_a_gpu(tmp_path, monkeypatch):
    """Row shards, a torchrun launch, a missing store and missing weights are refused before anything is loaded."""
    from morna_amd import cli
    from morna_amd.search import HASHING_SHARDS_REFUSAL, MornaSearch
    base = str(tmp_path / "idx")
    argv = ["hashing", "-x", base, "--junction-file", "j.gz", "-q", "1", "--features", "16,index"]
    with pytest.raises(IOError, match="no junction store"):
        cli.main(argv)
    open(base + ".junc.mor", "w").close()
    with pytest.raises(IOError) as e:
        cli.main(argv)
    assert "--unhashed needs the line weights" in str(e.value) and "repeated junctions" in str(e.value)
    open(base + ".shards.mor", "w").close()
    with pytest.raises(ValueError) as e:
        cli.main(argv)
    assert str(e.value) == HASHING_SHARDS_REFUSAL and "row shards" in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one process per shard"):
        cli.main(argv)
    monkeypatch.delenv("WORLD_SIZE")
    s = MornaSearch.__new__(MornaSearch)
    s.annoy_index = object()                    # stands for shards.LocalShards: not one AnnoyIndex
    with pytest.raises(ValueError, match="row shards"):
        s.hashing_sweep([1], 10, [16], "j.gz")


# ---- the ctypes table against the header's prototypes ------------------------------------------------------------------------
_NEW = ("morna_add_items_from_store", "morna_jstore_hash_rows_stats", "morna_jstore_row_norms")


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
    m = re.search(r"morna_add_items_from_store\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "s", "ext", "n", "line_hash", "n_lines"]
    m = re.search(r"morna_jstore_row_norms\s*\(([^)]*)\)", src)
    assert [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")] == ["s", "ext", "n", "pp_out"]
