"""Restricted search, host side: the bitmap and labels made from external sample ids, the refusals, the default search_k,
the command line's argparse errors and the ctypes signatures of the five calls against the header.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ID_MAP = {101: 0, 205: 1, 33: 2, 47: 3, 590: 4, 6: 5, 77: 6}      # external sample id -> internal id


def test_allow_bitmap_from_external_ids():
    from morna_amd.search import restriction_arrays
    n = len(ID_MAP)
    allow, group, n_groups = restriction_arrays(ID_MAP, n)
    assert allow is None and group is None and n_groups == 0
    allow, _, _ = restriction_arrays(ID_MAP, n, within=[33, 101, 6])
    assert allow.tolist() == [True, False, True, False, False, True, False]
    allow, _, _ = restriction_arrays(ID_MAP, n, without=[33, 77])
    assert allow.tolist() == [True, True, False, True, True, True, False]
    allow, _, _ = restriction_arrays(ID_MAP, n, within=[33, 101, 6, 590], without=[6, 47])
    assert allow.tolist() == [True, False, True, False, True, False, False]
    allow, _, _ = restriction_arrays(ID_MAP, n, within=[])
    assert not allow.any()
    for kw in (dict(within=[33, 9999]), dict(without=[9999]), dict(groups=[("a", [9999])])):
        with pytest.raises(ValueError, match="9999"):
            restriction_arrays(ID_MAP, n, **kw)


def test_group_labels_from_external_ids():
    from morna_amd.search import restriction_arrays
    n = len(ID_MAP)
    allow, group, n_groups = restriction_arrays(ID_MAP, n, groups=[("donor1", [205, 6]), ("empty", []), ("donor2", [77])])
    assert allow is None and n_groups == 3 and group.dtype == np.int32
    assert group.tolist() == [-1, 0, -1, -1, -1, 0, 2]
    allow, group, _ = restriction_arrays(ID_MAP, n, within=[205, 33], groups=[("g", [205, 205])])
    assert allow.tolist() == [False, True, True, False, False, False, False] and group.tolist() == [-1, 0, -1, -1, -1, -1, -1]
    with pytest.raises(ValueError, match="590.*donor1.*donor2"):
        restriction_arrays(ID_MAP, n, groups=[("donor1", [590]), ("donor2", [47, 590])])


def test_allow_bits_packing():
    from morna_amd.annoy import pack_allow_bits
    allow = np.zeros(70, bool)
    allow[[0, 31, 33, 69]] = True
    assert pack_allow_bits(allow).tolist() == [0x80000001, 0x2, 0x20]
    assert pack_allow_bits(np.ones(32, bool)).tolist() == [0xffffffff]
    assert pack_allow_bits(np.ones(33, bool)).tolist() == [0xffffffff, 1]


def test_default_search_k_under_an_allow_list():
    from morna_amd.search import INT32_MAX, MornaSearch, restricted_search_k
    assert restricted_search_k(200, 20, 50000, 50000) == 200 * 20
    assert restricted_search_k(200, 20, 50000, 25000) == 200 * 20 * 2
    assert restricted_search_k(200, 20, 50000, 24999) == 200 * 20 * 3          # ceil
    assert restricted_search_k(200, 20, 50000, 500) == 200 * 20 * 100
    assert restricted_search_k(200, 20, 50000, 3) == 200 * 20 * 16667
    assert restricted_search_k(200, 20, 50000, 0) == 200 * 20 * 50000          # (no item allowed: every answer is empty anyway)
    assert restricted_search_k(200, 1000, 10**7, 1) == INT32_MAX == 2**31 - 1

    class Handle(object):
        def get_n_trees(self):
            return 10

    class R(object):
        n_items, n_allowed = 1000, 100
    s = object.__new__(MornaSearch)
    s.annoy_index = Handle()
    r = R()
    r.allow = np.zeros(1000, bool)
    assert s._restricted_search_k(r, 20, -1) == 10 * 20 * 10 and s._restricted_search_k(r, 20, None) == 2000
    assert s._restricted_search_k(r, 20, 100) == 100                            # an explicit search_k is taken as given
    r.allow = None                                                              # groups only: annoy's own default
    assert s._restricted_search_k(r, 20, -1) == -1


def test_sharded_index_is_refused():
    from morna_amd.search import SHARDS_REFUSAL, MornaSearch
    s = object.__new__(MornaSearch)
    s.annoy_index = object()          # what LocalShards / DistShards are to restriction(): not one AnnoyIndex
    s.internal_id_map = ID_MAP
    with pytest.raises(ValueError) as e:
        s.restriction(within=[33])
    assert str(e.value) == SHARDS_REFUSAL and "shards" in SHARDS_REFUSAL
    with pytest.raises(ValueError):
        s._check_restriction(None, np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        s._check_restriction(object(), None)


@pytest.fixture()
def files(tmp_path):
    def write(name, text):
        p = tmp_path / name
        p.write_text(text)
        return str(p)
    return dict(a=write("a.txt", "1\n2\n3\n"), b=write("b.txt", "4\n5\n"), c=write("c.txt", "9\n3\n"),
                bad=write("bad.txt", "1\nx\n"), groups=write("g.tsv", "d1\t1,2\nd2\t3\n"), bad_groups=write("bg.tsv", "d 1\t1\n"))


def _refused(argv, capsys, text):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err, err


def test_argparse_errors_before_any_index_is_read(files, capsys):
    base = ["-x", "/nonexistent/index"]          # never opened: every case fails in the parser
    g = ["--leave-out-groups", files["groups"]]
    _refused(["search"] + base + g + ["--intropolis", "q.tsv.gz"], capsys, "--leave-out-groups cannot be used with --intropolis")
    _refused(["search"] + base + g + ["--supersamples", "s.tsv", "--junction-file", "j.gz"], capsys,
             "--leave-out-groups cannot be used with --supersamples")
    _refused(["search"] + base + g, capsys, "--leave-out-groups cannot be used with a query from a stream")
    _refused(["junctions"] + base + g + ["--junction-file", "j.gz", "-sf", "out"], capsys, "a query from a stream")
    _refused(["search"] + base + g + ["-q", "1", "--unhashed"], capsys, "--leave-out-groups cannot be used with --unhashed")
    _refused(["recovery"] + base + g + ["--intropolis", "q.gz", "--truth", "t.gz", "--junction-file", "j.gz"], capsys,
             "--leave-out-groups cannot be used with --intropolis")
    for sub in ("search", "recovery"):
        _refused([sub] + base + ["-q", "1", "--within", files["a"], "--without", files["c"]], capsys,
                 "--within and --without both name sample id 3")
    _refused(["search"] + base + ["-q", "1", "--within", files["bad"]], capsys, "line 2")
    _refused(["search"] + base + ["-q", "1", "--without", "/nonexistent/ids.txt"], capsys, "/nonexistent/ids.txt")
    _refused(["search"] + base + ["-q", "1", "--leave-out-groups", files["bad_groups"]], capsys, "label")
    _refused(["search"] + base + ["--within", files["a"], "-c", "100"], capsys, "cannot be used with -c")


def test_flags_parse_and_leave_today_s_command_lines_alone(files):
    from morna_amd import cli
    p = cli.build_parser()
    args = p.parse_args(["recovery", "-x", "i", "--query-ids", "1,2", "--within", files["a"], "--without", files["b"],
                         "--leave-out-groups", files["groups"]])
    cli._check_recovery_flags(p, args)
    cli._check_batch_flags(p, args)
    cli._check_restriction_flags(p, args)
    assert args.within_ids == [1, 2, 3] and args.without_ids == [4, 5]
    assert args.leave_out == [("d1", [1, 2]), ("d2", [3])] and args.restriction is None
    args = p.parse_args(["search", "-x", "i", "-q", "7"])
    cli._check_restriction_flags(p, args)
    assert args.within_ids is None and args.without_ids is None and args.leave_out is None and args.restriction is None
    assert cli._search_k(args) == 100


def test_cli_search_k_default():
    from morna_amd import cli

    class R(object):
        allow = np.ones(4, bool)
    p = cli.build_parser()
    args = p.parse_args(["search", "-x", "i", "-q", "7"])
    args.restriction = R()
    assert cli._search_k(args) == -1                 # scaled by the searcher
    args = p.parse_args(["search", "-x", "i", "-q", "7", "--search-k", "100"])
    args.restriction = R()
    assert cli._search_k(args) == 100                # as given
    args = p.parse_args(["search", "-x", "i", "-q", "7"])
    args.restriction = R()
    args.restriction.allow = None                    # leave-out groups alone: today's default
    assert cli._search_k(args) == 100


# ---- the ctypes table against the header's prototypes ----------------------------------------------------------------------

_NEW = ("morna_restriction_create", "morna_restriction_counts", "morna_restriction_free", "morna_get_nns_restricted",
        "morna_exact_search_restricted")


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
            assert got is w or (w is C.POINTER(C.c_void_p) and got == w), (name, i, got, w)
    # the argument order the issue's prototypes give
    m = re.search(r"morna_get_nns_restricted\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "r", "q", "items", "nq", "q_group", "k", "search_k", "ids", "dist", "count"]
    m = re.search(r"morna_exact_search_restricted\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "r", "q", "items", "nq", "q_group", "k", "ids", "dist", "count"]
