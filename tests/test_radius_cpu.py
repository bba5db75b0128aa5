"""Radius search and near-duplicate pairs, the parts that need no GPU: the restatement `ref_radius` the GPU
tests compare with -- the oracle's full list (oracle.capi.exact_search, k = the number of evaluated rows) cut at r -- and its
known answers on a hand-made matrix; pair_clusters; the line formats; the --max-distance parser and its refusals; the ctypes
signatures against the header; the symmetry of the oracle's cosine_distance.
"""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def capi():
    from oracle import capi as c
    c.lib()
    return c


def ref_radius(capi, X, q, r, after=-1, allow=None, groups=None, gq=-1):
    """The contract: the rows with id > after that `allow` holds and whose group is not gq are the evaluated rows; the
    oracle's list over exactly those rows, ids mapped back, cut after the last entry with distance <= r.  (A NaN anywhere:
    the oracle cannot order the list; the caller plants none here.)"""
    n = X.shape[0]
    e = np.ones(n, bool) if allow is None else np.asarray(allow, bool).copy()
    if groups is not None and gq >= 0:
        e &= np.asarray(groups) != gq
    e &= np.arange(n) > after
    rows = np.nonzero(e)[0]
    if len(rows) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float64)
    ids, d = capi.exact_search(X[rows], np.asarray(q, np.float64), len(rows))
    keep = d <= r
    assert not keep[np.argmin(keep):].any() or keep.all()      # the list ascends: the kept entries are a prefix
    return rows[ids[keep]], d[keep]


# rows 0 and 4 are parallel (4 = 2 * 0), 1 is orthogonal to 0, 2 lies between, 3 is opposite, 5 is the zero row
SIX = np.array([[1, 0], [0, 1], [1, 1], [-1, 0], [2, 0], [0, 0]], np.float32)
MID = math.sqrt(2.0 - 2.0 * 1.0 / math.sqrt(2.0))       # cosine_distance of (1, 0) and (1, 1)
ROOT2 = math.sqrt(2.0)


def test_ref_radius_known_answers(capi):
    q = [1.0, 0.0]
    full_ids, full_d = capi.exact_search(SIX, np.array(q), 6)
    assert full_ids.tolist() == [4, 0, 2, 5, 1, 3]                 # equal distance: higher id first
    assert full_d.tolist() == [0.0, 0.0, MID, ROOT2, ROOT2, 2.0]
    for r, want in ((0.0, [4, 0]), (0.5, [4, 0]), (MID, [4, 0, 2]), (np.nextafter(MID, 0.0), [4, 0]), (0.8, [4, 0, 2]),
                    (ROOT2, [4, 0, 2, 5, 1]), (np.nextafter(ROOT2, 0.0), [4, 0, 2]), (1.99, [4, 0, 2, 5, 1]),
                    (2.0, [4, 0, 2, 5, 1, 3]), (2.5, [4, 0, 2, 5, 1, 3])):
        ids, d = ref_radius(capi, SIX, q, r)
        assert ids.tolist() == want, r
        assert d.tobytes() == full_d[:len(want)].tobytes()
    assert ref_radius(capi, SIX, q, 2.0, after=0)[0].tolist() == [4, 2, 5, 1, 3]
    assert ref_radius(capi, SIX, q, 2.0, after=4)[0].tolist() == [5]
    assert ref_radius(capi, SIX, q, 2.0, after=5)[0].tolist() == []
    allow = np.array([1, 1, 0, 1, 0, 1], bool)
    assert ref_radius(capi, SIX, q, 1.5, allow=allow)[0].tolist() == [0, 5, 1]
    groups = np.array([0, 0, 1, -1, 1, -1], np.int32)
    assert ref_radius(capi, SIX, q, 2.0, groups=groups, gq=1)[0].tolist() == [0, 5, 1, 3]
    assert ref_radius(capi, SIX, q, 2.0, groups=groups, gq=-1)[0].tolist() == [4, 0, 2, 5, 1, 3]
    assert ref_radius(capi, SIX, q, 2.0, after=0, allow=allow, groups=groups, gq=0)[0].tolist() == [5, 3]
    # the zero query: every distance is sqrt(2)
    ids, d = ref_radius(capi, SIX, [0.0, 0.0], ROOT2)
    assert ids.tolist() == [5, 4, 3, 2, 1, 0] and set(d.tolist()) == {ROOT2}
    assert ref_radius(capi, SIX, [0.0, 0.0], 1.4)[0].tolist() == []


def test_oracle_distance_is_symmetric_bit_for_bit(capi):
    """d(i, j) and d(j, i): pq and pp * qq are sums and products of the same terms in the same order either way."""
    rng = np.random.default_rng(14)
    X = rng.standard_normal((400, 37)).astype(np.float32)
    X[1] = X[0] * np.float32(1.0 + 2.0 ** -20)            # near-parallel pairs as well
    X[3] = X[2] * np.float32(3.0)
    for i in range(200):
        a, b = X[2 * i], X[2 * i + 1]
        dab = capi.cosine_distance(a, b.astype(np.float64))
        dba = capi.cosine_distance(b, a.astype(np.float64))
        assert struct.pack("<d", dab) == struct.pack("<d", dba), i


def test_pair_clusters():
    from morna_amd.search import pair_clusters
    assert pair_clusters([]) == []
    assert pair_clusters([(5, 9, 0.1)]) == [[5, 9]]
    # a chain, a triple, two pairs of equal size (by their smallest id), ids out of order, a repeated edge
    pairs = [(30, 31, 0.1), (31, 32, 0.1), (32, 33, 0.2), (7, 2, 0.0), (2, 11, 0.0), (7, 11, 0.0), (50, 40, 0.3), (20, 21, 0.3),
             (20, 21, 0.3)]
    assert pair_clusters(pairs) == [[30, 31, 32, 33], [2, 7, 11], [20, 21], [40, 50]]
    assert pair_clusters([(1, 2), (3, 4), (2, 3)]) == [[1, 2, 3, 4]]
    big = [(i, i + 1, 0.0) for i in range(0, 5000)]        # a long chain: no recursion
    assert pair_clusters(big) == [list(range(5001))]


def test_line_formats():
    from morna_amd.search import (format_cluster_line, format_distance, format_pair_line, format_pairs_summary, pair_clusters,
                                  sort_pairs)
    nan = float("nan")
    pairs = sort_pairs([(3, 8, 0.25), (1, 9, 0.25), (4, 5, nan), (1, 2, 0.0), (2, 3, nan), (1, 4, 0.25)])
    assert [p[:2] for p in pairs] == [(2, 3), (4, 5), (1, 2), (1, 4), (1, 9), (3, 8)]
    assert format_pair_line(12, 40, 0.25) == "12\t40\t0.25\n"
    assert format_pair_line(12, 40, nan) == "12\t40\tnan\n"
    assert format_pair_line(12, 40, 0.1, ("liver", "liver;adult")) == "12\t40\t0.1\tliver\tliver;adult\n"
    assert format_distance(np.float64(1.0) / 3) == str(1.0 / 3)          # as `search -d` prints a distance
    clusters = pair_clusters(pairs)
    assert clusters == [[1, 2, 3, 4, 5, 8, 9]]
    assert format_pairs_summary(600, pairs, clusters) == "# samples 600\tpairs 6\tsamples in any pair 7\tlargest cluster 7\n"
    assert format_pairs_summary(600, [], []) == "# samples 600\tpairs 0\tsamples in any pair 0\tlargest cluster 0\n"
    assert format_cluster_line([2, 7, 11]) == "# cluster 3\t2,7,11\n"


def test_parse_max_distance():
    from morna_amd.search import parse_max_distance
    assert parse_max_distance("0.15") == 0.15 and parse_max_distance("0") == 0.0 and parse_max_distance("2.5") == 2.5
    assert parse_max_distance("1e-3") == 1e-3
    for bad in ("-0.1", "nan", "inf", "-inf", "abc", "", None):
        with pytest.raises(ValueError, match="--max-distance takes a distance"):
            parse_max_distance(bad)


def _refused(capsys, argv, message):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert message in err, err


def test_max_distance_refusals(capsys, tmp_path):
    base = ["search", "-x", str(tmp_path / "idx")]
    _refused(capsys, base + ["--max-distance", "0.1"], "--max-distance cannot be used without -e/--exact")
    _refused(capsys, base + ["--max-distance", "0.1", "-q", "3"], "--max-distance cannot be used without -e/--exact")
    _refused(capsys, base + ["-e", "--max-distance", "0.1", "-c", "10"], "--max-distance cannot be used with -c/--convergence-backoff")
    _refused(capsys, base + ["-e", "--max-distance", "0.1", "-rl"], "--max-distance cannot be used with -rl/--rawlist")
    _refused(capsys, base + ["-e", "--max-distance", "0.1", "-r", "0"], "-r takes a positive number of results")
    for bad in ("-1", "nan", "inf", "near"):
        _refused(capsys, base + ["-e", "--max-distance=" + bad], "--max-distance takes a distance")
    # the refusals of the flags it meets come in their own wording, as before
    _refused(capsys, base + ["-e", "--max-distance", "0.1", "--unhashed", "-q", "3"], "--unhashed cannot be used with -e/--exact")
    _refused(capsys, base + ["--max-distance", "0.1", "--unhashed", "-q", "3"], "--max-distance cannot be used without -e/--exact")
    _refused(capsys, base + ["-e", "--max-distance", "0.1", "--use-trees", "5"], "--use-trees cannot be used with -e/--exact")
    _refused(capsys, base + ["--max-distance", "0.1", "--use-trees", "5"], "--max-distance cannot be used without -e/--exact")
    # an index of row shards
    (tmp_path / "idx.shards.mor").write_text("2\n")
    _refused(capsys, base + ["-e", "--max-distance", "0.1"], "not available on an index of row shards")
    # the commands that do not take the flag
    for command in ("junctions", "recovery"):
        with pytest.raises(SystemExit):
            from morna_amd import cli
            cli.build_parser().parse_args([command, "-x", "idx", "--max-distance", "0.1"])
        capsys.readouterr()


def test_pairs_parser(capsys, tmp_path):
    from morna_amd import cli
    _refused(capsys, ["pairs", "-x", "idx"], "--max-distance")
    _refused(capsys, ["pairs", "-x", "idx", "--max-distance", "-2"], "--max-distance takes a distance")
    within, without = tmp_path / "in.txt", tmp_path / "out.txt"
    within.write_text("1\n2\n3\n")
    without.write_text("3\n")
    _refused(capsys, ["pairs", "-x", "idx", "--max-distance", "0.1", "--within", str(within), "--without", str(without)],
             "--within and --without both name sample id 3")
    _refused(capsys, ["pairs", "-x", "idx", "--max-distance", "0.1", "--within", str(tmp_path / "absent")], "absent")
    parser = cli.build_parser()
    args = parser.parse_args(["pairs", "-x", "idx", "--max-distance", "0.05", "--within", str(within), "-m", "--clusters",
                              "--summary-only"])
    cli._check_pairs_flags(parser, args)
    assert args.max_distance == 0.05 and args.within_ids == [1, 2, 3] and args.without_ids is None and args.leave_out is None
    assert args.metadata and args.clusters and args.summary_only
    # search: the distance parsed, -r noted only when given
    args = parser.parse_args(["search", "-x", str(tmp_path / "idx"), "-e", "--max-distance", "0.2"])
    cli._check_max_distance_flags(parser, args)
    assert args.max_distance == 0.2 and cli._radius_cap(args) is None and args.results == 20
    args = parser.parse_args(["search", "-x", str(tmp_path / "idx"), "-e", "--max-distance", "0.2", "-r", "7"])
    cli._check_max_distance_flags(parser, args)
    assert cli._radius_cap(args) == 7
    args = parser.parse_args(["search", "-x", str(tmp_path / "idx"), "-e"])
    cli._check_max_distance_flags(parser, args)
    assert cli._max_distance(args) is None


_CTYPE = {"double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int}


def test_ctypes_signatures_match_the_header():
    """Every parameter of the five declarations against its ctypes entry: a pointer is a pointer, a scalar has its width."""
    from morna_amd import _lib
    with open(os.path.join(ROOT, "include", "morna_hip.h")) as fh:
        src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    names = ["morna_exact_radius", "morna_radius_counts", "morna_radius_query", "morna_radius_free", "morna_exact_radius_stats"]
    for name in names:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(params), (name, params)
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p, t)
                if p.count("*") == 2:                      # an output pointer: written through
                    assert issubclass(t, C._Pointer), (name, p)
            else:
                assert t is _CTYPE[p.split()[-2]], (name, p, t)
    assert _lib.SIGNATURES["morna_exact_radius"][1][7] is C.c_double       # the radius
    assert _lib.SIGNATURES["morna_radius_query"][1][4]._type_ is C.c_int64  # len
