"""`morna cluster`, host side: the numpy restatements of the contract (kmeans_ref.py) pinned on a hand-made
matrix and against the oracle's cosine_distance, the seed sampler, the line formats, the -o writer against parse_groups_file,
every argparse refusal, and the ctypes signatures of the three calls against the header.  No GPU."""
import ctypes as C
import math
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from kmeans_ref import ref_assign, ref_distances, ref_kmeans, ref_scales  # noqa: F401


# rows along the axes (every s_i a power of two), the zero row and one diagonal row
HAND = np.array([[1, 0], [2, 0], [0, 1], [0, 4], [0, 0], [4, 0], [0, 2], [1, 1]], np.float32)


def test_hand_made_matrix():
    """Seeds 0 and 2: c0 = (1, 0), c1 = (0, 1).  t = 1: the axis rows go to their axis at distance 0; the zero row is at
    sqrt(2) from both and the diagonal row at sqrt(2 - 2 / sqrt(2)) from both: ties, cluster 0.  Update: c0 = (1, 0) + (2, 0) / 2
    + (4, 0) / 4 + (1, 1) * s7 (the zero row is skipped), s7 = 1 / sqrt(2); c1 = (0, 1) + (0, 4) / 4 + (0, 2) / 2.  t = 2: the
    diagonal row is now nearer c0, nothing moves: converged, and the centroids returned are the ones of the update."""
    s7 = 1.0 / math.sqrt(2.0)
    a1, d1 = ref_assign(HAND, HAND[[0, 2]].astype(np.float64))
    assert a1.tolist() == [0, 0, 1, 1, 0, 0, 1, 0] and a1.dtype == np.int32
    tie = math.sqrt(2.0 - (2.0 * 1.0) / math.sqrt(2.0 * 1.0))
    assert d1.tolist() == [0.0, 0.0, 0.0, 0.0, math.sqrt(2.0), 0.0, 0.0, tie]
    ok, s = ref_scales(HAND)
    assert ok.tolist() == [True, True, True, True, False, True, True, True]
    assert s[ok].tolist() == [1.0, 0.5, 1.0, 0.25, 0.25, 0.5, s7]
    out = ref_kmeans(HAND, [0, 2], 100)
    assert out["assign"].tolist() == [0, 0, 1, 1, 0, 0, 1, 0]
    assert out["centroids"].tolist() == [[((0.0 + 1.0) + 1.0) + 1.0 + s7, 0.0 + s7], [0.0, 3.0]]
    assert out["sizes"].tolist() == [5, 3] and out["iterations"] == 2 and out["converged"] is True
    assert out["dist"][2] == 0.0 and out["dist"][4] == math.sqrt(2.0) and 0 < out["dist"][7] < tie
    # max_iter 1: the seeds' own assignment, not converged, the seeds returned
    one = ref_kmeans(HAND, [0, 2], 1)
    assert one["iterations"] == 1 and one["converged"] is False and one["centroids"].tolist() == [[1.0, 0.0], [0.0, 1.0]]
    assert one["assign"].tolist() == a1.tolist() and one["dist"].tolist() == d1.tolist()
    # an allow-list: the rows left out show -1 and -1.0 and add nothing to a centroid
    allow = np.array([1, 1, 1, 1, 1, 0, 1, 0], bool)
    part = ref_kmeans(HAND, [0, 2], 100, allow)
    assert part["assign"].tolist() == [0, 0, 1, 1, 0, -1, 1, -1] and part["dist"][5] == -1.0 and part["dist"][7] == -1.0
    assert part["centroids"].tolist() == [[2.0, 0.0], [0.0, 3.0]] and part["sizes"].tolist() == [3, 3]
    # a cluster of the zero row alone keeps its centroid: the zero row and (1, 0) as seeds; every other row is nearer (1, 0)
    z = ref_kmeans(HAND[[4, 0, 1, 5, 7]], [0, 1], 100)
    assert z["assign"].tolist() == [0, 1, 1, 1, 1] and z["centroids"][0].tolist() == [0.0, 0.0] and z["converged"] is True


def test_ties_nan_and_order():
    # a NaN orders behind every number, all NaN goes to centroid 0; equal distances go to the lowest index
    X = np.array([[1, 2], [np.inf, 1], [3, 3]], np.float32)
    Cn = np.array([[np.inf, 0.0], [1.0, 2.0], [2.0, 4.0]])
    d = ref_distances(X, Cn)
    assert np.isnan(d[0, 0]) and d[0, 1] == d[0, 2]
    a, dist = ref_assign(X, Cn)
    assert a.tolist()[0] == 1 and np.isnan(d[1]).all() and a[1] == 0
    assert dist[1:2].tobytes() == np.array([np.nan]).tobytes()


def test_distances_equal_the_oracle():
    from oracle import capi
    rng = np.random.RandomState(5)
    X = (rng.standard_normal((20, 37)) * np.exp(rng.uniform(-20, 20, (20, 1)))).astype(np.float32)
    X[3] = 0
    Cn = rng.standard_normal((10, 37)) * np.exp(rng.uniform(-40, 40, (10, 1)))
    Cn[4] = 0
    Cn[5] = X[7].astype(np.float64) * 3
    d = ref_distances(X, Cn)
    for i in range(20):
        for j in range(10):
            want = capi.cosine_distance(X[i], Cn[j])
            assert d[i, j] == want or (np.isnan(want) and np.isnan(d[i, j])), (i, j)


def test_seed_sampler_formats_and_groups_file(tmp_path):
    from morna_amd.junctions import parse_groups_file
    from morna_amd.search import (SearchClusters, cluster_label, cluster_max_refusal, cluster_seed_items, cluster_table,
                                  format_clusters_header, format_clusters_row, format_clusters_sample, write_groups_file)
    assert cluster_seed_items([9, 2, 5, 7], 2, 3) == random.Random(3).sample([2, 5, 7, 9], 2)
    assert cluster_seed_items(range(100), 7, 0) == random.Random(0).sample(list(range(100)), 7)
    for k in (0, 5):
        with pytest.raises(ValueError) as e:
            cluster_seed_items([1, 2, 3, 4], k, 0)
        assert str(e.value) == cluster_max_refusal(k, 4)
    assert [cluster_label(j) for j in (0, 12, 4095)] == ["c0000", "c0012", "c4095"]
    assign = np.array([1, 0, -1, 1, 1, 0], np.int32)
    dist = np.array([0.5, 0.25, -1.0, 0.125, 0.125, 0.25])
    assert cluster_table(assign, dist, 3) == [(2, 0.25, 1), (3, (0.5 + 0.125 + 0.125) / 3, 3), (0, None, None)]
    nan = float("nan")
    t = cluster_table(np.array([0, 0, 0], np.int32), np.array([nan, 0.5, 0.5]), 1)
    assert t[0][0] == 3 and t[0][1] != t[0][1] and t[0][2] == 1
    assert format_clusters_header(3, 7, True, 5, 0.25) == "# clusters 3\titerations 7\tconverged yes\tsamples 5\tmean distance 0.25\n"
    assert format_clusters_header(1, 100, False, 0, nan).endswith("converged no\tsamples 0\tmean distance nan\n")
    assert format_clusters_row("c0001", 3, 0.25, 77) == "c0001\t3\t0.25\t77\n"
    assert format_clusters_row("c0002", 0, None, None, "-") == "c0002\t0\t-\t-\t-\n"
    assert format_clusters_row("c0000", 1, 0.0, 5, "('liver\\n',)") == "c0000\t1\t0.0\t5\t('liver\\n',)\n"
    assert format_clusters_sample(101, "c0003", 0.125) == "101\tc0003\t0.125\n"
    groups = [("c0000", [101, 7]), ("c0001", []), ("c0002", [3])]
    path = str(tmp_path / "clusters.tsv")
    write_groups_file(path, groups)
    assert parse_groups_file(path) == groups
    c = SearchClusters(groups, [2, 0, 1], [0.25, None, 0.0], [7, None, 3], [(101, 0, 0.5), (7, 0, 0.0), (3, 2, 0.0)], 4, True, {})
    assert c.header() == "# clusters 3\titerations 4\tconverged yes\tsamples 3\tmean distance %s\n" % str((0.5 + 0.0 + 0.0) / 3)
    assert c.rows() == "c0000\t2\t0.25\t7\nc0001\t0\t-\t-\nc0002\t1\t0.0\t3\n"
    assert c.rows({7: "x"}) == "c0000\t2\t0.25\t7\tx\nc0001\t0\t-\t-\t-\nc0002\t1\t0.0\t3\t-\n"
    assert c.sample_lines() == "101\tc0000\t0.5\n7\tc0000\t0.0\n3\tc0002\t0.0\n"


def _refused(argv, capsys, text):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err, err


def test_argparse_refusals_before_any_index_is_read(tmp_path, capsys, monkeypatch):
    from morna_amd.search import CLUSTER_SHARDS_REFUSAL
    base = ["cluster", "-x", "/nonexistent/index"]
    ids = tmp_path / "ids.txt"
    ids.write_text("1\n2\n")
    groups = tmp_path / "groups.tsv"
    groups.write_text("a\t1,2\n")
    _refused(base, capsys, "cluster needs -k")
    _refused(base + ["-k", "3", "-e"], capsys, "cluster cannot be used with -e/--exact")
    _refused(base + ["-k", "3", "--unhashed"], capsys, "cluster cannot be used with --unhashed")
    _refused(base + ["-k", "3", "--leave-out-groups", str(groups)], capsys, "cluster cannot be used with --leave-out-groups")
    _refused(base + ["-k", "0"], capsys, "-k takes 1 to 4096 groups (got 0)")
    _refused(base + ["-k", "4097"], capsys, "-k takes 1 to 4096 groups (got 4097)")
    _refused(base + ["-k", "3", "--max-iterations", "0"], capsys, "--max-iterations takes a positive number")
    _refused(base + ["--init-ids", str(ids), "--seed", "4"], capsys, "--seed and --init-ids cannot be used together")
    _refused(base + ["--init-ids", str(ids), "-k", "3"], capsys, "-k 3, but --init-ids names 2 samples")
    _refused(base + ["--init-ids", str(tmp_path / "missing.txt")], capsys, "missing.txt")
    twice = tmp_path / "twice.txt"
    twice.write_text("1\n2\n1\n")
    _refused(base + ["--init-ids", str(twice)], capsys, "names a sample twice")
    bad = tmp_path / "bad.txt"
    bad.write_text("1\nx\n")
    _refused(base + ["-k", "2", "--within", str(bad)], capsys, "not an integer sample id")
    _refused(base + ["-k", "2", "--within", str(ids), "--without", str(ids)], capsys, "--within and --without both name sample id 1")
    for flag in (["-r", "5"], ["--search-k", "10"], ["-q", "1"]):
        _refused(base + ["-k", "2"] + flag, capsys, "unrecognized arguments")
    # an index of row shards, and one process per shard
    sharded = str(tmp_path / "idx")
    open(sharded + ".shards.mor", "w").close()
    _refused(["cluster", "-x", sharded, "-k", "2"], capsys, CLUSTER_SHARDS_REFUSAL)
    monkeypatch.setenv("WORLD_SIZE", "2")
    _refused(base + ["-k", "2"], capsys, CLUSTER_SHARDS_REFUSAL)
    monkeypatch.delenv("WORLD_SIZE")


def test_flags_parse_and_library_side_refusals(monkeypatch):
    from morna_amd import cli, search
    from morna_amd.search import CLUSTER_SHARDS_REFUSAL, MornaSearch, cluster_max_refusal
    p = cli.build_parser()
    args = p.parse_args(["cluster", "-x", "i", "-k", "30"])
    assert (args.clusters, args.seed, args.init_ids, args.max_iterations, args.output, args.summary_only, args.metadata) == \
        (30, 0, None, 100, None, False, False)
    args = p.parse_args(["cluster", "-x", "i", "-k", "4", "--seed", "9", "-o", "c.tsv", "--summary-only", "-m", "--max-iterations", "7"])
    assert (args.seed, args.output, args.summary_only, args.metadata, args.max_iterations) == (9, "c.tsv", True, True, 7)
    assert not hasattr(p.parse_args(["search", "-x", "i", "-q", "7"]), "clusters")
    s = MornaSearch.__new__(MornaSearch)
    s.annoy_index = object()                    # stands for shards.LocalShards
    with pytest.raises(ValueError) as e:
        s.cluster_samples(3)
    assert str(e.value) == CLUSTER_SHARDS_REFUSAL

    class FakeIndex(object):                    # cluster_samples checks its arguments before the first library call
        def get_n_items(self):
            return 4
    monkeypatch.setattr(search, "AnnoyIndex", FakeIndex)
    s.annoy_index = FakeIndex()
    s.internal_id_map = {10: 0, 11: 1, 12: 2, 13: 3}
    for k in (0, 5):
        with pytest.raises(ValueError) as e:
            s.cluster_samples(k)
        assert str(e.value) == cluster_max_refusal(k, 4)
    with pytest.raises(ValueError, match="cluster needs k or init_ids"):
        s.cluster_samples()
    with pytest.raises(ValueError, match="k = 3, but 2 first centroids are named"):
        s.cluster_samples(3, init_ids=[10, 11])
    with pytest.raises(ValueError, match="Querying sample id 99 is not possible"):
        s.cluster_samples(init_ids=[10, 99])


def _ctype_of(decl):
    decl = re.sub(r"\bconst\b", "", decl).strip()
    stars = decl.count("*")
    base = decl.replace("*", " ").split()[0]
    if stars:
        return C.c_void_p
    return {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "int": C.c_int}[base]


def test_ctypes_signatures_match_the_header():
    from morna_amd import _lib
    with open(os.path.join(ROOT, "include", "morna_hip.h")) as fh:
        src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("morna_kmeans", "morna_kmeans_assign", "morna_kmeans_stats"):
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is _ctype_of(m.group(1)), name
        want = [_ctype_of(a) for a in m.group(2).split(",")]
        assert len(args) == len(want), name
        for i, (got, w) in enumerate(zip(args, want)):
            assert got is w, (name, i, got, w)
    m = re.search(r"morna_kmeans\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "r", "seed_items", "k", "max_iter", "assign_out", "dist_out", "centroids_out", "sizes_out", "info_out"]
    m = re.search(r"morna_kmeans_assign\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "r", "centroids", "k", "assign_out", "dist_out"]
