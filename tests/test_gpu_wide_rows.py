"""Rows wider than 8192 floats, up to the 32768 limit: the wide two_means form (forest.hip two_means_wide_kernel), the
split, the approximate and the exact searches at those widths, against the oracle bit for bit.  -m gpu

Rows are made in float32 chunks (a 33000 x 32768 matrix in fp64 would be 8.6 GB); the oracle is one thread, so only a
handful of queries is compared at the widest rows.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from width_forms import compare_approx as _compare_approx, compare_forest as _compare_forest, rows as _rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from oracle import capi as c
    c.lib()
    return c


@pytest.mark.parametrize("f,N,T", [(8448, 9000, 2),       # the first width past 8192
                                   (12000, 26000, 2),     # not a multiple of 256: padded rows, a tail of k-steps
                                   (16384, 34000, 2),
                                   (32768, 33000, 1)])    # the limit: one centroid is 128 KiB of LDS
def test_wide_forest_bit_exact_vs_oracle(capi, f, N, T, tmp_path):
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(31337 + f)
    X = _rows(rng, N, f)
    X[17] = 0.0                       # a zero row: norm == 0 paths, margin == 0 coin flips
    X[18] = X[19]                     # a duplicate pair
    o = capi.AnnoyOracle(f, mode=1)
    o.set_items(X)
    o.build(T)
    a = AnnoyIndex(f)
    a.add_items(X)
    a.build(T)
    st = a.forest_stats()
    assert st["split_rows"] == o.split_rows() and st["split_attempts"] == o.split_nodes()
    assert _compare_forest(a, o) >= T           # N > K = f + 2: every tree has split
    items = np.array([0, 17, 18, 19, N // 2, N - 1], np.int32)
    Q = rng.standard_normal((3, f), dtype=np.float32)
    _compare_approx(a, o, items, Q)
    if f == 16384:
        # save -> load in a fresh handle: the same forest and the same answers
        fn = str(tmp_path / "wide.annoy.mor")
        a.save(fn)
        b = AnnoyIndex(f)
        b.load(fn)
        fa, fb = a.get_forest(), b.get_forest()
        for key in ("node_rec", "perm", "hyperplanes", "hp_node"):
            assert np.asarray(fa[key]).tobytes() == np.asarray(fb[key]).tobytes(), key
        want = a.get_nns_by_item_batch(items, 10, -1)
        got = b.get_nns_by_item_batch(items, 10, -1)
        assert got[0].tolist() == want[0].tolist() and got[1].tobytes() == want[1].tobytes()


def test_wide_forest_subnormal_centroid_elements(capi):
    """As test_forest_subnormal_centroid_elements, at a width that takes the wide form: the quotients of the centroid
    update land among the subnormals and must take the division route."""
    from morna_amd.annoy import AnnoyIndex
    f, N, T = 12000, 13000, 1
    rng = np.random.default_rng(424242 + f)
    X = _rows(rng, N, f)
    q = f // 4
    X[:, :q] *= (2.0 ** rng.integers(-146, -132, q)).astype(np.float32)     # subnormal inputs
    X[:, q:2 * q] *= (2.0 ** rng.integers(-126, -120, q)).astype(np.float32)  # quotients by |x| subnormal
    assert (np.abs(X[:, :q]) < 1.2e-38).all() and (X[:, :q] != 0).any()
    o = capi.AnnoyOracle(f, mode=1)
    o.set_items(X)
    o.build(T)
    a = AnnoyIndex(f)
    a.add_items(X)
    a.build(T)
    _compare_forest(a, o)
    hp = a.get_forest()["hyperplanes"]
    tiny = np.abs(hp[:, :2 * q])
    assert ((tiny > 0) & (tiny < 1.2e-38)).any()            # the case under test did occur


@pytest.mark.parametrize("f", [16384, 32768])
def test_wide_exact_search_vs_oracle(capi, f):
    """Ids and fp64 distances bit-exact: the vector-ALU scan (nb < 32), the matrix-core scan (nb >= 32), by item."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(77 + f)
    N, k = 2500, 10
    X = _rows(rng, N, f)
    X[N // 2] = X[3]
    X[N // 2 + 1] = 2.0 * X[3]
    a = AnnoyIndex(f)
    a.add_items(X)
    for nb in (4, 40):
        Q = rng.standard_normal((nb, f))
        Q[0] = X[3]
        ids, d, cnt = a.exact_search_batch(Q, k)
        for qi in list(range(3)) + [nb - 1]:
            rid, rd = capi.exact_search(X, Q[qi], k)
            assert int(cnt[qi]) == len(rid)
            assert ids[qi].astype(np.int64).tolist() == rid.tolist()
            assert d[qi].tobytes() == rd.tobytes()
    items = np.array([3, 5, N - 1], np.int32)
    ids, d, cnt = a.exact_search_by_item_batch(items, k)
    for qi, it in enumerate(items):
        rid, rd = capi.exact_search(X, X[it].astype(np.float64), k)
        assert ids[qi].astype(np.int64).tolist() == rid.tolist()
        assert d[qi].tobytes() == rd.tobytes()


_SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, {root!r})
from morna_amd.annoy import AnnoyIndex
N, D, T = {N}, {D}, {T}
rng = np.random.default_rng(2027)
C = rng.standard_normal((6, D), dtype=np.float32)
X = np.empty((N, D), np.float32)
for r0 in range(0, N, 2048):
    r1 = min(N, r0 + 2048)
    X[r0:r1] = C[rng.integers(0, 6, r1 - r0)] + np.float32(0.3) * rng.standard_normal((r1 - r0, D), dtype=np.float32)
X[5] = 0.0
a = AnnoyIndex(D)
a.add_items(X)
a.build(T)
f = a.get_forest()
h = hashlib.sha256()
for key in ("node_rec", "perm", "hyperplanes", "hp_node"):
    h.update(np.ascontiguousarray(f[key]).tobytes())
print("forest", h.hexdigest())
for nq in (8, 100):
    items = np.arange(nq, dtype=np.int32) * 37 % N
    ids, d, cnt = a.get_nns_by_item_batch(items, 10, -1)
    print("items", nq, hashlib.sha256(ids.tobytes() + d.tobytes() + cnt.tobytes()).hexdigest())
    ids, d, cnt = a.get_nns_by_vector_batch(X[items] + np.float32(0.01), 10, 2000)
    print("vectors", nq, hashlib.sha256(ids.tobytes() + d.tobytes() + cnt.tobytes()).hexdigest())
"""


def test_wide_switch_invariance():
    """The build and search switches change nothing at 16384 (each run in its own process: the switches are read once)."""
    script = _SCRIPT.format(root=ROOT, N=18000, D=16384, T=2)
    outs = {}
    # (MORNA_TM_STRIP=0 launches what the default process launches: past 8192 floats the wide form runs whatever the
    # switches.  It stays as the check of exactly that; test_gpu_width_forms.py compares the two_means forms.)
    for env in ({}, {"MORNA_SPLIT_MM": "0"}, {"MORNA_TM_STRIP": "0"}, {"MORNA_QUERY_FILTER": "0"},
                {"MORNA_QUERY_DENSE": "0"}, {"MORNA_QUERY_SPREAD": "0"}):
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", script], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (env, r.stderr[-2000:])
        outs[tuple(env.items())] = r.stdout
    base = outs[()]
    assert base.count("\n") == 5
    for key, out in outs.items():
        assert out == base, key


def test_wide_limit():
    """Past 32768 floats the build and the exact search refuse with a ValueError that names the limit; the handle
    stays usable."""
    from morna_amd.annoy import AnnoyIndex
    f = 32769
    rng = np.random.default_rng(5)
    X = rng.standard_normal((8, f), dtype=np.float32)
    a = AnnoyIndex(f)
    a.add_items(X)
    with pytest.raises(ValueError, match="32768"):
        a.build(2)
    with pytest.raises(ValueError, match="32768"):
        a.exact_search_batch(rng.standard_normal((2, f)), 3)
    assert a.get_n_items() == 8
    assert a.get_item_vector(3) == pytest.approx(X[3].tolist())
    # the same process goes on building and searching at the limit
    b = AnnoyIndex(32768)
    b.add_items(X[:, :32768])
    b.build(1)
    ids, d, cnt = b.exact_search_by_item_batch(np.array([2], np.int32), 3)
    assert int(ids[0, 0]) == 2


def test_wide_features_vs_oracle(capi):
    """The feature matrix at 16384 columns, bit-exact against the oracle's on a synthetic intropolis set."""
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.index import prepare_csr
    from morna_amd.synth import synthetic_intropolis
    f, n_samples, threshold = 16384, 3000, 20
    d = synthetic_intropolis(n_samples, J=20000)
    keys, rp, s, c = d["keys"], d["row_ptr"], d["samples"], d["cov"]
    buf, off = capi.pack_keys(keys)
    ref = capi.index_features(buf, off, rp, s, c, n_samples, threshold, f)
    prep = prepare_csr(keys, rp, s, c, n_samples, threshold)
    a = AnnoyIndex(f)
    a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
    a.build_features(prep["n_items"])
    assert prep["n_items"] == ref["n_items"] > 100
    assert prep["ext_ids"].tolist() == ref["ext_ids"].tolist()
    assert a.get_items().tobytes() == ref["X"].tobytes()


def test_wide_sharded_one_rank_equals_unsharded():
    """The sharded entry points at 16384 on a 1-rank communicator (RCCL inside the library): the approximate and exact
    answers, by vector and by item, equal the unsharded ones."""
    from morna_amd.annoy import AnnoyIndex
    f, N, T, K = 16384, 18000, 2, 10
    rng = np.random.default_rng(616)
    X = _rows(rng, N, f)
    a = AnnoyIndex(f)
    a.add_items(X)
    a.build(T)
    a.comm_init(AnnoyIndex.comm_unique_id(), 0, 1)
    try:
        items = rng.choice(N, 40, replace=False).astype(np.int32)
        Q = np.ascontiguousarray(X[items[:6]] + np.float32(0.01) * rng.standard_normal((6, f), dtype=np.float32))

        def same(got, want):
            assert got[0].tolist() == want[0].tolist() and got[1].tobytes() == want[1].tobytes() and got[2].tolist() == want[2].tolist()

        same(a.get_nns_by_item_sharded(items, K, -1), a.get_nns_by_item_batch(items, K, -1))
        same(a.get_nns_by_vector_sharded(Q, K, -1), a.get_nns_by_vector_batch(Q, K, -1))
        same(a.exact_search_sharded(Q.astype(np.float64), K), a.exact_search_batch(Q.astype(np.float64), K))
        same(a.exact_search_by_item_sharded(items, K, [len(items)]), a.exact_search_by_item_batch(items, K))
    finally:
        a.comm_destroy()


def test_wide_cli_index_and_search(tmp_path, capi):
    """`morna index --features 16384` on more samples than a leaf holds, then `morna search -q ID -d` (with and without
    -e, which a by-member query does not use, as in the reference) and an exact stream search: the printed neighbours
    are those of an AnnoyIndex built directly on the same rows, and the exact ones those of the oracle."""
    import gzip
    import io
    from morna_amd import cli
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.search import MornaSearch, results_output
    from morna_amd.synth import synthetic_intropolis
    f, n_samples = 16384, 18000
    d = synthetic_intropolis(n_samples, J=20000)
    src = str(tmp_path / "i.tsv.gz")
    with gzip.open(src, "wt") as fh:
        for j, k in enumerate(d["keys"]):
            lo, hi = d["row_ptr"][j], d["row_ptr"][j + 1]
            fh.write("\t".join(k.split(" ") + ["+", "GT", "AG", ",".join(map(str, d["samples"][lo:hi])),
                                                ",".join(map(str, d["cov"][lo:hi]))]) + "\n")
    base = str(tmp_path / "wide")
    assert cli.main(["index", "--intropolis", src, "-x", base, "--features", str(f), "--n-trees", "4",
                     "-s", str(n_samples), "-t", "1"]) == 0
    ms = MornaSearch(basename=base)
    X = ms.annoy_index.get_items()
    assert X.shape[0] > f + 2 and X.shape[1] == f      # more items than a leaf holds: the forest splits
    direct = AnnoyIndex(f)
    direct.add_items(X)
    direct.build(4)
    sample = int(d["samples"][d["row_ptr"][11] + 2])
    internal = ms.internal_id_map[sample]
    want = io.StringIO()
    results_output(direct.get_nns_by_item(internal, 10, 100, include_distances=True), want)
    for extra in ([], ["-e"]):
        out = io.StringIO()
        assert cli.main(["search", "-x", base, "-q", str(sample), "-d", "-r", "10"] + extra, stdout=out) == 0
        assert out.getvalue() == want.getvalue() and out.getvalue().split("\n")[0].split("\t")[1] == str(internal)
    # exact: a raw stream of the sample's junctions
    q = []
    for j, k in enumerate(d["keys"]):
        lo, hi = d["row_ptr"][j], d["row_ptr"][j + 1]
        hit = np.nonzero(d["samples"][lo:hi] == sample)[0]
        if len(hit):
            c, a_, b_ = k.split(" ")
            q.append("%s\t%s\t%s\t%d\n" % (c, a_, b_, d["cov"][lo + hit[0]]))
    out = io.StringIO()
    assert cli.main(["search", "-x", base, "-f", "raw", "--exact", "-d", "-r", "10"], stdin=io.StringIO("".join(q)),
                    stdout=out) == 0
    got = [ln.split("\t") for ln in out.getvalue().strip().split("\n")]
    for ln in q:
        t = ln.strip().split("\t")
        if " ".join(t[:3]) in ms.sample_frequencies:
            ms.update_query((t[0], int(t[1]), int(t[2]), int(t[3])))
    ms.finalize_query()
    qv = np.array(ms.query_sample, np.float64)
    rid, rd = capi.exact_search(X, qv, 10)
    assert [int(g[1]) for g in got] == rid.tolist()
    assert [float(g[2]) for g in got] == rd.tolist()
    ids, dd, cnt = direct.exact_search_batch(qv[None, :], 10)
    assert ids[0].astype(np.int64).tolist() == rid.tolist() and dd[0].tobytes() == rd.tobytes()
