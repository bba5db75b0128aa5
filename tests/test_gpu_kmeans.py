"""Spherical k-means on the GPU (include/morna_hip.h, "spherical k-means").  -m gpu

The yardstick is kmeans_ref.py, the numpy restatement of the contract (pinned by hand and against the oracle in
test_kmeans_cpu.py).  Everything is compared as bytes: assignments, fp64 distances, centroids, sizes.  The distances of a shape
to its pool of 130 centroids are computed once; a case with k centroids reads the first k columns (d(i, c_j) does not depend
on the other centroids).
"""
import numpy as np
import pytest

from kmeans_ref import assign_from_distances, ref_assign, ref_distances, ref_kmeans

pytestmark = pytest.mark.gpu

SHAPES = [(700, 64), (8200, 64), (300, 1100), (300, 8192)]
KS = [1, 3, 31, 32, 33, 65, 130]
ZERO_ROW, DOUBLE, SCALED, HUGE, NAN_ROW, INF_ROW = 1, 10, 11, 12, 13, 14
_cache = {}


def _index(X):
    from morna_amd.annoy import AnnoyIndex
    a = AnnoyIndex(X.shape[1])
    a.add_items(X)
    return a


def _rows(n, D, seed):
    """Normal rows with a zero row, a doubled and a 2^-20 copy of row 5, a row times 1e25 (its fp32 squared norm overflows: outside
    the scan's domain), a row with a NaN and a row with an inf."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)).astype(np.float32)
    X[ZERO_ROW] = 0.0
    X[DOUBLE] = X[5] * np.float32(2.0)
    X[SCALED] = X[5] * np.float32(2.0 ** -20)
    X[HUGE] *= np.float32(1e25)
    X[NAN_ROW, 3] = np.nan
    X[INF_ROW, 7] = np.inf
    return X, rng


def _pool(X, rng):
    """130 centroids: 0 a widened stored row, 1 its copy (the lower index wins), 2 three times it; 3 / 4 / 5 row 6 with one
    element one fp64 ulp up, one fp32 ulp up, and as it is; 6 the zero centroid; 7 / 8 scaled so that the sum of squares is below
    2^-900 / above 2^890; 9..39 widened stored rows; the rest normal vectors."""
    D = X.shape[1]
    P = rng.standard_normal((130, D))
    P[0] = X[5].astype(np.float64)
    P[1] = P[0]
    P[2] = P[0] * 3.0
    P[3] = P[4] = P[5] = X[6].astype(np.float64)
    P[3, 2] = np.nextafter(P[3, 2], np.inf)
    P[4, 2] = float(np.nextafter(X[6, 2], np.float32(np.inf)))
    P[6] = 0.0
    P[7] *= 2.0 ** -460
    P[8] *= 2.0 ** 450
    P[9:40] = X[20:51].astype(np.float64)
    assert (P[7] * P[7]).sum() < 2.0 ** -900 and (P[8] * P[8]).sum() > 2.0 ** 890
    return P


def _shape(n, D):
    if (n, D) not in _cache:
        X, rng = _rows(n, D, 1500 + n + D)
        P = _pool(X, rng)
        _cache[(n, D)] = dict(X=X, P=P, d=ref_distances(X, P), index=_index(X))
    return _cache[(n, D)]


def _same(got, want, label):
    (ga, gd), (wa, wd) = got, want
    assert ga.dtype == np.int32 and gd.dtype == np.float64
    bad = np.nonzero(ga != wa)[0]
    assert len(bad) == 0, (label, "assign", bad[:8].tolist(), ga[bad[:8]].tolist(), wa[bad[:8]].tolist())
    assert gd.tobytes() == np.ascontiguousarray(wd, dtype=np.float64).tobytes(), (label, "dist")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,D", SHAPES)
def test_assign_against_the_restatement(n, D, k):
    s = _shape(n, D)
    a, X, d = s["index"], s["X"], s["d"][:, :k]
    want = assign_from_distances(d)
    # the inputs: the planted rows do what they are there for
    assert want[1][ZERO_ROW] == np.sqrt(2.0) and want[0][ZERO_ROW] == 0
    assert want[0][5] == 0 and want[0][DOUBLE] == 0 and want[0][SCALED] == 0          # copy and triple lose to the lower index
    if k > 8:
        assert want[0][6] in (3, 4, 5) and want[0][INF_ROW] == 6 and np.isnan(d[INF_ROW, :6]).all()
    got = a.kmeans_assign(s["P"][:k])
    _same(got, want, "all rows")
    stats = a.kmeans_stats()
    assert stats["iterations"] == 1 and stats["chains"] >= n and stats["largest"] == 0 and stats["scan_ms"] > 0
    assert stats["open_rows"] >= (1 if k > 1 else 0)                                   # row 5 ties between centroids 0 and 1
    # allow-lists: half of the rows, five rows, all rows
    for label, allow in (("half", np.arange(n) % 2 == 0), ("five", np.isin(np.arange(n), [1, 5, HUGE, NAN_ROW, n - 1])),
                         ("all", np.ones(n, bool))):
        r = a.restriction(allow=allow)
        got = a.kmeans_assign(s["P"][:k], restriction=r)
        _same(got, assign_from_distances(d, allow), label)
        assert (got[0][~allow] == -1).all() and (got[1][~allow] == -1.0).all()
        assert a.kmeans_stats()["chains"] >= int(allow.sum())


def _ladder(k_ladder):
    """700 x 64: rows 100..149 are one direction v at several scales; k_ladder centroids at the angles 0.5 + m 1e-7 from v, in a
    shuffled order: their true distances to those rows differ by 1e-7 a step, far below what the fp32 scan resolves."""
    rng = np.random.default_rng(77)
    X = rng.standard_normal((700, 64)).astype(np.float32)
    v = rng.standard_normal(64).astype(np.float32)
    X[100:150] = v[None, :] * (np.float32(2.0) ** rng.integers(-6, 7, 50)).astype(np.float32)[:, None]
    v64 = v.astype(np.float64)
    u = rng.standard_normal(64)
    u -= v64 * (u @ v64) / (v64 @ v64)
    vh, uh = v64 / np.sqrt(v64 @ v64), u / np.sqrt(u @ u)
    order = rng.permutation(k_ladder)
    Cn = np.array([np.cos(0.5 + m * 1e-7) * vh + np.sin(0.5 + m * 1e-7) * uh for m in order])
    return X, Cn, int(np.argmin(order))


@pytest.mark.parametrize("k_ladder", [40, 20], ids=["mfma-scan", "vector-scan"])
def test_ladder_inside_the_window_is_resolved_in_fp64(k_ladder):
    X, Cn, nearest = _ladder(k_ladder)
    want = ref_assign(X, Cn)
    assert (want[0][100:150] == nearest).all()
    d = ref_distances(X[100:101], Cn)[0]
    assert len(set(d.tolist())) == k_ladder and np.ptp(d) ** 2 < 1e-5                  # all distinct in fp64, all inside the window
    a = _index(X)
    _same(a.kmeans_assign(Cn), want, "ladder")
    stats = a.kmeans_stats()
    assert stats["open_rows"] >= 50 and stats["chains"] >= 700 + 50 * (k_ladder - 1) and stats["resolve_ms"] > 0


@pytest.mark.parametrize("k", [5, 35], ids=["vector-scan", "mfma-scan"])
def test_well_separated_rows_are_decided_by_the_scan(k):
    rng = np.random.default_rng(78)
    n = 700
    X = (0.05 * rng.standard_normal((n, 64))).astype(np.float32)
    X[np.arange(n), np.arange(n) % k] += np.float32(1.0)
    Cn = np.eye(64)[:k] * 1.5
    want = ref_assign(X, Cn)
    assert want[0].tolist() == (np.arange(n) % k).tolist()
    a = _index(X)
    for _ in range(2):                                                                 # the call repeated: the same bytes
        _same(a.kmeans_assign(Cn), want, "separated")
        stats = a.kmeans_stats()
        assert stats["open_rows"] == 0 and stats["chains"] == n


def test_refused_centroids_and_the_exact_search_afterwards():
    s = _shape(700, 64)
    a, P = s["index"], s["P"]
    Q = P[40:44]
    before = a.exact_search_batch(Q, 5)
    for bad in (np.nan, np.inf, 1e200):                                                # 1e200: the sum of squares overflows
        Cn = P[:9].copy()
        Cn[4, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            a.kmeans_assign(Cn)
        assert a.kmeans_stats()["chains"] == 0
    with pytest.raises(IndexError):
        a.kmeans_assign(P[:3, :10])
    _same(a.kmeans_assign(P[:9]), assign_from_distances(s["d"][:, :9]), "after a refusal")
    after = a.exact_search_batch(Q, 5)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()


# ---- the loop ---------------------------------------------------------------------------------------------------------------

def _same_run(got, want, label):
    _same((got["assign"], got["dist"]), (want["assign"], want["dist"]), label)
    assert got["centroids"].tobytes() == want["centroids"].tobytes(), (label, "centroids")
    assert got["sizes"].tolist() == want["sizes"].tolist(), (label, "sizes")
    assert (got["iterations"], got["converged"]) == (want["iterations"], want["converged"]), label


def _blobs():
    if "blobs" not in _cache:
        rng = np.random.default_rng(79)
        g = rng.standard_normal((5, 64))
        X = (g[np.arange(700) % 5] + 0.3 * rng.standard_normal((700, 64))).astype(np.float32)
        X[40] = 0.0
        X[45] = X[35]                                                                  # two identical rows of blob 0
        _cache["blobs"] = (X, _index(X))
    return _cache["blobs"]


def test_planted_blobs():
    X, a = _blobs()
    one = ref_kmeans(X, [0, 1, 2, 3, 4], 100)
    assert one["converged"] and (one["assign"][np.arange(700) != 40] == (np.arange(700) % 5)[np.arange(700) != 40]).all()
    got = a.kmeans([0, 1, 2, 3, 4], 100)
    _same_run(got, one, "one seed per blob")
    stats = a.kmeans_stats()
    assert stats["iterations"] == one["iterations"] and stats["largest"] == one["sizes"].max() and stats["update_ms"] > 0
    # all seeds in one blob: more iterations, and a cluster that ends empty and keeps its centroid
    crowded = ref_kmeans(X, [0, 5, 10, 15, 20], 100)
    assert crowded["converged"] and crowded["iterations"] > one["iterations"] and (crowded["sizes"] == 0).any()
    _same_run(a.kmeans([0, 5, 10, 15, 20], 100), crowded, "all seeds in one blob")
    # two identical rows as seeds: the first assignment gives the higher index nothing, and it keeps its centroid
    twin = ref_kmeans(X, [35, 45, 1], 1)
    assert twin["sizes"][1] == 0 and twin["sizes"][0] > 1
    _same_run(a.kmeans([35, 45, 1], 1), twin, "identical seeds, one assignment")
    twin = ref_kmeans(X, [35, 45, 1], 100)
    assert twin["converged"]
    _same_run(a.kmeans([35, 45, 1], 100), twin, "identical seeds")
    # a cluster of the zero row alone: it ties at sqrt(2) with every centroid and goes to cluster 0, whose seed it is; no row of
    # a blob is as far as sqrt(2) from its own blob's centroid
    zero = ref_kmeans(X, [40, 0, 1, 2, 3, 4], 100)
    assert zero["sizes"][0] == 1 and zero["assign"][40] == 0 and not zero["centroids"][0].any()
    _same_run(a.kmeans([40, 0, 1, 2, 3, 4], 100), zero, "zero row alone")
    for max_iter in (1, 2):                                                            # the centroids the assignment was made against
        want = ref_kmeans(X, [0, 5, 10, 15, 20], max_iter)
        assert not want["converged"] and want["iterations"] == max_iter
        _same_run(a.kmeans([0, 5, 10, 15, 20], max_iter), want, "max_iter %d" % max_iter)
    _same_run(a.kmeans([7], 100), ref_kmeans(X, [7], 100), "k = 1")


def test_k_equal_to_the_number_of_rows():
    X, _ = _blobs()
    X = X[:200]
    seeds = np.random.default_rng(3).permutation(200).tolist()
    want = ref_kmeans(X, seeds, 100)
    assert want["sizes"].max() >= 2 and (want["sizes"] == 0).sum() >= 1              # the zero row and the twin leave clusters empty
    _same_run(_index(X).kmeans(seeds, 100), want, "k = n")


def test_random_rows_on_the_mfma_scan():
    """8200 x 64 normal rows, k = 33: the MFMA scan every iteration; on such rows a sum taken in another order shows in the
    centroids' bytes."""
    rng = np.random.default_rng(80)
    X = rng.standard_normal((8200, 64)).astype(np.float32)
    seeds = rng.choice(8200, 33, replace=False).tolist()
    want = ref_kmeans(X, seeds, 6)
    assert want["iterations"] == 6 and want["sizes"].min() > 50
    a = _index(X)
    _same_run(a.kmeans(seeds, 6), want, "random rows")
    assert a.kmeans_stats()["iterations"] == 6
    # in another order the same sums give other bytes: the comparison above sees the order
    members = np.nonzero(want["assign"] == 0)[0]
    from kmeans_ref import ref_scales
    _, s = ref_scales(X)
    fwd = np.zeros(64)
    for i in members:
        fwd = fwd + X[i].astype(np.float64) * s[i]
    back = np.zeros(64)
    for i in members[::-1]:
        back = back + X[i].astype(np.float64) * s[i]
    assert fwd.tobytes() != back.tobytes()


def test_allow_list_equals_an_index_of_the_allowed_rows():
    X, a = _blobs()
    allow = np.ones(700, bool)
    allow[::3] = False
    allow[[40, 45]] = True
    kept = np.nonzero(allow)[0]
    seeds = [int(kept[i]) for i in (3, 50, 111, 260, 301, 422)]
    got = a.kmeans(seeds, 100, restriction=a.restriction(allow=allow))
    assert (got["assign"][~allow] == -1).all() and (got["dist"][~allow] == -1.0).all()
    _same_run(got, ref_kmeans(X, seeds, 100, allow), "allow-list")
    sub = _index(X[kept]).kmeans([int(np.searchsorted(kept, s)) for s in seeds], 100)
    assert got["assign"][kept].tolist() == sub["assign"].tolist()
    assert got["dist"][kept].tobytes() == sub["dist"].tobytes() and got["centroids"].tobytes() == sub["centroids"].tobytes()
    assert got["sizes"].tolist() == sub["sizes"].tolist() and got["iterations"] == sub["iterations"]


def test_refusals_through_the_raw_call():
    import ctypes as C
    from morna_amd import _lib
    from morna_amd.annoy import AnnoyIndex
    X, a = _blobs()
    L = _lib.lib()
    n = 700
    assign, info = np.empty(n, np.int32), np.zeros(2, np.int32)

    def raw(h, r, seeds, k, max_iter=10):
        seeds = np.ascontiguousarray(seeds, np.int32)
        rc = L.morna_kmeans(h, r, _lib.ptr(seeds), k, max_iter, _lib.ptr(assign), None, None, None, _lib.ptr(info))
        return rc, L.morna_last_error().decode()
    assert raw(a._h, None, [0, 1], 2)[0] == _lib.OK and info[0] >= 1
    for k in (0, -1, 4097, 701):
        rc, msg = raw(a._h, None, np.arange(max(k, 1)) % n, k)
        assert rc == _lib.E_INVALID and "4096" in msg, (k, msg)
    rc, msg = raw(a._h, None, [0, 1], 2, max_iter=0)
    assert rc == _lib.E_INVALID and "max_iter" in msg
    rc, msg = raw(a._h, None, [3, 9, 3], 3)
    assert rc == _lib.E_INVALID and "twice" in msg
    assert raw(a._h, None, [3, n], 2)[0] == _lib.E_RANGE and raw(a._h, None, [-1, 3], 2)[0] == _lib.E_RANGE
    allow = np.ones(n, bool)
    allow[9] = False
    r = a.restriction(allow=allow)
    rc, msg = raw(a._h, r._p, [3, 9], 2)
    assert rc == _lib.E_INVALID and "not eligible" in msg
    few = a.restriction(allow=np.arange(n) < 4)
    rc, msg = raw(a._h, few._p, [0, 1, 2, 3, 0], 5)
    assert rc == _lib.E_INVALID and "4 eligible" in msg
    grouped = a.restriction(groups=np.zeros(n, np.int32))
    rc, msg = raw(a._h, grouped._p, [0, 1], 2)
    assert rc == _lib.E_INVALID and "groups" in msg
    assert L.morna_kmeans(a._h, None, None, 2, 10, _lib.ptr(assign), None, None, None, _lib.ptr(info)) == _lib.E_INVALID
    stats = np.ones(8)
    assert L.morna_kmeans_stats(a._h, _lib.ptr(stats)) == _lib.OK and not stats.any()
    with pytest.raises(ValueError, match="groups"):
        a.kmeans_assign(X[:2].astype(np.float64), restriction=grouped)
    # k * n_items past 2^29: stated by the index's size, nothing of that size is allocated
    big = AnnoyIndex(4)
    big.add_items(np.ones((140000, 4), np.float32))
    assign_big = np.empty(140000, np.int32)
    seeds = np.arange(4096, dtype=np.int32)
    rc = L.morna_kmeans(big._h, None, _lib.ptr(seeds), 4096, 10, _lib.ptr(assign_big), None, None, None, _lib.ptr(info))
    assert rc == _lib.E_INVALID and "2^29" in L.morna_last_error().decode()
    empty = AnnoyIndex(8)
    rc = L.morna_kmeans(empty._h, None, _lib.ptr(seeds), 1, 10, _lib.ptr(assign), None, None, None, _lib.ptr(info))
    assert rc == _lib.E_EMPTY
    assert C.sizeof(C.c_int32) == 4


# ---- the loop at the sizes its kernels branch on ---------------------------------------------------------------------------
# kmeans_update_kernel takes a (cluster, 256 columns) per workgroup, kmeans_starts_kernel `ceil(k / 256)` clusters per thread,
# kmeans_hist / scatter / pick walk k in rounds of 256 threads, and radius_offsets_kernel scans 64 workgroup counts a pass.
# Every shape below states, on the reference, the condition that makes it reach the branch it is here for.

def _wide_blobs(D):
    """300 rows of D floats in 5 blobs with unit noise (seed 100 + D); row 40 is zero, row 45 a copy of row 35."""
    rng = np.random.default_rng(100 + D)
    g = rng.standard_normal((5, D))
    X = (g[np.arange(300) % 5] + 1.0 * rng.standard_normal((300, D))).astype(np.float32)
    X[40] = 0.0
    X[45] = X[35]
    return X


@pytest.mark.parametrize("D", [3, 37, 301, 1101, 4100, 8200])
def test_loop_on_wide_and_ragged_rows(D):
    """All five seeds in one blob, so the centroids travel for several iterations: the update's column blocks 0 .. 32 with
    dead threads in the last one, the norms of a width that is no multiple of 4, and the scan's images of fp64 centroids
    that are sums, at every row-width form of the scan."""
    X = _wide_blobs(D)
    want = ref_kmeans(X, [0, 5, 10, 15, 20], 100)
    assert want["converged"] and want["iterations"] >= 3, want["iterations"]
    assert want["sizes"].min() > 8, want["sizes"].tolist()                              # past KM_AHEAD: a second round of member rows
    a = _index(X)
    _same_run(a.kmeans([0, 5, 10, 15, 20], 100), want, "wide blobs D=%d" % D)
    stats = a.kmeans_stats()
    assert stats["iterations"] == want["iterations"] and stats["largest"] == want["sizes"].max()
    assert stats["chains"] >= 300 * want["iterations"]


def _many_clusters(n, D, k):
    """(rows, seeds) of the k > 256 shapes.  k = 4096: rows 4300 .. 4449 are scaled copies of row 0 with 1e-3 of noise, and the
    seeds are the rows 0 .. 4095."""
    rng = np.random.default_rng(n + D + k)
    X = rng.standard_normal((n, D)).astype(np.float32)
    if k == 4096:
        scale = np.linspace(0.5, 2.0, 150, dtype=np.float32)
        X[4300:4450] = X[0][None, :] * scale[:, None] + np.float32(1e-3) * rng.standard_normal((150, D)).astype(np.float32)
        return X, np.arange(4096)
    return X, rng.choice(n, size=k, replace=False)


@pytest.mark.parametrize("n,D,k,max_iter", [(2100, 3, 300, 4), (9000, 8, 1000, 3), (4500, 4, 4096, 3)])
def test_loop_with_more_than_256_clusters(n, D, k, max_iter):
    """kmeans_starts_kernel with 2, 4 and 16 clusters per thread, and the second and later rounds of 256 clusters in the
    histogram, the scatter and the pick; 9000 rows are nine member-list chunks, the last one ragged."""
    X, seeds = _many_clusters(n, D, k)
    want = ref_kmeans(X, seeds, max_iter)
    assert want["iterations"] >= 2 and want["sizes"].max() > 8, (want["iterations"], int(want["sizes"].max()))
    assert (want["sizes"][256:] > 0).any()
    if k == 4096:
        assert (want["sizes"] == 0).any() and want["sizes"][0] > 100, int(want["sizes"][0])
    a = _index(X)
    _same_run(a.kmeans(seeds, max_iter), want, "n=%d D=%d k=%d" % (n, D, k))
    stats = a.kmeans_stats()
    assert stats["iterations"] == want["iterations"] and stats["largest"] == want["sizes"].max()


@pytest.mark.parametrize("k", [257, 1000, 4096])
def test_assign_with_more_than_256_centroids(k):
    """1100 x 8: one assignment against k centroids (the first 40 are widened stored rows, two of them equal), with and
    without an allow-list of every other row."""
    if "many" not in _cache:
        rng = np.random.default_rng(1100 + 8)
        X = rng.standard_normal((1100, 8)).astype(np.float32)
        X[ZERO_ROW] = 0.0
        P = rng.standard_normal((4096, 8))
        P[:40] = X[100:140].astype(np.float64)
        P[300] = P[7]                                                                   # the lower index wins
        _cache["many"] = dict(X=X, P=P, d=ref_distances(X, P), index=_index(X))
    s = _cache["many"]
    a, d = s["index"], s["d"][:, :k]
    want = assign_from_distances(d)
    assert (want[0] >= 256).any() and want[0][107] == 7
    _same(a.kmeans_assign(s["P"][:k]), want, "k=%d" % k)
    assert a.kmeans_stats()["chains"] >= 1100
    allow = np.arange(1100) % 2 == 0
    got = a.kmeans_assign(s["P"][:k], restriction=a.restriction(allow=allow))
    _same(got, assign_from_distances(d, allow), "k=%d, every other row" % k)
    assert (got[0][~allow] == -1).all() and a.kmeans_stats()["chains"] >= 550


@pytest.mark.parametrize("k,max_iter", [(3, 4), (70, 3)], ids=["vector-scan", "mfma-scan"])
def test_loop_over_more_than_64_row_blocks(k, max_iter):
    """16700 x 8: 66 workgroups of 256 rows, so the prefix of their entry counts (radius_offsets_kernel) carries its running
    sum into a second pass of two entries; 17 member-list chunks, the last ragged.  Plain, and two rows in three allowed."""
    n = 16700
    if "blocks" not in _cache:
        X = np.random.default_rng(16700 + 8).standard_normal((n, 8)).astype(np.float32)
        _cache["blocks"] = (X, _index(X))
    X, a = _cache["blocks"]
    assert (n + 255) // 256 > 64
    allow = np.arange(n) % 3 != 2
    seeds = (np.random.default_rng(k).choice(n // 3, size=k, replace=False) * 3).tolist()   # rows the allow-list keeps
    for label, al in (("plain", None), ("two in three", allow)):
        want = ref_kmeans(X, seeds, max_iter, al)
        assert want["iterations"] == max_iter and want["sizes"].min() > 0
        n_elig = n if al is None else int(al.sum())
        assert (want["assign"][64 * 256:] >= 0).sum() > 0                               # eligible rows in blocks 64 and 65
        got = a.kmeans(seeds, max_iter, restriction=None if al is None else a.restriction(allow=al))
        _same_run(got, want, "16700 rows, k=%d, %s" % (k, label))
        stats = a.kmeans_stats()
        assert stats["chains"] >= n_elig * max_iter and stats["largest"] == want["sizes"].max()
