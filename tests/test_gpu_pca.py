"""Principal axes on the GPU (include/morna_hip.h, "principal axes").  -m gpu

The yardstick is pca_ref.py, the numpy restatement of the contract (pinned by hand and against numpy.linalg.eigh in
test_pca_cpu.py).  Axes, mean, values, the four figures of info and every coordinate are compared as bytes.  A shape's rows
are made once; most shapes run max_iter 1, 2 and 5 -- the bytes agree after any number of iterations -- and two run until
they converge.
"""
import numpy as np
import pytest

from pca_ref import PcaRefused, ref_pca, ref_project
from test_gpu_restrict import _stage_rows

pytestmark = pytest.mark.gpu

ZERO_ROW, TINY, HUGE, NAN_ROW, INF_ROW, TWIN = 1, 11, 12, 13, 14, 15
_cache = {}


def _index(X):
    from morna_amd.annoy import AnnoyIndex
    a = AnnoyIndex(X.shape[1])
    a.add_items(X)
    return a


def _rows(n, D, special=True):
    """n rows of D floats in 4 planted groups with unit noise; with `special` (n >= 20) a zero row, a row times 2^-60 and one
    times 2^60, a row with a NaN, a row with an inf, and a copy of row 5."""
    key = (n, D, special)
    if key not in _cache:
        rng = np.random.default_rng(1800 + 7 * n + D)
        g = 2.0 * rng.standard_normal((4, D))
        X = (g[np.arange(n) % 4] + rng.standard_normal((n, D))).astype(np.float32)
        if special:
            X[ZERO_ROW] = 0.0
            X[TINY] *= np.float32(2.0 ** -60)
            X[HUGE] *= np.float32(2.0 ** 60)
            X[NAN_ROW, 0] = np.nan
            X[INF_ROW, D - 1] = np.inf
            X[TWIN] = X[5]
        _cache[key] = (X, _index(X))
    return _cache[key]


def _same(got, want, label):
    for key in ("mean", "axes", "values"):
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape, (label, key)
        assert got[key].tobytes() == want[key].tobytes(), (label, key, np.abs(got[key] - want[key]).max())
    for key in ("iterations", "converged", "fitted"):
        assert got[key] == want[key], (label, key, got[key], want[key])
    assert np.float64(got["total_variance"]).tobytes() == np.float64(want["total_variance"]).tobytes(), (label, "total variance")


def _same_coords(got, want, label):
    assert got.dtype == np.float64 and got.shape == want.shape, label
    assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (label, np.nanmax(np.abs(got - want)))


def _fit_and_place(X, a, label, iters=(1, 2, 5), **kw):
    """The fit at every iteration count against the restatement; at the last one every stored row placed by item."""
    for max_iter in iters:
        want = ref_pca(X, max_iter=max_iter, **kw)
        got = a.pca(max_iterations=max_iter, **kw)
        _same(got, want, "%s max_iter %d" % (label, max_iter))
        stats = a.pca_stats()
        assert stats["iterations"] == want["iterations"] and stats["fitted"] == want["fitted"]
    coords = a.pca_project(got["axes"], got["mean"], items=np.arange(len(X), dtype=np.int32))
    _same_coords(coords, ref_project(want["axes"], want["mean"], X.astype(np.float64)), label + " coordinates")
    return got, coords


@pytest.mark.parametrize("center", [True, False], ids=["centred", "uncentred"])
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_row_block_edges(n, center):
    X, a = _rows(n, 64)
    got, coords = _fit_and_place(X, a, "n=%d" % n, p=3, extra=4, center=center, seed=n)
    assert got["fitted"] == n - 3 and np.isnan(coords[[ZERO_ROW, NAN_ROW, INF_ROW]]).all()
    assert np.isfinite(np.delete(coords, [ZERO_ROW, NAN_ROW, INF_ROW], axis=0)).all()
    assert coords[TWIN].tobytes() == coords[5].tobytes()
    if not center:
        assert not got["mean"].any()


@pytest.mark.parametrize("D", [1, 63, 64, 65, 255, 256, 257, 1100, 3000, 8960])
def test_column_block_edges(D):
    X, a = _rows(300, D)
    p, extra = (1, 0) if D == 1 else (2, 8)
    got, coords = _fit_and_place(X, a, "D=%d" % D, iters=(1, 2, 5) if D <= 257 else (1, 2), p=p, extra=extra, seed=3)
    assert got["fitted"] == 297 and np.isnan(coords[[ZERO_ROW, NAN_ROW, INF_ROW]]).all()
    # the scale of a row does not show: the rows times 2^-60 and 2^60 lie among the others
    assert np.abs(coords[[TINY, HUGE]]).max() <= np.nanmax(np.abs(coords))
    if D in (64, 1100):
        _fit_and_place(X, a, "D=%d uncentred" % D, iters=(2,), p=p, extra=extra, center=False, seed=3)


@pytest.mark.parametrize("p,extra", [(1, 0), (1, 8), (2, 0), (2, 8), (10, 0), (10, 8), (32, 0), (32, 8), (32, 32)])
def test_block_widths(p, extra):
    X, a = _rows(300, 100)
    _fit_and_place(X, a, "p=%d extra=%d" % (p, extra), iters=(1, 3), p=p, extra=extra, seed=p)


def test_block_of_all_but_one_row():
    X, a = _rows(20, 64, special=False)
    _fit_and_place(X, a, "b = m - 1", iters=(1, 2, 5), p=10, extra=9, seed=1)
    with pytest.raises(PcaRefused):
        ref_pca(X, 10, extra=10, max_iter=1)
    with pytest.raises(ValueError, match=r"min\(dim, rows fitted - 1\) = 19"):
        a.pca(10, extra=10, max_iterations=1)


@pytest.mark.parametrize("n,D,p", [(300, 64, 2), (513, 257, 10)])
def test_runs_until_converged(n, D, p):
    X, a = _rows(n, D)
    want = ref_pca(X, p, tol=1e-9, max_iter=500)
    assert want["converged"] and 2 <= want["iterations"] < 500
    got = a.pca(p, tol=1e-9, max_iterations=500)
    _same(got, want, "converged n=%d D=%d" % (n, D))
    # the variances of the axes are those of the coordinates of the fitted rows
    coords = a.pca_project(got["axes"], got["mean"], items=np.arange(n, dtype=np.int32))
    fitted = ~np.isnan(coords[:, 0])
    assert fitted.sum() == got["fitted"]
    assert np.allclose((coords[fitted] ** 2).mean(axis=0), got["values"], rtol=1e-6)
    assert got["values"].sum() <= got["total_variance"] * (1 + 1e-12) and (np.diff(got["values"]) <= 0).all()


def test_allow_list():
    """Half the rows are fitted and all are placed.  BS cuts its row blocks by item id, so an index of the allowed rows alone
    gives the same bytes when no block edge moves: with 250 rows both indexes hold one block.  With 700 rows the yardstick
    is the restatement under the same allow-list."""
    X, a = _rows(250, 64)
    allow = np.arange(250) % 2 == 1
    allow[[TINY, HUGE, INF_ROW]] = True
    got = a.pca(3, extra=4, seed=9, max_iterations=4, restriction=a.restriction(allow=allow))
    _same(got, ref_pca(X, 3, extra=4, seed=9, max_iter=4, allow=allow), "allow-list, 250 rows")
    kept = np.nonzero(allow)[0]
    sub = _index(X[kept]).pca(3, extra=4, seed=9, max_iterations=4)
    _same(got, sub, "an index of the allowed rows alone")
    coords = a.pca_project(got["axes"], got["mean"], items=np.arange(250, dtype=np.int32))
    _same_coords(coords, ref_project(got["axes"], got["mean"], X.astype(np.float64)), "all rows placed")
    assert np.isfinite(coords[~allow & (np.arange(250) != NAN_ROW)]).all()
    X, a = _rows(700, 64)
    allow = np.arange(700) % 2 == 0
    for max_iter in (1, 3):
        got = a.pca(2, extra=3, seed=2, max_iterations=max_iter, restriction=a.restriction(allow=allow))
        _same(got, ref_pca(X, 2, extra=3, seed=2, max_iter=max_iter, allow=allow), "allow-list, 700 rows")
        assert got["fitted"] == 349 and a.pca_stats()["fitted"] == 349                # (of the three skipped rows the inf row is even)


def test_determinism_and_query_sources():
    X, a = _rows(513, 257)
    one = a.pca(4, seed=5, max_iterations=3)
    two = a.pca(4, seed=5, max_iterations=3)
    _same(one, two, "the call repeated")
    other = a.pca(4, seed=6, max_iterations=3)
    assert other["axes"].tobytes() != one["axes"].tobytes()                           # (the seed is read)
    axes, mean = one["axes"], one["mean"]
    items = np.arange(65, dtype=np.int32) * 7
    batch = a.pca_project(axes, mean, items=items)
    for q in (0, 1, 64):
        alone = a.pca_project(axes, mean, items=items[q:q + 1])
        assert alone.tobytes() == batch[q:q + 1].tobytes(), q
    assert np.isnan(batch[2]).all() and items[2] == INF_ROW                            # (a host vector with an inf is refused: left out)
    finite = items != INF_ROW
    by_vector = a.pca_project(axes, mean, Q=X[items[finite]].astype(np.float64))
    assert by_vector.tobytes() == batch[finite].tobytes()
    # free vectors, a zero one among them; the staged rows against the same rows as vectors
    rng = np.random.default_rng(4)
    Q = rng.standard_normal((9, 257))
    Q[4] = 0.0
    got = a.pca_project(axes, mean, Q=Q)
    _same_coords(got, ref_project(axes, mean, Q), "vectors")
    assert np.isnan(got[4]).all() and np.isfinite(np.delete(got, 4, axis=0)).all()
    r64, _ = _stage_rows(a, 7, 11)
    staged = a.pca_project(axes, mean)
    _same_coords(staged, ref_project(axes, mean, r64), "staged rows")
    assert a.pca_project(axes, mean, Q=r64).tobytes() == staged.tobytes()


def test_stats_follow_their_definitions():
    X, a = _rows(513, 257)
    got = a.pca(4, seed=5, max_iterations=3)
    stats = a.pca_stats()
    assert stats["iterations"] == 3 and stats["fitted"] == got["fitted"] == 510
    assert stats["row_bytes"] == 4 * 257 * (513 + 510 * (2 + 2 * 3))
    for key in ("t_ms", "y_ms", "orth_ms", "small_ms"):
        assert 0.0 < stats[key] < 10000.0, (key, stats[key])
    assert 0.0 <= stats["eig_ms"] < 10000.0
    a.pca_project(got["axes"], got["mean"], items=np.arange(3, dtype=np.int32))
    assert a.pca_stats() == stats                                                      # (a projection leaves them)
    with pytest.raises(ValueError):
        a.pca(0)
    assert not any(a.pca_stats().values())


def test_refusals_through_the_raw_call():
    from morna_amd import _lib
    from morna_amd.annoy import AnnoyIndex
    L, ptr = _lib.lib(), _lib.ptr
    X, a = _rows(300, 64)
    n, D = X.shape
    axes, mean, values, info = np.zeros((64, D)), np.zeros(D), np.zeros(64), np.zeros(4)

    def fit(h=a, r=None, p=2, extra=8, center=1, seed=0, tol=1e-9, max_iter=2, out=axes):
        rc = L.morna_pca(h._h, r, p, extra, center, seed, tol, max_iter, ptr(out) if out is not None else None, ptr(mean), ptr(values),
                         ptr(info))
        return rc, L.morna_last_error().decode()
    assert fit()[0] == _lib.OK and info[0] == 2 and info[2] == 297
    for p, extra, word in ((0, 8, "0 components"), (33, 0, "33 components"), (-1, 0, "components"), (32, 33, "at most 64"),
                           (2, -1, "at most 64"), (2, 63, "at most 64")):
        rc, msg = fit(p=p, extra=extra)
        assert rc == _lib.E_INVALID and word in msg, (p, extra, msg)
    rc, msg = fit(p=32, extra=32)
    assert rc == _lib.OK, msg                                                          # b = 64 = dim
    narrow = _index(X[:, :40].copy())
    rc, msg = fit(h=narrow, p=32, extra=9)
    assert rc == _lib.E_INVALID and "min(dim, rows fitted - 1) = 40" in msg, msg
    for tol in (-1e-9, float("inf"), float("nan")):
        rc, msg = fit(tol=tol)
        assert rc == _lib.E_INVALID and "tol" in msg
    rc, msg = fit(max_iter=0)
    assert rc == _lib.E_INVALID and "max_iter = 0" in msg
    rc, msg = fit(out=None)
    assert rc == _lib.E_INVALID and "null buffer" in msg
    stats = np.ones(8)
    assert L.morna_pca_stats(a._h, ptr(stats)) == _lib.OK and not stats.any()
    # a restriction that holds groups; one that leaves fewer than 2 rows; all rows identical
    grouped = a.restriction(groups=np.zeros(n, np.int32))
    rc, msg = fit(r=grouped._p)
    assert rc == _lib.E_INVALID and "holds groups" in msg
    with pytest.raises(ValueError, match="groups"):
        a.pca(2, restriction=grouped)
    for allow, rows in ((np.arange(n) == 5, 1), (np.isin(np.arange(n), [ZERO_ROW, NAN_ROW, INF_ROW]), 0)):
        few = a.restriction(allow=allow)                                              # (held: the handle lives as long as the object)
        rc, msg = fit(r=few._p, p=1, extra=0)
        assert rc == _lib.E_INVALID and "%d rows to fit" % rows in msg, msg
    twins = np.zeros((40, D), np.float32)
    twins[:, 3] = 2.0                                                                  # (unit rows e_3: their mean is exact, Z is zero)
    same = _index(twins)
    rc, msg = fit(h=same, p=2, extra=2)
    assert rc == _lib.E_INVALID and "column 0 of Z W" in msg and "fewer than b = 4 independent" in msg, msg
    with pytest.raises(PcaRefused, match="column 0"):
        ref_pca(twins, 2, extra=2, max_iter=2)
    rc, msg = fit(h=same, p=2, extra=2, max_iter=1)                                    # (one iteration orthonormalises the start alone)
    assert rc == _lib.OK and values[0] == 0.0, (msg, values[0])
    empty = AnnoyIndex(D)
    assert fit(h=empty)[0] == _lib.E_EMPTY
    # the projection
    coords = np.zeros((5, 2))
    items = np.arange(5, dtype=np.int32)
    good = a.pca(2, max_iterations=2)

    def place(h=a, ax=good["axes"], mu=good["mean"], p=2, q=None, it=items, nq=5):
        rc = L.morna_pca_project(h._h, ptr(ax), ptr(mu), p, ptr(q), ptr(it), nq, ptr(coords))
        return rc, L.morna_last_error().decode()
    assert place()[0] == _lib.OK
    for bad in (np.nan, np.inf, -np.inf):
        ax = good["axes"].copy()
        ax[1, 7] = bad
        rc, msg = place(ax=ax)
        assert rc == _lib.E_INVALID and "axis 1" in msg, msg
        mu = good["mean"].copy()
        mu[3] = bad
        rc, msg = place(mu=mu)
        assert rc == _lib.E_INVALID and "mean" in msg, msg
    for p in (0, 33):
        assert place(p=p, ax=np.zeros((33, D)))[0] == _lib.E_INVALID
    assert place(it=np.array([0, n, 1, 2, 3], np.int32))[0] == _lib.E_RANGE
    Q = X[:5].astype(np.float64)
    rc, msg = place(q=Q)
    assert rc == _lib.E_INVALID and "not both" in msg
    Q[2, 1] = np.inf
    rc, msg = place(q=Q, it=None)
    assert rc == _lib.E_INVALID and msg.startswith("pca_project: query 2 "), msg
    rc, msg = place(h=_index(X), it=None)
    assert rc == _lib.E_INVALID and "no query source" in msg
    assert place(h=empty)[0] == _lib.E_EMPTY
    # a row-sharded handle: one that owns a communicator, here of one rank; giving it back lifts the refusal
    sharded = _index(X)
    sharded.comm_init(AnnoyIndex.comm_unique_id(), 0, 1)
    try:
        rc, msg = fit(h=sharded)
        assert rc == _lib.E_INVALID and "pca is not available on a row-sharded handle" in msg
        rc, msg = place(h=sharded)
        assert rc == _lib.E_INVALID and "pca_project is not available on a row-sharded handle" in msg
    finally:
        sharded.comm_destroy()
    assert fit(h=sharded)[0] == _lib.OK
    # the neighbours answer as before
    _same(a.pca(2, max_iterations=2), good, "after the refusals")
