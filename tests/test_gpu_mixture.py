"""The label mixture on the GPU (include/morna_hip.h, "label mixture").  -m gpu

The yardstick is mixture_ref.py, the numpy restatement of the contract (pinned by hand and against scipy.optimize.nnls in
test_mixture_cpu.py).  Everything is compared as bytes: the centroid sums, their counts and Gram matrix, the weights, the four
info values and the active flags.  A shape's rows and index are made once and shared.
"""
import numpy as np
import pytest

from mixture_ref import ref_label_centroids, ref_mixture

pytestmark = pytest.mark.gpu

SHAPES = [(300, 64), (700, 1100), (400, 3000)]
LS = [1, 2, 3, 8, 63, 64, 65, 128]          # both sides of one label per lane (64) and of the two-slot form
ZERO_ROW, HUGE, NAN_ROW, INF_ROW, UNLABELLED = 1, 12, 13, 14, 20
TOL, SWEEPS = 1e-9, 400
_cache = {}


def _index(X):
    from morna_amd.annoy import AnnoyIndex
    a = AnnoyIndex(X.shape[1])
    a.add_items(X)
    return a


def _shape(n, D):
    """Rows around 16 directions (dir_of: which), with a zero row, a row times 1e25, a row with a NaN and a row with an inf
    among them."""
    if (n, D) not in _cache:
        rng = np.random.default_rng(1600 + n + D)
        dirs = rng.standard_normal((16, D))
        dir_of = rng.integers(0, 16, n)
        X = (dirs[dir_of] + rng.standard_normal((n, D))).astype(np.float32)
        X[ZERO_ROW] = 0.0
        X[HUGE] *= np.float32(1e25)
        X[NAN_ROW, 3] = np.nan
        X[INF_ROW, 7] = np.inf
        _cache[(n, D)] = dict(X=X, dir_of=dir_of, index=_index(X))
    return _cache[(n, D)]


def _labels(s, L, seed):
    """Every item a label in [0, L) but a few without; label L - 1 is left empty when there are three or more.  The labels
    follow the rows' directions -- few labels merge directions, many labels share one -- so that centroids correlate as tissue
    centroids do without being all alike."""
    rng = np.random.default_rng(seed)
    n, used = len(s["dir_of"]), L if L < 3 else L - 1
    per = -(-used // 16)
    lab = ((s["dir_of"] * per + rng.integers(0, per, n)) % used).astype(np.int32)
    lab[rng.choice(n, n // 10, replace=False)] = -1
    lab[UNLABELLED] = -1
    return lab


def _same(got, want, label):
    names = ("weights", "info", "active")
    for g, w, name in zip(got, want, names):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w, dtype=g.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            assert False, (label, name, bad[:6].tolist(), [g[tuple(b)] for b in bad[:6]], [w[tuple(b)] for b in bad[:6]])


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n,D", SHAPES)
def test_label_centroids_are_the_restatements_bytes(n, D, L):
    s = _shape(n, D)
    a, X = s["index"], s["X"]
    lab = _labels(s, L, 7 * L + D)
    for allow in (None, np.arange(n) % 3 != 0):
        want = ref_label_centroids(X, lab, L, allow)
        r = None if allow is None else a.restriction(allow=allow)
        sums, counts, S = a.label_centroids(lab, L, restriction=r)
        assert counts.dtype == np.int32 and counts.tolist() == want[1].tolist()
        assert sums.tobytes() == want[0].tobytes() and S.tobytes() == want[2].tobytes()
        assert (S == S.T).all()
        if L >= 3:
            assert counts[L - 1] == 0 and not sums[L - 1].any()
        sums2, counts2, none = a.label_centroids(lab, L, restriction=r, gram=False)
        assert none is None and sums2.tobytes() == sums.tobytes() and counts2.tolist() == counts.tolist()
    # the planted rows: the zero, NaN and inf rows are skipped, the huge row is a member like any other
    planted = np.full(n, -1, np.int32)
    planted[[ZERO_ROW, HUGE, NAN_ROW, INF_ROW, 30]] = 0
    sums, counts, S = a.label_centroids(planted, 1)
    want = ref_label_centroids(X, planted, 1)
    assert counts.tolist() == [2] == want[1].tolist() and np.isfinite(sums).all() and sums.tobytes() == want[0].tobytes()


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n,D", SHAPES)
def test_mixture_by_item_and_by_vector_are_the_restatements_bytes(n, D, L):
    """By item every query leaves itself out of its label; the first items hold the planted rows (a zero row, NaN and inf rows:
    no fit; an item without a label: no patch).  300 queries on the small shape, more than the persistent grid has waves."""
    s = _shape(n, D)
    a, X = s["index"], s["X"]
    lab = _labels(s, L, 7 * L + D)
    nq = 300 if D == 64 else 65
    items = np.arange(nq, dtype=np.int32)
    want = ref_mixture(X, lab, L, items=items, tol=TOL, max_sweeps=SWEEPS)
    got = a.mixture(lab, L, items=items, tol=TOL, max_sweeps=SWEEPS)
    _same(got, want, "by item")
    w, info, active = got
    assert info[ZERO_ROW].tolist() == [0, 0, 0, -1] and info[NAN_ROW, 3] == -1 and info[INF_ROW, 3] == -1 and not w[NAN_ROW].any()
    assert (w >= 0).all() and not w[~active].any()
    if L >= 3:
        assert not active[:, L - 1].any()
    stats = a.mixture_stats()
    assert stats["queries"] == nq and stats["sweeps"] == int(info[:, 2].sum()) and stats["max_sweeps"] == int(info[:, 2].max())
    assert stats["open"] == int((info[:, 3] != 1).sum()) >= 3
    assert min(stats["centroids_ms"], stats["gram_ms"], stats["dots_ms"], stats["solve_ms"]) > 0
    # by vector: the same rows fit against centroids that still hold them, and vectors from outside
    rng = np.random.default_rng(5 * L + n)
    Q = np.concatenate([X[[0, 2, UNLABELLED]].astype(np.float64), rng.standard_normal((2, D)), np.zeros((1, D))])
    for k in (1, 3, len(Q)):
        _same(a.mixture(lab, L, Q=Q[:k], tol=TOL, max_sweeps=SWEEPS), ref_mixture(X, lab, L, Y=Q[:k], tol=TOL, max_sweeps=SWEEPS),
              "by vector %d" % k)
    # one query alone and inside the batch; a second call
    for q in (0, 2, nq - 1):
        alone = a.mixture(lab, L, items=items[q:q + 1], tol=TOL, max_sweeps=SWEEPS)
        _same(alone, tuple(x[q:q + 1] for x in got), "alone %d" % q)
    _same(a.mixture(lab, L, items=items, tol=TOL, max_sweeps=SWEEPS), got, "second call")


def test_staged_query_rows():
    from test_gpu_labels import _stage_single_cell_rows
    n, D, L = 300, 64, 8
    s = _shape(n, D)
    a, X = s["index"], s["X"]
    lab = _labels(s, L, 3)
    for nq in (3, 65):
        r64 = _stage_single_cell_rows(a, nq, 40 + nq)
        _same(a.mixture(lab, L, tol=TOL, max_sweeps=SWEEPS), ref_mixture(X, lab, L, Y=r64, tol=TOL, max_sweeps=SWEEPS), "staged %d" % nq)


def test_planted_labels_and_queries():
    n, D, L = 300, 64, 8
    X = _shape(n, D)["X"].copy()
    X[40:44] = X[50:54]                                   # labels 5 and 6 hold identical rows: the Gram matrix is singular
    a = _index(X)
    lab = np.full(n, -1, np.int32)
    lab[60:120], lab[120:180], lab[180:240] = 0, 1, 2
    lab[25] = 3                                           # a label whose only member is the query
    lab[[ZERO_ROW, 2]] = 4                                # one unskipped member: inactive for item 2 alone
    lab[40:44], lab[50:54] = 5, 6
    lab[[NAN_ROW, INF_ROW, HUGE]] = 0                     # skipped, skipped, a member
    lab7 = lab.copy()
    lab7[ZERO_ROW] = 7                                    # a label of zero rows: inactive for everyone
    lab7[2] = -1
    items = np.array([25, 2, ZERO_ROW, UNLABELLED, 41, 51, 70, HUGE, 130], np.int32)
    for name, labels in (("lone member", lab), ("zero label", lab7)):
        want = ref_mixture(X, labels, L, items=items, tol=TOL, max_sweeps=SWEEPS)
        got = a.mixture(labels, L, items=items, tol=TOL, max_sweeps=SWEEPS)
        _same(got, want, name)
    w, info, active = a.mixture(lab, L, items=items, tol=TOL, max_sweeps=SWEEPS)
    assert not active[0, 3] and active[1:, 3].all()       # label 3 is inactive for its only member, active for the others
    assert not active[1, 4] and active[0, 4] and not active[:, 7].any()
    assert info[2, 3] == -1                               # the zero row as a query
    assert (info[[0, 1, 3, 4, 5, 6, 7, 8], 3] >= 0).all()
    # (the duplicate labels 5 and 6: the weight goes where the restatement puts it, compared above)
    w7, _, active7 = a.mixture(lab7, L, items=items, tol=TOL, max_sweeps=SWEEPS)
    assert not active7[:, 7].any() and not active7[:, 4].any() and not w7[:, 7].any()
    # a NaN host query is refused
    Q = X[:3].astype(np.float64)
    Q[1, 5] = np.nan
    with pytest.raises(ValueError, match="^mixture: query 1 "):
        a.mixture(lab, L, Q=Q)
    # an allow-list: a query outside it gets no patch; the same bytes as an index that holds only the allowed rows
    allow = np.ones(n, bool)
    allow[[70, 71, 130, 200, 25]] = False
    r = a.restriction(allow=allow)
    got = a.mixture(lab, L, items=items, restriction=r, tol=TOL, max_sweeps=SWEEPS)
    _same(got, ref_mixture(X, lab, L, items=items, allow=allow, tol=TOL, max_sweeps=SWEEPS), "allow-list")
    assert not got[2][:, 3].any()                         # label 3 lost its only member to the allow-list
    Q = np.concatenate([X[[70, 130, 5]].astype(np.float64), np.random.default_rng(3).standard_normal((4, D))])
    small = _index(X[allow])
    _same(small.mixture(lab[allow], L, Q=Q, tol=TOL, max_sweeps=SWEEPS), a.mixture(lab, L, Q=Q, restriction=r, tol=TOL, max_sweeps=SWEEPS),
          "the allowed rows alone")
    by_item = a.mixture(lab, L, items=np.array([70, 130], np.int32), restriction=r, tol=TOL, max_sweeps=SWEEPS)
    _same(by_item, tuple(x[:2] for x in small.mixture(lab[allow], L, Q=Q, tol=TOL, max_sweeps=SWEEPS)), "outside the allow-list")


def test_stopping():
    n, D, L = 300, 64, 8
    s = _shape(n, D)
    a, X = s["index"], s["X"]
    lab = _labels(s, L, 3)
    items = np.arange(30, 95, dtype=np.int32)
    for sweeps in (1, 2):
        got = a.mixture(lab, L, items=items, tol=1e-300, max_sweeps=sweeps)
        _same(got, ref_mixture(X, lab, L, items=items, tol=1e-300, max_sweeps=sweeps), "max_sweeps %d" % sweeps)
        assert (got[1][:, 2] == sweeps).all() and (got[1][:, 3] == 0).all()
    # tol = 0: the fit runs until a sweep moves nothing, or to the end
    got = a.mixture(lab, L, items=items, tol=0.0, max_sweeps=300)
    _same(got, ref_mixture(X, lab, L, items=items, tol=0.0, max_sweeps=300), "tol 0")
    # a tolerance that part of the batch reaches inside the sweeps given and part does not
    full = a.mixture(lab, L, items=items, tol=1e-12, max_sweeps=SWEEPS)[1]
    cut = int(np.median(full[:, 2]))
    got = a.mixture(lab, L, items=items, tol=1e-12, max_sweeps=cut)
    _same(got, ref_mixture(X, lab, L, items=items, tol=1e-12, max_sweeps=cut), "mixed stopping")
    assert (got[1][:, 3] == 1).any() and (got[1][:, 3] == 0).any()
    assert a.mixture_stats()["open"] == int((got[1][:, 3] != 1).sum())


def test_planted_blends_are_recovered():
    """Three blobs at dim 64; the queries are normalised 0.7 / 0.3 and 0.5 / 0.3 / 0.2 sums of member rows.  The largest
    weights are on the planted labels in the planted order and every share is within 0.1 of the planted one -- a condition on
    the planted data, checked with the restatement first."""
    rng = np.random.default_rng(2024)
    D, per = 64, 40
    cent = rng.standard_normal((3, D))
    X = (np.repeat(cent, per, axis=0) + 0.25 * rng.standard_normal((3 * per, D))).astype(np.float32)
    lab = np.repeat(np.arange(3), per).astype(np.int32)
    unit = X.astype(np.float64) / np.linalg.norm(X.astype(np.float64), axis=1)[:, None]
    plans = [((0, 1), (0.7, 0.3)), ((2, 0), (0.7, 0.3)), ((1, 2, 0), (0.5, 0.3, 0.2)), ((2, 1, 0), (0.5, 0.3, 0.2))]
    Q = []
    for ls, ws in plans:
        # (the mean of a few unit member rows per label, weighted)
        Q.append(sum(wt * unit[l * per + rng.choice(per, 8, replace=False)].mean(axis=0) for l, wt in zip(ls, ws)))
    Q = np.array(Q)
    Q /= np.linalg.norm(Q, axis=1)[:, None]
    want = ref_mixture(X, lab, 3, Y=Q, tol=1e-12, max_sweeps=SWEEPS)
    got = _index(X).mixture(lab, 3, Q=Q, tol=1e-12, max_sweeps=SWEEPS)
    for w in (want[0], got[0]):
        for q, (ls, ws) in enumerate(plans):
            assert np.argsort(-w[q], kind="stable")[:len(ls)].tolist() == list(ls), (q, w[q])
            share = w[q] / w[q].sum()
            for l, wt in zip(ls, ws):
                assert abs(share[l] - wt) <= 0.1, (q, share, ls, ws)
    _same(got, want, "blends")
    assert (got[1][:, 3] == 1).all() and (got[1][:, 0] < 0.2).all()


def test_refusals_through_the_raw_call():
    from morna_amd import _lib
    from morna_amd._lib import lib, ptr
    from morna_amd.annoy import AnnoyIndex
    n, D, L = 300, 64, 4
    rng = np.random.default_rng(9)
    X = rng.standard_normal((n, D)).astype(np.float32)      # (label_sums, asked below, takes no row outside its scan's domain)
    a = _index(X)
    lab = rng.integers(-1, L, n).astype(np.int32)
    items = np.arange(30, 33, dtype=np.int32)
    Q = X[30:33].astype(np.float64)
    w, info, active = np.zeros((3, 200)), np.zeros((3, 4)), np.zeros((3, 200), np.uint8)
    sums, counts, S = np.zeros((200, D)), np.zeros(200, np.int32), np.zeros((200, 200))
    stats = np.ones(8)
    before_sums = a.label_sums(lab, L, items=items)
    before_assign = a.kmeans_assign(Q)

    def call(h=a, r=None, q=None, it=items, nq=3, labels=lab, nl=L, tol=1e-9, sweeps=100, out=w):
        return lib().morna_mixture(h._h, r, ptr(q), ptr(it), nq, ptr(labels), nl, tol, sweeps, ptr(out), ptr(info), ptr(active))

    def cents(h=a, r=None, labels=lab, nl=L):
        return lib().morna_label_centroids(h._h, r, ptr(labels), nl, ptr(sums), ptr(counts), ptr(S))
    assert call() == _lib.OK and cents() == _lib.OK
    assert lib().morna_mixture_stats(a._h, ptr(stats)) == _lib.OK and stats[0] > 0 and stats[4] == 0     # (the centroids alone)
    bad = lab.copy()
    bad[17] = L
    assert call(labels=bad) == _lib.E_INVALID and b"item 17" in lib().morna_last_error()
    assert cents(labels=bad) == _lib.E_INVALID and b"item 17" in lib().morna_last_error()
    bad[17] = -2
    assert call(labels=bad) == _lib.E_INVALID and b"item 17" in lib().morna_last_error()
    for nl in (0, 129):
        assert call(nl=nl) == _lib.E_INVALID and b"%d labels" % nl in lib().morna_last_error() and b"128" in lib().morna_last_error()
        assert cents(nl=nl) == _lib.E_INVALID and b"%d labels" % nl in lib().morna_last_error()
    assert call(nl=128) == _lib.OK
    for tol in (-1e-9, float("inf"), float("nan")):
        assert call(tol=tol) == _lib.E_INVALID and b"tol" in lib().morna_last_error()
    assert call(sweeps=0) == _lib.E_INVALID and b"max_sweeps = 0" in lib().morna_last_error()
    assert call(q=Q) == _lib.E_INVALID and b"not both" in lib().morna_last_error()
    # after a refusal the statistics say nothing ran
    assert lib().morna_mixture_stats(a._h, ptr(stats)) == _lib.OK and not stats.any()
    assert call(it=np.array([0, n, 1], np.int32)) == _lib.E_RANGE
    Qbad = Q.copy()
    Qbad[2, 1] = np.inf
    assert call(q=Qbad, it=None) == _lib.E_INVALID and lib().morna_last_error().startswith(b"mixture: query 2 ")
    assert call(out=None) == _lib.E_INVALID and b"null buffer" in lib().morna_last_error()
    assert call(nq=-1) == _lib.E_INVALID
    # a restriction that holds groups; one of another handle; an empty index
    r_groups = a.restriction(groups=np.zeros(n, np.int32))
    assert call(r=r_groups._p) == _lib.E_INVALID and b"holds groups" in lib().morna_last_error()
    assert cents(r=r_groups._p) == _lib.E_INVALID and b"holds groups" in lib().morna_last_error()
    r_allow = a.restriction(allow=np.ones(n, bool))
    assert call(r=r_allow._p) == _lib.OK
    other = _index(X)
    assert call(h=other, r=r_allow._p) == _lib.E_INVALID
    with pytest.raises(ValueError):
        other.mixture(lab, L, items=items, restriction=r_allow)
    empty = AnnoyIndex(D)
    assert call(h=empty, labels=np.zeros(1, np.int32)) == _lib.E_EMPTY and cents(h=empty, labels=np.zeros(1, np.int32)) == _lib.E_EMPTY
    # a row-sharded handle: one that owns a communicator, here of one rank; giving it back lifts the refusal
    sharded = _index(X)
    sharded.comm_init(AnnoyIndex.comm_unique_id(), 0, 1)
    try:
        assert call(h=sharded) == _lib.E_INVALID and b"mixture is not available on a row-sharded handle" in lib().morna_last_error()
        assert cents(h=sharded) == _lib.E_INVALID and b"label_centroids is not available on a row-sharded" in lib().morna_last_error()
        assert lib().morna_mixture_stats(sharded._h, ptr(stats)) == _lib.OK and not stats.any()
    finally:
        sharded.comm_destroy()
    assert call(h=sharded) == _lib.OK
    # the Python surface checks shapes before the call
    with pytest.raises(ValueError):
        a.mixture(lab[:-1], L, items=items)
    with pytest.raises(ValueError):
        a.mixture(lab, L, items=items, Q=Q)
    with pytest.raises(IndexError):
        a.mixture(lab, L, Q=Q[:, :5])
    # no staged rows on a fresh handle
    assert call(h=other, it=None) == _lib.E_INVALID and b"no query source" in lib().morna_last_error()
    # the neighbours of the family answer as before
    after_sums = a.label_sums(lab, L, items=items)
    assert after_sums[0].tobytes() == before_sums[0].tobytes() and after_sums[1].tobytes() == before_sums[1].tobytes()
    after_assign = a.kmeans_assign(Q)
    assert after_assign[0].tobytes() == before_assign[0].tobytes() and after_assign[1].tobytes() == before_assign[1].tobytes()
