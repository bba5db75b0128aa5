"""The exact search's fp32 window under stress: near-ties at the k-th distance and rows and queries across the float
range.  -m gpu

The exact search returns the oracle's ids, fp64 distances and -1 count bit for bit only if the window of
exact_scan_eps (exact.hip) really bounds the error of the fp32 scan that selects the candidates.  On random or TF-IDF rows
the k-th and (k+1)-th distances are far apart, so that bound is never tested there.  Here:

  * near-tie clusters: a few hundred rows fp32(b + s g_j) around a base row b, the query near b, the spreads s chosen so
    that consecutive true 2 - 2cos values are 1/500, 1/2 or 2 times the scan's window apart (far below, near and above
    its error), k inside the cluster; one cluster at 2 - 2cos ~ 1 (rows at 60 degrees, nothing nearer); exact ties by power-of-two
    scaling inside the clusters;
  * the float range: rows at scales 2^-149 .. 2^126, rows parallel to the query at scales where the fp32 norm underflows,
    is subnormal or overflows (the scan cannot bound those: they are re-ranked for every query), a zero row, a row of
    subnormals; queries of zero, of elements below and above fp32's range, one element of 1e30.

Every case is named by the code path it reaches: the scan (vector ALU with QT = 8 / 4 / 2 / 1 queries per pass, by
dpad, below 32 queries; matrix cores at 32 or more), the selection (k rounds: N <= 8192, k > 256 or MORNA_EXACT_SELECT2=0;
two passes: N > 8192 and k <= 256) and the query source (fp64 host queries, stored rows, fp32 queries in device memory).
The expected answers are oracle.capi.exact_search (the sequential fp64 restatement of exact_search_nn); numpy only builds
the data and chooses k.  A query for which cosine_distance is NaN for any row must come back with count -1.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from oracle import capi as c
    c.lib()
    return c


# ------------------------------------------------------------------------- data

def _unit_rows(rng, n, D):
    """n random fp32 rows of norm ~1, made in chunks."""
    out = np.empty((n, D), np.float32)
    for c0 in range(0, n, 4096):
        c1 = min(n, c0 + 4096)
        out[c0:c1] = rng.standard_normal((c1 - c0, D), dtype=np.float32) * np.float32(1.0 / np.sqrt(D))
    return out


def _cluster(rng, b, deltas, d0):
    """Rows fp32(b + s_j g_j) with g_j random and orthogonal to b, |g_j| = |b|: their 2 - 2cos to b is ~ s_j^2 (d0 + j
    deltas apart)."""
    D = b.shape[0]
    b64 = b.astype(np.float64)
    nb = np.linalg.norm(b64)
    rows = np.empty((len(deltas), D), np.float32)
    dist = d0 + np.cumsum(deltas)
    for j, t in enumerate(dist):
        g = rng.standard_normal(D)
        g -= (g @ b64) / (nb * nb) * b64
        g *= nb / np.linalg.norm(g)
        rows[j] = (b64 + np.sqrt(t) * g).astype(np.float32)
    return rows


def _sixty(rng, b, n, delta):
    """Rows at ~60 degrees from b: 2 - 2cos = 1 + j delta."""
    D = b.shape[0]
    u = b.astype(np.float64) / np.linalg.norm(b.astype(np.float64))
    rows = np.empty((n, D), np.float32)
    for j in range(n):
        c = 0.5 - j * delta / 2
        g = rng.standard_normal(D)
        g -= (g @ u) * u
        g /= np.linalg.norm(g)
        rows[j] = ((c * u + np.sqrt(1 - c * c) * g) * rng.uniform(0.5, 2.0)).astype(np.float32)
    return rows


def _scan_error(D, mfma):
    """The window of the scan that runs (exact_scan_eps, exact.hip: the matrix-core scan for batches of 32 queries or
    more, the vector-ALU scan below): the scale of that scan's error."""
    dpad = (D + 255) // 256 * 256
    u = 2.0 ** -24
    e_dot = (128 + dpad // 128 + 8) * u if mfma else (dpad // 64 + 8) * u
    e_norm = (dpad // 64 + 8) * u
    return 4 * (e_dot + e_norm + 2 * u + u / 8)


def _near_tie_matrix(D, N, seed, mfma):
    """Background rows at 2 - 2cos ~ 2 from everything, and four clusters of 400 rows: consecutive distances spaced far
    below, near and above the error of the scan that will run (1/500, 1/2 and 2 times its window) from 1e-4, and one at
    2 - 2cos ~ 1 (half the window apart).  40 rows of each cluster are power-of-two multiples of others of the same
    cluster (exact ties).  Returns X and the base rows (the queries are near them)."""
    rng = np.random.default_rng(seed)
    X = _unit_rows(rng, N, D)
    bases = _unit_rows(rng, 4, D) * np.float32(3.0)
    spots = rng.permutation(N)[:1600].reshape(4, 400)
    w = _scan_error(D, mfma)
    for c, delta in enumerate((w / 500, w / 2, 2 * w)):
        X[spots[c]] = _cluster(rng, bases[c], np.full(400, delta), 1e-4)
    X[spots[3]] = _sixty(rng, bases[3], 400, w / 2)
    for c in range(4):
        src = rng.choice(spots[c][:200], 40, replace=False)
        X[spots[c][360:]] = X[src] * np.float32(2.0) ** rng.integers(-3, 4, 40).astype(np.float32)[:, None]
    # nothing outside the clusters nearer than 1.5 to a base (the 60-degree cluster holds the nearest rows of its query)
    B = bases.astype(np.float64) / np.linalg.norm(bases.astype(np.float64), axis=1, keepdims=True)
    mask = np.ones(N, bool)
    mask[spots.ravel()] = False
    for i in np.nonzero(mask)[0]:
        x = X[i].astype(np.float64)
        if np.max(B @ x) / np.linalg.norm(x) > 0.25:
            X[i] = -X[i]
    return X, bases


def _near_tie_queries(rng, bases, nq):
    """Queries near the bases (fp64, 1e-7 relative noise), cycling through the four clusters."""
    Q = np.empty((nq, bases.shape[1]), np.float64)
    for i in range(nq):
        b = bases[i % 4].astype(np.float64)
        Q[i] = b * (1 + 1e-7 * rng.standard_normal(b.shape[0]))
    return Q


SCALES = (-149, -140, -126, -100, -80, -70, -64, -20, 0, 20, 60, 62, 64, 100, 126)
PARALLEL = (-100, -80, -70, -64, 0, 20, 60, 62, 64, 100)


def _float_range_matrix(D, N, seed, qbase):
    """Background unit rows; then, at the highest ids (the ones a tie at distance 0 puts first), 20 rows at each scale
    2^e of SCALES, the rows parallel to qbase at the scales of PARALLEL (exactly: powers of two), a zero row and a row of
    subnormals."""
    rng = np.random.default_rng(seed)
    X = _unit_rows(rng, N, D)
    i = N - 1
    for e in SCALES:
        for _ in range(20):
            if e <= -126:   # subnormal (or smallest normal) elements: small integer multiples of 2^-149 / 2^e
                X[i] = (rng.integers(-40, 41, D).astype(np.float32) * np.float32(2.0 ** (e + 3)) if e > -149
                        else rng.integers(-3, 4, D).astype(np.float32) * np.float32(2.0 ** -149))
            else:
                X[i] = rng.uniform(-1.0, 1.0, D).astype(np.float32) * np.float32(2.0 ** e)
            i -= 1
    for e in PARALLEL:
        X[i] = qbase * np.float32(2.0 ** e)
        assert np.isfinite(X[i]).all() and (X[i] != 0).all()
        i -= 1
    X[i] = 0.0
    X[i - 1] = 0.0
    X[i - 1, ::7] = np.float32(2.0 ** -149)
    return X


def _float_range_queries(qbase, D, rng):
    q = qbase.astype(np.float64)
    spike = rng.standard_normal(D)
    spike[D // 3] = 1e30
    # (2^-600: fp64 qq underflows to 0, cosine_distance gives 2 for every row; 2^500: pp qq overflows for the rows of 2^20
    # and above, which then get 2 as well)
    return np.stack([q, q * 2.0 ** -140, q * 2.0 ** 140, np.zeros(D), spike, q * 2.0 ** -80, q * 2.0 ** 62,
                     q * (1 + 1e-9 * rng.standard_normal(D)), q * 2.0 ** -600, q * 2.0 ** 500])


# ----------------------------------------------------------------------- checks

class _Oracle(object):
    """The expected answers for one matrix X."""

    def __init__(self, capi, X):
        self.capi, self.X = capi, X
        self.X64 = X.astype(np.float64)
        self.nx = np.sqrt(np.einsum("ij,ij->i", self.X64, self.X64))
        self.nan = {}

    def nan_anywhere(self, q):
        """cosine_distance is NaN for some row (the reference raises for the whole query): only a row all but parallel
        to q can give a negative radicand; numpy's fp64 cosine picks those out, the oracle decides."""
        key = q.tobytes()
        if key not in self.nan:
            with np.errstate(all="ignore"):
                cos = (self.X64 @ q) / (self.nx * np.linalg.norm(q))
            cand = np.nonzero(~(cos < 1.0 - 1e-9))[0]   # NaN cosines included
            self.nan[key] = any(np.isnan(self.capi.cosine_distance(self.X[r], q)) for r in cand)
        return self.nan[key]


def _check(orc, Qo, k, ids, d, cnt, sample, label):
    """Qo: the queries as the oracle sees them (fp64)."""
    X, capi = orc.X, orc.capi
    N = X.shape[0]
    for qi in sample:
        q = np.asarray(Qo[qi], np.float64)
        if orc.nan_anywhere(q):
            assert cnt[qi] == -1, (label, qi)
            continue
        rid, rd = capi.exact_search(X, q, k)
        m = len(rid)
        assert m == min(k, N)
        assert cnt[qi] == m, (label, qi, cnt[qi], m)
        assert ids[qi, :m].astype(np.int64).tolist() == rid.tolist(), (label, qi)
        assert d[qi, :m].tobytes() == rd.tobytes(), (label, qi)
        assert (ids[qi, m:] == -1).all() and np.isinf(d[qi, m:]).all(), (label, qi)


def _with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _packed(a, k, Q=None, q_dev_rows=None, items=None):
    """exact_search_packed, its message decoded (ids, dist, count); q_dev_rows: fp32 rows copied to device memory."""
    import torch
    from morna_amd.annoy import AnnoyIndex
    dev = torch.device("cuda", 0)
    nq = len(Q) if Q is not None else len(q_dev_rows) if q_dev_rows is not None else len(items)
    nbytes = AnnoyIndex.exact_packed_bytes(nq, k)
    msg = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    if q_dev_rows is not None:
        qd = torch.from_numpy(np.ascontiguousarray(q_dev_rows, np.float32)).to(dev)
        a.exact_search_packed(msg.data_ptr(), k, 0, q_dev=(qd.data_ptr(), nq))
    else:
        a.exact_search_packed(msg.data_ptr(), k, 0, Q=Q, items=items)
    a.synchronize()
    raw = msg.cpu().numpy()
    ids = raw[:nq * k * 4].view(np.int32).reshape(nq, k)
    cnt = raw[nq * k * 4:nq * (k + 1) * 4].view(np.int32)
    d = raw[nbytes - nq * k * 8:].view(np.float64).reshape(nq, k)
    return ids, d, cnt


# ----------------------------------------------------------------- near-ties

# (D, N): dpad 256 / 3072 / 8192 / 12032 -> QT = 8 / 4 / 2 / 1 below 32 queries; N <= 8192 (k-round selection) and
# N > 8192 (two-pass selection for k <= 256)
NEAR_TIE_SHAPES = [(200, 3000), (200, 9000), (3000, 3000), (3000, 9000), (8000, 2500), (8000, 8400), (12000, 2000),
                   (12000, 8400)]


def _case_id(D, N):
    """the scan of a small batch (QT) and the selection of k <= 256 this shape reaches"""
    return "%s-%s-D%d-N%d" % (_path(D, N, 1, 1).split("/")[0], "select2" if N > 8192 else "select_k", D, N)


def _path(D, N, nq, k, select2=True):
    dpad = (D + 255) // 256 * 256
    qt = 8 if dpad * 32 <= 65536 else 4 if dpad * 16 <= 65536 else 2 if dpad * 8 <= 65536 else 1
    scan = "mfma" if nq >= 32 else "vec_qt%d" % qt
    sel = "select2" if N > 8192 and k <= 256 and select2 else "select_k"
    return "%s/%s/D%d/N%d/k%d" % (scan, sel, D, N, k)


@pytest.mark.parametrize("D,N", NEAR_TIE_SHAPES, ids=[_case_id(*s) for s in NEAR_TIE_SHAPES])
def test_near_ties_host_queries(capi, D, N):
    """fp64 host queries near the cluster bases: both scans (8 and 40 queries), k = 1, k in the clusters (200: two-pass
    selection past 8192 rows; 300: the k-round form), k = N, k > N; N > 8192 also with MORNA_EXACT_SELECT2=0.  The
    clusters are spaced by the window of the scan each batch takes."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(D * N)
    for nq in (8, 40):
        X, bases = _near_tie_matrix(D, N, 7000 + D + N, nq >= 32)
        a = AnnoyIndex(D)
        a.add_items(X)
        orc = _Oracle(capi, X)
        Q = _near_tie_queries(rng, bases, nq)
        sample = [0, 1, 2, 3] if nq < 32 else [4, 5, 6, 7, 38, 39]
        for k in (1, 200, 300):
            ids, d, cnt = a.exact_search_batch(Q, k)
            _check(orc, Q, k, ids, d, cnt, sample, _path(D, N, nq, k))
            if N > 8192 and k <= 256:
                r0 = _with_env("MORNA_EXACT_SELECT2", "0", lambda: a.exact_search_batch(Q, k))
                assert r0[0].tolist() == ids.tolist() and r0[1].tobytes() == d.tobytes() and r0[2].tolist() == cnt.tolist()
    if D <= 3000:   # k = N and k > N: the oracle's insertion is O(N k), one query of each scan (the index of the last batch)
        Q = _near_tie_queries(rng, bases, 32)
        for k in (N, N + 5):
            ids, d, cnt = a.exact_search_batch(Q[:1], k)
            _check(orc, Q[:1], k, ids, d, cnt, [0], _path(D, N, 1, k))
        ids, d, cnt = a.exact_search_batch(Q, N + 5)
        _check(orc, Q, N + 5, ids, d, cnt, [3], _path(D, N, 32, N + 5))


@pytest.mark.parametrize("D,N", [(200, 9000), (3000, 3000), (12000, 2000)],
                         ids=[_case_id(*s) for s in [(200, 9000), (3000, 3000), (12000, 2000)]])
def test_near_ties_stored_and_device_queries(capi, D, N):
    """Cluster rows as the queries: by item (exact_widen_kernel) and as fp32 rows in device memory through the packed
    message (the sharded by-item search's path), below and above 32 queries, on clusters spaced by that scan's window."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(D + N)
    for nq in (6, 36):
        X, bases = _near_tie_matrix(D, N, 7000 + D + N, nq >= 32)
        a = AnnoyIndex(D)
        a.add_items(X)
        orc = _Oracle(capi, X)
        # the rows nearest to each base: stored rows inside the clusters
        near = [int(np.argmax((orc.X64 @ b) / orc.nx)) for b in bases.astype(np.float64)]
        items = np.array((near * 9)[:nq], np.int32)
        items[4:] = rng.integers(0, N, nq - 4)
        Qo = X[items].astype(np.float64)
        sample = [0, 1, 2, 3, nq - 1]
        for k in (1, 150):
            ids, d, cnt = a.exact_search_by_item_batch(items, k)
            _check(orc, Qo, k, ids, d, cnt, sample, "by_item/" + _path(D, N, nq, k))
            pi, pd, pc = _packed(a, k, q_dev_rows=X[items])
            assert pi.tolist() == ids.tolist() and pd.tobytes() == d.tobytes() and pc.tolist() == cnt.tolist()
            pi, pd, pc = _packed(a, k, items=items)
            assert pi.tolist() == ids.tolist() and pd.tobytes() == d.tobytes() and pc.tolist() == cnt.tolist()


def test_candidate_room_grows_past_a_tie_group(capi):
    """600 power-of-two multiples of one row (one distance) and k = 10: the tie group is larger than max(64, 4k), the host
    makes room and selects again; both selections, both scans."""
    from morna_amd.annoy import AnnoyIndex
    for N in (5000, 9000):
        X, bases = _near_tie_matrix(256, N, 44 + N, False)
        rng = np.random.default_rng(N)
        grp = rng.choice(N, 600, replace=False)
        X[grp] = X[grp[0]] * np.float32(2.0) ** rng.integers(-20, 21, 600).astype(np.float32)[:, None]
        a = AnnoyIndex(256)
        a.add_items(X)
        orc = _Oracle(capi, X)
        for nq in (3, 33):
            Q = np.repeat(X[grp[:1]].astype(np.float64), nq, axis=0)
            ids, d, cnt = a.exact_search_batch(Q, 10)
            _check(orc, Q, 10, ids, d, cnt, [0, nq - 1], _path(256, N, nq, 10))


def test_two_batches_in_one_call(capi):
    """N = 600 000 rows of D = 16 and 900 queries: batches of 2^29 / N = 894 and 6 queries, i.e. the matrix-core scan and
    then the vector scan in one call, with near-ties and rows at extreme scales.  A sample of both batches."""
    from morna_amd.annoy import AnnoyIndex
    D, N = 16, 600000
    rng = np.random.default_rng(16)
    qbase = rng.standard_normal(D).astype(np.float32)
    X = _float_range_matrix(D, N, 17, qbase)
    spots = rng.choice(N - 400, 300, replace=False)
    X[spots] = _cluster(rng, qbase, np.full(300, 1e-7), 1e-5)
    a = AnnoyIndex(D)
    a.add_items(X)
    orc = _Oracle(capi, X)
    Q = np.repeat(qbase[None].astype(np.float64), 900, axis=0) * (1 + 1e-8 * rng.standard_normal((900, D)))
    Q[1::7] *= 2.0 ** 70
    Q[895] = _float_range_queries(qbase, D, rng)[1]
    ids, d, cnt = a.exact_search_batch(Q, 20)
    assert 2 ** 29 // N == 894
    _check(orc, Q, 20, ids, d, cnt, [0, 1, 500, 893, 894, 895, 899], "mfma+vec_qt8/select2/two_batches")


# -------------------------------------------------------------- float range

FLOAT_SHAPES = [(300, 3000), (300, 9000), (3000, 2000), (8000, 2000), (12000, 8400)]


@pytest.mark.parametrize("D,N", FLOAT_SHAPES, ids=[_case_id(*s) for s in FLOAT_SHAPES])
def test_float_range(capi, D, N):
    """Rows at scales 2^-149 .. 2^126 and rows parallel to the query at scales where the fp32 norm underflows, is
    subnormal or overflows (distance 0 in fp64: k = 1 must find the highest of their ids); queries of zero, below and
    above fp32's range, a 1e30 spike.  Host queries (both scans), stored rows and device fp32 rows as queries."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(D + 3 * N)
    qbase = rng.standard_normal(D).astype(np.float32)
    X = _float_range_matrix(D, N, D + N, qbase)
    a = AnnoyIndex(D)
    a.add_items(X)
    orc = _Oracle(capi, X)
    Q = _float_range_queries(qbase, D, rng)
    for k in (1, 15, 300):
        ids, d, cnt = a.exact_search_batch(Q, k)
        _check(orc, Q, k, ids, d, cnt, range(len(Q)), "float_range/" + _path(D, N, len(Q), k))
        Q40 = np.concatenate([Q] * 5)
        ids, d, cnt = a.exact_search_batch(Q40, k)
        _check(orc, Q40, k, ids, d, cnt, range(len(Q)), "float_range/" + _path(D, N, len(Q40), k))
    # stored rows at every scale as the queries, and the same rows from device memory
    items = np.arange(N - 1, N - 1 - 20 * len(SCALES) - len(PARALLEL) - 2, -10).astype(np.int32)
    for k in (1, 20):
        ids, d, cnt = a.exact_search_by_item_batch(items, k)
        _check(orc, X[items].astype(np.float64), k, ids, d, cnt, range(len(items)),
               "float_range/by_item/" + _path(D, N, len(items), k))
        pi, pd, pc = _packed(a, k, q_dev_rows=X[items])
        assert pi.tolist() == ids.tolist() and pd.tobytes() == d.tobytes() and pc.tolist() == cnt.tolist()
        pi, pd, pc = _packed(a, k, Q=X[items].astype(np.float64))
        assert pi.tolist() == ids.tolist() and pd.tobytes() == d.tobytes() and pc.tolist() == cnt.tolist()


def test_only_rows_outside_the_window(capi):
    """Every row outside the scan's domain (norms that underflow or overflow in fp32), k below and above their number,
    N above and below 8192: the threshold is then set by no row, the candidates are the rows themselves."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(5)
    for N in (300, 8500):
        D = 64
        X = rng.uniform(-1, 1, (N, D)).astype(np.float32)
        X[: N // 2] *= np.float32(2.0 ** -90)
        X[N // 2:] *= np.float32(2.0 ** 100)
        a = AnnoyIndex(D)
        a.add_items(X)
        orc = _Oracle(capi, X)
        Q = rng.standard_normal((4, D))
        Q[1] = X[3]
        for k in (5, 200, N + 1):
            ids, d, cnt = a.exact_search_batch(Q, k)
            _check(orc, Q, k, ids, d, cnt, range(4), "outside_only/N%d/k%d" % (N, k))


def test_queries_where_the_fp64_arithmetic_leaves_the_normal_range(capi):
    """cosine_distance gives 2 whenever pp * qq underflows to 0 or overflows, whatever the cosine: a query of elements
    ~2^-600 (qq = 0) ties every row at sqrt(2), highest ids first; a query of 2^500 against a row of 2^20 parallel to it
    (fp32 norm well inside the scan's domain) gives that row sqrt(2), not 0.  Such queries are compared with every row.
    Both scans, both selections."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(600)
    for D, N in ((16, 200), (16, 9000), (300, 3000)):
        X = rng.standard_normal((N, D)).astype(np.float32)
        qb = rng.standard_normal(D).astype(np.float32)
        X[N // 3] = qb * np.float32(2.0 ** 20)
        X[N // 2] = qb
        a = AnnoyIndex(D)
        a.add_items(X)
        orc = _Oracle(capi, X)
        Q = np.stack([rng.standard_normal(D) * 2.0 ** -600, qb.astype(np.float64) * 2.0 ** 500,
                      qb.astype(np.float64) * 2.0 ** 440, qb.astype(np.float64) * 2.0 ** -440, qb.astype(np.float64)])
        assert (Q[0] ** 2).sum() == 0.0
        for nq in (5, 35):
            Qn = np.concatenate([Q] * 7)[:nq]
            for k in (1, 5):
                ids, d, cnt = a.exact_search_batch(Qn, k)
                _check(orc, Qn, k, ids, d, cnt, range(5), "fp64_range/" + _path(D, N, nq, k))
        rid, rd = capi.exact_search(X, Q[1], 1)
        assert rid[0] != N // 3                 # the parallel row is not the reference's answer there


def test_non_finite_queries_refused_non_finite_rows_reranked(capi):
    """Outside the contract: a host query with a NaN or inf element, or whose fp64 sum of squares overflows, gets
    ValueError (MORNA_E_INVALID), before any work (every rank of a sharded search holds the same queries).  Rows with a
    NaN or inf element are not refused: they are re-ranked for every query and get the reference's value (2 for a NaN
    row; NaN, so count -1, for an inf row), on the host, by-item and packed paths alike."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(3)
    X = rng.standard_normal((100, 32)).astype(np.float32)
    a = AnnoyIndex(32)
    a.add_items(X)
    for bad in (np.nan, np.inf, -np.inf, 1e200):
        Q = rng.standard_normal((3, 32))
        Q[1, 5] = bad
        with pytest.raises(ValueError):
            a.exact_search_batch(Q, 5)
    assert a.exact_search_batch(rng.standard_normal((2, 32)), 5)[2].tolist() == [5, 5]
    for N in (100, 9000):
        base = rng.standard_normal((N, 32)).astype(np.float32)
        for bad in (np.nan, np.inf):
            Xb = base.copy()
            Xb[40, 7] = bad
            Xb[N - 3] = np.nan
            b = AnnoyIndex(32)
            b.add_items(Xb)
            orc = _Oracle(capi, Xb)
            Q = rng.standard_normal((4, 32))
            Q[1] = Xb[5]
            items = np.array([1, 2, 40, N - 3], np.int32)
            for k in (1, 10):
                ids, d, cnt = b.exact_search_batch(Q, k)
                _check(orc, Q, k, ids, d, cnt, range(4), "non_finite_row/N%d/%s/k%d" % (N, bad, k))
                if bad == np.inf:
                    assert (cnt == -1).all()
                pi, pd, pc = _packed(b, k, Q=Q)
                assert pi.tolist() == ids.tolist() and pc.tolist() == cnt.tolist()
                assert pd.tobytes() == d.tobytes()
                ids, d, cnt = b.exact_search_by_item_batch(items, k)
                assert len(cnt) == 4
            b.add_item(40, X[40].tolist())          # the row made finite again: the list of rows is made anew
            assert b.exact_search_batch(rng.standard_normal((2, 32)), 5)[2].tolist() == [5, 5]
