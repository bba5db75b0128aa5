"""Exact radius search on the GPU (include/morna_hip.h, "radius search").  -m gpu

Two yardsticks, never the code under test: the CPU oracle (oracle.capi.exact_search over the evaluated rows with k = their
number, cut at r: test_radius_cpu.ref_radius) and, on the GPU, the existing exact searches with k = n_items, cut on the host.
Ids and the fp64 distances are compared as bytes, the counts as numbers.  The seeds were checked on the CPU: the random
families hold no query the oracle gives a NaN for except the planted ones, which the tests assert through the oracle.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_radius_cpu import ref_radius

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 64
COPY_OF, COPY, DOUBLE, ZERO, TINY = 3, 10, 11, 20, 21       # planted rows of the 64-wide families
TIE0, TIE1 = 100, 140                                        # 40 equal rows


@pytest.fixture(scope="module")
def capi():
    from oracle import capi as c
    c.lib()
    return c


def _family(n, seed, nq=65):
    """Normal rows with: an exact copy and a doubled copy of row 3, a zero row, a row whose fp32 squared norm lies below the
    scan's domain, 40 equal rows.  Queries: row 3 itself, then normal vectors; from 5 queries on, query 1 is the tie group's
    row and query 2 the zero vector."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)).astype(np.float32)
    X[COPY] = X[COPY_OF]
    X[DOUBLE] = X[COPY_OF] * np.float32(2.0)
    X[ZERO] = 0.0
    X[TINY] *= np.float32(2.0 ** -90)
    if n > TIE1:
        X[TIE0:TIE1] = rng.standard_normal(D).astype(np.float32)
    Q = rng.standard_normal((nq, D))
    Q[0] = X[COPY_OF].astype(np.float64)
    if nq >= 5 and n > TIE1:
        Q[1] = X[TIE0].astype(np.float64)
        Q[2] = 0.0
    return X, Q


def _index(X):
    from morna_amd.annoy import AnnoyIndex
    a = AnnoyIndex(X.shape[1])
    a.add_items(X)
    return a


def _nan_anywhere(capi, X, q, rows=None):
    """The oracle gives a NaN for some row of `rows` (all): numpy's fp64 cosine picks the near-parallel rows, the oracle decides."""
    X64 = X.astype(np.float64)
    with np.errstate(all="ignore"):
        cos = (X64 @ q) / (np.linalg.norm(X64, axis=1) * np.linalg.norm(q))
    cand = np.nonzero(~(cos < 1.0 - 1e-9))[0]
    if rows is not None:
        cand = np.intersect1d(cand, rows)
    return any(np.isnan(capi.cosine_distance(X[r], q)) for r in cand)


def _cut(ids, d, cnt, q, r, after=-1):
    """The yardstick list of query q (a row of a k = n_items exact search) cut at r: the entries with id > after and a
    distance <= r, then the NaN entries with id > after; the count the contract gives."""
    i, dd = ids[q], d[q]
    have = i >= 0
    i, dd = i[have], dd[have]
    if cnt[q] >= 0:
        i, dd = i[:cnt[q]], dd[:cnt[q]]
    keep = ((dd <= r) | np.isnan(dd)) & (i > after)
    i, dd = i[keep], dd[keep]
    return i, dd, (-1 if np.isnan(dd).any() else len(i))


def _same(got, counts, q, want, label):
    wi, wd, wc = want
    gi, gd = got[q]
    assert gi.dtype == np.int32 and gd.dtype == np.float64
    assert gi.tolist() == wi.tolist(), (label, q, len(gi), len(wi))
    assert gd.tobytes() == np.ascontiguousarray(wd).tobytes(), (label, q)
    assert counts[q] == wc, (label, q, counts[q], wc)


def _check_call(a, full, r, label, after=None, **kw):
    ids, d, cnt = full
    lists, counts = a.exact_radius(r, after=after, **kw)
    assert len(lists) == len(cnt) and counts.dtype == np.int64
    for q in range(len(cnt)):
        _same(lists, counts, q, _cut(ids, d, cnt, q, r, -1 if after is None else int(after[q])), label)
    return lists, counts


def _radii(full, q):
    """0, everything, the 20th distance of query q (inclusive), the double just below it, a long answer, nothing."""
    d = full[1][q]
    d20 = float(d[19])
    below_first = float(np.nextafter(np.nanmin(full[1][q:], axis=None), 0.0))      # below every distance of the normal queries
    return [0.0, 2.5, d20, float(np.nextafter(d20, 0.0)), float(d[min(len(d) - 1, int(0.61 * len(d)))]), below_first]


@pytest.mark.parametrize("n,nq", [(700, 3), (700, 33), (8200, 65), (50, 1)])
def test_by_vector_against_both_yardsticks(capi, n, nq):
    X, Q = _family(n, seed=1400 + n, nq=nq)
    a = _index(X)
    full = a.exact_search_batch(Q, n)
    # the inputs: no query fails, the copies are where the oracle puts them, the 20th and 21st distances of query 3 differ
    assert (full[2] == n).all()
    for q in range(nq):
        assert not _nan_anywhere(capi, X, Q[q]), q
    oid, od = capi.exact_search(X, Q[0], 4)
    assert sorted(oid[:3].tolist()) == [COPY_OF, COPY, DOUBLE] and od[3] > od[2]
    assert full[1][0][:3].tobytes() == od[:3].tobytes()          # the copies' distances are the oracle's, whatever they are
    qb = min(3, nq - 1)
    radii = _radii(full, qb) if n > 50 else [0.0, 2.5, float(full[1][0][19]), 1.0]
    if n > 50:
        assert full[1][qb][19] != full[1][qb][20]
    for r in radii:
        lists, counts = _check_call(a, full, r, "n=%d nq=%d r=%r" % (n, nq, r), Q=Q)
        for q in sorted(set([0, min(1, nq - 1), min(2, nq - 1), qb, nq - 1])) if (n <= 700 or r < 1.0) else [qb]:
            wi, wd = ref_radius(capi, X, Q[q], r)                # the CPU oracle
            _same(lists, counts, q, (wi, wd, len(wi)), "oracle n=%d r=%r" % (n, r))
    if n > TIE1 and nq >= 5:
        # the tie group: its 40 rows at one distance, higher id first; the zero query: every row at sqrt(2), or none
        lists, counts = a.exact_radius(float(full[1][1][39]), Q=Q)
        assert lists[1][0][:40].tolist() == list(range(TIE1 - 1, TIE0 - 1, -1)) and len(set(lists[1][1][:40].tolist())) == 1
        assert counts[2] == 0
        lists, counts = a.exact_radius(float(np.sqrt(2.0)), Q=Q)
        assert lists[2][0].tolist() == list(range(n - 1, -1, -1)) and counts[2] == n
    if n == 8200:
        long_r = radii[4]
        lists, counts = a.exact_radius(long_r, Q=Q)
        assert 4096 < counts[qb] < 8200                          # past the lists the device orders
        st = a.exact_radius_stats()
        assert st["batches"] == 1 and st["queries"] == nq and st["results"] == int(counts.sum())


@pytest.mark.parametrize("n,dim,nq", [(300, 1100, 5), (300, 8192, 33), (300, 8192, 2)])
def test_wide_rows(capi, n, dim, nq):
    """Dimension 1100 (no multiple of anything) and 8192, where the MFMA scan's error term is largest."""
    rng = np.random.default_rng(dim + nq)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[7] = X[2]
    Q = rng.standard_normal((nq, dim))
    Q[0] = X[2].astype(np.float64)
    a = _index(X)
    full = a.exact_search_batch(Q, n)
    assert (full[2] == n).all()
    d20 = float(full[1][1][19])
    assert full[1][1][19] != full[1][1][20]
    for r in (0.0, d20, float(np.nextafter(d20, 0.0)), float(full[1][1][150]), 2.5):
        lists, counts = _check_call(a, full, r, "dim=%d nq=%d r=%r" % (dim, nq, r), Q=Q)
        for q in (0, 1):
            wi, wd = ref_radius(capi, X, Q[q], r)
            _same(lists, counts, q, (wi, wd, len(wi)), "oracle dim=%d r=%r" % (dim, r))


def _stage_rows(a, nq, seed):
    """nq query rows staged on the handle through morna_build_query_rows (a small made-up vocabulary); the fp64 rows."""
    from morna_amd.index import ParsedLines, pack_vocab
    rng = np.random.default_rng(seed)
    J = 150
    keys = [("chr%d %d %d" % (1 + j % 20, 1000 + 7 * j, 2000 + 11 * j)).encode() for j in range(J)]
    freq = {k.decode(): int(rng.integers(1, 60)) for k in keys}
    key_off = np.zeros(J + 1, np.int64)
    np.cumsum([len(k) for k in keys], out=key_off[1:])
    rows = [np.sort(rng.choice(nq, size=int(rng.integers(1, nq + 1)), replace=False)) for _ in range(J)]
    row_ptr = np.zeros(J + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=row_ptr[1:])
    ids = np.concatenate(rows)
    prep = dict(key_bytes=np.frombuffer(b"".join(keys), np.uint8), key_off=key_off, row_ptr=row_ptr, ids=ids,
                cov=rng.integers(1, 200, len(ids)), idf=np.zeros(J), ext_ids=np.arange(nq, dtype=np.int64))
    a.build_query_rows(ParsedLines.from_arrays(prep, 100).query_terms(pack_vocab(freq), 100))
    r64, _ = a.get_query_rows()
    assert r64.shape == (nq, a.f) and r64.any(axis=1).all()
    return r64


@pytest.mark.parametrize("nq", [3, 33])
def test_by_item_and_staged_rows(capi, nq):
    n = 700
    X, _ = _family(n, seed=2100)
    a = _index(X)
    items = np.concatenate([[COPY_OF, TIE0, ZERO, TINY], np.random.default_rng(nq).choice(n, size=nq, replace=False)])[:nq].astype(np.int32)
    full = a.exact_search_by_item_batch(items, n)
    assert (full[2] == n).all()
    q3 = nq - 1
    for r in (0.0, float(full[1][q3][19]), float(np.nextafter(full[1][q3][19], 0.0)), 1.3, 2.5):
        lists, counts = _check_call(a, full, r, "items nq=%d r=%r" % (nq, r), items=items)
        wi, wd = ref_radius(capi, X, X[items[0]].astype(np.float64), r)
        _same(lists, counts, 0, (wi, wd, len(wi)), "oracle items r=%r" % r)
    # ids above: alone
    after = np.where(np.arange(nq) % 2 == 0, items, 350).astype(np.int32)
    lists, counts = _check_call(a, full, 1.3, "after nq=%d" % nq, after=after, items=items)
    wi, wd = ref_radius(capi, X, X[items[0]].astype(np.float64), 1.3, after=int(after[0]))
    _same(lists, counts, 0, (wi, wd, len(wi)), "oracle after")
    # the staged query rows
    R = _stage_rows(a, nq, seed=9 + nq)
    full = a.exact_search_query_rows(n)
    assert (full[2] == n).all()
    for r in (float(full[1][0][19]), 1.35, 2.5):
        lists, counts = _check_call(a, full, r, "staged nq=%d r=%r" % (nq, r))
        wi, wd = ref_radius(capi, X, R[nq - 1], r)
        _same(lists, counts, nq - 1, (wi, wd, len(wi)), "oracle staged r=%r" % r)


def _groups(rng, n, sizes=(1, 2, 40)):
    g = np.full(n, -1, np.int32)
    members = rng.choice(n, size=sum(sizes), replace=False)
    at = 0
    for label, size in enumerate(sizes):
        g[members[at:at + size]] = label
        at += size
    return g


@pytest.mark.parametrize("nq", [4, 33])
def test_restrictions_and_ids_above(capi, nq):
    """Allow-lists of half, 5, 0 and all rows, groups of 1, 2 and 40, `after` with a restriction: the GPU yardstick is the
    restricted exact search with k = n_items, the CPU one ref_radius."""
    n = 700
    X, Q = _family(n, seed=3100, nq=nq)
    a = _index(X)
    rng = np.random.default_rng(77)
    half = rng.random(n) < 0.5
    half[[ZERO, COPY]] = True
    half[[TINY, DOUBLE]] = False
    five = np.zeros(n, bool)
    five[rng.choice(n, size=5, replace=False)] = True
    groups = _groups(rng, n)
    qg = np.array([(-1, 0, 1, 2)[q % 4] for q in range(nq)], np.int32)
    after = rng.integers(-1, n, size=nq).astype(np.int32)
    for name, allow, grp in (("half", half, None), ("five", five, None), ("none", np.zeros(n, bool), None),
                             ("all", np.ones(n, bool), None), ("half+groups", half, groups), ("groups", None, groups)):
        rs = a.restriction(allow, grp)
        g = qg if grp is not None else None
        full = a.exact_search_restricted(rs, n, Q=Q, query_groups=g)
        assert (full[2] >= 0).all()
        for r in (0.0, 1.3, 2.5):
            lists, counts = _check_call(a, full, r, "%s r=%r" % (name, r), Q=Q, restriction=rs, query_groups=g)
            lists2, counts2 = _check_call(a, full, r, "%s after r=%r" % (name, r), after=after, Q=Q, restriction=rs, query_groups=g)
            for q in (0, nq - 1):
                gq = int(g[q]) if g is not None else -1
                wi, wd = ref_radius(capi, X, Q[q], r, allow=allow, groups=grp, gq=gq)
                _same(lists, counts, q, (wi, wd, len(wi)), "oracle %s r=%r" % (name, r))
                wi, wd = ref_radius(capi, X, Q[q], r, after=int(after[q]), allow=allow, groups=grp, gq=gq)
                _same(lists2, counts2, q, (wi, wd, len(wi)), "oracle %s after r=%r" % (name, r))


def _nan_partner(capi, row):
    """A row all but parallel to `row` for which the oracle gives NaN either way (3 * row, rounded to fp32)."""
    b = (row * np.float32(3.0)).astype(np.float32)
    assert np.isnan(capi.cosine_distance(b, row.astype(np.float64))) and np.isnan(capi.cosine_distance(row, b.astype(np.float64)))
    return b


def test_nan_rows_fail_a_query_only_when_evaluated(capi):
    """A row the oracle gives NaN for (seed 2 of a search on the CPU), and a row with an inf element: count -1 and the NaN
    entries last for the queries that evaluate them; not evaluated -- not allowed, in the query's group, at or below the id
    bound -- they fail nothing."""
    n = 700
    X, Q = _family(n, seed=4100, nq=5)
    base = np.random.default_rng(2).standard_normal(D).astype(np.float32)
    NANROW, INFROW = 300, 301
    X[NANROW] = _nan_partner(capi, base)
    Q[2] = np.random.default_rng(5).standard_normal(D)       # (no zero query here: a zero query gives 2 for an inf row too)
    Q[3] = base.astype(np.float64)
    a = _index(X)
    full = a.exact_search_batch(Q, n)
    assert full[2].tolist() == [n, n, n, -1, n] and _nan_anywhere(capi, X, Q[3]) and not _nan_anywhere(capi, X, Q[4])
    for r in (0.0, 0.5, 1.4, 2.5):
        lists, counts = _check_call(a, full, r, "nan r=%r" % r, Q=Q)
        assert counts[3] == -1 and lists[3][0][-1] == NANROW and np.isnan(lists[3][1][-1])
    # at or below the bound, not allowed, in the query's own group: not evaluated
    after = np.array([-1, -1, -1, NANROW, -1], np.int32)
    lists, counts = a.exact_radius(1.3, Q=Q, after=after)
    wi, wd = ref_radius(capi, X, Q[3], 1.3, after=NANROW)
    _same(lists, counts, 3, (wi, wd, len(wi)), "nan below the bound")
    allow = np.ones(n, bool)
    allow[NANROW] = False
    groups = np.full(n, -1, np.int32)
    groups[NANROW] = 0
    for rs, g, kw in ((a.restriction(allow, None), None, dict(allow=allow)),
                      (a.restriction(None, groups), np.array([-1, -1, -1, 0, -1], np.int32), dict(groups=groups, gq=0))):
        lists, counts = a.exact_radius(1.3, Q=Q, restriction=rs, query_groups=g)
        wi, wd = ref_radius(capi, X, Q[3], 1.3, **kw)
        _same(lists, counts, 3, (wi, wd, len(wi)), "nan not eligible")
    # a row with an inf element: NaN for every query that evaluates it
    X[INFROW, 5] = np.inf
    b = _index(X)
    full = b.exact_search_batch(Q, n)
    assert (full[2] == -1).all()
    lists, counts = _check_call(b, full, 1.2, "inf row", Q=Q)
    assert (counts == -1).all() and all(np.isnan(l[1][-1]) for l in lists)
    allow = np.ones(n, bool)
    allow[[NANROW, INFROW]] = False
    rs = b.restriction(allow, None)
    full = b.exact_search_restricted(rs, n, Q=Q)
    assert (full[2] == n - 2).all()
    _check_call(b, full, 1.2, "inf row not allowed", Q=Q, restriction=rs)
    after = np.full(5, INFROW, np.int32)
    lists, counts = b.exact_radius(1.2, Q=Q, after=after)
    for q in (0, 3):
        wi, wd = ref_radius(capi, X, Q[q], 1.2, after=INFROW)
        _same(lists, counts, q, (wi, wd, len(wi)), "inf row below the bound")


def _dump(lists, counts):
    return (counts.tobytes() + b"".join(i.tobytes() + d.tobytes() for i, d in lists))


_BATCH_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from test_gpu_radius import _family, _index, _dump
X, Q = _family(700, seed=5100, nq=33)
a = _index(X)
lists, counts = a.exact_radius(1.3, Q=Q)
st = a.exact_radius_stats()
sys.stdout.write("%%d %%d %%s\\n" %% (st["batches"], st["results"], _dump(lists, counts).hex()))
"""


def test_batch_edges_calls_and_lone_queries_give_the_same_bytes():
    X, Q = _family(700, seed=5100, nq=33)
    a = _index(X)
    lists, counts = a.exact_radius(1.3, Q=Q)
    st = a.exact_radius_stats()
    assert st["batches"] == 1
    # MORNA_RADIUS_BATCH=7 in a process of its own: five batches, the vector scan instead of the MFMA scan
    env = dict(os.environ, MORNA_RADIUS_BATCH="7")
    out = subprocess.run([sys.executable, "-c", _BATCH_SCRIPT % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    batches, results, blob = out.stdout.split()
    assert int(batches) == 5 and int(results) == st["results"]
    assert bytes.fromhex(blob) == _dump(lists, counts)
    # a second call, and every third query alone
    again = a.exact_radius(1.3, Q=Q)
    assert _dump(*again) == _dump(lists, counts)
    for q in range(0, 33, 3):
        one, c1 = a.exact_radius(1.3, Q=Q[q:q + 1])
        assert one[0][0].tobytes() == lists[q][0].tobytes() and one[0][1].tobytes() == lists[q][1].tobytes() and c1[0] == counts[q]


def _scan_eps(dim, mfma):
    """exact_scan_eps of exact.hip, restated: 4 (e_dot + e_norm + 2u + u/8)."""
    dpad = (dim + 255) // 256 * 256
    u = 2.0 ** -24
    e_dot = (128 + dpad // 128 + 8) * u if mfma else (dpad // 64 + 8) * u
    e_norm = (dpad // 64 + 8) * u
    return float(np.float32(4.0 * (e_dot + e_norm + 2 * u + u / 8)))


def test_stats_against_their_definitions():
    X, Q = _family(700, seed=6100, nq=33)
    a = _index(X)
    for nq, mfma in ((33, True), (5, False)):
        r = 1.25
        lists, counts = a.exact_radius(r, Q=Q[:nq])
        st = a.exact_radius_stats()
        assert st["queries"] == nq and st["batches"] == 1
        assert st["results"] == sum(len(i) for i, _ in lists) == int(counts.sum())
        assert st["candidates"] >= st["results"]
        w = float(np.nextafter(np.float32(r * r), np.float32(np.inf))) + _scan_eps(D, mfma)
        assert st["window"] == w
        # what is evaluated beyond the answer: every row for the zero query (query 2, outside the scan's domain: 700, none within
        # 1.25), the one row outside the domain for each of the others, and the rows inside the window but past r.  2 - 2cos of
        # normal 64-vectors has a density below 2 per unit (cos ~ N(0, 1 / 64)), so that share is under 2 eps rows per row
        eps = st["window"] - r * r
        assert 0 <= st["candidates"] - st["results"] - 700 - (nq - 1) <= 1 + 2 * eps * nq * 700
        assert st["scan_ms"] > 0 and st["select_ms"] > 0 and st["dist_ms"] > 0
    a.exact_radius(0.0, Q=Q[:0])
    st = a.exact_radius_stats()
    assert st["queries"] == 0 and st["results"] == 0 and st["scan_ms"] == 0


def test_refusals_through_the_raw_call():
    import ctypes as C
    from morna_amd import _lib
    from morna_amd._lib import lib, ptr
    from morna_amd.annoy import AnnoyIndex
    n = 300
    X, Q = _family(n, seed=7100, nq=3)
    a = _index(X)
    items = np.arange(3, dtype=np.int32)
    before = a.exact_search_batch(Q, 20)
    out = C.c_void_p()
    stats = np.ones(8)

    def call(h=a, r=None, q=None, it=items, nq=3, qg=None, after=None, radius=1.0, o=out):
        rc = lib().morna_exact_radius(h._h, r, ptr(q), ptr(it), nq, ptr(qg), ptr(after), radius, C.byref(o) if o is not None else None)
        if rc == _lib.OK:
            lib().morna_radius_free(o)
        else:
            assert o is None or o.value is None
        return rc
    assert call() == _lib.OK
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        assert call(radius=bad) == _lib.E_INVALID and b"radius" in lib().morna_last_error()
    assert lib().morna_exact_radius_stats(a._h, ptr(stats)) == _lib.OK and not stats.any()
    assert call(radius=2.0) == _lib.OK and call(radius=1e300) == _lib.OK and call(radius=0.0) == _lib.OK
    assert call(q=Q) == _lib.E_INVALID and b"not both" in lib().morna_last_error()
    assert call(it=None) == _lib.E_INVALID and b"no query source" in lib().morna_last_error()
    assert call(o=None) == _lib.E_INVALID
    Qbad = Q.copy()
    Qbad[1, 5] = np.nan
    assert call(q=Qbad, it=None) == _lib.E_INVALID and b"query 1" in lib().morna_last_error()
    assert call(it=np.array([0, n, 1], np.int32)) == _lib.E_RANGE
    qg = np.zeros(3, np.int32)
    assert call(qg=qg) == _lib.E_INVALID and b"query groups" in lib().morna_last_error()
    r_allow = a.restriction(allow=np.ones(n, bool))
    assert call(r=r_allow._p, qg=qg) == _lib.E_INVALID and b"query groups" in lib().morna_last_error()
    assert call(r=r_allow._p) == _lib.OK
    other = AnnoyIndex(D)
    other.add_items(X)
    assert call(h=other, r=r_allow._p) == _lib.E_INVALID
    # the result object's own calls
    assert lib().morna_radius_counts(None, ptr(stats)) == _lib.E_INVALID
    assert lib().morna_exact_radius_stats(a._h, None) == _lib.E_INVALID
    res = C.c_void_p()
    assert lib().morna_exact_radius(a._h, None, None, ptr(items), 3, None, None, 1.0, C.byref(res)) == _lib.OK
    pi, pd, ln = C.c_void_p(), C.c_void_p(), C.c_int64()
    assert lib().morna_radius_query(res, 3, C.byref(pi), C.byref(pd), C.byref(ln)) == _lib.E_RANGE
    assert lib().morna_radius_query(res, -1, C.byref(pi), C.byref(pd), C.byref(ln)) == _lib.E_RANGE
    assert lib().morna_radius_query(res, 0, C.byref(pi), C.byref(pd), C.byref(ln)) == _lib.OK and ln.value >= 1
    assert lib().morna_radius_free(res) == _lib.OK and lib().morna_radius_free(None) == _lib.OK
    # the exact search answers as before
    after = a.exact_search_batch(Q, 20)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    # more items on a handle with a live restriction: MORNA_E_STATE
    a.add_items(X[:10], first_id=n)
    assert call(r=r_allow._p) == _lib.E_STATE
    with pytest.raises(RuntimeError):
        a.exact_radius(1.0, items=items, restriction=r_allow)
    assert call() == _lib.OK
    # the Python surface checks shapes before the call
    with pytest.raises(ValueError):
        a.exact_radius(1.0, items=items, Q=Q)
    with pytest.raises(IndexError):
        a.exact_radius(1.0, Q=Q[:, :5])
    with pytest.raises(ValueError):
        a.exact_radius(1.0, items=items, query_groups=qg)
    with pytest.raises(ValueError):
        a.exact_radius(1.0, items=items, after=np.zeros(2, np.int32))
    with pytest.raises(ValueError):
        a.exact_radius(-0.5, items=items)


def _row_chunks(N, nb, threads=256):
    """exact_row_chunks of exact.hip, restated: the chunks of rows a query of a batch of nb is counted in."""
    chunks = max(1, min((2048 + nb - 1) // nb, (N + 2047) // 2048))
    chunk_rows = ((N + chunks - 1) // chunks + threads - 1) // threads * threads
    return (N + chunk_rows - 1) // chunk_rows


def test_more_than_64_chunk_counts_per_query():
    """135000 x 8.  A query's chunk counts (one per chunk of rows and one for the rows outside the scan's domain) are turned
    into offsets 64 at a time by one wave (radius_offsets_kernel), which carries its running sum from pass to pass: 3 queries
    have 66 + 1 counts (two passes, a tail of three), 32 and 33 queries 59 + 1 (one pass; a chunk is a multiple of 256 rows),
    and 3 queries over the first 131072 rows 64 + 1 (two passes, the second of one entry).  The yardstick is the fp64 chain
    in numpy (kmeans_ref.ref_distances), ordered by distance, then higher id first, and cut at r.  Queries 0 and 1 are rows
    131500 and 134990 plus 1e-3 of noise: their answers at every radius hold rows of the chunks 64 and 65."""
    from kmeans_ref import ref_distances
    N, dim = 135000, 8
    rng = np.random.default_rng(135000)
    X = rng.standard_normal((N, dim)).astype(np.float32)
    X[5] = 0.0                                                   # outside the scan's domain: a candidate of the last count
    Q = rng.standard_normal((33, dim))
    Q[0] = X[131500].astype(np.float64) + 1e-3 * rng.standard_normal(dim)
    Q[1] = X[134990].astype(np.float64) + 1e-3 * rng.standard_normal(dim)
    d = ref_distances(X, Q)                                      # [N, 33]
    assert not np.isnan(d).any()                                 # no query fails
    ids = np.arange(N)
    assert [_row_chunks(N, nb) + 1 for nb in (3, 32, 33)] == [67, 60, 60] and _row_chunks(131072, 3) + 1 == 65
    for n_rows, batches in ((N, (3, 32, 33)), (131072, (3,))):
        order = [np.lexsort((-ids[:n_rows], d[:n_rows, q])) for q in range(max(batches))]
        d0 = d[:n_rows, 0][order[0]]
        d20 = float(d0[19])
        assert d0[19] != d0[20]
        radii = (d20, float(np.nextafter(d20, 0.0)), float(d0[5000]))
        a = _index(X[:n_rows])
        for nq in batches:
            for r in radii:
                lists, counts = a.exact_radius(r, Q=Q[:nq])
                assert a.exact_radius_stats()["batches"] == 1
                for q in range(nq):
                    keep = order[q][:int(np.searchsorted(d[:n_rows, q][order[q]], r, side="right"))]
                    if n_rows == N and q < 2:
                        assert (keep >= 131072).any(), (q, r)    # results from the chunks 64 and 65
                    if r == radii[2] and q < 2:
                        assert len(keep) > 4096, (q, len(keep))  # past the lists the device orders
                    _same(lists, counts, q, (keep.astype(np.int32), d[:n_rows, q][keep], len(keep)),
                          "rows=%d nq=%d r=%r" % (n_rows, nq, r))
