"""morna_label_sums on the GPU (include/morna_hip.h, "label distance sums").  -m gpu

The core tests have no tolerance.  Rows with small-integer entries (|x| <= 8, dim <= 64) make every fp32 dot and norm of the
scan an exact integer, so the scan value is exactly float32(2 - 2 pq / sqrt(pp qq)) (2 where pp qq is 0) on either scan
kernel, and sums[q][g] is exactly the integer sum of floor(sqrt(float64(max(v, 0))) * 2^32 + 0.5) over the counted rows.
`scan_values` restates that arithmetic once for every query form: the query's fp32 image is the query times a power of two
(the scan's scaling, which cancels exactly), and for the staged query rows -- real numbers, one non-zero cell each -- every
product and square is one value rounded once, whatever the order of summation.  Real-valued rows are checked against fp64
numpy with the bound derived from the scan's own error bound.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 64
ONE = 2.0 ** 32
U = 2.0 ** -24


def scan_eps_half(dim, mfma):
    """exact_scan_eps / 2 of DESIGN.md: 2 (e_dot + e_norm + 2u + u/8) rounded as the float32 the library keeps."""
    dpad = (dim + 255) // 256 * 256
    e_dot = (128 + dpad // 128 + 8) * U if mfma else (dpad // 64 + 8) * U
    e_norm = (dpad // 64 + 8) * U
    return float(np.float32(2.0 * 2.0 * (e_dot + e_norm + 2 * U + U / 8))) / 2.0


def integer_rows(n, d, seed):
    """Integer rows in [-8, 8] with, at fixed places: one-hot rows (scan values exactly 0 or 2 among them), scaled copies,
    duplicates and a zero row."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    for i, (c, s) in enumerate([(0, 1), (0, 4), (1, -2), (1, 8), (2, 1), (0, -1)]):
        X[i] = 0
        X[i, c] = s                       # rows 0..5 one-hot: 0/1/5 parallel or opposite, 2/3 opposite, 4 orthogonal to them
    X[6] = 0                              # the zero row
    X[7] = np.clip(X[8], -4, 4)
    X[8] = X[7] * 2                       # a scaled copy
    X[9] = X[7]
    X[10] = X[7]                          # duplicates
    X[n - 1] = X[7] * -1                  # the last row: the opposite direction
    return X


def scan_values(X, Q):
    """float32 [nq, n]: the value the scan writes, for rows and queries whose fp32 arithmetic is exact or rounded once."""
    X64, Q = X.astype(np.float64), np.asarray(Q, np.float64)
    mx = np.abs(Q).max(axis=1)
    e = np.frexp(mx)[1]
    img = np.where(mx[:, None] > 0, np.ldexp(Q, (1 - e)[:, None]), 0.0).astype(np.float32).astype(np.float64)
    assert (np.count_nonzero(Q, axis=1) <= 1).all() or (img == np.ldexp(Q, (1 - e)[:, None])).all()
    pq = (img @ X64.T).astype(np.float32).astype(np.float64)
    qq = (img * img).sum(axis=1).astype(np.float32).astype(np.float64)
    pp = (X64 * X64).sum(axis=1)
    assert (pp < 2 ** 24).all() and (pp == np.floor(pp)).all()
    ppqq = qq[:, None] * pp[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ppqq > 0, np.float32(2.0 - 2.0 * pq / np.sqrt(ppqq)), np.float32(2.0)).astype(np.float32)


def fixed_point(v):
    return np.floor(np.sqrt(np.maximum(v, np.float32(0)).astype(np.float64)) * ONE + 0.5).astype(np.uint64)


def reference(v, labels, L, eligible=None, self_items=None):
    """(sums uint64 [nq, L], counts int32 [nq, L]) from scan values v [nq, n]: the contract, row by row."""
    nq, n = v.shape
    Dm = fixed_point(v)
    sums, counts = np.zeros((nq, L), np.uint64), np.zeros((nq, L), np.int32)
    for q in range(nq):
        counted = labels >= 0
        if eligible is not None:
            counted = counted & eligible[q]
        if self_items is not None:
            counted = counted.copy()
            counted[self_items[q]] = False
        np.add.at(sums[q], labels[counted], Dm[q][counted])
        np.add.at(counts[q], labels[counted], 1)
    return sums, counts


def make_labels(n, L, seed, lone=None):
    """int32 [n] in [-1, L): about one row in L + 1 unlabelled; with three labels or more label 1 is empty; with two or more
    the only member of label L - 1 is row `lone` (a query)."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(-1, L, size=n).astype(np.int32)
    if L >= 3:
        lab[lab == 1] = 0
    if L >= 2 and lone is not None:
        lab[lab == L - 1] = -1
        lab[lone] = L - 1
    return lab


_MADE = {}


def index_of(n, d=D, seed=5):
    """An AnnoyIndex of integer_rows(n, d), its rows, made once per module run."""
    from morna_amd.annoy import AnnoyIndex
    key = (n, d, seed)
    if key not in _MADE:
        X = integer_rows(n, d, seed)
        a = AnnoyIndex(d)
        a.add_items(X)
        _MADE[key] = (a, X)
    return _MADE[key]


def query_items(n, nq, seed=3):
    """nq distinct rows as queries: the special rows first (one-hot, zero, copies, the last row), then random ones."""
    special = [0, 1, 2, 4, 6, 7, 8, 9, n - 1]
    rng = np.random.default_rng(seed)
    rest = [int(i) for i in rng.permutation(n) if i not in special]
    return np.array((special + rest)[:nq] if nq >= 3 else ([7] + special)[:nq], np.int32)


@pytest.mark.parametrize("nq", [1, 3, 31, 32, 33, 200])
@pytest.mark.parametrize("n", [700, 8200])
def test_by_item_is_bit_exact(n, nq):
    """Both scans (the vector scan below 32 queries, the MFMA scan from 32), L = 1, 2, 64, 4096, an empty label, a label whose
    only member is the query, unlabelled rows; the row counts are no multiple of 128."""
    a, X = index_of(n)
    items = query_items(n, nq)
    v = scan_values(X, X[items])
    # the oracle is the formula of the contract, literally, for these integer queries
    X64 = X.astype(np.float64)
    pp = (X64 * X64).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        lit = np.where(pp[items][:, None] * pp[None, :] > 0,
                       np.float32(2.0 - 2.0 * (X64[items] @ X64.T) / np.sqrt(pp[None, :] * pp[items][:, None])), np.float32(2.0))
    assert (v == lit.astype(np.float32)).all()
    assert (v[:, 6] == 2).all() and (v == 0).any() and (v == 4).any()
    for L in (1, 2, 64, 4096):
        labels = make_labels(n, L, seed=L, lone=int(items[0]))
        sums, counts = a.label_sums(labels, L, items=items)
        want_s, want_c = reference(v, labels, L, self_items=items)
        assert sums.dtype == np.uint64 and counts.dtype == np.int32 and sums.shape == (nq, L)
        assert (counts == want_c).all(), (n, nq, L)
        assert (sums == want_s).all(), (n, nq, L)
        if L >= 2:
            assert counts[0, L - 1] == 0 and sums[0, L - 1] == 0          # its only member is query 0 itself
            assert nq == 1 or (counts[1:, L - 1] == 1).all()
        if L >= 3:
            assert (counts[:, 1] == 0).all() and (sums[:, 1] == 0).all()   # the empty label
        stats = a.label_sums_stats()
        assert stats["queries"] == nq and stats["batches"] == 1 and stats["counted"] == int(want_c.sum())
        assert stats["scan_eps"] == scan_eps_half(D, nq >= 32) and stats["scan_ms"] > 0 and stats["sums_ms"] > 0


def _stage_single_cell_rows(a, nq, seed):
    """nq query rows through morna_build_query_rows, one junction -- so one non-zero cell -- each; returns the fp64 rows."""
    from morna_amd.index import ParsedLines, pack_vocab
    rng = np.random.default_rng(seed)
    keys = [("chr%d %d %d" % (1 + j % 20, 1000 + 7 * j, 2000 + 11 * j)).encode() for j in range(nq)]
    freq = {k.decode(): int(rng.integers(1, 60)) for k in keys}
    key_off = np.zeros(nq + 1, np.int64)
    np.cumsum([len(k) for k in keys], out=key_off[1:])
    prep = dict(key_bytes=np.frombuffer(b"".join(keys), np.uint8), key_off=key_off, row_ptr=np.arange(nq + 1, dtype=np.int64),
                ids=np.arange(nq, dtype=np.int64), cov=rng.integers(1, 200, nq), idf=np.zeros(nq),
                ext_ids=np.arange(nq, dtype=np.int64))
    a.build_query_rows(ParsedLines.from_arrays(prep, 100).query_terms(pack_vocab(freq), 100))
    r64, _ = a.get_query_rows()
    assert r64.shape == (nq, a.f) and (np.count_nonzero(r64, axis=1) == 1).all()
    return r64


@pytest.mark.parametrize("nq", [5, 33])
def test_by_vector_and_staged_rows_are_bit_exact(nq):
    """The three query forms against the same oracle: by vector nothing is skipped (the queries are rows of the index and
    integer vectors that are not), and the staged query rows of morna_build_query_rows."""
    n = 700
    a, X = index_of(n)
    items = query_items(n, nq)
    L = 5
    labels = make_labels(n, L, seed=11, lone=int(items[0]))
    rng = np.random.default_rng(17)
    Q = np.concatenate([X[items[:nq // 2]].astype(np.float64), rng.integers(-8, 9, size=(nq - nq // 2, D)).astype(np.float64)])
    Q[-1] = 0.0                                                # a zero query: every value is 2
    v = scan_values(X, Q)
    sums, counts = a.label_sums(labels, L, Q=Q)
    want_s, want_c = reference(v, labels, L)
    assert (counts == want_c).all() and (sums == want_s).all()
    assert counts[0, L - 1] == 1                               # by vector the row equal to the query is counted
    assert (sums[-1] == want_c[-1].astype(np.uint64) * np.uint64(fixed_point(np.float32(2.0)))).all()
    # by item the same rows, the query itself skipped
    by_item = a.label_sums(labels, L, items=items[:nq // 2])
    want_i = reference(v[:nq // 2], labels, L, self_items=items[:nq // 2])
    assert (by_item[0] == want_i[0]).all() and (by_item[1] == want_i[1]).all()
    # the staged rows
    r64 = _stage_single_cell_rows(a, nq, seed=23)
    vs = scan_values(X, r64)
    got = a.label_sums(labels, L)
    want = reference(vs, labels, L)
    assert (got[1] == want[1]).all() and (got[0] == want[0]).all()
    again = a.label_sums(labels, L, Q=r64)                     # the same rows from the host: the same bytes
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


GROUP_SIZES = (1, 2, 40)


def _groups(rng, n, items):
    """int32 [n]: GROUP_SIZES[g] rows of group g, the first member of each a query; the others -1."""
    g = np.full(n, -1, np.int32)
    free = [int(i) for i in rng.permutation(n) if i not in items[:3]]
    at = 0
    for label, size in enumerate(GROUP_SIZES):
        g[items[label]] = label
        g[free[at:at + size - 1]] = label
        at += size - 1
    return g


@pytest.mark.parametrize("nq", [3, 33])
@pytest.mark.parametrize("n", [700, 3005])
def test_restrictions_are_bit_exact(n, nq):
    """Allow-lists of half, 5, 0 and all rows; groups of 1, 2 and 40 with q_group; 3005 rows reach into the bitmap's last
    word (its last row is allowed or not with the list)."""
    a, X = index_of(n)
    items = query_items(n, nq)
    L = 3
    labels = make_labels(n, L, seed=29, lone=int(items[0]))
    labels[n - 1] = 0
    v = scan_values(X, X[items])
    rng = np.random.default_rng(31)
    half = rng.random(n) < 0.5
    half[n - 1] = True
    other_half = ~half
    five = np.zeros(n, bool)
    five[rng.choice(n, size=5, replace=False)] = True
    groups = _groups(rng, n, items)
    qg = np.array([(-1, 0, 1, 2)[(q + 1) % 4] for q in range(nq)], np.int32)      # queries 0, 1, 2 carry their own groups
    own = groups[items]
    seen = set()
    for name, allow, grp, q_group in (("half", half, None, None), ("other half", other_half, None, None), ("five", five, None, None),
                                      ("none", np.zeros(n, bool), None, None), ("all", np.ones(n, bool), None, None),
                                      ("groups", None, groups, qg), ("groups, own", None, groups, own),
                                      ("half + groups", half, groups, qg), ("groups, no query group", None, groups, None)):
        r = a.restriction(allow=allow, groups=grp)
        eligible = np.ones((nq, n), bool) if allow is None else np.tile(allow, (nq, 1))
        if grp is not None and q_group is not None:
            for q in range(nq):
                if q_group[q] >= 0:
                    eligible[q] &= grp != q_group[q]
        sums, counts = a.label_sums(labels, L, items=items, restriction=r, query_groups=q_group)
        want_s, want_c = reference(v, labels, L, eligible=eligible, self_items=items)
        assert (counts == want_c).all() and (sums == want_s).all(), (name, n, nq)
        seen.add(counts.tobytes())
        if name == "none":
            assert not counts.any() and not sums.any()
        if name == "all":
            plain = a.label_sums(labels, L, items=items)
            assert plain[0].tobytes() == sums.tobytes() and plain[1].tobytes() == counts.tobytes()
    assert len(seen) >= 6                                     # the cases differ


def test_two_calls_a_relabelling_and_the_exact_search_around_it():
    n, nq, L = 8200, 40, 64
    a, X = index_of(n)
    items = query_items(n, nq)
    labels = make_labels(n, L, seed=37)
    before = a.exact_search_by_item_batch(items, 10)
    first = a.label_sums(labels, L, items=items)
    second = a.label_sums(labels, L, items=items)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    after = a.exact_search_by_item_batch(items, 10)
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    # relabelling by a permutation permutes the columns, byte for byte
    perm = np.random.default_rng(41).permutation(L).astype(np.int32)
    relabelled = np.where(labels >= 0, perm[np.maximum(labels, 0)], -1).astype(np.int32)
    third = a.label_sums(relabelled, L, items=items)
    assert third[0][:, perm].tobytes() == first[0].tobytes() and third[1][:, perm].tobytes() == first[1].tobytes()
    assert third[0].tobytes() != first[0].tobytes()
    # one query takes the vector scan and the (query, row chunk) grid, forty the MFMA scan and fewer chunks: on integer rows
    # both scans are exact, so the query they share has the same bytes
    one = a.label_sums(labels, L, items=items[:1])
    assert one[0].tobytes() == first[0][:1].tobytes() and one[1].tobytes() == first[1][:1].tobytes()
    v = scan_values(X, X[items[:1]])
    want = reference(v, labels, L, self_items=items[:1])
    assert (one[0] == want[0]).all() and (one[1] == want[1]).all()


def test_batch_edge_two_internal_batches():
    """524 320 rows of 8 integers, 1100 by-item queries: scan values of at most 2 GiB make two batches, of 1023 and 77.  The rows
    repeat 256 distinct ones, so the oracle is the contract over (query, distinct row) weighted by how often each distinct row
    carries each label -- the same integers."""
    from morna_amd.annoy import AnnoyIndex
    n, d, nq, L = 524320, 8, 1100, 3
    rng = np.random.default_rng(43)
    base = integer_rows(256, d, 47)
    which = rng.integers(0, 256, size=n)
    X = base[which]
    labels = rng.integers(-1, L, size=n).astype(np.int32)
    items = rng.choice(n, size=nq, replace=False).astype(np.int32)
    a = AnnoyIndex(d)
    a.add_items(X)
    sums, counts = a.label_sums(labels, L, items=items)
    stats = a.label_sums_stats()
    assert stats["batches"] == 2 and stats["queries"] == nq and stats["scan_eps"] == scan_eps_half(d, True)
    Dm = fixed_point(scan_values(base, X[items]))                       # [nq, 256]
    per = np.zeros((256, L), np.int64)
    np.add.at(per, (which[labels >= 0], labels[labels >= 0]), 1)
    want_s = Dm.astype(object).dot(per.astype(object))                  # Python integers: no rounding, no overflow
    want_c = np.tile(per.sum(axis=0), (nq, 1))
    for q in range(nq):                                                 # the query itself is not counted
        g = labels[items[q]]
        if g >= 0:
            want_s[q, g] -= int(Dm[q, which[items[q]]])
            want_c[q, g] -= 1
    assert (counts == want_c).all()
    assert (sums.astype(object) == want_s).all()
    assert stats["counted"] == int(want_c.sum())


@pytest.mark.parametrize("n,d", [(3000, 64), (700, 1100)])
def test_real_valued_rows_within_the_derived_bound(n, d):
    """Normal rows against fp64 numpy.  e is the scan's bound on |v - (2 - 2cos)| restated from DESIGN.md and asserted equal
    to what the statistics report; a sum of m terms then lies within sum [sqrt(max(v + e, 0)) - sqrt(max(v - e, 0))] of the
    reference, plus the quantisation m 2^-32 (2^-33 per term, and one unit for the reference's own rounding), plus 1e-9."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(53)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[3] = X[4] * np.float32(3.0)                            # a parallel pair: v near 0, where sqrt is steepest
    X[5] = 0.0
    a = AnnoyIndex(d)
    a.add_items(X)
    L = 7
    labels = make_labels(n, L, seed=59)
    X64 = X.astype(np.float64)
    norm = np.sqrt((X64 * X64).sum(axis=1))
    for nq in (5, 40):                                       # the vector scan, the MFMA scan
        items = np.concatenate([[3, 4, 5], rng.choice(np.arange(6, n), size=nq - 3, replace=False)]).astype(np.int32)
        sums, counts = a.label_sums(labels, L, items=items)
        e = scan_eps_half(d, nq >= 32)
        assert a.label_sums_stats()["scan_eps"] == e
        ppqq = norm[items][:, None] * norm[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            v_ref = np.where(ppqq > 0, 2.0 - 2.0 * (X64[items] @ X64.T) / ppqq, 2.0)
        for q in range(nq):
            counted = labels >= 0
            counted[items[q]] = False
            for g in range(L):
                rows = counted & (labels == g)
                ref = np.sqrt(np.maximum(v_ref[q, rows], 0.0)).sum()
                bound = (np.sqrt(np.maximum(v_ref[q, rows] + e, 0.0)) - np.sqrt(np.maximum(v_ref[q, rows] - e, 0.0))).sum() \
                    + rows.sum() * 2.0 ** -32 + 1e-9
                assert counts[q, g] == rows.sum()
                err = abs(int(sums[q, g]) / ONE - ref)
                assert err <= bound, (n, d, nq, q, g, err, bound)


def test_refusals_through_the_raw_call():
    from morna_amd import _lib
    from morna_amd._lib import lib, ptr
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(61)
    n, L = 300, 4
    X = rng.integers(-8, 9, size=(n, D)).astype(np.float32)
    a = AnnoyIndex(D)
    a.add_items(X)
    labels = make_labels(n, L, seed=67)
    items = np.arange(3, dtype=np.int32)
    Q = X[:3].astype(np.float64)
    sums, counts = np.zeros((3, 4100), np.uint64), np.zeros((3, 4100), np.int32)
    stats = np.ones(6)

    def call(h=a, r=None, q=None, it=items, nq=3, qg=None, lab=labels, nl=L):
        return lib().morna_label_sums(h._h, r, ptr(q), ptr(it), nq, ptr(qg), ptr(lab), nl, ptr(sums), ptr(counts))
    assert call() == _lib.OK
    # a label out of range, either way; L = 0 and L = 4097
    bad = labels.copy()
    bad[17] = L
    assert call(lab=bad) == _lib.E_INVALID and b"item 17" in lib().morna_last_error()
    bad[17] = -2
    assert call(lab=bad) == _lib.E_INVALID and b"item 17" in lib().morna_last_error()
    assert call(nl=0) == _lib.E_INVALID and b"0 labels" in lib().morna_last_error()
    assert call(nl=4097) == _lib.E_INVALID and b"4097 labels" in lib().morna_last_error()
    assert call(nl=4096, lab=labels) == _lib.OK
    # both query sources, and none (no query rows are staged)
    assert call(q=Q) == _lib.E_INVALID and b"not both" in lib().morna_last_error()
    assert call(it=None) == _lib.E_INVALID and b"no query source" in lib().morna_last_error()
    # after a refusal the statistics say nothing ran
    assert lib().morna_label_sums_stats(a._h, ptr(stats)) == _lib.OK and not stats.any()
    # a non-finite host query, an item outside the index
    Qbad = Q.copy()
    Qbad[1, 5] = np.inf
    assert call(q=Qbad, it=None) == _lib.E_INVALID and b"query 1" in lib().morna_last_error()
    assert call(it=np.array([0, n, 1], np.int32)) == _lib.E_RANGE
    # query groups without a restriction, and with one made without groups
    qg = np.zeros(3, np.int32)
    assert call(qg=qg) == _lib.E_INVALID and b"query groups" in lib().morna_last_error()
    r_allow = a.restriction(allow=np.ones(n, bool))
    assert call(r=r_allow._p, qg=qg) == _lib.E_INVALID and b"query groups" in lib().morna_last_error()
    assert call(r=r_allow._p) == _lib.OK
    # a restriction of another handle; a stale one
    other = AnnoyIndex(D)
    other.add_items(X)
    assert call(h=other, r=r_allow._p) == _lib.E_INVALID
    with pytest.raises(ValueError):
        other.label_sums(labels, L, items=items, restriction=r_allow)
    # a row outside the scan's domain: the call names the first
    tiny = AnnoyIndex(D)
    Xt = X.copy()
    Xt[40] = np.float32(1e-30)
    Xt[12] = np.float32(1e-30)
    tiny.add_items(Xt)
    assert call(h=tiny) == _lib.E_INVALID and b"row 12 " in lib().morna_last_error()
    with pytest.raises(ValueError, match="row 12 "):
        tiny.label_sums(labels, L, items=items)
    # more items on a handle with a live restriction: MORNA_E_STATE until it is made again
    a.add_items(X[:10], first_id=n)
    grown = np.concatenate([labels, labels[:10]])
    assert call(r=r_allow._p, lab=grown) == _lib.E_STATE
    with pytest.raises(RuntimeError):
        a.label_sums(grown, L, items=items, restriction=r_allow)
    assert call(lab=grown) == _lib.OK
    # the Python surface checks shapes before the call
    with pytest.raises(ValueError):
        a.label_sums(labels, L, items=items)                 # one label per item: 300 for 310 items
    with pytest.raises(ValueError):
        a.label_sums(grown, L, items=items, Q=Q)
    with pytest.raises(IndexError):
        a.label_sums(grown, L, Q=Q[:, :5])
    with pytest.raises(ValueError):
        a.label_sums(grown, L, items=items, query_groups=qg)
