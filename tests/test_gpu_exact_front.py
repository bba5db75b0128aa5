"""The exact family on one handle, call after call, and the refusals its three entry points share.  -m gpu

exact_search_any, label_sums and exact_radius (exact.hip) describe one workspace and keep it with the handle between calls,
together with the candidate room the last exact search needed (ex_ws, ex_cand, ex_cdist, rd_ws, lb_out, ex_cap).  The other
tests of these calls start from a fresh handle, so a pointer left stale by a regrow, or one caller's pieces overrunning
another's, would not show there.  Here every answer of a sequence of calls on one handle must equal, byte for byte, the
same call made first on a fresh handle over the same rows; the exact searches must equal the CPU oracle as well.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_exact_window import _Oracle, _check

pytestmark = pytest.mark.gpu

N, D = 2048, 24
OUTSIDE = N - 1      # the row outside the scan's domain: its fp32 squared norm underflows to 0 (below 2^-96 dpad)


@pytest.fixture(scope="module")
def capi():
    from oracle import capi as c
    c.lib()
    return c


def _rows():
    rng = np.random.default_rng(4242)
    X = rng.standard_normal((N, D)).astype(np.float32)
    items = np.linspace(3, N - 40, 40).astype(np.int32)
    # near-duplicates of the first ten query rows, so that the radius lists hold more than the row itself
    for j in range(10):
        X[1000 + 3 * j:1003 + 3 * j] = X[items[j]] * (1 + np.float32(0.02) * rng.standard_normal((3, D)).astype(np.float32))
    X[OUTSIDE] = np.float32(1e-30)
    Q = X[rng.permutation(N - 1)[:40]].astype(np.float64) + 0.05 * rng.standard_normal((40, D))
    return X, Q, items


def _index(X):
    from morna_amd.annoy import AnnoyIndex
    a = AnnoyIndex(D)
    a.add_items(X)
    return a


def _flat(answer):
    """every array of an answer, as bytes"""
    out = []
    for part in answer:
        if isinstance(part, (list, tuple)):
            out += _flat(part)
        else:
            out.append(np.asarray(part).tobytes())
    return out


def test_calls_share_one_handle(capi):
    X, Q, items = _rows()
    allow = (np.arange(N) % 5) != 0
    groups = (np.arange(N) % 7).astype(np.int32)
    q_groups = (items % 7).astype(np.int32)
    labels = (np.arange(N - 1) % 5).astype(np.int32)

    def restricted_radius(a):
        n = a.get_n_items()
        return a.exact_radius(0.6, items=items, restriction=a.restriction(allow[:n], groups[:n]), query_groups=q_groups, after=items)

    # (name, the call, for the exact searches: the queries as the oracle sees them and k)
    with_outside = [
        ("exact, 40 by vector, k 10", lambda a: a.exact_search_batch(Q, 10), Q, 10),
        ("radius, 40 by item", lambda a: a.exact_radius(0.6, items=items), None, 0),
        ("exact, 40 by item, k 300", lambda a: a.exact_search_by_item_batch(items, 300), X[items].astype(np.float64), 300),
        ("radius, restricted, after", restricted_radius, None, 0),
        ("exact, 3 by vector, k 10", lambda a: a.exact_search_batch(Q[:3], 10), Q[:3], 10),
    ]
    # label_sums refuses a row outside the domain: the same sequence with it on an index that ends before that row
    without = [
        ("exact, 40 by vector, k 10", lambda a: a.exact_search_batch(Q, 10), Q, 10),
        ("label sums, 5 by item", lambda a: a.label_sums(labels, 5, items=items[:5]), None, 0),
        ("radius, 40 by item", lambda a: a.exact_radius(0.6, items=items), None, 0),
        ("exact, 40 by item, k 300", lambda a: a.exact_search_by_item_batch(items, 300), X[items].astype(np.float64), 300),
        ("radius, restricted, after", restricted_radius, None, 0),
        ("label sums, 40 by vector", lambda a: a.label_sums(labels, 5, Q=Q), None, 0),
        ("exact, 3 by vector, k 10", lambda a: a.exact_search_batch(Q[:3], 10), Q[:3], 10),
    ]
    for rows, calls in ((X, with_outside), (X[:N - 1], without)):
        orc = _Oracle(capi, rows)
        shared = _index(rows)
        for name, call, Qo, k in calls:
            got = call(shared)
            first = call(_index(rows))
            assert _flat(got) == _flat(first), (len(rows), name)
            if Qo is not None:
                ids, d, cnt = got
                _check(orc, Qo, k, ids, d, cnt, range(len(Qo)), name)
            elif name.startswith("radius"):
                lists, counts = got
                assert max(len(ids) for ids, _ in lists) > 1, name   # (the lists are not empty: the comparison says something)


def test_refusals_of_the_three_entry_points():
    """The refusals of the common front that no other test pins, with the messages as they have always been."""
    from morna_amd import _lib
    from morna_amd._lib import lib, ptr
    from morna_amd.annoy import AnnoyIndex
    X, Q, items = _rows()
    a = _index(X)
    ids, d, cnt = np.empty((3, 4), np.int32), np.empty((3, 4), np.float64), np.empty(3, np.int32)

    def message():
        return lib().morna_last_error().decode()

    # an empty index, each call in its own words
    empty = AnnoyIndex(D)
    with pytest.raises(ValueError, match="^exact search on an empty index$"):
        empty.exact_search_batch(Q[:3], 4)
    with pytest.raises(ValueError, match="^exact search on an empty index$"):
        empty.exact_search_by_item_batch(items[:3], 4)
    with pytest.raises(ValueError, match="^label_sums on an empty index$"):
        empty.label_sums(np.zeros(0, np.int32), 5, Q=Q[:3])
    with pytest.raises(ValueError, match="^exact_radius on an empty index$"):
        empty.exact_radius(0.5, Q=Q[:3])
    assert lib().morna_exact_search(empty._h, ptr(Q), 3, 4, ptr(ids), ptr(d), ptr(cnt)) == _lib.E_EMPTY
    # k = 0, a negative k, a negative number of queries
    for nq, k in ((3, 0), (3, -1), (-1, 4)):
        assert lib().morna_exact_search(a._h, ptr(Q), nq, k, ptr(ids), ptr(d), ptr(cnt)) == _lib.E_INVALID
        assert message() == "exact search: k must be positive"
        assert lib().morna_exact_search_by_item(a._h, ptr(items), nq, k, ptr(ids), ptr(d), ptr(cnt)) == _lib.E_INVALID
        assert message() == "exact search: k must be positive"
    labels = np.zeros(N, np.int32)
    sums, counts = np.zeros((3, 5), np.uint64), np.zeros((3, 5), np.int32)
    assert lib().morna_label_sums(a._h, None, None, ptr(items), -1, None, ptr(labels), 5, ptr(sums), ptr(counts)) == _lib.E_INVALID
    assert message() == "label_sums: a negative number of queries"
    out = C.c_void_p()
    assert lib().morna_exact_radius(a._h, None, None, ptr(items), -1, None, None, 0.5, C.byref(out)) == _lib.E_INVALID
    assert message() == "exact_radius: a negative number of queries" and out.value is None
    # a query with an inf element; an item id equal to N: the exact search's words (the other two calls share them)
    Qbad = Q[:3].copy()
    Qbad[1, 7] = np.inf
    with pytest.raises(ValueError, match="^exact search: query 1 has a non-finite element or sum of squares$"):
        a.exact_search_batch(Qbad, 4)
    with pytest.raises(ValueError, match="^exact search: query 1 has a non-finite element or sum of squares$"):
        a.exact_radius(0.5, Q=Qbad)
    with pytest.raises(ValueError, match="^exact search: query 1 has a non-finite element or sum of squares$"):
        a.label_sums(labels, 5, Q=Qbad)
    at_n = np.array([0, N, 1], np.int32)
    with pytest.raises(IndexError, match=r"^Item index %d out of range \[0, %d\)$" % (N, N)):
        a.exact_search_by_item_batch(at_n, 4)
    with pytest.raises(IndexError, match=r"^Item index %d out of range \[0, %d\)$" % (N, N)):
        a.exact_radius(0.5, items=at_n)
    # label_sums with the row outside the domain (the label check comes first, the query check before this one)
    with pytest.raises(ValueError, match=r"^label_sums: row %d lies outside the domain of the scan \(its squared norm underflows, "
                                         r"overflows or is not finite\); 1 such rows$" % OUTSIDE):
        a.label_sums(labels, 5, items=items[:3])
    with pytest.raises(IndexError, match=r"^Item index %d out of range" % N):
        a.label_sums(labels, 5, items=at_n)
    # the radius range and a label equal to L, message and all
    for bad, text in ((-0.5, "-0.5"), (float("nan"), "nan")):
        with pytest.raises(ValueError, match="^exact_radius: the radius %s is not a finite number >= 0$" % text):
            a.exact_radius(bad, items=items[:3])
    labels[17] = 5
    with pytest.raises(ValueError, match=r"^label_sums: item 17 has the label 5, outside \[-1, 5\)$"):
        a.label_sums(labels, 5, items=items[:3])
    # after the refusals the handle answers as a fresh one does
    assert _flat(a.exact_search_batch(Q[:3], 4)) == _flat(_index(X).exact_search_batch(Q[:3], 4))
