"""Restricted search on the GPU: allow-lists and leave-out groups (include/morna_hip.h, "restricted search").  -m gpu

Exact: the oracle is a second AnnoyIndex that holds only the eligible rows (one per distinct g_q), ids mapped back; ids,
the fp64 distances as bytes and the counts are compared.  Approximate: the oracle is the unrestricted call with k' = n and the
same explicit search_k, filtered to the eligible items and cut to k on the host.  Rows are seeded numpy normals through
AnnoyIndex.add_items.  Every case is named by the code path it reaches: the register / strided / two-pass selection and the
vector / matrix-core scan of the exact search; the spread, batch, fused and dense forms and the LDS / global bitmap of the
approximate one.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 64
GROUP_SIZES = (1, 2, 40)        # group g holds GROUP_SIZES[g] items
Q_GROUPS = (-1, 0, 1, 2)        # the labels the queries carry, in turn: at most 4 distinct g_q


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


def _groups(rng, n):
    """int32 labels [n]: GROUP_SIZES[g] items of label g, the others -1."""
    g = np.full(n, -1, np.int32)
    members = rng.choice(n, size=sum(GROUP_SIZES), replace=False)
    at = 0
    for label, size in enumerate(GROUP_SIZES):
        g[members[at:at + size]] = label
        at += size
    return g


def _query_groups(nq):
    return np.array([Q_GROUPS[q % len(Q_GROUPS)] for q in range(nq)], np.int32)


def _eligible(n, allow, groups, gq):
    e = np.ones(n, bool) if allow is None else allow.copy()
    if groups is not None and gq >= 0:
        e &= groups != gq
    return e


def _cases(rng, n, keep=(), drop=()):
    """(name, allow or None, groups or None) -- about half the rows, 5 rows, no row, all rows, and the half allow-list
    with the groups; `keep` are allowed and `drop` are not in the half lists."""
    half = rng.random(n) < 0.5
    half[list(keep)] = True
    half[list(drop)] = False
    five = np.zeros(n, bool)
    five[rng.choice(n, size=min(5, n), replace=False)] = True
    return [("half", half, None), ("five", five, None), ("none", np.zeros(n, bool), None), ("all", np.ones(n, bool), None),
            ("half+groups", half, _groups(rng, n)), ("groups", None, _groups(rng, n))]


def _stage_rows(a, nq, seed):
    """nq query rows staged on the handle through morna_build_query_rows (a small made-up vocabulary); returns the fp64
    rows and their fp32 image."""
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
    r64, r32 = a.get_query_rows()
    assert r64.shape == (nq, a.f) and r64.any(axis=1).all()
    return r64, r32


# ------------------------------------------------------------------------------------------------------------ exact

def _exact_matrix(n, seed):
    """Normal rows, and: a zero row and a row outside the scan's domain each once allowed (`keep`) and once not (`drop`)
    by the half lists, and -- not allowed -- a scaled copy of the 20th nearest allowed row of query 0: a row inside the
    window of the 20th eligible scan value.  Returns X, the vector queries, keep, drop."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D)).astype(np.float32)
    Q = rng.standard_normal((33, D))
    zero_in, zero_out, small_in, big_out, copy_out = 11, 12, 13, 14, 15
    X[zero_in] = 0.0
    X[zero_out] = 0.0
    X[small_in] *= np.float32(2.0 ** -90)      # fp32 norm2 below the domain
    X[big_out] *= np.float32(2.0 ** 100)       # fp32 norm2 overflows
    return X, Q, (zero_in, small_in), (zero_out, big_out, copy_out)


def _plant_window_row(X, Q, half, row):
    """X[row] = 2 * (the 20th nearest row of query 0 among the rows `half` allows): the same cosine, so its scan value is
    within the window of the 20th eligible one."""
    X64 = X.astype(np.float64)
    with np.errstate(all="ignore"):
        cos = (X64 @ Q[0]) / (np.linalg.norm(X64, axis=1) * np.linalg.norm(Q[0]))
    cos[~half] = -np.inf
    cos[~np.isfinite(cos)] = -np.inf
    kth = int(np.argsort(-cos)[19])
    X[row] = X[kth] * np.float32(2.0)
    return kth


class _Subsets(object):
    """The oracle: an AnnoyIndex of the eligible rows per (case, g_q), made on first use."""

    def __init__(self, X):
        self.X, self.made = X, {}

    def get(self, name, allow, groups, gq):
        from morna_amd.annoy import AnnoyIndex
        key = (name, gq if groups is not None else -1)
        if key not in self.made:
            at = np.nonzero(_eligible(len(self.X), allow, groups, gq))[0]
            sub = None
            if len(at):
                sub = AnnoyIndex(D)
                sub.add_items(self.X[at])
            self.made[key] = (sub, at)
        return self.made[key]


def _exact_expected(subsets, name, allow, groups, qg, k, Q=None, rows=None):
    """Per query: the subset index's answer to the same query (fp64 vector, or the fp32 row widened), ids mapped back."""
    nq = len(qg)
    ids = np.full((nq, k), -1, np.int32)
    d = np.full((nq, k), np.inf)
    cnt = np.zeros(nq, np.int32)
    Qv = Q if Q is not None else rows.astype(np.float64)
    for gq in sorted(set(qg.tolist())):
        sub, at = subsets.get(name, allow, groups, gq)
        sel = np.nonzero(qg == gq)[0]
        if sub is None:
            continue
        si, sd, sc = sub.exact_search_batch(Qv[sel], k)
        ids[sel] = np.where(si >= 0, at[np.clip(si, 0, len(at) - 1)], -1)
        d[sel], cnt[sel] = sd, sc
    return ids, d, cnt


def _same(got, want, label):
    assert got[2].tolist() == want[2].tolist(), (label, got[2].tolist(), want[2].tolist())
    assert got[0].tolist() == want[0].tolist(), label
    assert got[1].tobytes() == want[1].tobytes(), label


def _exact_shape(n, nq, select2):
    from morna_amd.annoy import AnnoyIndex
    X, Qall, keep, drop = _exact_matrix(n, 1000 + n)
    rng = np.random.default_rng(n + nq)
    cases = _cases(rng, n, keep, drop)
    kth = _plant_window_row(X, Qall, cases[0][1], drop[2])
    a = AnnoyIndex(D)
    a.add_items(X)
    subsets = _Subsets(X)
    Q = Qall[:nq]
    items = rng.choice(n, size=nq, replace=False).astype(np.int32)
    items[0] = keep[0] if nq > 3 else items[0]         # (a zero row as the query: every row ties at sqrt(2))
    r64, _ = _stage_rows(a, nq, n)
    qg_all = _query_groups(nq)

    def run():
        unrestricted = a.exact_search_batch(Q, 20)
        assert (unrestricted[2] == 20).all()
        for name, allow, groups in cases:
            r = a.restriction(allow, groups)
            qg = qg_all if groups is not None else None
            want_g = qg_all if groups is not None else np.full(nq, -1, np.int32)
            n_elig = int(_eligible(n, allow, groups, -1).sum())
            for k in (1, 20, 300):
                label = "exact/n%d/nq%d/%s/k%d" % (n, nq, name, k)
                got = a.exact_search_restricted(r, k, Q=Q, query_groups=qg)
                _same(got, _exact_expected(subsets, name, allow, groups, want_g, k, Q=Q), label + "/vector")
                if groups is None:
                    assert (got[2] == min(k, n_elig)).all(), label
                if name == "all":
                    _same(got, a.exact_search_batch(Q, k), label + "/unrestricted")
                if name == "half" and k == 20:   # the planted copy is in the window of query 0's 20th value, and not allowed
                    assert drop[2] not in got[0][0].tolist() and kth in got[0][0].tolist(), label
                got = a.exact_search_restricted(r, k, items=items, query_groups=qg)
                _same(got, _exact_expected(subsets, name, allow, groups, want_g, k, rows=X[items]), label + "/item")
                got = a.exact_search_restricted(r, k, query_groups=qg)
                _same(got, _exact_expected(subsets, name, allow, groups, want_g, k, Q=r64), label + "/staged")
    if select2:
        run()
    else:
        _with_env("MORNA_EXACT_SELECT2", "0", run)


@pytest.mark.parametrize("nq", [3, 33], ids=["vector_scan", "mfma_scan"])
@pytest.mark.parametrize("n,select2", [(700, True), (8200, True), (8200, False)],
                         ids=["register_form", "two_pass_form", "strided_form"])
def test_exact_equals_the_index_of_the_eligible_rows(n, select2, nq):
    _exact_shape(n, nq, select2)


@pytest.mark.parametrize("n", [700, 8200], ids=["register_form", "two_pass_form"])
def test_exact_count_minus_one_only_for_an_eligible_row(n):
    """A row with an inf element: cosine_distance is NaN for it, so the unrestricted search reports count -1 for every
    query (tests/test_gpu_exact_window.py).  Not eligible: the restricted counts are not -1; eligible: they are, as on the
    index of the eligible rows."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(77 + n)
    X = rng.standard_normal((n, D)).astype(np.float32)
    bad = n // 3
    X[bad, 7] = np.inf
    a = AnnoyIndex(D)
    a.add_items(X)
    subsets = _Subsets(X)
    groups = _groups(rng, n)
    groups[bad] = 2 if groups[bad] < 0 else groups[bad]
    for nq in (3, 33):
        Q = rng.standard_normal((nq, D))
        assert (a.exact_search_batch(Q, 5)[2] == -1).all()
        without = rng.random(n) < 0.5
        without[bad] = False
        within = without.copy()
        within[bad] = True
        qg = np.where(np.arange(nq) % 2 == 0, groups[bad], -1).astype(np.int32)
        for name, allow, grp, q_groups in (("without", without, None, None), ("within", within, None, None),
                                           ("own_group", None, groups, qg)):
            r = a.restriction(allow, grp)
            want_g = q_groups if q_groups is not None else np.full(nq, -1, np.int32)
            for k in (1, 20):
                got = a.exact_search_restricted(r, k, Q=Q, query_groups=q_groups)
                label = "minus_one/n%d/nq%d/%s/k%d" % (n, nq, name, k)
                if name == "without":
                    assert (got[2] == k).all(), label
                elif name == "within":
                    assert (got[2] == -1).all(), label
                else:
                    assert got[2].tolist() == [k if g == groups[bad] else -1 for g in qg.tolist()], label
                want = _exact_expected(subsets, "%s/nq%d" % (name, nq), allow, grp, want_g, k, Q=Q)   # (the lists are per nq)
                assert got[2].tolist() == want[2].tolist(), label
                ok = got[2] >= 0        # (the lists of a count -1 are for diagnosis only)
                assert got[0][ok].tolist() == want[0][ok].tolist() and got[1][ok].tobytes() == want[1][ok].tobytes(), label


# ------------------------------------------------------------------------------------------------------ approximate

_INDEXES = {}


def _approx_index(n, dim, trees):
    from morna_amd.annoy import AnnoyIndex
    key = (n, dim, trees)
    if key not in _INDEXES:
        rng = np.random.default_rng(n * 31 + dim)
        X = rng.standard_normal((n, dim)).astype(np.float32)
        a = AnnoyIndex(dim)
        a.add_items(X)
        a.build(trees, seed=5)
        _INDEXES[key] = (a, X)
    return _INDEXES[key]


def _approx_expected(full, n, allow, groups, qg, k):
    """The unrestricted answer with k' = n, filtered to the eligible items and cut to k."""
    fi, fd, fc = full
    nq = len(fc)
    ids = np.full((nq, k), -1, np.int32)
    d = np.full((nq, k), np.inf, np.float32)
    cnt = np.zeros(nq, np.int32)
    for q in range(nq):
        e = _eligible(n, allow, groups, int(qg[q]))
        lst = fi[q, :fc[q]]
        keep = np.nonzero(e[lst])[0][:k]
        ids[q, :len(keep)], d[q, :len(keep)], cnt[q] = lst[keep], fd[q, :fc[q]][keep], len(keep)
    return ids, d, cnt


def _approx_check(a, X, nq, search_k, ks, cases, seed, staged=True, label=""):
    n = len(X)
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nq, X.shape[1])).astype(np.float32)
    items = rng.choice(n, size=nq, replace=nq > n).astype(np.int32)
    sources = [("vector", dict(Q=Q), a.get_nns_by_vector_batch(Q, n, search_k)),
               ("item", dict(items=items), a.get_nns_by_item_batch(items, n, search_k))]
    if staged:
        _, r32 = _stage_rows(a, nq, seed)
        sources.append(("staged", dict(), a.get_nns_by_vector_batch(r32, n, search_k)))
    qg_all = _query_groups(nq)
    for name, allow, groups in cases:
        r = a.restriction(allow, groups)
        qg = qg_all if groups is not None else None
        want_g = qg_all if groups is not None else np.full(nq, -1, np.int32)
        for k in ks:
            for src, kw, full in sources:
                got = a.get_nns_restricted(r, k, search_k, query_groups=qg, **kw)
                want = _approx_expected(full, n, allow, groups, want_g, k)
                _same(got, want, "approx/%s/n%d/nq%d/sk%d/%s/k%d/%s" % (label, n, nq, search_k, name, k, src))
                if name == "none":
                    assert (got[2] == 0).all()
        if name == "all":
            for src, kw, full in sources[:2]:
                plain = (a.get_nns_by_vector_batch(Q, 20, search_k) if src == "vector"
                         else a.get_nns_by_item_batch(items, 20, search_k))
                _same(a.get_nns_restricted(r, 20, search_k, **kw), plain, "approx/%s/all_equals_unrestricted/%s" % (label, src))


@pytest.mark.parametrize("nq,search_k", [(1, 10), (1, 2000), (5, 10), (5, 2000), (70, 2000), (200, 2000)],
                         ids=["spread1_first_leaf_ends", "spread1", "spread5_first_leaf_ends", "spread5", "batch70", "dense200"])
def test_approximate_3000(nq, search_k):
    """n = 3000 x 64, 10 trees: the spread form (with a search_k the first leaf ends, where the unrestricted call takes the
    leaf's slice of the permutation as it is), the batch form, the dense filter form."""
    a, X = _approx_index(3000, D, 10)
    cases = _cases(np.random.default_rng(nq + search_k), 3000)
    _approx_check(a, X, nq, search_k, (1, 20, 300), cases, seed=nq * 7 + search_k, label="lds_bitmap")


def test_approximate_3000_fused_traverse():
    a, X = _approx_index(3000, D, 10)
    cases = _cases(np.random.default_rng(70), 3000)
    _with_env("MORNA_QUERY_SPLIT_TRAVERSE", "0",
              lambda: _approx_check(a, X, 70, 2000, (1, 20, 300), cases, seed=71, label="fused"))


def test_approximate_roots_are_leaves():
    """n = 50 <= K: every root is a leaf."""
    a, X = _approx_index(50, D, 10)
    for nq in (1, 5, 70):
        cases = _cases(np.random.default_rng(nq), 50)
        _approx_check(a, X, nq, 30, (1, 20, 300), cases, seed=nq, label="roots_are_leaves")
    _with_env("MORNA_QUERY_SPLIT_TRAVERSE", "0",
              lambda: _approx_check(a, X, 70, 30, (1, 20), _cases(np.random.default_rng(3), 50), seed=4, label="roots_are_leaves_fused"))


def test_approximate_register_free_rows():
    """Rows whose dpad / 256 is none of the descent's register forms take NV = 0 (wave_dot): dim 1100 pads to 1280, five
    float4 per lane -- the one-wave descent for 5 queries, the fused traversal for 70 (the batch form's root kernel has no
    such form either).  dim 1300 (1536: six per lane) is a register form of a width no other test here has."""
    a, X = _approx_index(600, 1100, 4)
    for nq in (5, 70):
        cases = _cases(np.random.default_rng(nq), 600)
        _approx_check(a, X, nq, 3000, (1, 20), cases[:1] + cases[4:5], seed=nq, staged=False, label="nv0_dim1100")
    a, X = _approx_index(600, 1300, 4)
    cases = _cases(np.random.default_rng(9), 600)
    _approx_check(a, X, 5, 3000, (20,), cases[4:5], seed=10, staged=False, label="dim1300")


def test_approximate_global_bitmap():
    """n = 524 320 x 8, 2 trees: the bitmap passes 64 KiB and the global-bitmap instantiations run (the last word's bits past
    n stay out of it: n is a multiple of 32 here, n + 5 below)."""
    n = 524320
    a, X = _approx_index(n, 8, 2)
    rng = np.random.default_rng(8)
    cases = [c for c in _cases(rng, n) if c[0] in ("half", "none", "half+groups")]
    _approx_check(a, X, 5, 400, (1, 20), cases, seed=1, staged=False, label="global_bitmap_spread")
    _approx_check(a, X, 5, 5, (20,), cases[:1], seed=2, staged=False, label="global_bitmap_first_leaf_ends")
    _approx_check(a, X, 70, 400, (20,), cases[:1] + cases[2:], seed=3, staged=False, label="global_bitmap_batch")
    _with_env("MORNA_QUERY_SPLIT_TRAVERSE", "0",
              lambda: _approx_check(a, X, 70, 400, (20,), cases[2:], seed=4, staged=False, label="global_bitmap_fused"))


def test_padding_bits_of_the_last_word():
    """n = 3005: 29 bits of the last bitmap word are past n.  An allow bitmap handed over raw with those bits SET is the
    same restriction as one with them clear."""
    import ctypes as C
    from morna_amd._lib import check, lib, ptr
    from morna_amd.annoy import Restriction, pack_allow_bits
    a, X = _approx_index(3005, D, 10)
    rng = np.random.default_rng(5)
    allow = rng.random(3005) < 0.3
    bits = pack_allow_bits(allow)
    bits[-1] |= np.uint32(0xffffffff << (3005 % 32) & 0xffffffff)
    out = C.c_void_p()
    check(lib().morna_restriction_create(a._h, ptr(bits), None, C.byref(out)))
    raw = Restriction(a, out, None)
    r = a.restriction(allow)
    assert (raw.n_items, raw.n_allowed, raw.n_grouped) == (3005, int(allow.sum()), 0) == (r.n_items, r.n_allowed, r.n_grouped)
    Q = rng.standard_normal((5, D)).astype(np.float32)
    for k in (20, 3005):
        _same(a.get_nns_restricted(raw, k, 3000, Q=Q), a.get_nns_restricted(r, k, 3000, Q=Q), "padding/approx")
        _same(a.exact_search_restricted(raw, k, Q=Q.astype(np.float64)), a.exact_search_restricted(r, k, Q=Q.astype(np.float64)),
              "padding/exact")
    got = a.exact_search_restricted(raw, 3005, Q=Q.astype(np.float64))
    assert (got[2] == int(allow.sum())).all() and got[0].max() < 3005


def test_unrestricted_call_after_a_restricted_one():
    a, X = _approx_index(3000, D, 10)
    rng = np.random.default_rng(6)
    Q = rng.standard_normal((5, D)).astype(np.float32)
    items = np.arange(5, dtype=np.int32)
    before = (a.get_nns_by_vector_batch(Q, 20, 100), a.get_nns_by_item_batch(items, 20, -1), a.exact_search_batch(Q.astype(np.float64), 20))
    r = a.restriction(rng.random(3000) < 0.1, _groups(rng, 3000))
    a.get_nns_restricted(r, 20, 100, Q=Q, query_groups=_query_groups(5))
    a.get_nns_restricted(r, 20, -1, items=items)
    a.exact_search_restricted(r, 20, Q=Q.astype(np.float64))
    after = (a.get_nns_by_vector_batch(Q, 20, 100), a.get_nns_by_item_batch(items, 20, -1), a.exact_search_batch(Q.astype(np.float64), 20))
    for b, c in zip(before, after):
        _same(c, b, "unrestricted_after_restricted")


_FILTER_OFF = """
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import test_gpu_restrict as t
a, X = t._approx_index(3000, t.D, 10)
for nq in (70, 200):
    t._approx_check(a, X, nq, 2000, (1, 20), t._cases(np.random.default_rng(nq), 3000), seed=nq, label="filter_off")
print("filter off ok")
"""


def test_approximate_without_the_candidate_filter():
    """MORNA_QUERY_FILTER=0 is read once per process: a process of its own."""
    env = dict(os.environ, MORNA_QUERY_FILTER="0")
    r = subprocess.run([sys.executable, "-c", _FILTER_OFF.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "filter off ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------------------ other

def test_state_and_argument_errors():
    import ctypes as C
    from morna_amd import _lib
    from morna_amd._lib import lib, ptr
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(2)
    X = rng.standard_normal((300, D)).astype(np.float32)
    a = AnnoyIndex(D)
    a.add_items(X)
    groups = _groups(rng, 300)
    r = a.restriction(rng.random(300) < 0.5, groups)
    assert (r.n_items, r.n_grouped) == (300, sum(GROUP_SIZES))
    Q = rng.standard_normal((3, D))
    assert a.exact_search_restricted(r, 5, Q=Q)[2].tolist() == [5, 5, 5]
    # wrong-length arrays
    with pytest.raises(ValueError):
        a.restriction(allow=np.ones(299, bool))
    with pytest.raises(ValueError):
        a.restriction(groups=np.zeros(301, np.int32))
    with pytest.raises(ValueError):
        a.exact_search_restricted(r, 5, Q=Q, query_groups=np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        a.exact_search_restricted(a.restriction(np.ones(300, bool)), 5, Q=Q, query_groups=np.zeros(3, np.int32))
    with pytest.raises(IndexError):
        a.exact_search_restricted(r, 5, Q=rng.standard_normal((3, D + 1)))
    with pytest.raises(ValueError):
        a.exact_search_restricted(r, 5, Q=Q, items=np.arange(3))
    with pytest.raises(IndexError):
        a.exact_search_restricted(r, 5, items=np.array([300], np.int32))
    # through the raw call: no restriction is an error, not an unrestricted search; staged rows of another count
    ids, d, cnt = np.zeros((3, 5), np.int32), np.zeros((3, 5)), np.zeros(3, np.int32)
    rc = lib().morna_exact_search_restricted(a._h, None, ptr(Q), None, 3, None, 5, ptr(ids), ptr(d), ptr(cnt))
    assert rc == _lib.E_INVALID and b"no restriction" in lib().morna_last_error()
    rc = lib().morna_exact_search_restricted(a._h, r._p, None, None, 3, None, 5, ptr(ids), ptr(d), ptr(cnt))
    assert rc == _lib.E_STATE                  # no query rows are staged
    _stage_rows(a, 4, 1)
    rc = lib().morna_exact_search_restricted(a._h, r._p, None, None, 3, None, 5, ptr(ids), ptr(d), ptr(cnt))
    assert rc == _lib.E_INVALID
    other = AnnoyIndex(D)
    other.add_items(X)
    rc = lib().morna_exact_search_restricted(other._h, r._p, ptr(Q), None, 3, None, 5, ptr(ids), ptr(d), ptr(cnt))
    assert rc == _lib.E_INVALID
    with pytest.raises(ValueError):
        other.exact_search_restricted(r, 5, Q=Q)
    # the approximate search wants a built index
    with pytest.raises(RuntimeError):
        a.get_nns_restricted(r, 5, Q=Q.astype(np.float32))
    # more items on a handle with a live restriction: MORNA_E_STATE until it is made again
    a.add_items(X[:10], first_id=300)
    rc = lib().morna_exact_search_restricted(a._h, r._p, ptr(Q), None, 3, None, 5, ptr(ids), ptr(d), ptr(cnt))
    assert rc == _lib.E_STATE
    with pytest.raises(RuntimeError):
        a.exact_search_restricted(r, 5, Q=Q)
    r2 = a.restriction(np.ones(310, bool))
    assert a.exact_search_restricted(r2, 5, Q=Q)[2].tolist() == [5, 5, 5]
    a.build(4)
    with pytest.raises(RuntimeError):
        a.get_nns_restricted(r, 5, Q=Q.astype(np.float32))
    assert a.get_nns_restricted(r2, 5, Q=Q.astype(np.float32))[2].tolist() == [5, 5, 5]
    empty = AnnoyIndex(D)
    out = C.c_void_p()
    assert lib().morna_restriction_create(empty._h, None, None, C.byref(out)) == _lib.E_EMPTY
