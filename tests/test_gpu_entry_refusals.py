"""What the entry layer of the C ABI refuses before it reaches a worker: one table of malformed calls through _lib.lib(),
each with the code and the whole message it is answered with, and, where one call is malformed in two ways, which refusal
wins.  The messages are literals: they pin the wording of csrc/api.hip, they are not read from it.

Two families resolve "query vectors, stored items, or the staged query rows", and with nothing staged they answer
differently: the approximate family and exact_search_restricted say MORNA_E_STATE, "no query rows: ..."; label_sums,
exact_radius and mixture say MORNA_E_INVALID, "...: no query source (...)".  Both are on record here.

Every case is refused on the host: none launches a kernel.  Two refusals of label_centroids / mixture (the label count) are
made by their worker in mixture.hip, before its first launch; they are in the table because the issue of the entry layer
names them, with the bound the worker states (MORNA_MIXTURE_LABELS_MAX = 128).  The range of k of kmeans / kmeans_assign is
checked behind the scan front of exact.hip and is left out.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, NQ, L, K = 8, 4, 3, 2, 2
OK, E_INVALID, E_STATE, E_RANGE = 0, -1, -3, -4

NULL_H = "null index handle"
NO_ROWS = "no query rows: call morna_build_query_rows first"
NOT_BOTH = "%s: give query vectors or items, not both"
NO_SOURCE = "%s: no query source (give query vectors or items, or call morna_build_query_rows first)"
MISMATCH = "%s: 2 queries asked for, 3 query rows are staged"
Q_GROUPS = "%s: query groups need a restriction that holds the items' groups"
NO_RESTRICTION = "%s: no restriction (use the unrestricted call)"
SHARDED = "%s is not available on a row-sharded handle"
NULL_BUF = "%s: null buffer"
NULL_PTR = "%s: null pointer"
NOT_BUILT = "index has not been built: call build() before searching"


def _stage_rows(a, nq):
    """nq query rows staged on the handle through morna_build_query_rows (a small made-up vocabulary)"""
    from morna_amd.index import ParsedLines, pack_vocab
    rng = np.random.default_rng(5)
    J = 40
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


class Calls(object):
    """Every rewritten entry point as a call that is well-formed by default (stored items as the queries); a keyword makes
    it malformed.  h: an AnnoyIndex or None; every other argument: a numpy array, a ctypes pointer or None."""

    def __init__(self):
        from morna_amd._lib import lib, ptr
        self.lib, self.ptr = lib(), ptr
        rng = np.random.default_rng(3)
        self.X = rng.standard_normal((N, D)).astype(np.float32)
        self.Q32 = self.X[:NQ].copy()
        self.Q64 = self.X[:NQ].astype(np.float64)
        self.items = np.arange(NQ, dtype=np.int32)
        self.qg = np.zeros(NQ, np.int32)
        self.labels = (np.arange(N) % L).astype(np.int32)
        self.seeds = np.array([0, 5], np.int32)
        self.cents = self.X[[0, 5]].astype(np.float64)
        self.trees, self.sks = np.array([1], np.int32), np.array([4], np.int32)
        self.ids, self.cnt = np.zeros((NQ, K), np.int32), np.zeros(NQ, np.int32)
        self.d32, self.d64 = np.zeros((NQ, K), np.float32), np.zeros((NQ, K), np.float64)
        self.cell = [np.zeros((1, 1, NQ), np.int32) for _ in range(4)]         # ncand, ndots, hits, count
        self.sums, self.counts = np.zeros((NQ, L), np.uint64), np.zeros((NQ, L), np.int32)
        self.assign, self.dist = np.zeros(N, np.int32), np.zeros(N, np.float64)
        self.cent_out, self.sizes, self.info2 = np.zeros((K, D)), np.zeros(K, np.int32), np.zeros(2, np.int32)
        self.csums, self.ccounts, self.gram = np.zeros((L, D)), np.zeros(L, np.int32), np.zeros((L, L))
        self.weights, self.info, self.active = np.zeros((NQ, L)), np.zeros((NQ, 4)), np.zeros((NQ, L), np.uint8)
        self.radius_out = C.c_void_p()

    def _h(self, h):
        return None if h is None else h._h

    def _r(self, r):
        return None if r is None else r._p

    def prefix(self, h, q=None, it="items", nq=NQ, ids="ids", trees=1):
        p = self.ptr
        return self.lib.morna_get_nns_prefix(self._h(h), p(q), p(self._a(it)), nq, K, -1, trees, p(self._a(ids)), p(self.d32), p(self.cnt))

    def _a(self, x):
        return getattr(self, x) if isinstance(x, str) else x

    def sweep(self, h, q=None, it="items", nq=NQ):
        p = self.ptr
        return self.lib.morna_search_sweep(self._h(h), p(q), p(self._a(it)), nq, K, p(self.trees), 1, p(self.sks), 1, None, None, None,
                                           p(self.cell[0]), p(self.cell[1]))

    def recall(self, h, q=None, it="items", nq=NQ, k=K, hits="hits"):
        p = self.ptr
        hits = self.cell[2] if hits == "hits" else hits
        return self.lib.morna_recall_sweep(self._h(h), p(q), p(self._a(it)), nq, k, p(self.trees), 1, p(self.sks), 1, p(hits), None,
                                           p(self.cell[0]), p(self.cell[1]), None, None, None, None)

    def nns_restricted(self, h, r, q=None, it="items", nq=NQ, qg=None, ids="ids"):
        p = self.ptr
        return self.lib.morna_get_nns_restricted(self._h(h), self._r(r), p(q), p(self._a(it)), nq, p(qg), K, -1, p(self._a(ids)),
                                                 p(self.d32), p(self.cnt))

    def exact_restricted(self, h, r, q=None, it="items", nq=NQ, qg=None, ids="ids"):
        p = self.ptr
        return self.lib.morna_exact_search_restricted(self._h(h), self._r(r), p(q), p(self._a(it)), nq, p(qg), K, p(self._a(ids)),
                                                      p(self.d64), p(self.cnt))

    def label_sums(self, h, r=None, q=None, it="items", nq=NQ, qg=None, lab="labels", nl=L, sums="sums", counts="counts"):
        p = self.ptr
        return self.lib.morna_label_sums(self._h(h), self._r(r), p(q), p(self._a(it)), nq, p(qg), p(self._a(lab)), nl, p(self._a(sums)),
                                         p(self._a(counts)))

    def radius(self, h, r=None, q=None, it="items", nq=NQ, qg=None, out="out"):
        p = self.ptr
        self.radius_out = C.c_void_p(1)     # (never dereferenced: a refusal past the null check must clear it)
        return self.lib.morna_exact_radius(self._h(h), self._r(r), p(q), p(self._a(it)), nq, p(qg), None, 2.0,
                                           C.byref(self.radius_out) if out == "out" else None)

    def kmeans(self, h, seeds="seeds", assign="assign", info="info2"):
        p = self.ptr
        return self.lib.morna_kmeans(self._h(h), None, p(self._a(seeds)), K, 5, p(self._a(assign)), p(self.dist), p(self.cent_out),
                                     p(self.sizes), p(self._a(info)))

    def kmeans_assign(self, h, cents="cents", assign="assign"):
        p = self.ptr
        return self.lib.morna_kmeans_assign(self._h(h), None, p(self._a(cents)), K, p(self._a(assign)), p(self.dist))

    def centroids(self, h, lab="labels", nl=L, sums="csums", counts="ccounts"):
        p = self.ptr
        return self.lib.morna_label_centroids(self._h(h), None, p(self._a(lab)), nl, p(self._a(sums)), p(self._a(counts)), p(self.gram))

    def mixture(self, h, q=None, it="items", nq=NQ, lab="labels", nl=L, weights="weights", info="info"):
        p = self.ptr
        return self.lib.morna_mixture(self._h(h), None, p(q), p(self._a(it)), nq, p(self._a(lab)), nl, 1e-9, 100, p(self._a(weights)),
                                      p(self._a(info)), p(self.active))

    # the statistics of a family: (reader, doubles); and a well-formed call that leaves them non-zero
    STATS = dict(sweep=("morna_search_sweep_stats", 4), label=("morna_label_sums_stats", 6), radius=("morna_exact_radius_stats", 8),
                 kmeans=("morna_kmeans_stats", 8), mixture=("morna_mixture_stats", 8))

    def read_stats(self, family, h):
        name, n = self.STATS[family]
        out = np.full(n, -1.0)
        assert getattr(self.lib, name)(h._h, self.ptr(out)) == OK
        return out

    def prime(self, family, h):
        if family == "radius":
            assert self.radius(h) == OK
            assert self.lib.morna_radius_free(self.radius_out) == OK
        else:
            call = dict(sweep=self.sweep, label=self.label_sums, kmeans=self.kmeans, mixture=self.mixture)[family]
            assert call(h) == OK, self.lib.morna_last_error()
        assert self.read_stats(family, h).any(), family


def _table(c, a, unbuilt, sharded, r_groups, r_allow):
    """(name, staged rows the case needs (0, 3 or None: either), the call, code, message, statistics family or None)"""
    Q32, Q64, qg = c.Q32, c.Q64, c.qg
    T = []

    def add(name, staged, call, code, msg, family=None):
        T.append((name, staged, call, code, msg, family))

    # ---- the approximate family: E_STATE with nothing staged
    add("prefix null handle", None, lambda: c.prefix(None), E_INVALID, NULL_H)
    add("prefix null ids", None, lambda: c.prefix(a, ids=None), E_INVALID, NULL_BUF % "get_nns_prefix")
    add("prefix null ids wins over both", None, lambda: c.prefix(a, q=Q32, ids=None), E_INVALID, NULL_BUF % "get_nns_prefix")
    add("prefix both", None, lambda: c.prefix(a, q=Q32), E_INVALID, NOT_BOTH % "get_nns_prefix")
    add("prefix both wins over unbuilt", None, lambda: c.prefix(unbuilt, q=Q32), E_INVALID, NOT_BOTH % "get_nns_prefix")
    add("prefix nothing staged", 0, lambda: c.prefix(a, it=None), E_STATE, NO_ROWS)
    add("prefix nothing staged wins over unbuilt", 0, lambda: c.prefix(unbuilt, it=None), E_STATE, NO_ROWS)
    add("prefix nothing staged wins over trees", 0, lambda: c.prefix(a, it=None, trees=0), E_STATE, NO_ROWS)
    add("prefix staged count", 3, lambda: c.prefix(a, it=None, nq=2), E_INVALID, MISMATCH % "get_nns_prefix")
    add("prefix staged count wins over trees", 3, lambda: c.prefix(a, it=None, nq=2, trees=2), E_INVALID, MISMATCH % "get_nns_prefix")
    add("prefix unbuilt", None, lambda: c.prefix(unbuilt), E_STATE, NOT_BUILT)
    add("prefix unbuilt wins over trees", None, lambda: c.prefix(unbuilt, trees=0), E_STATE, NOT_BUILT)
    add("prefix 0 trees", None, lambda: c.prefix(a, trees=0), E_RANGE, "get_nns_prefix: 0 trees asked for, the forest has 1")
    add("prefix 2 trees", None, lambda: c.prefix(a, trees=2), E_RANGE, "get_nns_prefix: 2 trees asked for, the forest has 1")

    add("sweep null handle", None, lambda: c.sweep(None), E_INVALID, NULL_H)
    add("sweep both", None, lambda: c.sweep(a, q=Q32), E_INVALID, NOT_BOTH % "search_sweep", "sweep")
    add("sweep nothing staged", 0, lambda: c.sweep(a, it=None), E_STATE, NO_ROWS, "sweep")
    add("sweep staged count", 3, lambda: c.sweep(a, it=None, nq=2), E_INVALID, MISMATCH % "search_sweep", "sweep")

    add("recall null handle", None, lambda: c.recall(None), E_INVALID, NULL_H)
    add("recall null hits", None, lambda: c.recall(a, hits=None), E_INVALID, NULL_BUF % "recall_sweep", "sweep")
    add("recall null hits wins over k", None, lambda: c.recall(a, hits=None, k=257), E_INVALID, NULL_BUF % "recall_sweep", "sweep")
    add("recall k", None, lambda: c.recall(a, k=257), E_INVALID, "recall_sweep: n = 257 is above the supported 256", "sweep")
    add("recall k wins over both", None, lambda: c.recall(a, q=Q32, k=257), E_INVALID,
        "recall_sweep: n = 257 is above the supported 256", "sweep")
    add("recall both", None, lambda: c.recall(a, q=Q32), E_INVALID, NOT_BOTH % "recall_sweep", "sweep")
    add("recall nothing staged", 0, lambda: c.recall(a, it=None), E_STATE, NO_ROWS, "sweep")
    add("recall staged count", 3, lambda: c.recall(a, it=None, nq=2), E_INVALID, MISMATCH % "recall_sweep", "sweep")

    for name, call in (("get_nns_restricted", c.nns_restricted), ("exact_search_restricted", c.exact_restricted)):
        Q = Q32 if call == c.nns_restricted else Q64
        add(name + " null handle", None, lambda call=call: call(None, r_groups), E_INVALID, NULL_H)
        add(name + " null ids", None, lambda call=call: call(a, r_groups, ids=None), E_INVALID, NULL_BUF % name)
        add(name + " null ids wins over no restriction", None, lambda call=call: call(a, None, ids=None), E_INVALID, NULL_BUF % name)
        add(name + " no restriction", None, lambda call=call: call(a, None), E_INVALID, NO_RESTRICTION % name)
        add(name + " no restriction, query groups", None, lambda call=call: call(a, None, qg=qg), E_INVALID, Q_GROUPS % name)
        add(name + " query groups, no item groups", None, lambda call=call: call(a, r_allow, qg=qg), E_INVALID, Q_GROUPS % name)
        add(name + " query groups win over both", None, lambda call=call, Q=Q: call(a, r_allow, q=Q, qg=qg), E_INVALID, Q_GROUPS % name)
        add(name + " both", None, lambda call=call, Q=Q: call(a, r_groups, q=Q, qg=qg), E_INVALID, NOT_BOTH % name)
        # (exact_search_restricted takes fp64 queries as label_sums does, and answers as the approximate family does)
        add(name + " nothing staged", 0, lambda call=call: call(a, r_groups, it=None), E_STATE, NO_ROWS)
        add(name + " staged count", 3, lambda call=call: call(a, r_groups, it=None, nq=2), E_INVALID, MISMATCH % name)

    # ---- the whole-scan entry points: E_INVALID with nothing staged; the statistics read zero after every refusal
    add("label_sums null handle", None, lambda: c.label_sums(None), E_INVALID, NULL_H)
    for what in ("lab", "sums", "counts"):
        add("label_sums null " + what, None, lambda what=what: c.label_sums(a, **{what: None}), E_INVALID, NULL_BUF % "label_sums", "label")
    add("label_sums null wins over labels", None, lambda: c.label_sums(a, sums=None, nl=0), E_INVALID, NULL_BUF % "label_sums", "label")
    add("label_sums 0 labels", None, lambda: c.label_sums(a, nl=0), E_INVALID, "label_sums: 0 labels, 1 to 4096 are taken", "label")
    add("label_sums 4097 labels", None, lambda: c.label_sums(a, nl=4097), E_INVALID, "label_sums: 4097 labels, 1 to 4096 are taken", "label")
    add("label_sums labels win over both", None, lambda: c.label_sums(a, q=Q64, nl=0), E_INVALID,
        "label_sums: 0 labels, 1 to 4096 are taken", "label")
    add("label_sums both", None, lambda: c.label_sums(a, q=Q64), E_INVALID, NOT_BOTH % "label_sums", "label")
    add("label_sums both wins over query groups", None, lambda: c.label_sums(a, q=Q64, qg=qg), E_INVALID, NOT_BOTH % "label_sums", "label")
    add("label_sums query groups, no restriction", None, lambda: c.label_sums(a, qg=qg), E_INVALID, Q_GROUPS % "label_sums", "label")
    add("label_sums query groups, no item groups", None, lambda: c.label_sums(a, r=r_allow, qg=qg), E_INVALID, Q_GROUPS % "label_sums", "label")
    add("label_sums query groups win over sharded", None, lambda: c.label_sums(sharded, qg=qg), E_INVALID, Q_GROUPS % "label_sums", "label")
    add("label_sums sharded", None, lambda: c.label_sums(sharded), E_INVALID, SHARDED % "label_sums", "label")
    add("label_sums sharded wins over nothing staged", None, lambda: c.label_sums(sharded, it=None), E_INVALID, SHARDED % "label_sums", "label")
    add("label_sums nothing staged", 0, lambda: c.label_sums(a, it=None), E_INVALID, NO_SOURCE % "label_sums", "label")
    add("label_sums staged count", 3, lambda: c.label_sums(a, it=None, nq=2), E_INVALID, MISMATCH % "label_sums", "label")

    add("exact_radius null handle", None, lambda: c.radius(None), E_INVALID, NULL_H)
    add("exact_radius null out", None, lambda: c.radius(a, out=None), E_INVALID, NULL_BUF % "exact_radius", "radius")
    add("exact_radius null out wins over both", None, lambda: c.radius(a, q=Q64, out=None), E_INVALID, NULL_BUF % "exact_radius", "radius")
    add("exact_radius both", None, lambda: c.radius(a, q=Q64), E_INVALID, NOT_BOTH % "exact_radius", "radius")
    add("exact_radius both wins over query groups", None, lambda: c.radius(a, q=Q64, qg=qg), E_INVALID, NOT_BOTH % "exact_radius", "radius")
    add("exact_radius query groups, no restriction", None, lambda: c.radius(a, qg=qg), E_INVALID, Q_GROUPS % "exact_radius", "radius")
    add("exact_radius query groups, no item groups", None, lambda: c.radius(a, r=r_allow, qg=qg), E_INVALID, Q_GROUPS % "exact_radius", "radius")
    add("exact_radius query groups win over sharded", None, lambda: c.radius(sharded, qg=qg), E_INVALID, Q_GROUPS % "exact_radius", "radius")
    add("exact_radius sharded", None, lambda: c.radius(sharded), E_INVALID, SHARDED % "exact_radius", "radius")
    add("exact_radius sharded wins over nothing staged", None, lambda: c.radius(sharded, it=None), E_INVALID, SHARDED % "exact_radius", "radius")
    add("exact_radius nothing staged", 0, lambda: c.radius(a, it=None), E_INVALID, NO_SOURCE % "exact_radius", "radius")
    add("exact_radius staged count", 3, lambda: c.radius(a, it=None, nq=2), E_INVALID, MISMATCH % "exact_radius", "radius")

    add("kmeans null handle", None, lambda: c.kmeans(None), E_INVALID, NULL_H)
    for what in ("seeds", "assign", "info"):
        add("kmeans null " + what, None, lambda what=what: c.kmeans(a, **{what: None}), E_INVALID, NULL_BUF % "kmeans", "kmeans")
    add("kmeans null wins over sharded", None, lambda: c.kmeans(sharded, assign=None), E_INVALID, NULL_BUF % "kmeans", "kmeans")
    add("kmeans sharded", None, lambda: c.kmeans(sharded), E_INVALID, SHARDED % "kmeans", "kmeans")
    add("kmeans_assign null handle", None, lambda: c.kmeans_assign(None), E_INVALID, NULL_H)
    for what in ("cents", "assign"):
        add("kmeans_assign null " + what, None, lambda what=what: c.kmeans_assign(a, **{what: None}), E_INVALID, NULL_BUF % "kmeans_assign",
            "kmeans")
    add("kmeans_assign null wins over sharded", None, lambda: c.kmeans_assign(sharded, cents=None), E_INVALID, NULL_BUF % "kmeans_assign",
        "kmeans")
    add("kmeans_assign sharded", None, lambda: c.kmeans_assign(sharded), E_INVALID, SHARDED % "kmeans_assign", "kmeans")

    add("label_centroids null handle", None, lambda: c.centroids(None), E_INVALID, NULL_H)
    for what in ("lab", "sums", "counts"):
        add("label_centroids null " + what, None, lambda what=what: c.centroids(a, **{what: None}), E_INVALID, NULL_BUF % "label_centroids",
            "mixture")
    add("label_centroids null wins over sharded", None, lambda: c.centroids(sharded, sums=None), E_INVALID, NULL_BUF % "label_centroids",
        "mixture")
    add("label_centroids sharded", None, lambda: c.centroids(sharded), E_INVALID, SHARDED % "label_centroids", "mixture")
    add("label_centroids sharded wins over labels", None, lambda: c.centroids(sharded, nl=0), E_INVALID, SHARDED % "label_centroids", "mixture")
    add("label_centroids 0 labels", None, lambda: c.centroids(a, nl=0), E_INVALID, "label_centroids: 0 labels, 1 to 128 are taken", "mixture")
    add("label_centroids 4097 labels", None, lambda: c.centroids(a, nl=4097), E_INVALID, "label_centroids: 4097 labels, 1 to 128 are taken",
        "mixture")

    add("mixture null handle", None, lambda: c.mixture(None), E_INVALID, NULL_H)
    for what in ("lab", "weights", "info"):
        add("mixture null " + what, None, lambda what=what: c.mixture(a, **{what: None}), E_INVALID, NULL_BUF % "mixture", "mixture")
    add("mixture null wins over both", None, lambda: c.mixture(a, q=Q64, info=None), E_INVALID, NULL_BUF % "mixture", "mixture")
    add("mixture both", None, lambda: c.mixture(a, q=Q64), E_INVALID, NOT_BOTH % "mixture", "mixture")
    add("mixture both wins over sharded", None, lambda: c.mixture(sharded, q=Q64), E_INVALID, NOT_BOTH % "mixture", "mixture")
    add("mixture sharded", None, lambda: c.mixture(sharded), E_INVALID, SHARDED % "mixture", "mixture")
    add("mixture sharded wins over nothing staged", None, lambda: c.mixture(sharded, it=None), E_INVALID, SHARDED % "mixture", "mixture")
    add("mixture nothing staged", 0, lambda: c.mixture(a, it=None), E_INVALID, NO_SOURCE % "mixture", "mixture")
    add("mixture nothing staged wins over labels", 0, lambda: c.mixture(a, it=None, nl=0), E_INVALID, NO_SOURCE % "mixture", "mixture")
    add("mixture staged count", 3, lambda: c.mixture(a, it=None, nq=2), E_INVALID, MISMATCH % "mixture", "mixture")
    add("mixture 0 labels", None, lambda: c.mixture(a, nl=0), E_INVALID, "mixture: 0 labels, 1 to 128 are taken", "mixture")
    add("mixture 4097 labels", None, lambda: c.mixture(a, nl=4097), E_INVALID, "mixture: 4097 labels, 1 to 128 are taken", "mixture")

    # ---- the five readers: search_sweep_stats looks at the handle first and words its null differently
    out = np.zeros(8)
    for fn, null_stats in (("search_sweep_stats", NULL_BUF), ("label_sums_stats", NULL_PTR), ("exact_radius_stats", NULL_PTR),
                           ("kmeans_stats", NULL_PTR), ("mixture_stats", NULL_PTR)):
        f = getattr(c.lib, "morna_" + fn)
        null_h = NULL_H if fn == "search_sweep_stats" else NULL_PTR % fn
        add(fn + " null handle", None, lambda f=f: f(None, c.ptr(out)), E_INVALID, null_h)
        add(fn + " null stats", None, lambda f=f: f(a._h, None), E_INVALID, null_stats % fn)
        add(fn + " null handle and stats", None, lambda f=f: f(None, None), E_INVALID, null_h)
    return T


def test_every_refusal_of_the_entry_layer():
    from morna_amd.annoy import AnnoyIndex
    c = Calls()

    def index(build):
        h = AnnoyIndex(D)
        h.add_items(c.X)
        if build:
            h.build(1)
        return h
    a, unbuilt, sharded = index(True), index(False), index(True)
    r_groups = a.restriction(groups=np.arange(N, dtype=np.int32) % 3)
    r_allow = a.restriction(allow=np.ones(N, bool))
    # the statistics of the sharded handle are made non-zero while it is an ordinary one: every call is refused afterwards
    for family in Calls.STATS:
        c.prime(family, sharded)
    sharded.comm_init(AnnoyIndex.comm_unique_id(), 0, 1)     # a row-sharded handle: one that owns a communicator, here of one rank
    failures, ran = [], 0
    try:
        table = _table(c, a, unbuilt, sharded, r_groups, r_allow)
        for staged in (0, 3):
            if staged:
                _stage_rows(a, staged)
            for name, needs, call, code, msg, family in table:
                if needs is not None and needs != staged:
                    continue
                on_sharded = "sharded" in name
                if family and not on_sharded:
                    c.prime(family, a)
                rc = call()
                got = c.lib.morna_last_error().decode()
                ran += 1
                if (rc, got) != (code, msg):
                    failures.append("%s (%d rows staged): %d %r, expected %d %r" % (name, staged, rc, got, code, msg))
                if family and c.read_stats(family, sharded if on_sharded else a).any():
                    failures.append("%s (%d rows staged): the statistics are not zero after the refusal" % (name, staged))
                if name.startswith("exact_radius") and "null" not in name and c.radius_out.value is not None:
                    failures.append("%s: *out was not cleared" % name)
    finally:
        sharded.comm_destroy()
    assert not failures, "\n".join(failures)
    assert ran == sum(2 if needs is None else 1 for _, needs, _, _, _, _ in table)
    # the handles still answer: nothing above left one in a bad state
    assert c.prefix(a) == OK and c.label_sums(a) == OK and c.mixture(sharded) == OK
