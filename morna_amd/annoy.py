"""AnnoyIndex-shaped front end of the HIP library.

Mirrors the surface of ``annoy.AnnoyIndex`` that morna uses (reference call
sites in commanderson/morna morna.py): constructor 166/543/1171, ``add_item``
406/423, ``build`` 425, ``save`` 439, ``load`` 544/1172, ``get_nns_by_vector``
651/659, ``get_nns_by_item`` 762/769/1191, ``get_item_vector`` 702,
``get_n_items`` 1174 -- same positional arguments, same return shapes
(``include_distances=True`` -> ``(ids, distances)``, else a bare list).

Everything numeric happens in libmorna_hip.so on the MI355X; this module only
marshals numpy buffers through ctypes.  Batched variants (``*_batch``) expose
what the C ABI really does: many queries per launch.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, ptr, read_stats

# the doubles of every morna_*_stats call of an index, in the order of the C array (the *_stats methods say what they mean)
SWEEP_STATS = (("descents", int), ("cells", int), ("rows_canonical", int), ("contraction", int))
LABEL_SUMS_STATS = (("scan_ms", float), ("sums_ms", float), ("queries", int), ("batches", int), ("counted", int), ("scan_eps", float))
RADIUS_STATS = (("scan_ms", float), ("select_ms", float), ("dist_ms", float), ("queries", int), ("batches", int), ("candidates", int),
                ("results", int), ("window", float))
KMEANS_STATS = (("scan_ms", float), ("pick_ms", float), ("resolve_ms", float), ("update_ms", float), ("open_rows", int), ("chains", int),
                ("iterations", int), ("largest", int))
MIXTURE_STATS = (("centroids_ms", float), ("gram_ms", float), ("dots_ms", float), ("solve_ms", float), ("queries", int), ("sweeps", int),
                 ("max_sweeps", int), ("open", int))
PCA_STATS = (("t_ms", float), ("y_ms", float), ("orth_ms", float), ("small_ms", float), ("eig_ms", float), ("iterations", int),
             ("fitted", int), ("row_bytes", int))


def pack_allow_bits(allow):
    """A boolean array [n] as the uint32 words of morna_restriction_create: bit i of word i // 32, low bit first."""
    allow = np.ascontiguousarray(allow, dtype=bool)
    padded = np.zeros((len(allow) + 31) // 32 * 32, bool)
    padded[:len(allow)] = allow
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def _results(nq, n, dist_dtype):
    """The (ids, distances, counts) buffers of nq answers of n entries."""
    return np.empty((nq, n), np.int32), np.empty((nq, n), dist_dtype), np.empty(nq, np.int32)


class Restriction(object):
    """A restriction of the searches of one AnnoyIndex (AnnoyIndex.restriction; include/morna_hip.h, "restricted search"):
    n_items, n_allowed and n_grouped as the library counted them, `groups` the items' labels (int32 [n_items]) or None.
    The bitmap and the labels live on the index's device until the object goes."""

    def __init__(self, owner, handle, groups):
        self.owner, self._p, self.groups = owner, handle, groups
        counts = np.zeros(3, np.int64)
        check(lib().morna_restriction_counts(self._p, ptr(counts)))
        self.n_items, self.n_allowed, self.n_grouped = (int(x) for x in counts)

    def __del__(self):
        p = getattr(self, "_p", None)
        owner = getattr(self, "owner", None)
        if p is not None and p.value and owner is not None and getattr(owner, "_h", None) is not None and owner._h.value:
            try:
                lib().morna_restriction_free(p)
            except Exception:
                pass
        self._p = C.c_void_p()


class AnnoyIndex(object):
    def __init__(self, f, metric='angular', device=0):
        if metric != 'angular':
            raise ValueError("morna uses AnnoyIndex(dim, metric='angular') only (morna.py:166); got %r" % (metric,))
        self.f = int(f)
        self._h = C.c_void_p()
        check(lib().morna_index_create(self.f, int(device), C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().morna_index_destroy(h)
            except Exception:
                pass
            self._h = C.c_void_p()

    # ---- items -----------------------------------------------------------
    def add_item(self, i, vector):
        v = np.ascontiguousarray(vector, dtype=np.float64)
        if v.shape != (self.f,):
            raise IndexError("Vector has wrong length (expected %d, got %d)" % (self.f, v.size))
        check(lib().morna_add_item(self._h, int(i), ptr(v)))

    def add_items(self, rows, first_id=0):
        """Bulk add_item for ids first_id.. (rows already fp32)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.f:
            raise IndexError("rows must be [n, %d]" % self.f)
        check(lib().morna_add_items_f32(self._h, int(first_id), ptr(rows), rows.shape[0]))

    def add_items_from_store(self, store, sample_ids, line_hash):
        """The items become 0 .. len(sample_ids) - 1: item i the hashed row, at this index's width, of the junction store's
        sample sample_ids[i] (external ids; repeats allowed), made on the GPU from the store row, the store's weights
        (JunctionStore.set_weights) and line_hash, the int32 hash of every line's key (junctions.line_hashes).  Only the ids,
        and the hashes when they differ from the last call's, go to the device (include/morna_hip.h, "hashed rows from store
        rows").  IndexError for an id the store lacks, RuntimeError for a built index or a store without weights."""
        ids = np.ascontiguousarray([int(s) for s in sample_ids], dtype=np.int64)
        line_hash = np.ascontiguousarray(line_hash, dtype=np.int32)
        if line_hash.ndim != 1:
            raise ValueError("add_items_from_store takes one hash per line (a 1-d array)")
        check(lib().morna_add_items_from_store(self._h, store._p, ptr(ids), len(ids), ptr(line_hash), len(line_hash)))

    def get_n_items(self):
        return int(lib().morna_get_n_items(self._h))

    def get_item_vector(self, i):
        out = np.empty(self.f, dtype=np.float32)
        check(lib().morna_get_item_vector(self._h, int(i), ptr(out)))
        return [float(x) for x in out]

    def get_item_vectors(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.empty((len(ids), self.f), dtype=np.float32)
        check(lib().morna_get_item_vectors(self._h, ptr(ids), len(ids), ptr(out)))
        return out

    def get_item_vectors_into(self, ids, out_ptr):
        """Rows of `ids` written to out_ptr: [len(ids), f] fp32 in HOST or this DEVICE's memory."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        check(lib().morna_get_item_vectors(self._h, ptr(ids), len(ids), C.c_void_p(int(out_ptr))))

    def get_item_vectors_dev(self, ids, out_ptr):
        """Rows of `ids` written to out_ptr ([len(ids), f] fp32, this device's memory) in the order of the handle's
        stream: no host wait."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        check(lib().morna_get_item_vectors_dev(self._h, ptr(ids), len(ids), C.c_void_p(int(out_ptr))))

    def stream_ptr(self):
        """The handle's HIP stream (hipStream_t as an integer), e.g. for torch.cuda.ExternalStream."""
        out = C.c_void_p()
        check(lib().morna_get_stream(self._h, C.byref(out)))
        return int(out.value or 0)

    def get_nns_by_vector_ptr(self, q_ptr, nq, n, search_k=-1):
        """get_nns_by_vector_batch for nq contiguous fp32 rows at a raw (host or device) address."""
        ids, d, cnt = _results(nq, n, np.float32)
        check(lib().morna_get_nns_by_vector(self._h, C.c_void_p(int(q_ptr)), int(nq), int(n), int(search_k),
                                            ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def get_nns_by_vector_packed(self, q_ptr, nq, n, search_k, id_offset, packed_ptr):
        """Row-sharded search, device hand-over: answers to nq fp32 queries at q_ptr (host or device) written to
        packed_ptr (this device's memory) as the [nq, 2n] int32 message of the top-k all-gather.  Enqueued on the
        handle's stream (stream_ptr()), not waited for."""
        check(lib().morna_get_nns_by_vector_packed(self._h, C.c_void_p(int(q_ptr)), int(nq), int(n), int(search_k),
                                                   int(id_offset), C.c_void_p(int(packed_ptr))))

    def merge_topk_packed(self, gathered_ptr, world, nq, kk, n):
        """Merge of the all-gathered messages [world, nq, 2kk] (device memory) on the device."""
        ids, d, cnt = _results(nq, n, np.float32)
        check(lib().morna_merge_topk_packed(self._h, C.c_void_p(int(gathered_ptr)), int(world), int(nq), int(kk), int(n),
                                            ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def get_items(self):
        out = np.empty((self.get_n_items(), self.f), dtype=np.float32)
        check(lib().morna_get_items(self._h, ptr(out)))
        return out

    def get_norms2(self):
        out = np.empty(self.get_n_items(), dtype=np.float32)
        check(lib().morna_get_norms2(self._h, ptr(out)))
        return out

    # ---- fused feature build (MornaIndex uses this instead of add_item) ----
    def stage_junctions(self, key_bytes, key_off, row_ptr, item_ids, cov, idf):
        key_bytes = np.ascontiguousarray(key_bytes, dtype=np.uint8)
        key_off = np.ascontiguousarray(key_off, dtype=np.int64)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        item_ids = np.ascontiguousarray(item_ids, dtype=np.int32)
        cov = np.ascontiguousarray(cov, dtype=np.int32)
        idf = np.ascontiguousarray(idf, dtype=np.float64)
        J = len(key_off) - 1
        if len(row_ptr) != J + 1 or len(idf) != J or len(item_ids) != len(cov):
            raise ValueError("stage_junctions: inconsistent array lengths")
        check(lib().morna_stage_junctions(self._h, ptr(key_bytes), ptr(key_off), J, ptr(row_ptr),
                                          ptr(item_ids), ptr(cov), ptr(idf)))

    def stage_item_order(self, order_key):
        """order_key[i] for internal id i: a key in which the lines' sample lists ascend (the external sample ids of an
        intropolis file).  A performance hint for build_features; the matrix does not depend on it."""
        order_key = np.ascontiguousarray(order_key, dtype=np.int64)
        check(lib().morna_stage_item_order(self._h, ptr(order_key), len(order_key)))

    def build_features(self, n_items):
        check(lib().morna_build_features(self._h, int(n_items)))

    def unstage_junctions(self):
        check(lib().morna_unstage_junctions(self._h))

    def hash_keys(self, key_bytes, key_off):
        key_bytes = np.ascontiguousarray(key_bytes, dtype=np.uint8)
        key_off = np.ascontiguousarray(key_off, dtype=np.int64)
        J = len(key_off) - 1
        h = np.empty(J, np.int32)
        col = np.empty(J, np.int32)
        sign = np.empty(J, np.int32)
        check(lib().morna_hash_keys(self._h, ptr(key_bytes), ptr(key_off), J, ptr(h), ptr(col), ptr(sign)))
        return h, col, sign

    # ---- forest ----------------------------------------------------------
    def build(self, n_trees, seed=0):
        check(lib().morna_build(self._h, int(n_trees), int(seed) & 0xFFFFFFFF))
        return True

    def get_n_trees(self):
        return int(lib().morna_get_n_trees(self._h))

    def forest_stats(self):
        st = _lib.ForestStats()
        check(lib().morna_get_forest_stats(self._h, C.byref(st)))
        return st.as_dict()

    def get_forest(self):
        """dict(node_rec [n_nodes,6], perm [T,N], hyperplanes [n_split,f], hp_node [n_split])."""
        st = self.forest_stats()
        rec = np.empty((st["n_nodes"], 6), np.int32)
        perm = np.empty((st["n_trees"], st["n_items"]), np.int32)
        hp = np.empty((max(st["n_split"], 1), self.f), np.float32)
        hp_node = np.empty(max(st["n_split"], 1), np.int32)
        check(lib().morna_get_forest(self._h, ptr(rec), ptr(perm), ptr(hp), ptr(hp_node)))
        return dict(node_rec=rec, perm=perm, hyperplanes=hp[:st["n_split"]], hp_node=hp_node[:st["n_split"]])

    def split_order(self):
        """item_at [n_items]: the item each row of the split contraction stood for in the last build (from its second level
        on), or None when that build did not order its rows.  For tests and scripts/active_pairs_probe.py."""
        out = np.empty(self.get_n_items(), np.int32)
        rc = lib().morna_debug_split_order(self._h, ptr(out))
        if rc == _lib.E_STATE:
            return None
        check(rc)
        return out

    # ---- search ------------------------------------------------------------
    def get_nns_by_vector_batch(self, Q, n, search_k=-1, n_trees=None):
        """n_trees: search the first n_trees trees only (morna_get_nns_prefix): the answer of an index built with that
        many trees on the same rows and seed; None: the whole forest."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        if Q.ndim != 2 or Q.shape[1] != self.f:
            raise IndexError("queries must be [nq, %d]" % self.f)
        nq = Q.shape[0]
        ids, d, cnt = _results(nq, n, np.float32)
        if n_trees is not None:
            check(lib().morna_get_nns_prefix(self._h, ptr(Q), None, nq, int(n), int(search_k), int(n_trees), ptr(ids), ptr(d),
                                             ptr(cnt)))
            return ids, d, cnt
        check(lib().morna_get_nns_by_vector(self._h, ptr(Q), nq, int(n), int(search_k), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def get_nns_by_item_batch(self, items, n, search_k=-1, n_trees=None):
        """n_trees: as get_nns_by_vector_batch."""
        items = np.ascontiguousarray(items, dtype=np.int32)
        nq = items.shape[0]
        ids, d, cnt = _results(nq, n, np.float32)
        if n_trees is not None:
            check(lib().morna_get_nns_prefix(self._h, None, ptr(items), nq, int(n), int(search_k), int(n_trees), ptr(ids), ptr(d),
                                             ptr(cnt)))
            return ids, d, cnt
        check(lib().morna_get_nns_by_item(self._h, ptr(items), nq, int(n), int(search_k), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def get_nns_by_vector(self, vector, n, search_k=-1, include_distances=False, n_trees=None):
        v = np.ascontiguousarray(vector, dtype=np.float32)   # annoy stores/queries fp32
        if v.shape != (self.f,):
            raise IndexError("Vector has wrong length (expected %d, got %d)" % (self.f, v.size))
        ids, d, cnt = self.get_nns_by_vector_batch(v[None, :], n, search_k, n_trees=n_trees)
        m = int(cnt[0])
        out = [int(x) for x in ids[0, :m]]
        if include_distances:
            return out, [float(x) for x in d[0, :m]]
        return out

    def _query_source(self, Q, items, qtype):
        """(Q, items, nq) of a call that takes query vectors Q (made [nq, f] of qtype), stored rows `items` (int32 [nq]) or
        neither: the rows staged by build_query_rows."""
        if Q is not None and items is not None:
            raise ValueError("give query vectors or items, not both")
        if Q is not None:
            Q = np.ascontiguousarray(Q, dtype=qtype)
            if Q.ndim != 2 or Q.shape[1] != self.f:
                raise IndexError("queries must be [nq, %d]" % self.f)
            nq = Q.shape[0]
        elif items is not None:
            items = np.ascontiguousarray(items, dtype=np.int32)
            if items.ndim != 1:
                raise ValueError("items must be one-dimensional")
            nq = items.shape[0]
        else:
            nq = getattr(self, "_qrows_n", 0)
        return Q, items, nq

    def _sweep_args(self, trees, search_ks, Q, items):
        Q, items, nq = self._query_source(Q, items, np.float32)
        trees = np.ascontiguousarray(trees, dtype=np.int32).reshape(-1)
        search_ks = np.ascontiguousarray(search_ks, dtype=np.int32).reshape(-1)
        return Q, items, nq, trees, search_ks

    def search_sweep(self, n, trees, search_ks, Q=None, items=None, lists=True):
        """Every cell of trees x search_ks from this one forest (morna_search_sweep), for the query vectors Q, the stored
        rows `items`, or (neither) the rows of build_query_rows: cell (i, j) is what
        get_nns_*_batch(..., n, search_ks[j], n_trees=trees[i]) answers.  Both lists strictly ascending and positive, at
        most 64 entries.  Returns a dict: ids / dist [n_t, n_s, nq, n] and count [n_t, n_s, nq] (lists=False: left out and
        not copied), ncand and ndots [n_t, n_s, nq] (unique candidates and hyperplane dots of every cell)."""
        Q, items, nq, trees, search_ks = self._sweep_args(trees, search_ks, Q, items)
        shape = (len(trees), len(search_ks), nq)
        out = dict(ncand=np.empty(shape, np.int32), ndots=np.empty(shape, np.int32))
        if lists:
            out.update(ids=np.empty(shape + (n,), np.int32), dist=np.empty(shape + (n,), np.float32), count=np.empty(shape, np.int32))
        check(lib().morna_search_sweep(self._h, ptr(Q), ptr(items), nq, int(n), ptr(trees), len(trees), ptr(search_ks),
                                       len(search_ks), ptr(out.get("ids")), ptr(out.get("dist")), ptr(out.get("count")),
                                       ptr(out["ncand"]), ptr(out["ndots"])))
        return out

    def recall_sweep(self, n, trees, search_ks, Q=None, items=None, lists=False):
        """search_sweep beside one exact search of the same queries (morna_recall_sweep; n <= 256): hits [n_t, n_s, nq], the
        ids every cell shares with the exact answer (-1: the exact search failed for the query, exact_count -1),
        exact_count [nq], ncand, ndots; lists=True adds ids / dist / count and exact_ids [nq, n]."""
        Q, items, nq, trees, search_ks = self._sweep_args(trees, search_ks, Q, items)
        shape = (len(trees), len(search_ks), nq)
        out = dict(hits=np.empty(shape, np.int32), exact_count=np.empty(nq, np.int32), ncand=np.empty(shape, np.int32),
                   ndots=np.empty(shape, np.int32))
        if lists:
            out.update(ids=np.empty(shape + (n,), np.int32), dist=np.empty(shape + (n,), np.float32), count=np.empty(shape, np.int32),
                       exact_ids=np.empty((nq, n), np.int32))
        check(lib().morna_recall_sweep(self._h, ptr(Q), ptr(items), nq, int(n), ptr(trees), len(trees), ptr(search_ks),
                                       len(search_ks), ptr(out["hits"]), ptr(out["exact_count"]), ptr(out["ncand"]),
                                       ptr(out["ndots"]), ptr(out.get("ids")), ptr(out.get("dist")), ptr(out.get("count")),
                                       ptr(out.get("exact_ids"))))
        return out

    def sweep_stats(self):
        """Of the last search_sweep / recall_sweep: descents, cells, rows read by canonical dots, contraction (0 / 1)."""
        return read_stats(lib().morna_search_sweep_stats, self._h, SWEEP_STATS)

    def get_nns_by_item(self, i, n, search_k=-1, include_distances=False, n_trees=None):
        ids, d, cnt = self.get_nns_by_item_batch(np.array([i], np.int32), n, search_k, n_trees=n_trees)
        m = int(cnt[0])
        out = [int(x) for x in ids[0, :m]]
        if include_distances:
            return out, [float(x) for x in d[0, :m]]
        return out

    def exact_search_batch(self, Q, n):
        """exact_search_nn (morna.py:681-716) for fp64 queries [nq, f]."""
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[1] != self.f:
            raise IndexError("queries must be [nq, %d]" % self.f)
        nq = Q.shape[0]
        ids, d, cnt = _results(nq, n, np.float64)
        check(lib().morna_exact_search(self._h, ptr(Q), nq, int(n), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def exact_search_by_item_batch(self, items, n):
        """exact_search_nn for stored rows as the queries (morna_exact_search_by_item): only the item numbers are sent."""
        items = np.ascontiguousarray(items, dtype=np.int32)
        nq = items.shape[0]
        ids, d, cnt = _results(nq, n, np.float64)
        check(lib().morna_exact_search_by_item(self._h, ptr(items), nq, int(n), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    # ---- restricted search (allow-lists and leave-out groups; no counterpart in annoy) ----
    def restriction(self, allow=None, groups=None):
        """A Restriction of this index's searches.  allow: booleans [n_items], the items a search may return (None: all);
        groups: int32 labels [n_items], negative for none (None: no item has one).  A query of a restricted search that
        carries the label g >= 0 is not answered with an item of label g."""
        n = self.get_n_items()
        bits = None
        if allow is not None:
            allow = np.asarray(allow)
            if allow.shape != (n,):
                raise ValueError("allow must hold one entry per item (%d), got shape %r" % (n, allow.shape))
            bits = pack_allow_bits(allow)
        if groups is not None:
            if np.shape(groups) != (n,):
                raise ValueError("groups must hold one label per item (%d), got shape %r" % (n, np.shape(groups)))
            groups = np.ascontiguousarray(groups, dtype=np.int32)
        out = C.c_void_p()
        check(lib().morna_restriction_create(self._h, ptr(bits), ptr(groups), C.byref(out)))
        return Restriction(self, out, groups)

    def _restriction_ptr(self, restriction, optional=True):
        """The handle of a restriction, which must be one of this index; optional: None for None."""
        if restriction is None and optional:
            return None
        if not isinstance(restriction, Restriction) or restriction.owner is not self:
            raise ValueError("the restriction was not made by this index (AnnoyIndex.restriction)")
        return restriction._p

    def _restricted_queries(self, restriction, Q, items, query_groups, qtype, optional=False):
        """(restriction pointer, Q, items, nq, query_groups): _query_source under a restriction (optional: or None), with the
        label every query carries"""
        r = self._restriction_ptr(restriction, optional)
        if restriction is None and query_groups is not None:
            raise ValueError("query groups need a restriction made with groups")
        Q, items, nq = self._query_source(Q, items, qtype)
        if query_groups is not None:
            if restriction.groups is None:
                raise ValueError("query groups need a restriction made with groups")
            query_groups = np.ascontiguousarray(query_groups, dtype=np.int32)
            if query_groups.shape != (nq,):
                raise ValueError("query_groups must hold one label per query (%d), got shape %r" % (nq, query_groups.shape))
        return r, Q, items, nq, query_groups

    def get_nns_restricted(self, restriction, n, search_k=-1, Q=None, items=None, query_groups=None):
        """get_nns_by_vector_batch (Q), get_nns_by_item_batch (items) or get_nns_by_query_rows (neither) under a
        restriction; query_groups: the label every query carries (int32 [nq], negative: none), None: no query has one."""
        r, Q, items, nq, query_groups = self._restricted_queries(restriction, Q, items, query_groups, np.float32)
        ids, d, cnt = _results(nq, n, np.float32)
        check(lib().morna_get_nns_restricted(self._h, r, ptr(Q), ptr(items), nq, ptr(query_groups), int(n),
                                             int(search_k), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def exact_search_restricted(self, restriction, n, Q=None, items=None, query_groups=None):
        """exact_search_batch (Q, fp64), exact_search_by_item_batch (items) or exact_search_query_rows (neither) under a
        restriction: the answer of the same search on an index of the eligible rows only, ids mapped back."""
        r, Q, items, nq, query_groups = self._restricted_queries(restriction, Q, items, query_groups, np.float64)
        ids, d, cnt = _results(nq, n, np.float64)
        check(lib().morna_exact_search_restricted(self._h, r, ptr(Q), ptr(items), nq, ptr(query_groups), int(n),
                                                  ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    # ---- label distance sums (include/morna_hip.h, "label distance sums"; no counterpart in annoy) ----
    def label_sums(self, item_label, n_labels, Q=None, items=None, restriction=None, query_groups=None):
        """For every query and every label, the sum of the angular distances to the items that carry the label, in fixed
        point, and their number: (sums uint64 [nq, n_labels], counts int32 [nq, n_labels]); mean distance = sums / 2**32 /
        counts.  item_label: int32 [n_items] in [-1, n_labels), -1 for none.  Queries: Q (fp64 [nq, f]), items (stored rows:
        the item itself is not counted), or neither: the staged query rows.  restriction / query_groups: as
        exact_search_restricted; None: every item is eligible."""
        item_label = self._item_labels(item_label)
        n_labels = int(n_labels)
        r, Q, items, nq, query_groups = self._restricted_queries(restriction, Q, items, query_groups, np.float64, optional=True)
        sums = np.zeros((nq, max(n_labels, 0)), np.uint64)
        counts = np.zeros((nq, max(n_labels, 0)), np.int32)
        check(lib().morna_label_sums(self._h, r, ptr(Q), ptr(items), nq, ptr(query_groups), ptr(item_label), n_labels, ptr(sums),
                                     ptr(counts)))
        return sums, counts

    def label_sums_stats(self):
        """Of the last label_sums: scan ms, sums-kernel ms, queries, batches, items counted, the scan's error bound."""
        return read_stats(lib().morna_label_sums_stats, self._h, LABEL_SUMS_STATS)

    # ---- radius search (include/morna_hip.h, "radius search"; no counterpart in annoy) ----
    def exact_radius(self, radius, Q=None, items=None, restriction=None, query_groups=None, after=None):
        """Every item within the exact fp64 distance `radius` of every query: (lists, counts).  lists[q] is (ids int32,
        dist float64) in the order of exact_search_batch (distance ascending, equal distance: higher id first); counts int64
        [nq] is the list's length, or -1 where the reference would raise (the list then ends with its NaN entries).
        Queries: Q (fp64 [nq, f]), items (stored rows), or neither: the staged query rows.  restriction / query_groups: as
        exact_search_restricted; None: every item is eligible.  after: int32 [nq], only items with id > after[q]."""
        r, Q, items, nq, query_groups = self._restricted_queries(restriction, Q, items, query_groups, np.float64, optional=True)
        if after is not None:
            after = np.ascontiguousarray(after, dtype=np.int32)
            if after.shape != (nq,):
                raise ValueError("after must hold one id per query (%d), got shape %r" % (nq, after.shape))
        out = C.c_void_p()
        check(lib().morna_exact_radius(self._h, r, ptr(Q), ptr(items), nq, ptr(query_groups), ptr(after), float(radius), C.byref(out)))
        r = out
        try:
            counts = np.zeros(nq, np.int64)
            check(lib().morna_radius_counts(r, ptr(counts)))
            # the lists lie one after the other in the result object: one copy of each array, then views per query.  A list's
            # length is its count, except where the count is -1 (asked for, query by query: they are few)
            pi, pd, n = C.c_void_p(), C.c_void_p(), C.c_int64()
            lens = counts.copy()
            for q in np.nonzero(counts < 0)[0].tolist():
                check(lib().morna_radius_query(r, q, C.byref(pi), C.byref(pd), C.byref(n)))
                lens[q] = n.value
            off = np.zeros(nq + 1, np.int64)
            np.cumsum(lens, out=off[1:])
            total = int(off[-1])
            ids, dist = np.zeros(0, np.int32), np.zeros(0, np.float64)
            if total:
                check(lib().morna_radius_query(r, 0, C.byref(pi), C.byref(pd), C.byref(n)))
                ids = np.ctypeslib.as_array(C.cast(pi, C.POINTER(C.c_int32)), shape=(total,)).copy()
                dist = np.ctypeslib.as_array(C.cast(pd, C.POINTER(C.c_double)), shape=(total,)).copy()
            off = off.tolist()
            return [(ids[off[q]:off[q + 1]], dist[off[q]:off[q + 1]]) for q in range(nq)], counts
        finally:
            lib().morna_radius_free(r)

    def exact_radius_stats(self):
        """Of the last exact_radius: scan ms, selection ms, distance ms, queries, batches, candidates (fp64 chains run),
        result entries, the window the scan values were compared with."""
        return read_stats(lib().morna_exact_radius_stats, self._h, RADIUS_STATS)

    # ---- spherical k-means (include/morna_hip.h, "spherical k-means"; no counterpart in annoy) ----
    def kmeans(self, seed_items, max_iterations=100, restriction=None):
        """Spherical k-means over the stored rows from the rows `seed_items` (distinct, eligible) as the first centroids: a dict
        of assign (int32 [n_items], -1 for a row the restriction does not allow), dist (float64 [n_items], the distance to
        the centroid the row was assigned against, -1.0 where assign is -1), centroids (float64 [k, f], the ones the last
        assignment was made against), sizes (int32 [k]), iterations and converged.  restriction: an allow-list only."""
        seeds = np.ascontiguousarray(seed_items, dtype=np.int32)
        if seeds.ndim != 1:
            raise ValueError("seed_items must be one-dimensional")
        k, n = int(seeds.shape[0]), self.get_n_items()
        assign = np.empty(n, np.int32)
        dist = np.empty(n, np.float64)
        centroids = np.empty((k, self.f), np.float64)
        sizes = np.empty(k, np.int32)
        info = np.zeros(2, np.int32)
        check(lib().morna_kmeans(self._h, self._restriction_ptr(restriction), ptr(seeds), k, int(max_iterations), ptr(assign),
                                 ptr(dist), ptr(centroids), ptr(sizes), ptr(info)))
        return dict(assign=assign, dist=dist, centroids=centroids, sizes=sizes, iterations=int(info[0]), converged=bool(info[1]))

    def kmeans_assign(self, centroids, restriction=None):
        """One assignment of every stored row to the nearest of `centroids` (fp64 [k, f]): (assign int32 [n_items], dist
        float64 [n_items]), as kmeans returns them."""
        centroids = np.ascontiguousarray(centroids, dtype=np.float64)
        if centroids.ndim != 2 or centroids.shape[1] != self.f:
            raise IndexError("centroids must be [k, %d]" % self.f)
        n = self.get_n_items()
        assign = np.empty(n, np.int32)
        dist = np.empty(n, np.float64)
        check(lib().morna_kmeans_assign(self._h, self._restriction_ptr(restriction), ptr(centroids), int(centroids.shape[0]),
                                        ptr(assign), ptr(dist)))
        return assign, dist

    def kmeans_stats(self):
        """Of the last kmeans / kmeans_assign: ms of scan, pick, resolve and update; open rows, fp64 chains run, iterations,
        the largest cluster of the last iteration."""
        return read_stats(lib().morna_kmeans_stats, self._h, KMEANS_STATS)

    # ---- label mixture (include/morna_hip.h, "label mixture"; no counterpart in annoy) ----
    def _item_labels(self, item_label):
        if np.shape(item_label) != (self.get_n_items(),):
            raise ValueError("item_label must hold one label per item (%d), got shape %r" % (self.get_n_items(), np.shape(item_label)))
        return np.ascontiguousarray(item_label, dtype=np.int32)

    def label_centroids(self, item_label, n_labels, restriction=None, gram=True):
        """The ordered fp64 sums of the unit rows of every label, as kmeans' update makes them: (sums float64 [n_labels, f],
        counts int32 [n_labels], the members that were not skipped, gram float64 [n_labels, n_labels] or None).  item_label:
        int32 [n_items] in [-1, n_labels).  restriction: an allow-list only."""
        item_label = self._item_labels(item_label)
        n_labels = int(n_labels)
        sums = np.zeros((max(n_labels, 0), self.f), np.float64)
        counts = np.zeros(max(n_labels, 0), np.int32)
        S = np.zeros((max(n_labels, 0), max(n_labels, 0)), np.float64) if gram else None
        check(lib().morna_label_centroids(self._h, self._restriction_ptr(restriction), ptr(item_label), n_labels, ptr(sums),
                                          ptr(counts), ptr(S)))
        return sums, counts, S

    def mixture(self, item_label, n_labels, Q=None, items=None, restriction=None, tol=1e-9, max_sweeps=10000):
        """Every query as a non-negative combination of the label centroids: (weights float64 [nq, n_labels], info float64
        [nq, 4] = squared residual, KKT residual, sweeps, status (1 converged, 0 not, -1 no fit), active bool [nq, n_labels]).
        Queries: Q (fp64 [nq, f]), items (stored rows: such a query is left out of its own label's centroid), or neither: the
        staged query rows.  restriction: an allow-list only."""
        item_label = self._item_labels(item_label)
        n_labels = int(n_labels)
        Q, items, nq = self._query_source(Q, items, np.float64)
        weights = np.zeros((nq, max(n_labels, 0)), np.float64)
        info = np.zeros((nq, 4), np.float64)
        active = np.zeros((nq, max(n_labels, 0)), np.uint8)
        check(lib().morna_mixture(self._h, self._restriction_ptr(restriction), ptr(Q), ptr(items), nq, ptr(item_label), n_labels,
                                  float(tol), int(max_sweeps), ptr(weights), ptr(info), ptr(active)))
        return weights, info, active.astype(bool)

    def mixture_stats(self):
        """Of the last label_centroids / mixture: ms of the centroid step, the Gram, the query dots and the solver; queries,
        sweeps summed, the largest sweep count, queries that did not converge (status != 1)."""
        return read_stats(lib().morna_mixture_stats, self._h, MIXTURE_STATS)

    # ---- principal axes (include/morna_hip.h, "principal axes"; no counterpart in annoy) ----
    def pca(self, p=10, extra=8, center=True, seed=0, tol=1e-9, max_iterations=500, restriction=None):
        """The p leading principal axes of the unit-scaled stored rows (of the allowed rows under a restriction, an allow-list
        only) by a block power iteration over p + extra columns: a dict of axes (float64 [p, f]), mean (float64 [f], zeros
        with center=False), values (float64 [p], the variances along the axes), iterations, converged, fitted (rows that
        took part) and total_variance."""
        p = int(p)
        axes = np.zeros((max(p, 0), self.f), np.float64)
        mean = np.zeros(self.f, np.float64)
        values = np.zeros(max(p, 0), np.float64)
        info = np.zeros(4, np.float64)
        check(lib().morna_pca(self._h, self._restriction_ptr(restriction), p, int(extra), 1 if center else 0, int(seed) & (2 ** 64 - 1),
                              float(tol), int(max_iterations), ptr(axes), ptr(mean), ptr(values), ptr(info)))
        return dict(axes=axes, mean=mean, values=values, iterations=int(info[0]), converged=bool(info[1]), fitted=int(info[2]),
                    total_variance=float(info[3]))

    def pca_project(self, axes, mean, Q=None, items=None):
        """The coordinates (float64 [nq, p]) of the query vectors Q (fp64 [nq, f]), the stored rows `items`, or (neither) the
        staged query rows on `axes` (fp64 [p, f]) about `mean` (fp64 [f]); NaN for a query without a direction."""
        axes = np.ascontiguousarray(axes, dtype=np.float64)
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        if axes.ndim != 2 or axes.shape[1] != self.f or mean.shape != (self.f,):
            raise IndexError("axes must be [p, %d] and mean [%d]" % (self.f, self.f))
        Q, items, nq = self._query_source(Q, items, np.float64)
        coords = np.zeros((nq, axes.shape[0]), np.float64)
        check(lib().morna_pca_project(self._h, ptr(axes), ptr(mean), int(axes.shape[0]), ptr(Q), ptr(items), nq, ptr(coords)))
        return coords

    def pca_stats(self):
        """Of the last pca: ms of the T passes, the Y passes, the orthonormalisations, the small products and the host's
        eigen step; iterations, rows fitted, bytes of rows read."""
        return read_stats(lib().morna_pca_stats, self._h, PCA_STATS)

    # ---- query rows built on the device (MornaSearch.queries_from_intropolis) ----
    def build_query_rows(self, terms):
        """Rows of the query samples of `terms` (index.ParsedLines from ParsedLines.query_terms) on this handle, beside the
        index; they replace the rows of an earlier call."""
        self._qrows_n = 0
        check(lib().morna_build_query_rows(self._h, terms._p))
        self._qrows_n = int(terms.n_items)

    def get_query_rows(self):
        """(fp64 rows [nq, f], their fp32 image [nq, f]) of the last build_query_rows."""
        nq = getattr(self, "_qrows_n", 0)
        r64 = np.empty((nq, self.f), np.float64)
        r32 = np.empty((nq, self.f), np.float32)
        check(lib().morna_get_query_rows(self._h, ptr(r64), ptr(r32)))
        return r64, r32

    def get_nns_by_query_rows(self, n, search_k=-1, n_trees=None):
        """get_nns_by_vector_batch with the resident fp32 query rows as the queries; n_trees: as there."""
        nq = getattr(self, "_qrows_n", 0)
        ids, d, cnt = _results(nq, n, np.float32)
        if n_trees is not None:
            check(lib().morna_get_nns_prefix(self._h, None, None, nq, int(n), int(search_k), int(n_trees), ptr(ids), ptr(d),
                                             ptr(cnt)))
            return ids, d, cnt
        check(lib().morna_get_nns_by_query_rows(self._h, int(n), int(search_k), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def exact_search_query_rows(self, n):
        """exact_search_batch with the resident fp64 query rows as the queries (they do not cross PCIe)."""
        nq = getattr(self, "_qrows_n", 0)
        ids, d, cnt = _results(nq, n, np.float64)
        check(lib().morna_exact_search_query_rows(self._h, int(n), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    # ---- row-sharded search, communicator inside the library (comm.hip) --------
    @staticmethod
    def comm_unique_id():
        """128 bytes from ncclGetUniqueId: made by ONE rank and handed to the others by the caller."""
        out = np.zeros(_lib.COMM_ID_BYTES, np.uint8)
        check(lib().morna_comm_unique_id(ptr(out)))
        return out.tobytes()

    def comm_init(self, unique_id, rank, world):
        uid = np.frombuffer(bytes(unique_id), np.uint8).copy()
        if len(uid) != _lib.COMM_ID_BYTES:
            raise ValueError("a communicator id has %d bytes" % _lib.COMM_ID_BYTES)
        check(lib().morna_comm_init(self._h, ptr(uid), int(rank), int(world)))

    def comm_destroy(self):
        check(lib().morna_comm_destroy(self._h))

    def comm_info(self, offsets=True):
        """(rank, world, offsets[world + 1] or None); asking for the offsets is a collective."""
        r, w = C.c_int32(), C.c_int32()
        check(lib().morna_comm_info(self._h, C.byref(r), C.byref(w), None))
        off = None
        if offsets:
            off = np.zeros(w.value + 1, np.int64)
            check(lib().morna_comm_info(self._h, C.byref(r), C.byref(w), ptr(off)))
        return r.value, w.value, off

    def get_nns_by_vector_sharded(self, Q, n, search_k=-1):
        """Q: [nq, f] fp32 (host array) or (device pointer, nq); the same on every rank.  Merged global ids."""
        if isinstance(Q, tuple):
            q_ptr, nq = C.c_void_p(int(Q[0])), int(Q[1])
        else:
            Q = np.ascontiguousarray(Q, dtype=np.float32)
            q_ptr, nq = ptr(Q), Q.shape[0]
        ids, d, cnt = _results(nq, n, np.float32)
        check(lib().morna_get_nns_by_vector_sharded(self._h, q_ptr, nq, int(n), int(search_k), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def get_nns_by_item_sharded(self, local_items, n, search_k=-1, n_each=None):
        """Every rank's own items as queries; answers for all ranks' queries (rank 0's first).  n_each: every rank's
        query count -- the output arrays are sized from it (the C entry point can exchange the counts itself; a caller
        that does not know them all-gathers them first, as dist.ShardedSearch does)."""
        items = np.ascontiguousarray(local_items, dtype=np.int32)
        if n_each is None:
            if self.comm_info(offsets=False)[1] != 1:
                raise ValueError("n_each (every rank's query count) is required when there is more than one rank")
            n_each = [len(items)]
        n_each = np.ascontiguousarray(n_each, dtype=np.int64)
        nq = int(n_each.sum())
        ids, d, cnt = _results(nq, n, np.float32)
        check(lib().morna_get_nns_by_item_sharded(self._h, ptr(items), len(items), ptr(n_each), int(n), int(search_k),
                                                  ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def exact_search_sharded(self, Q, n):
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        nq = Q.shape[0]
        ids, d, cnt = _results(nq, n, np.float64)
        check(lib().morna_exact_search_sharded(self._h, ptr(Q), nq, int(n), ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    def exact_search_by_item_sharded(self, local_items, n, n_each):
        items = np.ascontiguousarray(local_items, dtype=np.int32)
        n_each = np.ascontiguousarray(n_each, dtype=np.int64)
        nq = int(n_each.sum())
        ids, d, cnt = _results(nq, n, np.float64)
        check(lib().morna_exact_search_by_item_sharded(self._h, ptr(items), len(items), ptr(n_each), int(n),
                                                       ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    @staticmethod
    def exact_packed_bytes(nq, n):
        return int(lib().morna_exact_packed_bytes(int(nq), int(n)))

    def exact_search_packed(self, packed_ptr, n, id_offset, Q=None, q_dev=None, items=None):
        """Per-shard exact answers packed in HBM at packed_ptr (exact_packed_bytes(nq, n) bytes), enqueued."""
        qp = dp = ip = None
        if Q is not None:
            Q = np.ascontiguousarray(Q, dtype=np.float64)
            qp, nq = ptr(Q), Q.shape[0]
        elif q_dev is not None:
            dp, nq = C.c_void_p(int(q_dev[0])), int(q_dev[1])
        else:
            items = np.ascontiguousarray(items, dtype=np.int32)
            ip, nq = ptr(items), len(items)
        check(lib().morna_exact_search_packed(self._h, qp, dp, ip, nq, int(n), int(id_offset), C.c_void_p(int(packed_ptr))))

    def merge_exact_packed(self, gathered_ptr, world, nq, kk, n):
        ids, d, cnt = _results(nq, n, np.float64)
        check(lib().morna_merge_exact_packed(self._h, C.c_void_p(int(gathered_ptr)), int(world), int(nq), int(kk), int(n),
                                             ptr(ids), ptr(d), ptr(cnt)))
        return ids, d, cnt

    # ---- persistence ---------------------------------------------------------
    def save(self, fn):
        check(lib().morna_save(self._h, str(fn).encode()))
        return True

    def load(self, fn):
        check(lib().morna_load(self._h, str(fn).encode()))
        return True

    # ---- measurement -----------------------------------------------------------
    def timer_enable(self, on=True, only=None):
        """only: names of the kernel groups to bracket with events (default: all of them)."""
        mask = (1 if on else 0) if only is None else sum(2 << _lib.TIMER_NAMES.index(n) for n in only)
        check(lib().morna_timer_enable(self._h, mask))

    def timer_reset(self):
        check(lib().morna_timer_reset(self._h))

    def timers(self):
        out = {}
        for i, name in enumerate(_lib.TIMER_NAMES):
            ms, n, b = C.c_double(0), C.c_int64(0), C.c_int64(0)
            check(lib().morna_timer_read(self._h, i, C.byref(ms), C.byref(n), C.byref(b)))
            out[name] = dict(ms=ms.value, launches=n.value, bytes=b.value)
        return out

    def synchronize(self):
        check(lib().morna_synchronize(self._h))
