"""The helpers the binding layers share (annoy.py, junctions.py, _lib.py, search.py), with no library loaded: the query
source of a call, the reader behind every *_stats method, the CSR of unhashed queries, the refusal on an index of row
shards, and the statistics and the chunk loop of the label scans."""
import numpy as np
import pytest

from morna_amd import _lib, annoy, junctions, search
from morna_amd.annoy import AnnoyIndex
from morna_amd.search import MornaSearch


def _index(f=4, staged=3):
    a = AnnoyIndex.__new__(AnnoyIndex)          # (no handle: nothing here reaches the library)
    a.f, a._qrows_n = f, staged
    return a


# ---------------------------------------------------------------------------------------------------- AnnoyIndex._query_source

@pytest.mark.parametrize("qtype", [np.float32, np.float64])
def test_query_source_vectors_items_and_staged_rows(qtype):
    a = _index()
    Q, items, nq = a._query_source([[1, 2, 3, 4], [5, 6, 7, 8]], None, qtype)
    assert (items, nq) == (None, 2) and Q.dtype == qtype and Q.shape == (2, 4) and Q.flags.c_contiguous
    Q, items, nq = a._query_source(None, [7, 1, 2, 9, 0], qtype)
    assert (Q, nq) == (None, 5) and items.dtype == np.int32 and items.tolist() == [7, 1, 2, 9, 0]
    assert a._query_source(None, None, qtype) == (None, None, 3)
    fresh = AnnoyIndex.__new__(AnnoyIndex)
    fresh.f = 4
    assert fresh._query_source(None, None, qtype) == (None, None, 0)         # nothing staged yet


def test_query_source_refusals():
    a = _index()
    with pytest.raises(ValueError) as e:
        a._query_source(np.zeros((1, 4)), [0], np.float64)
    assert str(e.value) == "give query vectors or items, not both"
    for bad in (np.zeros(4), np.zeros((2, 5)), np.zeros((2, 2, 4))):
        with pytest.raises(IndexError) as e:
            a._query_source(bad, None, np.float32)
        assert str(e.value) == "queries must be [nq, 4]"
    with pytest.raises(ValueError) as e:
        a._query_source(None, [[0, 1], [2, 3]], np.float32)
    assert str(e.value) == "items must be one-dimensional"


def test_restricted_queries_without_a_restriction():
    a = _index()
    assert a._restricted_queries(None, None, [1, 2], None, np.float64, optional=True)[0] is None
    with pytest.raises(ValueError, match="query groups need a restriction made with groups"):
        a._restricted_queries(None, None, [1, 2], [0, 0], np.float64, optional=True)
    for call in (lambda: a._restricted_queries(None, None, [1, 2], None, np.float64), lambda: a._restriction_ptr(object())):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "the restriction was not made by this index (AnnoyIndex.restriction)"


def test_results_buffers():
    ids, d, cnt = annoy._results(3, 5, np.float64)
    assert (ids.shape, ids.dtype, d.shape, d.dtype, cnt.shape, cnt.dtype) == ((3, 5), np.int32, (3, 5), np.float64, (3,), np.int32)
    assert annoy._results(0, 2, np.float32)[1].dtype == np.float32


# ------------------------------------------------------------------------------------------------------------ _lib.read_stats

STATS_TABLES = {
    "sweep": (annoy.SWEEP_STATS, "descents cells rows_canonical contraction", "iiii"),
    "label_sums": (annoy.LABEL_SUMS_STATS, "scan_ms sums_ms queries batches counted scan_eps", "ffiiif"),
    "exact_radius": (annoy.RADIUS_STATS, "scan_ms select_ms dist_ms queries batches candidates results window", "fffiiiif"),
    "kmeans": (annoy.KMEANS_STATS, "scan_ms pick_ms resolve_ms update_ms open_rows chains iterations largest", "ffffiiii"),
    "mixture": (annoy.MIXTURE_STATS, "centroids_ms gram_ms dots_ms solve_ms queries sweeps max_sweeps open", "ffffiiii"),
    "nearest": (junctions.NEAREST_STATS, "candidates max_candidates passes kernel_ms bytes queries_per_pass norms_ms window", "iiifiiff"),
    "explain": (junctions.EXPLAIN_STATS, "pairs entries passes kernel_ms bytes queries_per_pass", "iiifii"),
    "recovery": (junctions.RECOVERY_STATS, "kernel_ms bytes workgroups", "fii"),
    "pool": (junctions.POOL_STATS, "kernel_ms bytes_read bytes_written workgroups", "fiii"),
    "thin": (junctions.THIN_STATS, "kernel_ms bytes_read bytes_written draws workgroups", "fiiii"),
    "hash_rows": (junctions.HASH_ROWS_STATS, "kernel_ms bytes_read bytes_written workgroups", "fiii"),
}


@pytest.mark.parametrize("which", sorted(STATS_TABLES))
def test_read_stats_keys_order_and_types(which, monkeypatch):
    fields, keys, kinds = STATS_TABLES[which]
    monkeypatch.setattr(_lib, "check", lambda rc: None if rc == 0 else pytest.fail("rc %d" % rc))
    seen = []

    def fn(handle, p):                          # fills 0, 1, 2, ... as a morna_*_stats call fills its doubles
        import ctypes as C
        seen.append(handle)
        out = C.cast(p, C.POINTER(C.c_double))
        for i in range(len(fields)):
            out[i] = float(i)
        return 0
    got = _lib.read_stats(fn, "the handle", fields)
    assert seen == ["the handle"]
    assert list(got) == keys.split() and list(got.values()) == list(range(len(fields)))
    assert [type(v) for v in got.values()] == [int if c == "i" else float for c in kinds]


def test_read_stats_raises_what_check_raises(monkeypatch):
    def check(rc):
        raise ValueError("label_sums_stats: null pointer")
    monkeypatch.setattr(_lib, "check", check)
    with pytest.raises(ValueError, match="null pointer"):
        _lib.read_stats(lambda h, p: -1, None, annoy.LABEL_SUMS_STATS)


# ------------------------------------------------------------------------------------------------------ junctions._pack_queries

def test_pack_queries():
    q_ptr, q_line, q_cov = junctions._pack_queries([])
    assert q_ptr.tolist() == [0] and (q_ptr.dtype, q_line.dtype, q_cov.dtype) == (np.int64, np.int32, np.int32)
    assert len(q_line) == 0 and len(q_cov) == 0
    q_ptr, q_line, q_cov = junctions._pack_queries([([], [])])
    assert q_ptr.tolist() == [0, 0] and len(q_line) == 0 and q_line.dtype == np.int32
    q_ptr, q_line, q_cov = junctions._pack_queries([([2, 5, 9], [1, 1, 4]), (np.array([7]), np.array([3], np.int64))])
    assert q_ptr.tolist() == [0, 3, 4] and q_line.tolist() == [2, 5, 9, 7] and q_cov.tolist() == [1, 1, 4, 3]
    assert (q_line.dtype, q_cov.dtype) == (np.int32, np.int32)
    for bad in ([([1, 2], [1])], [([[1, 2]], [[1, 2]])]):
        with pytest.raises(ValueError) as e:
            junctions._pack_queries(bad)
        assert str(e.value) == "an unhashed query is a pair of 1-d arrays of one length: lines and coverages"


# ------------------------------------------------------------------------------------------------- MornaSearch._device_index

def _search(kind):
    from morna_amd.shards import DistShards, LocalShards
    s = MornaSearch.__new__(MornaSearch)
    cls = {"index": AnnoyIndex, "local": LocalShards, "dist": DistShards}[kind]
    s.annoy_index = cls.__new__(cls)
    s.sample_count = 10
    return s


TORCHRUN = ("batch search is not available with one process per shard (torchrun): run it in one process, which loads every "
            "shard of the index")


def test_device_index_refusals():
    _search("index")._device_index()
    _search("index")._device_index(search.LABELS_SHARDS_REFUSAL)
    _search("local")._device_index()                                   # in-process shards serve the batch searches
    with pytest.raises(ValueError) as e:
        _search("local")._device_index(search.LABELS_SHARDS_REFUSAL)
    assert str(e.value) == search.LABELS_SHARDS_REFUSAL
    for refusal in (None, search.MIXTURE_SHARDS_REFUSAL):              # one process per shard: the RuntimeError comes first
        with pytest.raises(RuntimeError) as e:
            _search("dist")._device_index(refusal)
        assert str(e.value) == TORCHRUN


def test_callers_of_device_index():
    for call in (lambda s: s._check_batch_possible(), lambda s: s.search_member_n_batch([1], 5, -1), lambda s: s.junction_store(),
                 lambda s: s.cluster_samples(k=2), lambda s: s.search_recall([0], 5, [1], [10]),
                 lambda s: s.label_separation([0], [("a", [1])]), lambda s: s.label_mixture([0], [("a", [1])])):
        s = _search("dist")
        s._junction_store = None
        with pytest.raises(RuntimeError) as e:
            call(s)
        assert str(e.value) == TORCHRUN
    for call, refusal in ((lambda s: s.cluster_samples(k=2), search.CLUSTER_SHARDS_REFUSAL),
                          (lambda s: s.search_recall([0], 5, [1], [10]), search.TREES_SHARDS_REFUSAL),
                          (lambda s: s.label_separation([0], [("a", [1])]), search.LABELS_SHARDS_REFUSAL),
                          (lambda s: s.label_mixture([0], [("a", [1])]), search.MIXTURE_SHARDS_REFUSAL)):
        with pytest.raises(ValueError) as e:
            call(_search("local"))
        assert str(e.value) == refusal
    _search("local")._check_batch_possible()                           # only the first check
    s = _search("local")
    s.internal_id_map = {}
    with pytest.raises(ValueError, match="Querying sample id 1 is not possible because no internal id is mapped"):
        s.search_member_n_batch([1], 5, -1)


def test_internal_ids():
    s = MornaSearch.__new__(MornaSearch)
    s.internal_id_map = {10: 0, 12: 1}
    assert s._internal_ids([12, 10, 12]) == [1, 0, 1]
    with pytest.raises(ValueError) as e:
        s._internal_ids([10, 11])
    assert str(e.value) == ("Querying sample id 11 is not possible because no internal id is mapped to that sample id. Likely no "
                            "sample with that id was included in the index.")


# ------------------------------------------------------------------------------------------ the label scans' shared pieces

def test_accumulate_stats_sums_and_maxima():
    total = {name: kind() for name, kind in annoy.LABEL_SUMS_STATS}
    assert total == dict(scan_ms=0.0, sums_ms=0.0, queries=0, batches=0, counted=0, scan_eps=0.0)
    search.accumulate_stats(total, dict(scan_ms=1.5, sums_ms=0.25, queries=4, batches=1, counted=30, scan_eps=2e-7), maxima=("scan_eps",))
    search.accumulate_stats(total, dict(scan_ms=0.5, sums_ms=0.5, queries=3, batches=2, counted=12, scan_eps=1e-7), maxima=("scan_eps",))
    assert total == dict(scan_ms=2.0, sums_ms=0.75, queries=7, batches=3, counted=42, scan_eps=2e-7)
    assert [type(v) for v in total.values()] == [float, float, int, int, int, float]
    total = {name: kind() for name, kind in annoy.MIXTURE_STATS}
    for sweeps, most in ((10, 4), (25, 9), (3, 2)):
        search.accumulate_stats(total, dict(centroids_ms=1.0, gram_ms=0.0, dots_ms=0.0, solve_ms=2.0, queries=2, sweeps=sweeps,
                                            max_sweeps=most, open=1), maxima=("max_sweeps",))
    assert (total["sweeps"], total["max_sweeps"], total["open"], total["queries"], total["solve_ms"]) == (38, 9, 3, 6, 6.0)


def test_vectors_or_items():
    source, q = search.vectors_or_items(np.zeros((2, 4), np.float32))
    assert source == "Q" and q.dtype == np.float64 and q.shape == (2, 4)
    source, q = search.vectors_or_items(iter([3, 1, 2]))
    assert source == "items" and q.dtype == np.int32 and q.tolist() == [3, 1, 2]
    assert search.vectors_or_items(np.array([4, 5]))[0] == "items"


def test_chunked_call_slices_and_assembly():
    slices = []

    def call(q0, q1):
        slices.append((q0, q1))
        return np.arange(q0, q1) * 10, np.arange(q0, q1)[:, None] * np.ones((1, 2))
    a, b = np.full(5, -1), np.full((5, 2), -1.0)
    search.chunked_call(call, 5, 2, (a, b))
    assert slices == [(0, 2), (2, 4), (4, 5)]
    assert a.tolist() == [0, 10, 20, 30, 40] and b[:, 1].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    slices[:] = []
    search.chunked_call(call, 0, 2, (a, b))
    assert slices == []


def test_result_rows_shared_by_both_shapes():
    s = MornaSearch.__new__(MornaSearch)
    ids = np.array([[4, 2, -1], [7, -1, -1], [0, 0, 0]], np.int32)
    d = np.array([[0.5, 1.0, np.inf], [0.25, np.inf, np.inf], [0, 0, 0]])
    cnt = np.array([2, 1, -1], np.int32)
    rows = s._batch_results(ids, d, cnt, True, False)
    assert rows[0] == ([4, 2], [0.5, 1.0]) and rows[1] == ([7], [0.25]) and isinstance(rows[2], ValueError)
    assert s._batch_results(ids, d, cnt, False, False)[0] == ([4, 2],)
    lists = [(ids[0, :2], d[0, :2]), (ids[1, :1], d[1, :1]), (ids[2, :0], d[2, :0])]
    assert s._radius_results(lists, [2, 1, -1], True, False, None)[:2] == rows[:2]
    assert s._radius_results(lists, [2, 1, -1], True, False, 1)[0] == ([4], [0.5])
    assert all(type(x) is int for x in rows[0][0]) and all(type(x) is float for x in rows[0][1])
