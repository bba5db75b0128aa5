"""morna_add_items_from_store on the GPU: the hashed rows of store rows, byte for byte the restatement of
test_hashrows_cpu.py (ref_hash_rows: Python floats, sequential per cell) at every width, the canonical norms and the state
of the handle afterwards those of a second handle given the same rows through add_items, the refusals through the raw call,
the statistics, and morna_jstore_row_norms.  Stores are made from arrays.  -m gpu"""
import ctypes as C

import numpy as np
import pytest

from test_hashrows_cpu import ref_hash_rows
from test_unhashed_cpu import RefUnhashed

pytestmark = pytest.mark.gpu

N_LINES, N_SAMPLES = 3000, 200
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
SAME = slice(1000, 1300)              # a run of 300 lines with one and the same hash
# 16384 fp64 cells are the most one pass of the kernel holds in LDS: 16384 is the last one-pass width, 16385 and 32768 take two;
# up to 8960 cells a workgroup has 256 threads (four waves share the cells), past them 512 (eight)
WIDTHS = [1, 2, 3, 40, 256, 257, 3000, 8960, 8961, 16384, 16385, 32768]


def ext_of(i):
    return 500 + 2 * i


def make_store(rows, n_lines, w=None):
    from morna_amd.junctions import JunctionStore
    ext = np.array([ext_of(i) for i in range(len(rows))], np.int64)
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(l) for l, _ in rows])
    line = np.concatenate([np.asarray(l, np.int32) for l, _ in rows] + [np.zeros(0, np.int32)])
    cov = np.concatenate([np.asarray(c, np.int32) for _, c in rows] + [np.zeros(0, np.int32)])
    store = JunctionStore.from_arrays(ext, ptr, line, cov, n_lines)
    if w is not None:
        store.set_weights(w)
    return store, ext


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(12)
    w = np.where(rng.random(N_LINES) < 0.25, 0.0, rng.uniform(0.05, 6.0, N_LINES))          # zeros interleaved
    w[:4] = [1.5, 0.75, 2.0, 3.0]
    line_hash = rng.integers(INT32_MIN, INT32_MAX + 1, N_LINES).astype(np.int32)
    line_hash[:4] = [0, -1, INT32_MIN, INT32_MAX]
    line_hash[SAME] = 123456789
    assert (w[SAME] != 0).sum() > 150 and (w[SAME] == 0).sum() > 30
    lengths = LENGTHS + [int(x) for x in rng.integers(1, 400, N_SAMPLES - len(LENGTHS))]
    rows = []
    for i, n in enumerate(lengths):
        if n == 1000:                  # the long row holds the four special hashes and the whole run
            fixed = np.concatenate([np.arange(4), np.arange(SAME.start, SAME.stop)])
            rest = rng.choice(np.setdiff1d(np.arange(N_LINES), fixed), size=n - len(fixed), replace=False)
            l = np.sort(np.concatenate([fixed, rest])).astype(np.int32)
        else:
            l = np.sort(rng.choice(N_LINES, size=n, replace=False)).astype(np.int32)
        c = np.ceil(rng.lognormal(1.0, 1.5, size=n)).astype(np.int64)
        if n >= 63:                    # coverages 0, negative and 2^31 - 1 among the others
            at = rng.choice(n, size=9, replace=False)
            c[at[:3]], c[at[3:6]], c[at[6:]] = 0, -c[at[3:6]] - 1, INT32_MAX
        rows.append((l, c.astype(np.int32)))
    assert any((c < 0).any() for _, c in rows)
    store, ext = make_store(rows, N_LINES, w)
    return dict(rows=rows, w=w, line_hash=line_hash, store=store, ext=ext, ref={})


def reference(world, D):
    """ref_hash_rows of every row at width D, computed once."""
    if D not in world["ref"]:
        world["ref"][D] = ref_hash_rows(world["rows"], world["w"], world["line_hash"], D)
    return world["ref"][D]


def twin(rows32):
    """A second handle given the same rows through add_items."""
    from morna_amd.annoy import AnnoyIndex
    t = AnnoyIndex(rows32.shape[1])
    t.add_items(rows32)
    return t


# ---- byte for byte against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_rows_and_norms_at_every_width(world, D):
    from morna_amd.annoy import AnnoyIndex
    want = reference(world, D)
    h = AnnoyIndex(D)
    h.add_items_from_store(world["store"], world["ext"], world["line_hash"])
    assert h.get_n_items() == N_SAMPLES
    got = h.get_items()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()
    assert not got[0].any() and np.count_nonzero(got[8]) > 0                # the row without entries; the long row
    assert h.get_norms2().tobytes() == twin(want).get_norms2().tobytes()
    stats = world["store"].hash_rows_stats()
    entries = sum(len(l) for l, _ in world["rows"])
    assert stats["kernel_ms"] > 0 and stats["workgroups"] == N_SAMPLES
    assert stats["bytes_read"] == 8 * entries + 12 * N_LINES
    assert stats["bytes_written"] == 4 * N_SAMPLES * ((D + 255) // 256 * 256)


def test_one_chain_and_the_floored_modulo(world):
    """D = 1: every entry of a row in one cell, one chain.  D = 3: the negative hashes' floored modulo."""
    one = reference(world, 1)
    l, c = world["rows"][8]
    s = 0.0
    for j, cov in zip(l.tolist(), c.tolist()):
        if world["w"][j] != 0.0:
            t = float(cov) * float(world["w"][j])
            s = s + (-t if world["line_hash"][j] < 0 else t)
    assert one[8, 0] == np.float32(s)
    assert (-1) % 3 == 2 and INT32_MIN % 3 == 1                                         # Python's, which the contract names
    only = [(np.array([1], np.int32), np.array([4], np.int32)), (np.array([2], np.int32), np.array([4], np.int32))]
    three = ref_hash_rows(only, world["w"], world["line_hash"], 3)
    assert three.tolist() == [[0, 0, -3.0], [0, -8.0, 0]]
    from morna_amd.annoy import AnnoyIndex
    store, ext = make_store(only, N_LINES, world["w"])
    h = AnnoyIndex(3)
    h.add_items_from_store(store, ext, world["line_hash"])
    assert h.get_items().tobytes() == three.tobytes()


# ---- the order probe ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("places", [(10, 11, 12), (254, 255, 256), (0, 257, 514)],
                         ids=["one_chunk", "across_a_chunk_edge", "256_entries_between"])
def test_terms_of_a_cell_are_added_in_line_order(places):
    """A cell whose terms are, in line order, +2^60, +1, -2^60 is 0.0; in any other order it is 1.0."""
    from morna_amd.annoy import AnnoyIndex
    D, cell, n = 40, 5, 600
    assert (2.0 ** 60 + 1.0) - 2.0 ** 60 == 0.0 and (2.0 ** 60 - 2.0 ** 60) + 1.0 == 1.0 and (1.0 - 2.0 ** 60) + 2.0 ** 60 == 0.0
    rng = np.random.default_rng(places[1])
    line_hash = (rng.integers(0, 1000, n) * D + rng.integers(6, 35, n)).astype(np.int32)  # the others: columns 6 .. 34
    line_hash[rng.random(n) < 0.5] *= -1                                                  # (negated: D - column, 6 .. 34 again)
    w = rng.uniform(0.5, 2.0, n)
    a, b, c = places
    line_hash[[a, b, c]] = [cell, cell + 7 * D, cell - 3 * D]
    w[[a, b, c]] = [2.0 ** 60, 1.0, 2.0 ** 60]
    assert [int(x) % D for x in line_hash[[a, b, c]]] == [cell] * 3 and int(((line_hash.astype(np.int64) % D) == cell).sum()) == 3
    rows = [(np.arange(n, dtype=np.int32), np.ones(n, np.int32)), (np.array([a, b, c], np.int32), np.ones(3, np.int32))]
    store, ext = make_store(rows, n, w)
    h = AnnoyIndex(D)
    h.add_items_from_store(store, ext, line_hash)
    got = h.get_items()
    assert got[0, cell] == 0.0 and got[1, cell] == 0.0
    assert got.tobytes() == ref_hash_rows(rows, w, line_hash, D).tobytes()


# ---- independence and determinism --------------------------------------------------------------------------------------------
def test_a_row_does_not_depend_on_the_batch_or_the_call(world):
    from morna_amd.annoy import AnnoyIndex
    store, ext, line_hash = world["store"], world["ext"], world["line_hash"]
    want = reference(world, 3000)
    h = AnnoyIndex(3000)
    h.add_items_from_store(store, ext[8:9], line_hash)                                  # alone
    assert h.get_n_items() == 1 and h.get_items().tobytes() == want[8:9].tobytes()
    batch = [int(x) for x in ext[100:132]] + [int(ext[8])] + [int(x) for x in ext[40:72]]   # inside a batch of 65
    h.add_items_from_store(store, batch, line_hash)
    got = h.get_items()
    assert got.shape[0] == 65 and got[32].tobytes() == want[8].tobytes()
    assert got.tobytes() == want[[(int(e) - 500) // 2 for e in batch]].tobytes()
    h.add_items_from_store(store, [ext[8], ext[5], ext[8]], line_hash)                  # the same id named twice
    got = h.get_items()
    assert got[0].tobytes() == got[2].tobytes() == want[8].tobytes() and got[1].tobytes() == want[5].tobytes()
    assert store.hash_rows_stats()["bytes_read"] == 8 * (2 * 1000 + 255) + 12 * N_LINES
    first = AnnoyIndex(3000)
    first.add_items_from_store(store, ext, line_hash)
    a = first.get_items()
    first.add_items_from_store(store, ext, line_hash)                                   # two calls
    assert first.get_items().tobytes() == a.tobytes() == want.tobytes()
    narrow = AnnoyIndex(64)                                                             # another width of the same store
    narrow.add_items_from_store(store, ext, line_hash)
    assert narrow.get_items().tobytes() == ref_hash_rows(world["rows"], world["w"], line_hash, 64).tobytes()
    assert first.get_items().tobytes() == want.tobytes()
    other = (line_hash.astype(np.int64) * 31 % 65521).astype(np.int32)                  # other hashes, then the first again
    narrow.add_items_from_store(store, ext, other)
    assert narrow.get_items().tobytes() == ref_hash_rows(world["rows"], world["w"], other, 64).tobytes()
    narrow.add_items_from_store(store, ext, line_hash.copy())
    assert narrow.get_items().tobytes() == ref_hash_rows(world["rows"], world["w"], line_hash, 64).tobytes()


def test_other_weights_give_other_rows(world):
    """set_weights between two calls: the rows are those of the weights set, not of the first call's."""
    from morna_amd.annoy import AnnoyIndex
    w2 = np.where(world["w"] == 0, 1.0, 0.0) + np.roll(world["w"], 7)
    store, ext = make_store(world["rows"][:20], N_LINES, world["w"])
    h = AnnoyIndex(40)
    h.add_items_from_store(store, ext, world["line_hash"])
    assert h.get_items().tobytes() == reference(world, 40)[:20].tobytes()
    store.set_weights(w2)
    h.add_items_from_store(store, ext, world["line_hash"])
    assert h.get_items().tobytes() == ref_hash_rows(world["rows"][:20], w2, world["line_hash"], 40).tobytes()


_WALK_CHILD = """
import hashlib, sys
import numpy as np
sys.path.insert(0, %r)
from morna_amd.annoy import AnnoyIndex
from morna_amd.junctions import JunctionStore
z = np.load(%r)
store = JunctionStore.from_arrays(z["ext"], z["ptr"], z["line"], z["cov"], int(z["n_lines"]))
store.set_weights(z["w"])
for D in (1, 40, 3000, 16385):
    h = AnnoyIndex(D)
    h.add_items_from_store(store, z["ext"], z["line_hash"])
    print(D, hashlib.sha256(h.get_items().tobytes()).hexdigest(), hashlib.sha256(h.get_norms2().tobytes()).hexdigest())
"""


def test_the_walk_form_gives_the_same_bytes(world, tmp_path):
    """MORNA_HASHROWS_WALK=1, read once per process: a process of its own makes the rows with the form in which every thread
    walks every staged entry; their digests are those of the restatement."""
    import hashlib
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = world["rows"]
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(l) for l, _ in rows])
    path = str(tmp_path / "store.npz")
    np.savez(path, ext=world["ext"], ptr=ptr, line=np.concatenate([l for l, _ in rows]), cov=np.concatenate([c for _, c in rows]),
             n_lines=N_LINES, w=world["w"], line_hash=world["line_hash"])
    r = subprocess.run([sys.executable, "-c", _WALK_CHILD % (root, path)], env=dict(os.environ, MORNA_HASHROWS_WALK="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [line.split() for line in r.stdout.splitlines()]
    assert [int(g[0]) for g in got] == [1, 40, 3000, 16385]
    for D, rows_digest, norms_digest in got:
        want = reference(world, int(D))
        assert rows_digest == hashlib.sha256(want.tobytes()).hexdigest(), D
        assert norms_digest == hashlib.sha256(twin(want).get_norms2().tobytes()).hexdigest(), D


# ---- the handle afterwards -----------------------------------------------------------------------------------------------------
def test_the_handle_searches_and_builds_as_one_given_the_rows(world):
    from morna_amd.annoy import AnnoyIndex
    D = 40
    want = reference(world, D)
    h = AnnoyIndex(D)
    h.add_items(np.ones((7, D), np.float32))                       # host rows, norms and an exact search of earlier items
    h.exact_search_by_item_batch(np.arange(7, dtype=np.int32), 3)
    h.add_items_from_store(world["store"], world["ext"], world["line_hash"])
    t = twin(want)
    items = np.arange(N_SAMPLES, dtype=np.int32)
    def same(a, b):                                                # (ids, distances, counts): the lists up to their counts
        assert a[2].tobytes() == b[2].tobytes() and (a[2] > 0).any()
        for q, m in enumerate(np.maximum(a[2], 0).tolist()):
            assert a[0][q, :m].tobytes() == b[0][q, :m].tobytes() and a[1][q, :m].tobytes() == b[1][q, :m].tobytes()

    same(h.exact_search_by_item_batch(items, 12), t.exact_search_by_item_batch(items, 12))
    h.build(4)
    t.build(4)
    same(h.get_nns_by_item_batch(items, 12, 60), t.get_nns_by_item_batch(items, 12, 60))
    fa, fb = h.get_forest(), t.get_forest()
    assert sorted(fa) == sorted(fb)
    for key in fa:
        assert fa[key].tobytes() == fb[key].tobytes(), key
    assert h.get_items().tobytes() == want.tobytes()
    with pytest.raises(RuntimeError, match="You can't add an item to a built index"):
        h.add_items_from_store(world["store"], world["ext"], world["line_hash"])
    # and items added to it afterwards sit beside the rows from the store
    g = AnnoyIndex(D)
    g.add_items_from_store(world["store"], world["ext"][:5], world["line_hash"])
    g.add_items(np.full((1, D), 2.0, np.float32), first_id=5)
    got = g.get_items()
    assert got.shape == (6, D) and got[:5].tobytes() == want[:5].tobytes() and (got[5] == 2.0).all()


# ---- the refusals, through the raw call ------------------------------------------------------------------------------------------
def test_refusals_leave_the_store_and_the_handle_usable(world):
    from morna_amd import _lib
    from morna_amd.annoy import AnnoyIndex
    from morna_amd._lib import lib, ptr
    nonneg = [(l, np.abs(c.astype(np.int64)).clip(0, 1000).astype(np.int32)) for l, c in world["rows"][:40]]
    store, ext = make_store(nonneg, N_LINES, world["w"])
    line_hash = world["line_hash"]
    lists = [[int(x) for x in ext[:9]], [int(x) for x in ext[20:30]]]
    kept = store.retain(lists, 0.3, 5)
    near = store.nearest_by_sample(ext, ext[:6], 5)
    h = AnnoyIndex(40)
    h.add_items_from_store(store, ext, line_hash)
    rows = h.get_items()
    assert store.hash_rows_stats()["kernel_ms"] > 0

    def call(handle, st, ids, n, hashes, n_lines):
        rc = lib().morna_add_items_from_store(handle, st, ptr(ids), n, ptr(hashes), n_lines)
        stats = store.hash_rows_stats()
        if rc != _lib.OK and st is not None:
            assert stats == {"kernel_ms": 0.0, "bytes_read": 0, "bytes_written": 0, "workgroups": 0}
        return rc, lib().morna_last_error().decode()

    ids = np.ascontiguousarray(ext, np.int64)
    assert call(None, store._p, ids, len(ids), line_hash, N_LINES)[0] == _lib.E_INVALID
    assert call(h._h, None, ids, len(ids), line_hash, N_LINES)[0] == _lib.E_INVALID
    assert call(h._h, store._p, None, len(ids), line_hash, N_LINES)[0] == _lib.E_INVALID
    assert call(h._h, store._p, ids, len(ids), None, N_LINES)[0] == _lib.E_INVALID
    rc, msg = call(h._h, store._p, ids, len(ids), line_hash[:-1].copy(), N_LINES - 1)
    assert rc == _lib.E_INVALID and str(N_LINES - 1) in msg and str(N_LINES) in msg
    if _lib.device_count() >= 2:
        far = AnnoyIndex(40, device=1)
        rc, msg = call(far._h, store._p, ids, len(ids), line_hash, N_LINES)
        assert rc == _lib.E_INVALID and "device 1" in msg and "device 0" in msg
    bare, _ = make_store(nonneg[:3], N_LINES)
    rc, msg = call(h._h, bare._p, ids[:3].copy(), 3, line_hash, N_LINES)
    assert rc == _lib.E_STATE and "weights" in msg
    built = AnnoyIndex(40)
    built.add_items(rows)
    built.build(2)
    rc, msg = call(built._h, store._p, ids, len(ids), line_hash, N_LINES)
    assert rc == _lib.E_STATE and msg == "You can't add an item to a built index"
    unknown = ids.copy()
    unknown[5] = 424243
    rc, msg = call(h._h, store._p, unknown, len(ids), line_hash, N_LINES)
    assert rc == _lib.E_RANGE and "424243" in msg
    rc, msg = call(h._h, store._p, ids, 0, line_hash, N_LINES)
    assert rc == _lib.E_EMPTY and msg == "no internal ids were assigned: no sample passes the sample threshold"
    wide = AnnoyIndex(32769)
    rc, msg = call(wide._h, store._p, ids, len(ids), line_hash, N_LINES)
    assert rc == _lib.E_INVALID and "32768" in msg
    wide_rows = twin(np.ones((2, 32769), np.float32))
    rc_build = lib().morna_build(wide_rows._h, 1, 0)
    assert rc == rc_build and msg == lib().morna_last_error().decode()                 # what morna_build returns
    # the handle still holds its rows, the store answers retain and nearest as before, and the next call works
    assert h.get_n_items() == len(ext) and h.get_items().tobytes() == rows.tobytes()
    for a, b in zip(store.retain(lists, 0.3, 5), kept):
        assert a.lines.tobytes() == b.lines.tobytes() and a.masks.tobytes() == b.masks.tobytes() and a.coverages == b.coverages
    for a, b in zip(store.nearest_by_sample(ext, ext[:6], 5), near):
        assert a.tobytes() == b.tobytes()
    h.add_items_from_store(store, ext[:7], line_hash)
    assert h.get_items().tobytes() == rows[:7].tobytes()
    stats = store.hash_rows_stats()
    assert stats["kernel_ms"] > 0 and stats["workgroups"] == 7 and stats["bytes_written"] == 4 * 7 * 256
    assert stats["bytes_read"] == 8 * sum(len(l) for l, _ in nonneg[:7]) + 12 * N_LINES
    # the timers of the others are their own
    assert store.nearest_stats()["kernel_ms"] > 0 and store.timers()["retain"][0] > 0


# ---- row norms -------------------------------------------------------------------------------------------------------------------
def test_row_norms_in_and_out_of_the_cache(world):
    from morna_amd import _lib
    from morna_amd._lib import lib, ptr
    nonneg = [(l, np.abs(c.astype(np.int64)).clip(0, 10**6).astype(np.int32)) for l, c in world["rows"][:60]]
    store, ext = make_store(nonneg, N_LINES, world["w"])
    ref = RefUnhashed(nonneg, world["w"])
    assert store.row_norms(ext).tobytes() == ref.pp.tobytes()                           # before any search: nothing cached
    cached = ext[10:30]
    store.nearest_by_sample(cached, cached[:3], 4)                                      # the cache holds rows 10 .. 29
    ask = [int(ext[12]), int(ext[8]), int(ext[45]), int(ext[12]), int(ext[0]), int(ext[29])]   # in it, out of it, one twice
    got = store.row_norms(ask)
    assert got.dtype == np.float64 and got.tobytes() == ref.pp[[(e - 500) // 2 for e in ask]].tobytes()
    assert got[4] == 0.0                                                                # the row without entries
    ids, d, cnt = store.nearest_by_sample(cached, cached[:3], 4)
    assert store.nearest_stats()["norms_ms"] == 0.0                                     # ... and still holds them
    assert store.row_norms([]).shape == (0,)
    with pytest.raises(IndexError, match="424243"):
        store.row_norms([int(ext[0]), 424243])
    bare, _ = make_store(nonneg[:3], N_LINES)
    with pytest.raises(RuntimeError, match="weights"):
        bare.row_norms([int(ext[0])])
    out = np.zeros(1, np.float64)
    assert lib().morna_jstore_row_norms(None, ptr(np.array([1], np.int64)), 1, ptr(out)) == _lib.E_INVALID
    assert lib().morna_jstore_row_norms(store._p, None, 1, ptr(out)) == _lib.E_INVALID
    with pytest.raises(ValueError) as e:                                                # a negative coverage, as the search
        world["store"].row_norms([int(world["ext"][8])])
    assert "negative coverage" in str(e.value) and str(int(world["ext"][8])) in str(e.value)
