"""The junction store past one round of the tile scan: `retain`, `pool`, `recovery`, `recovery_sweep`, `explain`,
`nearest_by_sample` and `thin` on stores of 64, 65 and 130 tiles of 4096 lines (jstore_big.make_case), whole arrays byte for
byte against the numpy restatements the tile-edge tests use (test_junctions_cpu.ref_retain, test_pool_cpu.ref_pool,
test_recovery_cpu.ref_hist, explain_ref.py, test_unhashed_cpu.RefUnhashed, test_thin_cpu.ref_thin).

jstore_tile_scan_kernel takes the tiles of a list 64 at a time and carries its running totals from round to round; the
stores of the other modules have at most four tiles, so only here does a second round run: at 262145 lines with one lane, at
528391 with a full one and a third of two lanes, the last tile of 7 lines.  The stores are very sparse (14400 entries), with
runs of tiles nobody holds inside the first and the second round, so a carry that is dropped, doubled or not zero-extended
through an empty run moves bytes in every output.  Integers, and fp64 values fixed by contract; no tolerance.  -m gpu"""
import numpy as np
import pytest

import jstore_big as big
from explain_ref import assert_pair, explain_pair
from test_gpu_recovery import GRID8, GRID15
from test_gpu_recovery_sweep import PREFIXES
from test_gpu_unhashed import assert_same
from test_pool_cpu import ref_pool
from test_recovery_cpu import ref_hist
from test_thin_cpu import CHUNK, ref_thin
from test_unhashed_cpu import RefUnhashed

pytestmark = pytest.mark.gpu

FILTERS = [(0.0, 10**6), (0.5, 3), (1.0, 1), (1.0, 2**40)]     # the tile-edge tests' three, and "held by all" alone
LARGEST = big.SIZES[-1]
_cases = {}


def case_of(n_lines):
    """Each store is made once; the largest carries the deep rows of the thinning test."""
    if n_lines not in _cases:
        _cases[n_lines] = big.make_case(n_lines, deep=n_lines == LARGEST)
        _cases[n_lines]["rounds"] = big.check_planted(_cases[n_lines])
    return _cases[n_lines]


@pytest.fixture(scope="module", params=big.SIZES)
def case(request):
    return case_of(request.param)


@pytest.fixture(scope="module")
def largest():
    return case_of(LARGEST)


def entries(case, samples):
    return sum(len(case["rows"][s][0]) for s in samples)


def corners(n_lines):
    """Truth lines in the first, the 64th, the 65th and the last tile."""
    return sorted(set(j for j in (5, 63 * big.TILE + 9, 262143, 262144, 64 * big.TILE + 11, n_lines - 1) if j < n_lines))


# ---- the filter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f, c", FILTERS)
def test_retain_equals_restatement(case, f, c):
    store, lists, n = case["store"], case["lists"], case["n_lines"]
    kept = store.retain(lists, f, c)
    assert len(kept) == len(lists)
    for q, lst in enumerate(lists):
        lines, masks, cov_ptr, cov = big.retained_arrays(case, lst, f, c)
        got = kept[q]
        assert (got.lines.dtype, got.masks.dtype, got._cov_ptr.dtype, got._cov.dtype) == (np.int32, np.uint64, np.int64, np.int32)
        assert got.lines.tobytes() == lines.tobytes(), (n, f, c, q)
        assert got.masks.tobytes() == masks.tobytes(), (n, f, c, q)
        assert got._cov_ptr.tobytes() == cov_ptr.tobytes(), (n, f, c, q)
        assert got._cov.tobytes() == cov.tobytes(), (n, f, c, q)
    assert len(kept[2]) == 0 and len(kept[1]) > 0 and len(kept[3]) > 0        # the empty list, and the non-empty one behind it
    if (f, c) == (0.0, 10**6):                                 # everything: both rounds' totals as check_planted read them
        assert len(kept[0]) == sum(case["rounds"]) and len(kept[1]) == big.PER_SAMPLE + 1
        assert set(big.planted_lines(n)) <= set(kept[3].lines.tolist())
    if (f, c) == (1.0, 2**40):                                 # held by all eleven
        assert set(kept[3].lines.tolist()) >= set(big.planted_lines(n)) and (kept[3].masks == np.uint64(2**11 - 1)).all()
    assert store.timers()["retain"][0] > 0 and store.timers()["retain"][1] == 8 * entries(case, [s for lst in lists for s in lst])


def test_retain_does_not_depend_on_the_batch(case):
    """64 copies of the 64-result list and one other: q_off of every list is the sum of many totals of many tiles."""
    store, lists = case["store"], case["lists"]
    want = [big.retained_arrays(case, lists[q], 0.5, 3) for q in (0, 4)]
    many = store.retain([lists[0]] * 64 + [lists[4]], 0.5, 3)
    for q, got in enumerate(many):
        for a, b in zip((got.lines, got.masks, got._cov_ptr, got._cov), want[q // 64]):
            assert a.tobytes() == b.tobytes(), (case["n_lines"], q)


# ---- the pool ------------------------------------------------------------------------------------------------------------------
def test_pool_equals_restatement(case):
    store, rows, groups, n = case["store"], case["rows"], case["groups"], case["n_lines"]
    want = [ref_pool(rows, n, g) for g in groups]
    got = store.pool(groups)
    assert len(got) == len(groups)
    for g in range(len(groups)):
        assert (got[g].lines.dtype, got[g].sums.dtype, got[g].holders.dtype) == (np.int32, np.int64, np.int32)
        assert got[g].lines.tobytes() == want[g][0].tobytes(), (n, g)
        assert got[g].sums.tobytes() == want[g][1].tobytes(), (n, g)
        assert got[g].holders.tobytes() == want[g][2].tobytes(), (n, g)
    assert len(got[2]) == 0 and len(got[0]) == big.PER_SAMPLE + 1
    at = int(np.searchsorted(want[4][0], big.BIG_LINE))         # three coverages of 2^31 - 1 on one line: read from the restatement
    assert want[4][0][at] == big.BIG_LINE and want[4][1][at] >= 3 * big.BIG > 2**32 and want[4][2][at] >= 3
    assert set(big.planted_lines(n)) <= set(want[4][0].tolist())
    stats = store.pool_stats()
    assert stats["bytes_read"] == 2 * 8 * entries(case, [s for g in groups for s in g])
    assert stats["bytes_written"] == 16 * sum(len(w[0]) for w in want)
    assert stats["workgroups"] == len(groups) * big.n_tiles(n) and stats["kernel_ms"] > 0


# ---- recovery ------------------------------------------------------------------------------------------------------------------
def truths_of(case):
    n, rows = case["n_lines"], case["rows"]
    return [corners(n), rows[1005][0], corners(n), [], np.arange(n)]


def test_recovery_equals_restatement(case):
    store, rows, lists, n = case["store"], case["rows"], case["lists"], case["n_lines"]
    truths = truths_of(case)
    got = store.recovery(lists, truths, GRID8)
    assert got.dtype == np.int64 and got.shape == (len(lists), 2, 65, 9)
    assert got.tobytes() == np.stack([ref_hist(rows, n, lst, t, GRID8) for lst, t in zip(lists, truths)]).tobytes()
    assert got[2, 1, 0, 0] == len(corners(n)) and got[2].sum() == len(corners(n)) and got[4, 1].sum() == n
    stats = store.recovery_stats()
    assert stats["bytes"] == 8 * entries(case, [s for lst in lists for s in lst]) + 4 * sum(len(t) for t in truths)
    assert stats["workgroups"] == len(lists) * big.n_tiles(n) and stats["kernel_ms"] > 0
    truth_ids = [1000, 1005, big.EMPTY, 1007, 1005]
    for min_cov in (1, 3):
        got = store.recovery_by_sample(lists, truth_ids, GRID15, truth_min_coverage=min_cov)
        want = [ref_hist(rows, n, lst, rows[s][0][rows[s][1] >= min_cov], GRID15) for lst, s in zip(lists, truth_ids)]
        assert got.tobytes() == np.stack(want).tobytes(), (n, min_cov)
    stats = store.recovery_stats()
    assert stats["bytes"] == 8 * (entries(case, [s for lst in lists for s in lst]) + entries(case, truth_ids))
    assert stats["workgroups"] == len(lists) * big.n_tiles(n)


def test_recovery_sweep_equals_restatement(case):
    store, rows, lists, n = case["store"], case["rows"], case["lists"], case["n_lines"]
    truths = truths_of(case)
    want = np.stack([np.stack([ref_hist(rows, n, lst[:p], t, GRID15) for p in PREFIXES]) for lst, t in zip(lists, truths)])
    got = store.recovery_sweep(lists, truths, GRID15, PREFIXES)
    assert got.dtype == np.int64 and got.shape == (len(lists), len(PREFIXES), 2, 65, 16)
    for i, p in enumerate(PREFIXES):
        assert got[:, i].tobytes() == want[:, i].tobytes(), (n, p)
    assert not np.array_equal(got[0, 0], got[0, 7]) and np.array_equal(got[1, 0], got[1, 7])
    stats = store.recovery_stats()
    assert stats["workgroups"] == len(lists) * big.n_tiles(n) and stats["kernel_ms"] > 0
    truth_ids = [1000, 1005, big.EMPTY, 1007, 1005]
    got = store.recovery_sweep_by_sample(lists, truth_ids, GRID8, [5, 20, 64])
    want = [[ref_hist(rows, n, lst[:p], rows[s][0][rows[s][1] >= 1], GRID8) for p in (5, 20, 64)] for lst, s in zip(lists, truth_ids)]
    assert got.tobytes() == np.array(want).tobytes()


# ---- at 528391 lines alone: explain, the unhashed search at 8 queries per pass, and thinning past 1024 chunks ---------------------
def weights(n_lines):
    """A fifth of the lines at weight 0; the planted lines and BIG_LINE keep a weight, so the every-seventh rows meet."""
    rng = np.random.Generator(np.random.PCG64(5))
    w = np.where(rng.random(n_lines) < 0.2, 0.0, rng.uniform(0.05, 6.0, n_lines))
    w[big.planted_lines(n_lines)] = [1.5, 0.25, 3.0, 2.0, 0.75, 5.0]
    return w


def test_explain_equals_restatement(largest):
    store, rows, n = largest["store"], largest["rows"], largest["n_lines"]
    w = weights(n)
    store.set_weights(w)
    query, results = 1007, [1014, 1021, 1003, big.EMPTY, 1007, 1014, 1002]        # every-seventh rows, others, itself, one twice
    got = store.explain_by_sample([query], [results], 10)
    assert len(got) == 1 and len(got[0]) == len(results)
    want = [explain_pair(*rows[query], *rows[s], w, 10) for s in results]
    for rank, pair in enumerate(want):
        assert_pair(got[0][rank], pair, "rank %d" % rank)
    assert want[0]["shared"] >= len(big.planted_lines(n)) and want[3]["shared"] == 0 and want[4]["distance"] < 1e-7
    assert {0, 262143, 262144, n - 1} <= set(want[0]["lines"])
    stats = store.explain_stats()
    assert stats["queries_per_pass"] == 8 and stats["passes"] == 1 and stats["pairs"] == len(results)


def test_nearest_by_sample_takes_8_queries_per_pass(largest):
    """528391 lines are more than 32768: choose_qt (csrc/jnearest_dev.hpp) takes 8 queries per pass, which the other modules
    reach through the environment override alone."""
    store, rows, n = largest["store"], largest["rows"], largest["n_lines"]
    w = weights(n)
    assert 0.15 < (w == 0.0).mean() < 0.25
    store.set_weights(w)
    population = [s for s in big.sparse_ids() if s != big.FIRST_ID]               # (the row with the negative coverage is refused)
    ref = RefUnhashed([rows[s] for s in population], w)
    queries = [1007, 1003, big.EMPTY, 1050, 1014, 1002, 1071, 1001, 1035]         # nine: a second pass of one
    ids, d, cnt = store.nearest_by_sample(population, queries, 10)
    for q, s in enumerate(queries):
        assert_same((ids[q], d[q], cnt[q]), ref, *rows[s], k=10)
    stats = store.nearest_stats()
    assert stats["queries_per_pass"] == 8 and stats["passes"] == 2 and stats["kernel_ms"] > 0
    assert stats["bytes"] == 8 * entries(largest, population) * 2


def test_thin_past_1024_chunks(largest):
    """42 rows of 50000 entries are 1050 chunks of 2048: jstore_ptr_kernel, which scans the chunk counts with 1024 threads,
    runs with two counts per thread (and with none for the threads past the 525th)."""
    store, rows = largest["store"], largest["rows"]
    ids = big.deep_ids()
    chunks = sum(-(-len(rows[s][0]) // CHUNK) for s in ids)
    assert chunks == 1050 > 1024 and all(rows[s][1].min() >= 1 and rows[s][1].max() <= 3 for s in ids)
    for keep, seed in ((2**31, 8675309), (429496730, 1)):
        got = store.thin(ids, keep, seed)
        survivors = 0
        for q, s in enumerate(ids):
            lines, cov = ref_thin(rows, s, keep, seed)
            assert (got[q].lines.dtype, got[q].cov.dtype) == (np.int32, np.int32)
            assert got[q].lines.tobytes() == lines.tobytes() and got[q].cov.tobytes() == cov.tobytes(), (s, keep, seed)
            survivors += len(lines)
        assert 0 < survivors < entries(largest, ids)
        stats = store.thin_stats()
        assert stats["workgroups"] == chunks and stats["draws"] == sum(int(rows[s][1].sum()) for s in ids)
        assert stats["bytes_written"] == 4 * entries(largest, ids) + 8 * survivors
