"""Near-duplicate pairs on the GPU: a 600-row matrix with 12 planted duplicate pairs, a triple, a chain
A - B - C whose ends are farther apart than r, and a pair the oracle gives NaN for.  The yardsticks are the exact by-item
lists with k = n_items cut on the host and the oracle's cosine_distance.  -m gpu"""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, R = 600, 64, 0.3
PAIRS = [(20 + 2 * i, 400 + 3 * i) for i in range(12)]
TRIPLE = (100, 250, 501)
CHAIN = (130, 131, 570)
NAN_PAIR = (77, 333)


@pytest.fixture(scope="module")
def capi():
    from oracle import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def planted(capi):
    rng = np.random.default_rng(1414)
    X = rng.standard_normal((N, D)).astype(np.float32)

    def near(a, sigma):
        return (X[a] + sigma * rng.standard_normal(D)).astype(np.float32)
    for a, b in PAIRS:
        X[b] = near(a, 0.1)
    X[PAIRS[0][1]] = X[PAIRS[0][0]]                              # one of them an exact copy
    X[TRIPLE[1]], X[TRIPLE[2]] = near(TRIPLE[0], 0.08), near(TRIPLE[0], 0.08)
    step = 0.22 * rng.standard_normal(D)
    X[CHAIN[1]] = (X[CHAIN[0]] + step).astype(np.float32)
    X[CHAIN[2]] = (X[CHAIN[0]] + 2 * step).astype(np.float32)
    X[NAN_PAIR[0]] = np.random.default_rng(2).standard_normal(D).astype(np.float32)     # (seed 2: found by a search on the CPU)
    X[NAN_PAIR[1]] = X[NAN_PAIR[0]] * np.float32(3.0)

    def d(i, j):
        return capi.cosine_distance(X[i], X[j].astype(np.float64))
    # the planting, asserted through the oracle
    for a, b in PAIRS:
        assert d(a, b) <= R
    assert d(*PAIRS[0]) == 0.0
    assert max(d(TRIPLE[0], TRIPLE[1]), d(TRIPLE[0], TRIPLE[2]), d(TRIPLE[1], TRIPLE[2])) <= R
    assert d(CHAIN[0], CHAIN[1]) <= R and d(CHAIN[1], CHAIN[2]) <= R and d(CHAIN[0], CHAIN[2]) > R
    assert np.isnan(d(*NAN_PAIR)) and np.isnan(d(NAN_PAIR[1], NAN_PAIR[0]))
    from morna_amd.annoy import AnnoyIndex
    a = AnnoyIndex(D)
    a.add_items(X)
    items = np.arange(N, dtype=np.int32)
    return dict(X=X, a=a, items=items, full=a.exact_search_by_item_batch(items, N), d=d)


def _expected_pairs(full, keep=lambda i, j: True):
    """The i < j entries of the full exact lists cut at R, and the NaN entries: {(i, j): distance bytes}."""
    ids, dist, cnt = full
    want = {}
    for i in range(N):
        sel = ((dist[i] <= R) | np.isnan(dist[i])) & (ids[i] > i)
        for j, dd in zip(ids[i][sel].tolist(), dist[i][sel].tolist()):
            if keep(i, j):
                want[(i, j)] = struct.pack("<d", dd)
    return want


def _searcher(a, ext_of):
    """A MornaSearch around an index made in memory: sample id ext_of[i] is item i."""
    from morna_amd.search import MornaSearch
    s = MornaSearch.__new__(MornaSearch)
    s.basename, s.annoy_index = None, a
    s.internal_id_map = {int(e): i for i, e in enumerate(ext_of)}
    return s


def test_pairs_are_the_upper_entries_of_the_full_lists(planted, capi):
    a, items, full = planted["a"], planted["items"], planted["full"]
    assert sorted(np.nonzero(full[2] < 0)[0].tolist()) == sorted(NAN_PAIR)       # no unplanted failing query
    lists, counts = a.exact_radius(R, items=items, after=items)
    got = {(i, int(j)): struct.pack("<d", dd) for i in range(N) for j, dd in zip(lists[i][0].tolist(), lists[i][1].tolist())}
    want = _expected_pairs(full)
    assert got == want
    planted_pairs = set(PAIRS) | {(TRIPLE[0], TRIPLE[1]), (TRIPLE[0], TRIPLE[2]), (TRIPLE[1], TRIPLE[2]), (CHAIN[0], CHAIN[1]),
                                  (CHAIN[1], CHAIN[2]), NAN_PAIR}
    assert set(got) == planted_pairs                             # nothing else in normal rows 1.4 apart
    for (i, j), b in got.items():                                # the distances are the oracle's
        assert b == struct.pack("<d", planted["d"](i, j)) or (i, j) == NAN_PAIR
    assert np.isnan(struct.unpack("<d", got[NAN_PAIR])[0])
    assert counts[NAN_PAIR[0]] == -1 and counts[NAN_PAIR[1]] == 0 and counts[CHAIN[0]] == 1
    assert lists[TRIPLE[0]][0].tolist() in ([TRIPLE[1], TRIPLE[2]], [TRIPLE[2], TRIPLE[1]])


def test_distance_is_symmetric_bit_for_bit(planted):
    """d(i, j) from query i and d(j, i) from query j, the by-item search without `after`: the same bytes."""
    a, items = planted["a"], planted["items"]
    lists, _ = a.exact_radius(1.25, items=items)
    seen = {}
    for i in range(N):
        for j, dd in zip(lists[i][0].tolist(), lists[i][1].tolist()):
            seen[(i, j)] = struct.pack("<d", dd)
    assert len(seen) > 4 * N
    for (i, j), b in seen.items():
        assert seen[(j, i)] == b, (i, j)


def test_sample_pairs_clusters_and_leave_out_groups(planted):
    from morna_amd.search import pair_clusters
    a = planted["a"]
    ext = 1000 + 7 * np.arange(N)[::-1]                          # external ids: descending in the internal id
    s = _searcher(a, ext)
    pairs = s.sample_pairs(R)
    e = lambda i: int(ext[i])
    key = lambda i, j: (min(e(i), e(j)), max(e(i), e(j)))
    assert pairs[0][:2] == key(*NAN_PAIR) and np.isnan(pairs[0][2])              # the NaN pair is present and first
    rest = pairs[1:]
    assert [(p[2], p[0], p[1]) for p in rest] == sorted((p[2], p[0], p[1]) for p in rest) and all(p[0] < p[1] for p in pairs)
    want = _expected_pairs(planted["full"])
    assert {p[:2]: struct.pack("<d", p[2]) for p in pairs} == {key(i, j): b for (i, j), b in want.items()}
    clusters = pair_clusters(pairs)
    assert [len(c) for c in clusters] == [3, 3] + [2] * 13
    assert sorted(e(i) for i in TRIPLE) in clusters[:2] and sorted(e(i) for i in CHAIN) in clusters[:2]
    assert sorted(e(i) for i in NAN_PAIR) in clusters and all(sorted(e(i) for i in p) in clusters for p in PAIRS)
    # never pair two samples of one group: the triple and two pairs are one donor each; the chain's ends share a group, so
    # its two links stay; a sample no group names pairs as before
    groups = [("t", [e(i) for i in TRIPLE]), ("p0", [e(i) for i in PAIRS[0]]), ("p1", [e(i) for i in PAIRS[1]]),
              ("ends", [e(CHAIN[0]), e(CHAIN[2])]), ("half", [e(PAIRS[2][0]), e(5)])]
    grouped = s.sample_pairs(R, restriction=s.restriction(groups=groups))
    gone = {key(TRIPLE[0], TRIPLE[1]), key(TRIPLE[0], TRIPLE[2]), key(TRIPLE[1], TRIPLE[2]), key(*PAIRS[0]), key(*PAIRS[1])}
    assert [p for p in pairs if p[:2] not in gone][1:] == grouped[1:] and grouped[0][:2] == pairs[0][:2]
    assert len(grouped) == len(pairs) - 5
    # an allow-list: only pairs of allowed samples
    allowed = [e(i) for i in range(N) if i % 2 == 0]
    inside = s.sample_pairs(R, restriction=s.restriction(within=allowed))
    assert [p[:2] for p in inside] == [p[:2] for p in pairs if p[0] in allowed and p[1] in allowed]
    assert 0 < len(inside) < len(pairs)
