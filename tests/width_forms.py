"""What the tests that compare a forest and its searches with oracle mode 1 share (test_gpu_wide_rows.py,
test_gpu_width_forms.py and its child processes, test_gpu_caller_width_forms.py).  Not a test module.

  rows / compare_forest / compare_approx   the row generator and the node-for-node and answer-for-answer comparisons
  tm_form / tm_timer                        which two_means form the library takes at a row width and a level's node
                                            count: a restatement of the dispatch in forest_host.hpp (fb_attempt)
  descent_nv                                which form of the search's descent and root-margin kernels a row width takes: a
                                            restatement of row_nv in knn.hip
  check_width                               one shape end to end: forest, split counters, searches in three batch
                                            sizes, and the launch counts of the two two_means timers
"""
import numpy as np

SEARCHES = ((10, -1), (20, 100), (5, 1))    # (results, search_k) of the by-item searches; by vector: 10 results
TM_WAVE_NV = (1, 2, 3, 4, 6, 8, 12)         # float4 per lane with a one-wave register form
TM_STRIP_NV = (4, 8, 12, 16, 20, 24, 28, 32)
TM_WIDE_NG = (12, 16, 24, 32)               # groups of four k-steps the wide form is unrolled for


def rows(rng, N, f, nc=12, noise=0.3, chunk=2048):
    """Clustered float32 rows, built chunk by chunk in float32."""
    centers = rng.standard_normal((nc, f), dtype=np.float32)
    X = np.empty((N, f), np.float32)
    for r0 in range(0, N, chunk):
        r1 = min(N, r0 + chunk)
        X[r0:r1] = centers[rng.integers(0, nc, r1 - r0)]
        X[r0:r1] += np.float32(noise) * rng.standard_normal((r1 - r0, f), dtype=np.float32)
    return X


def compare_forest(a, o):
    """GPU forest vs oracle mode 1, node for node (as test_gpu_parity.py does)."""
    f = a.get_forest()
    rec = f["node_rec"]
    assert o.n_nodes() == rec.shape[0]
    hp_of = {int(n): i for i, n in enumerate(f["hp_node"])}
    n_split = 0
    for nid in range(rec.shape[0]):
        nd = o.node(nid)
        kind, tree, start, count, c0, c1 = [int(x) for x in rec[nid]]
        assert kind == nd["kind"], nid
        assert tree == nd["tree"], nid
        assert count == nd["n_desc"], nid
        if kind == 1:
            assert f["perm"][tree, start:start + count].tolist() == nd["items"].tolist(), nid
        else:
            n_split += 1
            assert (c0, c1) == (nd["child0"], nd["child1"]), nid
            assert f["hyperplanes"][hp_of[nid]].tobytes() == nd["v"].tobytes(), nid
    return n_split


def compare_approx(a, o, items, Q):
    for n, sk in ((10, -1), (20, 100)):
        ids, d, cnt = a.get_nns_by_item_batch(items, n, sk)
        for qi, it in enumerate(items):
            rid, rd = o.get_nns_by_item(int(it), n, sk, include_distances=True)
            m = int(cnt[qi])
            assert ids[qi, :m].tolist() == rid, (it, n, sk)
            assert d[qi, :m].tobytes() == np.array(rd, np.float32).tobytes(), (it, n, sk)
    ids, d, cnt = a.get_nns_by_vector_batch(Q, 10, -1)
    for qi in range(len(Q)):
        rid, rd = o.get_nns_by_vector(Q[qi], 10, -1, include_distances=True)
        assert ids[qi, :int(cnt[qi])].tolist() == rid
        assert d[qi, :int(cnt[qi])].tobytes() == np.array(rd, np.float32).tobytes()


# ---- the two_means dispatch, restated ---------------------------------------------------------------------------------

def tm_form(f, A, n_cus, strip_on=True):
    """(form, template argument) of the two_means launch for rows of f floats at a level (or a retry) of A nodes on a
    device of n_cus compute units; strip_on False: MORNA_TM_STRIP=0.  form is "wave" (one wave per node), "strip"
    (four waves per node), "wide" (rows past 8192 floats) or "lds" (centroids in LDS; argument None)."""
    dpad = (f + 255) // 256 * 256
    nv = dpad // 256
    if dpad > 8192:
        ng = nv // 4
        return "wide", [n for n in TM_WIDE_NG if ng <= n][0]
    if strip_on and A <= 2 * n_cus and nv in TM_STRIP_NV:
        return "strip", nv
    if nv in TM_WAVE_NV:
        return "wave", nv
    return "lds", None


DESCENT_NV = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)   # float4 per lane the search's one-wave kernels have a register form of


def descent_nv(f, max_nv):
    """The template argument NV of a search kernel that is dispatched over the row width, for rows of f floats: a restatement of
    row_nv in knn.hip.  max_nv is what the call site instantiates: 32 for the plain and the restricted descent, 12 for the sweep
    descent and the root margins by query groups (which do not exist where this returns 0).  0: the register-free form."""
    nv = (f + 255) // 256
    return nv if nv in DESCENT_NV and nv <= max_nv else 0


def tm_timer(form):
    """The timer a launch of that form is counted under: the wide form counts as strips."""
    return "tm_strip" if form in ("strip", "wide") else "tm_wave"


def level_census(o):
    """From the oracle: ({level: split nodes on it}, split nodes, split nodes that are the child of a split node).  A
    level's split nodes are the nodes of that level's first two_means launch."""
    per_level, below = {}, 0
    n = o.n_nodes()
    info = [o.node(nid) for nid in range(n)]
    for nd in info:
        if nd["kind"] == 0:
            per_level[nd["level"]] = per_level.get(nd["level"], 0) + 1
            below += sum(1 for c in (nd["child0"], nd["child1"]) if info[c]["kind"] == 0)
    return per_level, sum(per_level.values()), below


def expected_timers(f, per_level, n_cus, strip_on=True):
    """{timer: levels whose first launch counts under it}.  (A retry of a level has fewer nodes than its first launch: it
    can only move from the one-wave to the strip form, at levels of more than 2 * n_cus nodes.)"""
    out = {"tm_strip": 0, "tm_wave": 0}
    for A in per_level.values():
        out[tm_timer(tm_form(f, A, n_cus, strip_on)[0])] += 1
    return out


# ---- one shape, end to end --------------------------------------------------------------------------------------------

def query_items(N, n_all=96):
    """n_all distinct items: 0, the zero row 17, one of the duplicates, the last item and the other duplicate first."""
    head = [0, 17, 18, N - 1, 19]
    rest = [int(x) for x in (np.arange(1, 4 * n_all) * 7919) % N]
    out = head + [x for x in dict.fromkeys(rest) if x not in head]
    return np.array(out[:n_all], np.int32)


def _same(part, whole, first, count):
    """Rows [0, count) of the answer `part` are rows [first, first + count) of `whole`: (ids, distances, counts)."""
    for r in range(count):
        m = int(whole[2][first + r])
        assert int(part[2][r]) == m, (first, r)
        assert part[0][r].tobytes() == whole[0][first + r].tobytes(), (first, r)
        assert part[1][r, :m].tobytes() == whole[1][first + r, :m].tobytes(), (first, r)


def check_searches(a, o, N, f, rng, n_oracle=24):
    """By item and by vector, in batches of 96 (root margins by query groups where the width has them, then the descents),
    24 (the spread form) and 1: the first n_oracle answers against the oracle, and the same bytes whatever the batch."""
    items = query_items(N)
    Q = rng.standard_normal((len(items), f), dtype=np.float32)
    n_single = 5                                             # the five special items, each in a batch of its own
    for n, sk in SEARCHES:
        big = a.get_nns_by_item_batch(items, n, sk)
        for qi in range(n_oracle):
            rid, rd = o.get_nns_by_item(int(items[qi]), n, sk, include_distances=True)
            m = int(big[2][qi])
            assert big[0][qi, :m].tolist() == rid, (int(items[qi]), n, sk)
            assert big[1][qi, :m].tobytes() == np.array(rd, np.float32).tobytes(), (int(items[qi]), n, sk)
        _same(a.get_nns_by_item_batch(items[:24], n, sk), big, 0, 24)
        for qi in range(n_single):
            _same(a.get_nns_by_item_batch(items[qi:qi + 1], n, sk), big, qi, 1)
    big = a.get_nns_by_vector_batch(Q, 10, -1)
    for qi in range(n_oracle):
        rid, rd = o.get_nns_by_vector(Q[qi], 10, -1, include_distances=True)
        m = int(big[2][qi])
        assert big[0][qi, :m].tolist() == rid, qi
        assert big[1][qi, :m].tobytes() == np.array(rd, np.float32).tobytes(), qi
    _same(a.get_nns_by_vector_batch(Q[:24], 10, -1), big, 0, 24)
    _same(a.get_nns_by_vector_batch(Q[:1], 10, -1), big, 0, 1)


def check_width(capi, f, N, T, n_cus, strip_on=True, n_oracle=24, wide=False):
    """Rows of f floats (seed 31337 + f, a zero row, a duplicate pair), T trees: the forest and its split counters against
    the oracle, the searches, and the two_means forms the build must have launched.  Returns (form, argument) of the
    shallowest level."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(31337 + f)
    X = rows(rng, N, f)
    X[17] = 0.0                       # a zero row: norm == 0 paths, margin == 0 coin flips
    X[18] = X[19]                     # a duplicate pair
    o = capi.AnnoyOracle(f, mode=1)
    o.set_items(X)
    o.build(T)
    per_level, n_split, below = level_census(o)
    # the shape does what it is here for: it splits below the roots (a wide row: every root splits)
    if wide:
        assert n_split >= T, (n_split, T)
    else:
        assert n_split >= 4 and below >= 1, (n_split, below)
    a = AnnoyIndex(f)
    a.timer_enable(only=["tm_strip", "tm_wave"])
    a.add_items(X)
    a.build(T)
    st = a.forest_stats()
    assert st["split_rows"] == o.split_rows() and st["split_attempts"] == o.split_nodes()
    assert compare_forest(a, o) == n_split
    launches = {k: v["launches"] for k, v in a.timers().items() if k in ("tm_strip", "tm_wave")}
    want = expected_timers(f, per_level, n_cus, strip_on)
    for name in ("tm_strip", "tm_wave"):
        assert (launches[name] >= want[name]) if want[name] else (launches[name] == 0), (f, launches, want)
    check_searches(a, o, N, f, rng, n_oracle)
    return tm_form(f, per_level[0], n_cus, strip_on)
