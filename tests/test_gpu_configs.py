"""BASELINE.json's configurations, each exactly as stated, under -m gpu.

  configs[1]  synthetic intropolis 10k samples x 3000 features, 200 trees, k = 20: feature matrix bit-exact, forest, queries,
              exact search.
  configs[2]  synthetic intropolis 50k samples x 3000 features, 200 trees, 1000 by-item queries, k = 20,
              search_k = 100 -- built as bench.py builds it: feature matrix bit-exact against the oracle; the first
              trees of the forest node for node against oracle mode 1 (a tree's Kiss32 streams depend on its own
              number only, so tree t of a 200-tree forest IS tree t of an 8-tree forest); invariants over all 200;
              every returned distance = the fp64 angular distance of the returned id; recall@20 against the exact
              search, and against the FAITHFUL annoy restatement (oracle mode 0) at 24 trees, same search_k.
  configs[3]  rows cut into shards of ONE data set (global idf, global first-seen ids): the 50k set cut 8 ways in one
              process and 2 ways over two ranks (gloo, one device) -- stacked shard matrices byte-identical to the single
              index, sharded exact search identical, approximate recall not worse; a 25k x 3000 shard through
              ShardedSearch on a 1-rank RCCL group; the 200k-sample set itself cut 8 ways, one shard against the oracle's
              matrix of the whole set (scripts/c4_200k_shard.py).  The 8-GPU run itself is the driver's.
  configs[4]  50k x 8192 exact all-pairs at its real size on one GPU (50 000 by-item queries x 50 000 rows, 32 sampled
              queries bit-exact against the oracle); one GPU's share of the 8-way cut (its 6250-row shard x all 50 000
              queries) through ShardedSearch on a 1-rank RCCL group; the 6250 x 6250 diagonal block.

Parity unpinned for the forest at N > K (no reference fixture has N > K, annoy is absent): what is pinned is the
feature matrix and the exact search; the forest is compared with this repository's restatements of annoy.
"""
import os
import socket

import numpy as np
import pytest

from test_gpu_scale import _check_forest, _true_ang

pytestmark = pytest.mark.gpu

D3, T3, Q3, K3, SEARCH_K = 3000, 200, 1000, 20, 100


@pytest.fixture(scope="module")
def capi():
    from oracle import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def c3():
    """configs[2], as bench.py's default run builds it."""
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.index import prepare_csr
    from morna_amd.synth import query_items, synthetic_intropolis
    data = synthetic_intropolis(50_000, J=70_000)
    prep = prepare_csr(data["keys"], data["row_ptr"], data["samples"], data["cov"], data["sample_count"], 100)
    a = AnnoyIndex(D3)
    a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
    a.stage_item_order(prep["ext_ids"])
    a.build_features(prep["n_items"])
    a.build(T3, seed=0)
    X = a.get_items()
    items = query_items(prep["n_items"], Q3)
    return dict(index=a, data=data, prep=prep, X=X, items=items, N=prep["n_items"])


def test_c3_feature_matrix_bit_exact_vs_oracle(c3, capi):
    """morna.py:344-388 + the fp64 -> fp32 hand-off of 405-424 over all 1e8 (sample, coverage) pairs."""
    data = c3["data"]
    buf, off = capi.pack_keys(data["keys"])
    ref = capi.index_features(buf, off, data["row_ptr"], data["samples"], data["cov"], data["sample_count"], 100, D3,
                              max_items=c3["N"])
    assert ref["n_items"] == c3["N"] == 50_000
    assert ref["ext_ids"].tolist() == c3["prep"]["ext_ids"].tolist()
    assert c3["X"].tobytes() == ref["X"].tobytes()


def _compare_tree(f, hp_of, o, gpu_root, ora_root):
    """One tree of the GPU forest against one tree of the oracle's, by structure (node ids differ when the two
    forests have different numbers of trees)."""
    rec, perm = f["node_rec"], f["perm"]
    stack, n = [(gpu_root, ora_root)], 0
    while stack:
        g, r = stack.pop()
        nd = o.node(r)
        kind, tree, start, count, c0, c1 = [int(x) for x in rec[g]]
        assert kind == nd["kind"] and count == nd["n_desc"], (g, r)
        if kind == 1:
            assert perm[tree, start:start + count].tolist() == nd["items"].tolist(), (g, r)
        else:
            assert f["hyperplanes"][hp_of[g]].tobytes() == nd["v"].tobytes(), (g, r)
            stack.append((c0, nd["child0"]))
            stack.append((c1, nd["child1"]))
        n += 1
    return n


def test_c3_forest_invariants_and_first_trees_vs_oracle(c3, capi):
    a, N = c3["index"], c3["N"]
    st = _check_forest(a, N, T3, D3 + 2)
    assert st["max_depth"] >= 5                       # ceil(log2(50000 / 3002)) = 5
    n_ref = 6
    o = capi.AnnoyOracle(D3, mode=1)
    o.set_items(c3["X"])
    o.build(n_ref)
    f = a.get_forest()
    hp_of = {int(n): i for i, n in enumerate(f["hp_node"])}
    roots = o.roots()
    nodes = sum(_compare_tree(f, hp_of, o, t, roots[t]) for t in range(n_ref))
    assert nodes == o.n_nodes()


def test_c3_queries_distances_and_recall_vs_exact(c3):
    """1000 by-item queries at morna's defaults (k = 20, search_k = 100; morna.py:762-774, 892-896)."""
    a, X, items = c3["index"], c3["X"], c3["items"]
    ids, d, cnt = a.get_nns_by_item_batch(items, K3, SEARCH_K)
    assert (cnt == K3).all()
    for qi in range(0, Q3, 5):                        # every fifth query: fp64 distances of 4000 pairs on the host
        it = int(items[qi])
        assert ids[qi, 0] == it and d[qi, 0] < 1e-3
        assert np.allclose(d[qi], _true_ang(X, X[it], ids[qi]), atol=2e-5)
        # ranked by (2 - 2 cos, id) as annoy does; the square root that is reported can make two different keys
        # print equal: ascending distances, distinct ids
        assert (np.diff(d[qi]) >= 0).all() and len(set(ids[qi].tolist())) == K3
    # an answer does not depend on which queries share its batch: 1000 at once go through the 256 x 256 form of the filter
    # contraction (whole rounds of the chip) + the 128 x 128 form for the rows behind, 400 at once through the 128 x 128
    # form alone, 40 / 8 / 1 at once through the spread form (a query's root margins and candidate dots dealt out over the
    # chip, canonical dots for every candidate) -- and 40 through the one-workgroup-per-query form it replaces for small
    # batches (per-candidate fp16 filter): four different routes, one result
    for part in (400, 40, 8, 1):
        pi, pd, pc = a.get_nns_by_item_batch(items[:part], K3, SEARCH_K)
        assert pi.tolist() == ids[:part].tolist() and pd.tobytes() == d[:part].tobytes() and pc.tolist() == cnt[:part].tolist(), part
    os.environ["MORNA_QUERY_SPREAD"] = "0"
    try:
        pi, pd, pc = a.get_nns_by_item_batch(items[:40], K3, SEARCH_K)
    finally:
        del os.environ["MORNA_QUERY_SPREAD"]
    assert pi.tolist() == ids[:40].tolist() and pd.tobytes() == d[:40].tobytes() and pc.tolist() == cnt[:40].tolist()
    # by vector, one query at a time (what `morna search` does): the stored row as the query vector
    for qi in (0, 17, 333):
        one = a.get_nns_by_vector(X[items[qi]].tolist(), K3, SEARCH_K, include_distances=True)
        assert one[0] == ids[qi].tolist() and np.array(one[1], np.float32).tobytes() == d[qi].tobytes()
    eids, ed, ecnt = a.exact_search_batch(X[items].astype(np.float64), K3)
    assert (ecnt == K3).all()
    recall = np.mean([len(set(ids[i].tolist()) & set(eids[i].tolist())) / float(K3) for i in range(Q3)])
    assert recall >= 0.95, recall                     # one leaf of ~2500 rows holds a query's cluster mates
    c3["recall_200_trees"] = float(recall)
    c3["exact_ids"] = eids


def test_c3_recall_vs_faithful_annoy_restatement(c3, capi):
    """Stand-in for "within tolerance of the reference CPU path" (annoy itself is not installable): the faithful
    restatement (oracle mode 0: one sequential Kiss32 stream, depth-first) and the GPU forest, both with 24 trees
    on the same 50k x 3000 matrix, same search_k = 100 and k = 20, on 120 queries.  Tolerance: recall@20 of the
    GPU forest >= the restatement's - 0.05 (both against the exact search)."""
    from morna_amd.annoy import AnnoyIndex
    X, items = c3["X"], c3["items"][:120]
    T = 24
    o = capi.AnnoyOracle(D3, mode=0)
    o.set_items(X)
    o.build(T)
    g = AnnoyIndex(D3)
    g.add_items(X)
    g.build(T)
    eids = c3["index"].exact_search_batch(X[items].astype(np.float64), K3)[0]
    ids, d, cnt = g.get_nns_by_item_batch(items, K3, SEARCH_K)
    hit_g = hit_o = 0
    for qi, it in enumerate(items):
        true = set(eids[qi].tolist())
        hit_g += len(true & set(ids[qi, :int(cnt[qi])].tolist()))
        hit_o += len(true & set(o.get_nns_by_item(int(it), K3, SEARCH_K)))
    rg, ro = hit_g / (K3 * len(items)), hit_o / (K3 * len(items))
    assert rg >= ro - 0.05, (rg, ro)


def test_c3_eight_trees_bit_exact_vs_oracle_mode1(c3, capi):
    """The same matrix with 8 trees: whole forest and search results (k = 20, search_k = 100 and -1) equal to
    oracle mode 1 -- the node-for-node check of test_gpu_parity.py at the headline row count."""
    from morna_amd.annoy import AnnoyIndex
    from test_gpu_parity import _compare_forest
    X, N = c3["X"], c3["N"]
    T = 8
    o = capi.AnnoyOracle(D3, mode=1)
    o.set_items(X)
    o.build(T)
    g = AnnoyIndex(D3)
    g.add_items(X)
    g.build(T)
    st = g.forest_stats()
    assert st["split_rows"] == o.split_rows() and st["split_attempts"] == o.split_nodes()
    _compare_forest(g, o, N, T)
    items = c3["items"][:48]
    for sk in (SEARCH_K, -1):
        ids, d, cnt = g.get_nns_by_item_batch(items, K3, sk)
        for qi, it in enumerate(items):
            rid, rd = o.get_nns_by_item(int(it), K3, sk, include_distances=True)
            m = int(cnt[qi])
            assert ids[qi, :m].tolist() == rid, (it, sk)
            assert d[qi, :m].tobytes() == np.array(rd, np.float32).tobytes(), (it, sk)


def test_c2_10k_samples_as_stated(capi):
    """configs[1] as stated: synthetic intropolis 10k samples x 3000 features, 200 trees, k = 20 on one GPU -- the feature leg
    (bit-exact against the oracle), the forest (invariants over all 200 trees; the first 4 trees node for node against oracle
    mode 1), 1000 by-item queries at morna's defaults (distances = fp64 angular distance of the returned ids, recall vs the
    exact search), and the exact search against the oracle."""
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.index import prepare_csr
    from morna_amd.synth import query_items, synthetic_intropolis
    data = synthetic_intropolis(10_000, J=70_000)
    prep = prepare_csr(data["keys"], data["row_ptr"], data["samples"], data["cov"], data["sample_count"], 100)
    N = prep["n_items"]
    assert N == 10_000
    a = AnnoyIndex(D3)
    a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
    a.stage_item_order(prep["ext_ids"])
    a.build_features(N)
    X = a.get_items()
    buf, off = capi.pack_keys(data["keys"])
    ref = capi.index_features(buf, off, data["row_ptr"], data["samples"], data["cov"], data["sample_count"], 100, D3, max_items=N)
    assert X.tobytes() == ref["X"].tobytes()
    a.build(T3, seed=0)
    st = _check_forest(a, N, T3, D3 + 2)
    assert st["max_depth"] >= 2                       # ceil(log2(10000 / 3002)) = 2
    o = capi.AnnoyOracle(D3, mode=1)
    o.set_items(X)
    o.build(4)
    f = a.get_forest()
    hp_of = {int(n): i for i, n in enumerate(f["hp_node"])}
    roots = o.roots()
    assert sum(_compare_tree(f, hp_of, o, t, roots[t]) for t in range(4)) == o.n_nodes()
    items = query_items(N, Q3)
    ids, d, cnt = a.get_nns_by_item_batch(items, K3, SEARCH_K)
    assert (cnt == K3).all() and (ids[:, 0] == items).all()
    for qi in range(0, Q3, 10):
        assert np.allclose(d[qi], _true_ang(X, X[int(items[qi])], ids[qi]), atol=2e-5)
    eids, ed, ecnt = a.exact_search_by_item_batch(items, K3)
    assert (ecnt == K3).all()
    recall = np.mean([len(set(ids[i].tolist()) & set(eids[i].tolist())) / float(K3) for i in range(Q3)])
    assert recall >= 0.95, recall
    for qi in range(0, Q3, 50):
        rid, rd = capi.exact_search(X, X[int(items[qi])].astype(np.float64), K3)
        assert eids[qi].tolist() == rid.tolist() and ed[qi].tobytes() == rd.tobytes()


def _build_shard_from_prep(prep, sample_count, rank, world, n_trees, device=0):
    """Row shard `rank` of `world` of the data set behind `prep`: lines cut by the library (global idf, global first-seen
    ids), feature matrix, forest.  Returns (index, id_offset, n_local)."""
    from morna_amd.index import ParsedLines, build_shard
    return build_shard(ParsedLines.from_arrays(prep, sample_count), D3, n_trees, rank, world, device=device)


def test_c4_eight_way_cut_of_one_data_set_stacks_to_the_single_index(c3):
    """configs[3]'s partition (rows cut 8 ways) applied to the 50k data set: eight 6250-row shards, each
    built from ITS lines with the GLOBAL idf and global first-seen ids -- stacked, they are the single index's matrix
    byte for byte (which test_c3_feature_matrix_bit_exact_vs_oracle pins to the oracle), and the row-sharded exact
    search is the single index's exact search."""
    from morna_amd.index import shard_bounds
    from morna_amd.shards import merge_topk_exact, merge_topk_native
    X, N, prep = c3["X"], c3["N"], c3["prep"]
    world = 8
    bounds = shard_bounds(N, world)
    assert bounds == [6250 * g for g in range(9)]
    items = c3["items"][:96]
    Q = X[items]
    ex, ap = [], []
    for g in range(world):
        a, off, n = _build_shard_from_prep(prep, c3["data"]["sample_count"], g, world, 20)
        assert (off, n) == (bounds[g], 6250)
        assert a.get_items().tobytes() == X[off:off + n].tobytes(), g
        assert a.get_norms2().tobytes() == c3["index"].get_norms2()[off:off + n].tobytes(), g
        ex.append(a.exact_search_batch(Q.astype(np.float64), K3))
        ap.append(a.get_nns_by_vector_batch(Q, K3, SEARCH_K))
        del a
    glob = lambda g, ids: np.where(ids >= 0, ids.astype(np.int64) + bounds[g], -1)     # noqa: E731
    eids, ed, ecnt = merge_topk_exact(np.stack([glob(g, r[0]) for g, r in enumerate(ex)]), np.stack([r[1] for r in ex]), K3)
    wids, wd, wcnt = c3["index"].exact_search_batch(Q.astype(np.float64), K3)
    assert eids.tolist() == wids.astype(np.int64).tolist() and ed.tobytes() == wd.tobytes() and ecnt.tolist() == wcnt.tolist()
    # approximate: eight 20-tree forests inspect at least what one 200-tree forest does (one leaf per shard at search_k = 100)
    aids = merge_topk_native(np.stack([glob(g, r[0]) for g, r in enumerate(ap)]), np.stack([r[1] for r in ap]), K3)[0]
    wa = c3["index"].get_nns_by_item_batch(items, K3, SEARCH_K)[0]
    rec_s = np.mean([len(set(aids[i].tolist()) & set(wids[i].tolist())) / float(K3) for i in range(len(items))])
    rec_w = np.mean([len(set(wa[i].tolist()) & set(wids[i].tolist())) / float(K3) for i in range(len(items))])
    assert rec_s >= rec_w - 0.02, (rec_s, rec_w)


def _two_way_worker(rank, world, port, tmp, ret):
    import torch
    import torch.distributed as dist
    from morna_amd.dist import ShardedSearch
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        z = np.load(os.path.join(tmp, "prep.npz"))
        prep = {k: z[k] for k in z.files}
        prep["n_items"] = int(prep.pop("n_items"))
        X = np.load(os.path.join(tmp, "X.npy"), mmap_mode="r")
        want = np.load(os.path.join(tmp, "want.npz"))
        a, off, n = _build_shard_from_prep(prep, int(prep.pop("sample_count")), rank, world, T3)
        assert (off, n) == (25_000 * rank, 25_000)
        assert a.get_items().tobytes() == np.ascontiguousarray(X[off:off + n]).tobytes()   # this rank's rows of the ONE matrix
        _check_forest(a, n, T3, D3 + 2)
        ss = ShardedSearch(a, rank, world, n)
        assert ss.offsets.tolist() == [0, 25_000, 50_000]
        items = want["items"]
        Q = np.ascontiguousarray(X[items])
        eids, ed, ecnt = ss.exact_search(Q.astype(np.float64), K3)
        assert eids.tolist() == want["eids"].astype(np.int64).tolist() and ed.tobytes() == want["ed"].tobytes()
        assert ecnt.tolist() == want["ecnt"].tolist()
        ids, d, cnt = ss.get_nns_by_vector(Q, K3, SEARCH_K)
        assert (cnt == K3).all()
        rec_s = np.mean([len(set(ids[i].tolist()) & set(eids[i].tolist())) / float(K3) for i in range(len(items))])
        assert rec_s >= float(want["recall_single"]) - 0.01, (rec_s, float(want["recall_single"]))
        # by item: every rank asks about rows of ITS shard (the form bench.py's strong-scaling run uses)
        mine = items[(items >= off) & (items < off + n)] - off
        n_each = [int(((items >= 25_000 * g) & (items < 25_000 * (g + 1))).sum()) for g in range(world)]
        ids2, d2, cnt2 = ss.get_nns_by_local_items(mine.astype(np.int32), K3, SEARCH_K, n_each=n_each)
        order = np.concatenate([np.nonzero((items >= 25_000 * g) & (items < 25_000 * (g + 1)))[0] for g in range(world)])
        assert ids2.tolist() == ids[order].tolist() and np.asarray(d2).tobytes() == np.asarray(d)[order].tobytes()
        ret[rank] = "ok"
    finally:
        dist.destroy_process_group()


def test_c3_two_way_cut_two_ranks_real_shards_gloo(c3, tmp_path):
    """ONE synthetic_intropolis(50_000) cut into two row shards, one per rank (two processes sharing the
    device, gloo between them -- RCCL refuses two ranks on one GPU): each rank's matrix is its rows of the single index's
    matrix byte for byte; the sharded exact search equals the single index's (ids + fp64 distances); the sharded
    approximate search is not worse in recall than the single 200-tree index."""
    import torch.multiprocessing as mp
    prep = c3["prep"]
    np.savez(tmp_path / "prep.npz", sample_count=c3["data"]["sample_count"],
             **{k: (np.asarray(v) if k != "freq" else np.zeros(0)) for k, v in prep.items() if k not in ("freq", "X_host")})
    np.save(tmp_path / "X.npy", c3["X"])
    items = np.sort(c3["items"][:128])
    a = c3["index"]
    eids, ed, ecnt = a.exact_search_batch(c3["X"][items].astype(np.float64), K3)
    sids = a.get_nns_by_item_batch(items, K3, SEARCH_K)[0]
    rec = np.mean([len(set(sids[i].tolist()) & set(eids[i].tolist())) / float(K3) for i in range(len(items))])
    np.savez(tmp_path / "want.npz", items=items, eids=eids, ed=ed, ecnt=ecnt, recall_single=rec)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_two_way_worker, args=(2, port, str(tmp_path), ret), nprocs=2, join=True)
    assert dict(ret) == {0: "ok", 1: "ok"}


def test_c4_shard_25k_through_sharded_search_one_rank_rccl(c3, capi):
    """configs[3]: what ONE GPU of a row-sharded index does -- a 25k x 3000 shard (the second half of the 50k data set cut
    two ways: global idf and ids, not a data set of its own) with its own 200-tree forest, queried through ShardedSearch
    on a 1-rank RCCL group (query rows stay in HBM, top-k all-gather over RCCL, merge kernel).  The 200k-sample set of
    configs[3] itself is cut 8 ways in test_c4_200k_sample_set_cut_eight_ways_one_shard_vs_oracle below."""
    import torch
    import torch.distributed as dist
    from morna_amd.dist import ShardedSearch
    from morna_amd.synth import query_items
    a, off, N = _build_shard_from_prep(c3["prep"], c3["data"]["sample_count"], 1, 2, T3)
    assert (off, N) == (25_000, 25_000)
    _check_forest(a, N, T3, D3 + 2)
    X = a.get_items()
    assert X.tobytes() == c3["X"][off:].tobytes()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        ss = ShardedSearch(a, 0, 1, N)
        items = query_items(N, Q3)
        ids, d, cnt = ss.get_nns_by_local_items(items, K3, SEARCH_K)
        want = a.get_nns_by_item_batch(items, K3, SEARCH_K)
        assert ids.tolist() == want[0].astype(np.int64).tolist()
        assert np.asarray(d, np.float32).tobytes() == want[1].tobytes() and cnt.tolist() == want[2].tolist()
        eids, ed, ecnt = ss.exact_search(X[items[:200]].astype(np.float64), K3)
        recall = np.mean([len(set(ids[i].tolist()) & set(eids[i].tolist())) / float(K3) for i in range(200)])
        assert recall >= 0.95, recall
        for qi in range(0, 200, 8):
            rid, rd = capi.exact_search(X, X[items[qi]].astype(np.float64), K3)
            assert eids[qi].tolist() == rid.tolist() and ed[qi].tobytes() == rd.tobytes()
    finally:
        dist.destroy_process_group()


def test_c4_200k_sample_set_cut_eight_ways_one_shard_vs_oracle():
    """configs[3] at its stated size: ONE 200 000-sample data set, global pre-pass, cut into 8 row shards; shard 3
    (25 000 rows) built on the GPU and compared byte for byte with rows 75 000 .. 100 000 of the oracle's matrix of the WHOLE
    data set; its exact search against the oracle; a step through the in-library sharded path on a 1-rank RCCL
    communicator (scripts/c4_200k_shard.py, whose output is kept as profiles/r03_c4_200k_shard.json).  In a process of its
    own: 4e8 (sample, coverage) pairs take ~15 GB of host memory while the shard is cut."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "c4_200k_shard.py"), "3"], cwd=root, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout[r.stdout.index("{"):])
    assert out["n_items"] == 200_000 and out["shard"] == {"rank": 3, "world": 8, "id_offset": 75_000, "rows": 25_000,
                                                          "nnz": out["shard"]["nnz"], "lines": out["shard"]["lines"]}
    assert out["shard_matrix_equals_rows_of_the_whole_oracle_matrix"] is True
    assert out["exact_search_of_the_shard_equals_oracle"] is True
    assert out["recall_at_20_vs_exact_within_the_shard"] >= 0.95
    assert out["forest"]["max_depth"] >= 4            # ceil(log2(25000 / 3002)) = 4 (K = 3002)


def test_c5_exact_all_pairs_shard_8192(capi):
    """configs[4]: exact brute-force all-pairs k-NN at D = 8192 on one GPU's shard of the 50k samples (6250 rows):
    morna.py:681-716 run with every indexed row as the query.  TF-IDF rows of the synthetic intropolis: cluster
    mates are strongly correlated and their distances to a query nearly tie, which is what the candidate window of
    the fp32 matrix-core scan has to survive (exact.hip eps)."""
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.index import prepare_csr
    from morna_amd.synth import synthetic_intropolis
    D, k = 8192, 20
    data = synthetic_intropolis(6250, J=70_000)
    prep = prepare_csr(data["keys"], data["row_ptr"], data["samples"], data["cov"], data["sample_count"], 100)
    N = prep["n_items"]
    assert N == 6250
    a = AnnoyIndex(D)
    a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
    a.build_features(N)
    X = a.get_items()
    Q = X.astype(np.float64)
    ids, d, cnt = a.exact_search_batch(Q, k)
    assert (cnt == k).all()                            # no row of this data set is parallel to another
    assert (ids[:, 0] == np.arange(N)).all() and (d[:, 0] == 0.0).all()   # sqrt(RN(pp * pp)) == pp: a row is at 0 from itself
    assert (np.diff(d, axis=1) >= 0).all()
    rng = np.random.default_rng(5)
    for qi in rng.choice(N, 64, replace=False):
        rid, rd = capi.exact_search(X, Q[qi], k)
        assert ids[qi].astype(np.int64).tolist() == rid.tolist(), qi
        assert d[qi].tobytes() == rd.tobytes(), qi
    # the same through the few-queries path (vector-ALU scan): identical answers, whichever scan selects
    ids2, d2, _ = a.exact_search_batch(Q[:16], k)
    assert ids2.tolist() == ids[:16].tolist() and d2.tobytes() == d[:16].tobytes()


@pytest.fixture(scope="module")
def c5(c3):
    """configs[4]'s matrix at its real size: the 50k-sample data set at 8192 features (1.64 GB of fp32 rows, one GPU)."""
    from morna_amd.annoy import AnnoyIndex
    prep = c3["prep"]
    a = AnnoyIndex(8192)
    a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
    a.stage_item_order(prep["ext_ids"])
    a.build_features(prep["n_items"])
    a.unstage_junctions()
    return dict(index=a, X=a.get_items(), N=prep["n_items"])


def test_c5_exact_all_pairs_full_size_by_item_one_gpu(c5, capi):
    """configs[4] as stated: 50k samples x 8192 features, exact brute-force k-NN of EVERY item against all items
    (morna.py:681-716 with query_sample = the item's own row) -- 50 000 x 50 000 x 8192, on one GPU, through
    morna_exact_search_by_item (only the item numbers cross PCIe; the library batches the queries).  32 sampled queries
    bit-exact against the oracle (ids + fp64 distances); every query: itself first at distance 0, k results, ascending."""
    a, X, N = c5["index"], c5["X"], c5["N"]
    k = 20
    items = np.arange(N, dtype=np.int32)
    ids, d, cnt = a.exact_search_by_item_batch(items, k)
    assert (cnt == k).all()
    assert (ids[:, 0] == items).all() and (d[:, 0] == 0.0).all()
    assert (np.diff(d, axis=1) >= 0).all()
    assert all(len(set(r)) == k for r in ids[::97].tolist())
    rng = np.random.default_rng(5)
    for qi in rng.choice(N, 32, replace=False):
        rid, rd = capi.exact_search(X, X[qi].astype(np.float64), k)
        assert ids[qi].astype(np.int64).tolist() == rid.tolist(), qi
        assert d[qi].tobytes() == rd.tobytes(), qi
    # a batch small enough for the vector-ALU scan, and the same queries handed over as fp64 vectors: one answer
    sub = items[:600]
    ids2, d2, _ = a.exact_search_by_item_batch(sub[:16], k)
    assert ids2.tolist() == ids[:16].tolist() and d2.tobytes() == d[:16].tobytes()
    ids3, d3, _ = a.exact_search_batch(X[sub].astype(np.float64), k)         # the same queries handed over as fp64 vectors
    assert ids3.tolist() == ids[:600].tolist() and d3.tobytes() == d[:600].tobytes()
    # the two-pass selection (shards of more than 8192 rows) against the k-round one it replaces
    os.environ["MORNA_EXACT_SELECT2"] = "0"
    try:
        ids4, d4, _ = a.exact_search_by_item_batch(sub, k)
    finally:
        del os.environ["MORNA_EXACT_SELECT2"]
    assert ids4.tolist() == ids[:600].tolist() and d4.tobytes() == d[:600].tobytes()
    c5["all_pairs"] = (ids, d)


def test_c5_one_gpus_share_of_the_all_pairs_through_sharded_search(c3, c5, capi):
    """configs[4] on 8 GPUs, what ONE of them does: its 6250-row shard (cut from the one data set) answers ALL 50 000
    queries, through ShardedSearch.exact_search on a 1-rank RCCL group (per-shard exact search packed in HBM ->
    ncclAllGather -> merge kernel, all inside the library)."""
    import torch
    import torch.distributed as dist
    from morna_amd.dist import ShardedSearch
    from morna_amd.index import ParsedLines
    X, N = c5["X"], c5["N"]
    k, g, world = 20, 3, 8
    part = ParsedLines.from_arrays(c3["prep"], c3["data"]["sample_count"]).shard(g, world)
    from morna_amd.annoy import AnnoyIndex
    a = AnnoyIndex(8192)
    part.stage(a)
    a.build_features(part.n_items)
    a.unstage_junctions()
    off, n = part.id_offset, part.n_items
    assert (off, n) == (18750, 6250)
    Xs = a.get_items()
    assert Xs.tobytes() == X[off:off + n].tobytes()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        ss = ShardedSearch(a, 0, 1, n)
        assert ss.in_library
        ids, d, cnt = ss.exact_search(X.astype(np.float64), k)               # 50 000 queries x 6250 rows
        assert ids.shape == (N, k) and (cnt == k).all() and (np.diff(d, axis=1) >= 0).all()
        own = np.arange(off, off + n)
        assert (ids[own, 0] == np.arange(n)).all() and (d[own, 0] == 0.0).all()     # a row of the shard finds itself
        rng = np.random.default_rng(6)
        for qi in rng.choice(N, 16, replace=False):
            rid, rd = capi.exact_search(Xs, X[qi].astype(np.float64), k)
            assert ids[qi].tolist() == rid.tolist() and d[qi].tobytes() == rd.tobytes(), qi
        # by item: the shard's own rows as queries, no query vectors from the host at all
        ids2, d2, cnt2 = ss.exact_search_by_local_items(np.arange(n, dtype=np.int32), k, n_each=[n])
        assert ids2.tolist() == ids[own].tolist() and d2.tobytes() == d[own].tobytes()
        ss.close()
    finally:
        dist.destroy_process_group()
    if "all_pairs" in c5:
        # the whole matrix's answer restricted to this shard's rows can only be a subsequence of the shard's own answer
        wi, wd = c5["all_pairs"]
        for qi in range(0, N, 997):
            mine = [(i - off) for i in wi[qi].tolist() if off <= i < off + n]
            assert mine == [i for i in ids[qi].tolist() if i in set(mine)]


def test_exact_search_row_parallel_to_the_query_raises(capi, tmp_path):
    """cosine_distance (morna.py:101-114) takes math.sqrt(2 - 2 pq / sqrt(pp qq)): for a row all but parallel to
    the query the radicand can round below zero and the reference raises ValueError -- for the whole query,
    since it evaluates every row (morna.py:697-700).  The library reports such a query with count -1 whatever
    rank the row would have had, and MornaSearch.exact_search_nn raises."""
    from morna_amd.annoy import AnnoyIndex
    rng = np.random.default_rng(99)
    D, N = 96, 400
    X = rng.standard_normal((N, D)).astype(np.float32)
    # scaled copies of one row: parallel in exact arithmetic, off by roundings in fp32/fp64; find a query for which
    # the oracle (same fp64 operations as Python) does produce a NaN for some of them
    for s in range(40):
        X[100 + s] = X[7] * np.float32(1.0 + 0.37 * (s + 1))
    q = None
    for cand in range(100, 140):
        qq = X[cand].astype(np.float64) * 1.7
        dist = [capi.cosine_distance(X[r], qq) for r in [7] + list(range(100, 140))]
        if np.isnan(dist).any():
            q, n_nan = qq, int(np.isnan(dist).sum())
            break
    assert q is not None, "no negative radicand among 40 x 41 near-parallel pairs"
    a = AnnoyIndex(D)
    a.add_items(X)
    a.build(2)
    for k in (3, 60):                                  # k below and above the number of parallel rows
        ids, d, cnt = a.exact_search_batch(np.stack([q, rng.standard_normal(D)]), k)
        assert cnt[0] == -1 and cnt[1] == k
    # through the reference-shaped front end
    from morna_amd.search import MornaSearch
    s = MornaSearch.__new__(MornaSearch)
    s.annoy_index, s.query_sample, s.basename = a, [float(v) for v in q], str(tmp_path / "x")
    with pytest.raises(ValueError):
        s.exact_search_nn(3)
    s.query_sample = [float(v) for v in rng.standard_normal(D)]
    assert len(s.exact_search_nn(3)[0]) == 3
