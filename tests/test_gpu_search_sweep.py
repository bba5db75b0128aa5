"""The (tree count, search_k) sweep and its recall counts on the GPU (include/morna_hip.h, "search sweep"; DESIGN.md 8,
N11).  -m gpu

The oracle of cell (i, j) is morna_get_nns_prefix with n_trees_used = trees[i] and search_k = search_ks[j] (itself checked
against smaller forests in test_gpu_tree_prefix): ids, fp32 distance bytes and counts.  A cell's ncand is the count of the
same prefix call with k = n (every candidate found is returned); its ndots comes from the query timer's byte count of that
call, which is 4 * dim * (hyperplane dots + unique candidates + 1) summed over the queries.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_tree_prefix import D, ROOT, index, queries, rows

pytestmark = pytest.mark.gpu

N = 3000
TREES = (1, 3, 8)
SEARCH_KS = (1, 10, 66, 67, 500, 4000)     # 66 / 67: the sides of one full leaf (K = 66); 4000: more than n


def sources(a, nq, seed):
    Q, items = queries(N, D, nq, seed)
    return [("vector", dict(Q=Q), lambda k, s, t: a.get_nns_by_vector_batch(Q, k, s, n_trees=t)),
            ("item", dict(items=items), lambda k, s, t: a.get_nns_by_item_batch(items, k, s, n_trees=t))]


def rows_read(a, call):
    """hyperplane dots + unique candidates + 1, summed over the queries of `call` (the query timer's algorithmic bytes)."""
    a.timer_enable(True, only=["query"])
    a.timer_reset()
    call()
    a.synchronize()
    b = a.timers()["query"]["bytes"]
    a.timer_enable(False)
    assert b % (4 * a.f) == 0
    return b // (4 * a.f)


@pytest.mark.parametrize("nq", [1, 3, 65, 200])
def test_every_cell_equals_the_prefix_call(nq):
    a = index(N, D, 8)
    for name, kw, prefix in sources(a, nq, seed=nq + 100):
        for k in (1, 20, 100):
            out = a.search_sweep(k, TREES, SEARCH_KS, **kw)
            assert out["ids"].shape == (len(TREES), len(SEARCH_KS), nq, k)
            for i, t in enumerate(TREES):
                for j, s in enumerate(SEARCH_KS):
                    ids, d, cnt = prefix(k, s, t)
                    tag = "%s/nq%d/k%d/t%d/sk%d" % (name, nq, k, t, s)
                    assert out["count"][i, j].tolist() == cnt.tolist(), tag
                    assert out["ids"][i, j].tolist() == ids.tolist(), tag
                    assert out["dist"][i, j].tobytes() == d.tobytes(), tag
        st = a.sweep_stats()
        assert st["descents"] == nq * len(TREES) and st["cells"] == nq * len(TREES) * len(SEARCH_KS)
        # (k = 100 here) the whole-batch contraction runs by the rule of the plain search: nq >= 40 and nq * K >= 2 n
        dense = nq >= 40 and nq * (D + 2) >= 2 * N
        assert st["contraction"] == int(dense)
        if dense:     # only the candidates some cell's filter lets through get a canonical dot: at least every answer
            assert int(out["count"][:, -1].sum()) <= st["rows_canonical"] < int(out["ncand"][:, -1].sum())
        else:
            assert st["rows_canonical"] == int(out["ncand"][:, -1].sum())
        # ncand: every candidate the prefix call found comes back when k = n
        for i, t in enumerate(TREES):
            for j, s in enumerate(SEARCH_KS):
                assert out["ncand"][i, j].tolist() == prefix(N, s, t)[2].tolist(), "ncand/%s/nq%d/t%d/sk%d" % (name, nq, t, s)
        # ndots: summed over the batch for every cell ...
        for i, t in enumerate(TREES):
            for j, s in enumerate(SEARCH_KS):
                total = rows_read(a, lambda: prefix(20, s, t))
                assert total == int(out["ndots"][i, j].sum()) + int(out["ncand"][i, j].sum()) + nq, \
                    "ndots/%s/nq%d/t%d/sk%d" % (name, nq, t, s)
    # ... and query by query (by item, three of the queries)
    _, items = queries(N, D, nq, seed=nq + 100)
    out = a.search_sweep(20, TREES, SEARCH_KS, items=items, lists=False)
    assert set(out) == {"ncand", "ndots"}
    for q in sorted(set((0, nq // 2, nq - 1))):
        for i, t in enumerate(TREES):
            for j, s in enumerate(SEARCH_KS):
                one = rows_read(a, lambda: a.get_nns_by_item_batch(items[q:q + 1], 20, s, n_trees=t))
                assert one == int(out["ndots"][i, j, q]) + int(out["ncand"][i, j, q]) + 1, "ndots/q%d/t%d/sk%d" % (q, t, s)
    assert (out["ndots"][:, 0] >= np.array(TREES)[:, None]).all()          # the root dots are included


def test_filter_form_equals_canonical_form():
    """A batch of 200 takes the fp16 filter through one contraction; MORNA_SWEEP_FILTER=0 (read per call) takes canonical
    dots for every candidate.  The same bytes either way, by item and by vector, and for the recall counts."""
    from test_gpu_restrict import _with_env
    a = index(N, D, 8)
    for name, kw, _ in sources(a, 200, seed=77):
        for k in (1, 20, 100):
            got = a.recall_sweep(k, TREES, SEARCH_KS, lists=True, **kw)
            assert a.sweep_stats()["contraction"] == 1
            want = _with_env("MORNA_SWEEP_FILTER", "0", lambda: a.recall_sweep(k, TREES, SEARCH_KS, lists=True, **kw))
            assert a.sweep_stats()["contraction"] == 0
            for key in want:
                assert got[key].tobytes() == want[key].tobytes(), (name, k, key)


def test_two_batches_equal_one_batch_slices():
    """10000 queries over 3 tree counts to search_k 4000 (cap = 3000): a query costs at least n_t * 12 * cap = 108000 bytes
    of the 1 GiB workspace, so at most 9942 fit in a batch: two batches, the second ragged.  The same queries swept in slices
    of 2500 are one batch each; every returned array is their concatenation along the query axis."""
    a = index(N, D, 8)
    nq, k, sks, step = 10000, 20, (10, 4000), 2500
    for name, kw, _ in sources(a, nq, seed=31):
        (key, val), = kw.items()
        got = a.search_sweep(k, TREES, sks, **kw)
        assert a.sweep_stats()["descents"] == nq * len(TREES)
        parts = [a.search_sweep(k, TREES, sks, **{key: val[at:at + step]}) for at in range(0, nq, step)]
        assert set(got) == {"ids", "dist", "count", "ncand", "ndots"}
        for out in got:
            want = np.concatenate([p[out] for p in parts], axis=2)
            assert got[out].shape == want.shape and got[out].tobytes() == want.tobytes(), (name, out)


def test_null_outputs_repeats_and_the_default_search():
    from morna_amd._lib import check, lib, ptr
    a = index(N, D, 8)
    Q, items = queries(N, D, 5, seed=9)
    before = (a.get_nns_by_vector_batch(Q, 20, -1), a.get_nns_by_item_batch(items, 20, 500))
    one = a.search_sweep(20, TREES, SEARCH_KS, Q=Q)
    two = a.search_sweep(20, TREES, SEARCH_KS, Q=Q)
    for key in one:
        assert one[key].tobytes() == two[key].tobytes(), key
    trees, sks = np.array(TREES, np.int32), np.array(SEARCH_KS, np.int32)
    shape = (len(TREES), len(SEARCH_KS), 5)
    for keep in range(5):                      # one output at a time, the others NULL
        bufs = [np.full(shape + (20,), -7, np.int32), np.full(shape + (20,), -7, np.float32), np.full(shape, -7, np.int32),
                np.full(shape, -7, np.int32), np.full(shape, -7, np.int32)]
        args = [ptr(b) if i == keep else None for i, b in enumerate(bufs)]
        check(lib().morna_search_sweep(a._h, ptr(Q), None, 5, 20, ptr(trees), 3, ptr(sks), 6, *args))
        assert bufs[keep].tobytes() == one[("ids", "dist", "count", "ncand", "ndots")[keep]].tobytes()
    check(lib().morna_search_sweep(a._h, None, ptr(items), 5, 20, ptr(trees), 3, ptr(sks), 6, None, None, None, None, None))
    after = (a.get_nns_by_vector_batch(Q, 20, -1), a.get_nns_by_item_batch(items, 20, 500))
    for b, c in zip(before, after):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(b, c))


def test_roots_are_leaves_and_register_free_rows():
    """50 rows (every root is a leaf: no root dots) and dim 1100 (the NV = 0 descent)."""
    for n, dim, T, trees, sks in ((50, D, 8, (1, 3, 8), (1, 30, 51, 4000)), (600, 1100, 4, (2, 4), (10, 3000))):
        a = index(n, dim, T)
        for nq in (3, 70):
            Q, items = queries(n, dim, nq, seed=nq)
            for kw, prefix in ((dict(Q=Q), lambda k, s, t: a.get_nns_by_vector_batch(Q, k, s, n_trees=t)),
                               (dict(items=items), lambda k, s, t: a.get_nns_by_item_batch(items, k, s, n_trees=t))):
                out = a.search_sweep(20, trees, sks, **kw)
                for i, t in enumerate(trees):
                    for j, s in enumerate(sks):
                        ids, d, cnt = prefix(20, s, t)
                        assert (out["ids"][i, j].tolist(), out["dist"][i, j].tobytes(), out["count"][i, j].tolist()) == \
                            (ids.tolist(), d.tobytes(), cnt.tolist()), (n, dim, nq, t, s)
                        assert out["ncand"][i, j].tolist() == prefix(n, s, t)[2].tolist()
                if n == 50:
                    assert (out["ndots"] == 0).all()


@pytest.mark.parametrize("k", [20, 256, 3500], ids=["k20", "k256", "k_above_n"])
def test_recall_hits(k):
    """hits = |approx ids n exact ids| from the lists the same call returned; exact_count against exact_search_*_batch."""
    a = index(N, D, 8)
    for nq in (3, 200):
        Q, items = queries(N, D, nq, seed=k + nq)
        for kw, exact in ((dict(Q=Q), lambda kk: a.exact_search_batch(Q.astype(np.float64), kk)),
                          (dict(items=items), lambda kk: a.exact_search_by_item_batch(items, kk))):
            if k > 256:
                with pytest.raises(ValueError) as e:
                    a.recall_sweep(k, TREES, SEARCH_KS, **kw)
                assert "256" in str(e.value)
                continue
            out = a.recall_sweep(k, TREES, SEARCH_KS, lists=True, **kw)
            ex_ids, _, ex_cnt = exact(k)
            assert out["exact_count"].tolist() == ex_cnt.tolist() and out["exact_ids"].tolist() == ex_ids.tolist()
            plain = a.search_sweep(k, TREES, SEARCH_KS, **kw)
            for key in plain:
                assert out[key].tobytes() == plain[key].tobytes(), key
            for i in range(len(TREES)):
                for j in range(len(SEARCH_KS)):
                    for q in range(nq):
                        want = -1 if ex_cnt[q] < 0 else \
                            len(set(out["ids"][i, j, q, :out["count"][i, j, q]].tolist()) & set(ex_ids[q, :ex_cnt[q]].tolist()))
                        assert out["hits"][i, j, q] == want, (k, nq, i, j, q)
            short = a.recall_sweep(k, TREES, SEARCH_KS, **kw)
            assert set(short) == {"hits", "exact_count", "ncand", "ndots"} and short["hits"].tobytes() == out["hits"].tobytes()


def test_recall_k_above_n_items():
    """k above the number of rows: short exact and approximate lists."""
    a = index(50, D, 8)
    _, items = queries(50, D, 4, seed=2)
    out = a.recall_sweep(200, (1, 8), (10, 4000), items=items, lists=True)
    assert out["exact_count"].tolist() == [50] * 4 and (out["hits"][-1, -1] == 50).all()
    assert (out["hits"] == out["count"]).all()        # every approximate id is a row, and every row is in the exact list


def test_recall_of_a_query_the_exact_search_fails_for():
    """100 stored rows with a scaled copy each: the row and its copy are parallel, and where cosine_distance's radicand
    rounds below zero for such a pair the exact search reports count -1 for the query.  hits is -1 exactly there."""
    from morna_amd.annoy import AnnoyIndex
    X = rows(N, D).copy()
    X[1:200:2] = X[0:200:2] * np.linspace(0.3, 3.1, 100, dtype=np.float32)[:, None]
    a = AnnoyIndex(D)
    a.add_items(X)
    a.build(3, seed=5)
    items = np.arange(200, dtype=np.int32)
    out = a.recall_sweep(20, (1, 3), (10, 500), items=items)
    assert out["exact_count"].tolist() == a.exact_search_by_item_batch(items, 20)[2].tolist()
    failed = out["exact_count"] < 0
    assert failed.any() and not failed.all()
    assert (out["hits"][:, :, failed] == -1).all() and (out["hits"][:, :, ~failed] >= 0).all()


def test_refusals():
    from morna_amd.annoy import AnnoyIndex
    a = index(N, D, 8)
    Q, items = queries(N, D, 3, seed=4)
    for call in (a.search_sweep, a.recall_sweep):
        for trees, sks in (((3, 1), (10, 20)), ((1, 3), (20, 10)), ((1, 1), (10, 20)), ((1, 3), (10, 10)), ((), (10,)), ((1,), ()),
                           (tuple(range(1, 66)), (10,)), ((1,), tuple(range(1, 66))), ((0, 1), (10,)), ((1,), (-1, 10)),
                           ((1,), (0, 10))):
            with pytest.raises(ValueError):
                call(20, trees, sks, Q=Q)
        with pytest.raises(IndexError) as e:
            call(20, (1, 9), (10,), items=items)
        assert "9" in str(e.value) and "8" in str(e.value)
        with pytest.raises(IndexError):
            call(20, (1,), (10,), items=np.array([N], np.int32))
        with pytest.raises(ValueError):
            call(20, (1,), (10,), Q=Q, items=items)
        with pytest.raises(ValueError):
            call(0, (1,), (10,), Q=Q)
        with pytest.raises(IndexError):
            call(20, (1,), (10,), Q=Q[:, :-1])
        assert a.sweep_stats() == dict(descents=0, cells=0, rows_canonical=0, contraction=0)
    out = a.search_sweep(20, tuple(range(1, 9)), tuple(range(1, 65)), items=items[:1], lists=False)     # 64 entries are taken
    assert out["ncand"].shape == (8, 64, 1)
    unbuilt = AnnoyIndex(D)
    unbuilt.add_items(rows(100, D))
    with pytest.raises(RuntimeError):
        unbuilt.search_sweep(5, (1,), (10,), items=items % 100)
    with pytest.raises(RuntimeError):
        unbuilt.recall_sweep(5, (1,), (10,), items=items % 100)


def test_staged_query_rows():
    """Neither Q nor items: the rows of build_query_rows; the recall's exact search takes their fp64 rows."""
    from test_gpu_restrict import _stage_rows
    a = index(N, D, 8)
    with_rows = index(N, D, 3)
    r64, r32 = _stage_rows(with_rows, 7, seed=3)
    out = with_rows.recall_sweep(20, (1, 3), (10, 500), lists=True)
    by_vector = with_rows.search_sweep(20, (1, 3), (10, 500), Q=r32)
    for key in by_vector:
        assert out[key].tobytes() == by_vector[key].tobytes(), key
    assert out["exact_ids"].tolist() == with_rows.exact_search_batch(r64, 20)[0].tolist()
    fresh = index(N, D, 1)
    if getattr(fresh, "_qrows_n", 0) == 0:
        with pytest.raises(RuntimeError):
            fresh.search_sweep(20, (1,), (10,))
    assert a is not with_rows


def test_c_caller(tmp_path):
    """tests/c/sweep_caller.c compiled against the header alone and run."""
    from morna_amd import _lib
    exe = str(tmp_path / "sweep_caller")
    cc = os.environ.get("CC", "cc")
    libdir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "c", "sweep_caller.c"), "-o", exe, "-L", libdir, "-lmorna_hip", "-lm",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sweep_caller: ok" in r.stdout, r.stdout + r.stderr
