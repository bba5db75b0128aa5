"""Tree-prefix search on the GPU (include/morna_hip.h, "tree-prefix search").  -m gpu

The oracle of `n_trees=t` on a T-tree handle is a second handle built with t trees on the same rows and seed: ids, the
fp32 distances as bytes and the counts are compared.  Rows are seeded numpy normals through AnnoyIndex.add_items, as the
restricted-search tests make theirs.  The cases are named by the code path they reach: the spread form (1 and 5 queries, with
a search_k the first leaf ends, where the leaf's slice of the permutation is the candidate list), the gather form (70), the
whole-batch contraction (200), the fused traversal, the unfiltered refine, roots that are leaves, rows without a register
form.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 64
SEED = 5
_INDEXES = {}


def rows(n, dim):
    return np.random.default_rng(n * 31 + dim).standard_normal((n, dim)).astype(np.float32)


def index(n, dim, trees):
    """One handle per (rows, tree count), shared by the tests of this module and of test_gpu_search_sweep."""
    from morna_amd.annoy import AnnoyIndex
    key = (n, dim, trees)
    if key not in _INDEXES:
        a = AnnoyIndex(dim)
        a.add_items(rows(n, dim))
        a.build(trees, seed=SEED)
        _INDEXES[key] = a
    return _INDEXES[key]


def queries(n, dim, nq, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nq, dim)).astype(np.float32), rng.choice(n, size=nq, replace=nq > n).astype(np.int32)


def same(got, want, label):
    assert got[2].tolist() == want[2].tolist(), label + " counts"
    assert got[0].tolist() == want[0].tolist(), label + " ids"
    assert got[1].tobytes() == want[1].tobytes(), label + " distance bytes"


def renumbered(rec, t, T):
    """node_rec of the first t trees of a T-tree forest, node ids renumbered in order; None when a kept node points at a
    dropped one."""
    keep = np.nonzero(rec[:, 1] < t)[0]
    new_id = np.full(len(rec) + 1, -1, np.int64)          # (index -1 -> -1: a leaf's children)
    new_id[keep] = np.arange(len(keep))
    out = rec[keep].copy()
    for col in (4, 5):
        child = out[:, col]
        if ((child >= 0) & (new_id[child] < 0)).any():
            return None
        out[:, col] = np.where(child >= 0, new_id[child], -1)
    return out, keep


def test_premise_a_forest_holds_its_prefixes():
    """Trees 0-2 of the 8-tree forest are the 3-tree forest: permutations and hyperplanes byte for byte, the node records
    after renumbering (node ids are breadth-first in (level, tree, position) order, so the kept ids keep their order)."""
    f8, f3 = index(3000, D, 8).get_forest(), index(3000, D, 3).get_forest()
    assert f8["perm"][:3].tobytes() == f3["perm"].tobytes()
    cut, keep = renumbered(f8["node_rec"], 3, 8)
    assert cut.tolist() == f3["node_rec"].tolist()
    # hyperplanes in node order on both sides
    new_id = {int(old): i for i, old in enumerate(keep)}
    hp8 = {new_id[int(node)]: f8["hyperplanes"][i].tobytes() for i, node in enumerate(f8["hp_node"]) if int(node) in new_id}
    hp3 = {int(node): f3["hyperplanes"][i].tobytes() for i, node in enumerate(f3["hp_node"])}
    assert hp8 == hp3
    assert (f8["node_rec"][:8, 1] == np.arange(8)).all()   # the roots are nodes 0 .. T-1


def check_prefix(n, dim, T, t, nqs, search_ks, ks, label):
    big, small = index(n, dim, T), index(n, dim, t)
    for nq in nqs:
        Q, items = queries(n, dim, nq, seed=nq * 13 + t)
        for search_k in search_ks:
            for k in ks:
                tag = "%s/T%d/t%d/nq%d/sk%d/k%d" % (label, T, t, nq, search_k, k)
                same(big.get_nns_by_vector_batch(Q, k, search_k, n_trees=t), small.get_nns_by_vector_batch(Q, k, search_k), tag + "/vector")
                same(big.get_nns_by_item_batch(items, k, search_k, n_trees=t), small.get_nns_by_item_batch(items, k, search_k), tag + "/item")


@pytest.mark.parametrize("nq", [1, 5, 70, 200], ids=["spread1", "spread5", "gather70", "dense200"])
@pytest.mark.parametrize("t", [3, 1])
def test_prefix_equals_the_smaller_forest(t, nq):
    """search_k -1 (k * t), 10 (the first leaf ends the search), 500, 4000 (the queue runs empty); k 1, 20, 100 (past
    KTH_MAX_K) and 3000 (more than the candidates found: short lists)."""
    check_prefix(3000, D, 8, t, (nq,), (-1, 10, 500, 4000), (1, 20, 100, 3000), "3000x64")


def test_prefix_one_query_forms():
    big, small = index(3000, D, 8), index(3000, D, 3)
    Q, items = queries(3000, D, 1, seed=3)
    assert big.get_nns_by_vector(Q[0], 20, 500, True, n_trees=3) == small.get_nns_by_vector(Q[0], 20, 500, True)
    assert big.get_nns_by_item(int(items[0]), 20, -1, n_trees=3) == small.get_nns_by_item(int(items[0]), 20, -1)
    assert big.get_nns_by_item(int(items[0]), 20, -1, True, n_trees=3) == small.get_nns_by_item(int(items[0]), 20, -1, True)


def test_prefix_roots_are_leaves():
    """n = 50 <= K: every root is a leaf."""
    check_prefix(50, D, 8, 3, (1, 5, 70), (-1, 30, 4000), (1, 20, 100), "roots_are_leaves")


def test_prefix_register_free_rows():
    """dim 1100 pads to 1280, five float4 per lane: the NV = 0 descent."""
    check_prefix(600, 1100, 4, 2, (5, 70), (-1, 3000), (1, 20), "nv0_dim1100")


_CHILD = """
import sys
import torch
sys.path[:0] = [{root!r}, {tests!r}]
import test_gpu_tree_prefix as t
t.check_prefix(3000, t.D, 8, 3, (5, 70, 200), (-1, 10, 500, 4000), (1, 20, 100), {label!r})
t.check_prefix(50, t.D, 8, 3, (70,), (30,), (20,), {label!r} + "/roots_are_leaves")
print("child ok")
"""


@pytest.mark.parametrize("name", ["MORNA_QUERY_SPLIT_TRAVERSE", "MORNA_QUERY_FILTER"])
def test_prefix_other_forms(name):
    """MORNA_QUERY_SPLIT_TRAVERSE=0 (the fused traversal) and MORNA_QUERY_FILTER=0 (read once per process): each in a process
    of its own."""
    env = dict(os.environ, **{name: "0"})
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), label=name + "=0")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_whole_forest_is_the_plain_call():
    """n_trees = the forest's count is bit-identical to the call without the argument, and a default call after a prefix
    call is unchanged."""
    a = index(3000, D, 8)
    for nq in (1, 5, 70, 200):
        Q, items = queries(3000, D, nq, seed=nq)
        before = [a.get_nns_by_vector_batch(Q, 20, sk) for sk in (-1, 10, 500)] + [a.get_nns_by_item_batch(items, 20, -1)]
        same(a.get_nns_by_vector_batch(Q, 20, -1, n_trees=8), before[0], "whole/vector/nq%d" % nq)
        same(a.get_nns_by_item_batch(items, 20, -1, n_trees=8), before[3], "whole/item/nq%d" % nq)
        a.get_nns_by_vector_batch(Q, 20, -1, n_trees=3)
        a.get_nns_by_item_batch(items, 100, 4000, n_trees=1)
        after = [a.get_nns_by_vector_batch(Q, 20, sk) for sk in (-1, 10, 500)] + [a.get_nns_by_item_batch(items, 20, -1)]
        for b, c in zip(before, after):
            same(c, b, "default_after_prefix/nq%d" % nq)


def test_two_batches_equal_one_batch_slices():
    """24000 queries at search_k 4000: cap = min(n, search_k + K) = 3000, the candidate arrays alone are 16 * cap = 48000
    bytes per query, so the 1 GiB workspace rule allows at most 22369 queries per batch whatever the forest's node count:
    two batches, the second ragged, where every offset by the batch's first query is.  The same queries in slices of 4096
    are one batch each.  By item, by vector, and restricted with an allow-list and a leave-out group per query."""
    from test_gpu_restrict import _groups, _query_groups
    a = index(3000, D, 8)
    nq, k, search_k, step = 24000, 20, 4000, 4096
    Q, items = queries(3000, D, nq, seed=24)
    rng = np.random.default_rng(24)
    r = a.restriction(rng.random(3000) < 0.5, _groups(rng, 3000))
    qg = _query_groups(nq)
    for name, call in (("item", lambda s: a.get_nns_by_item_batch(items[s], k, search_k)),
                       ("vector", lambda s: a.get_nns_by_vector_batch(Q[s], k, search_k)),
                       ("restricted", lambda s: a.get_nns_restricted(r, k, search_k, items=items[s], query_groups=qg[s]))):
        got = call(slice(0, nq))
        parts = [call(slice(at, at + step)) for at in range(0, nq, step)]
        same(got, [np.concatenate([p[i] for p in parts]) for i in range(3)], "two_batches/" + name)
        assert (got[2] > 0).all()


def test_prefix_staged_query_rows():
    """Neither Q nor items: the rows of build_query_rows, as get_nns_by_query_rows takes them."""
    from test_gpu_restrict import _stage_rows
    big, small = index(3000, D, 8), index(3000, D, 3)
    for nq in (5, 70):
        _, r32 = _stage_rows(big, nq, seed=nq)
        for search_k in (-1, 500):
            same(big.get_nns_by_query_rows(20, search_k, n_trees=3), small.get_nns_by_vector_batch(r32, 20, search_k), "staged/nq%d" % nq)
            same(big.get_nns_by_query_rows(20, search_k, n_trees=8), big.get_nns_by_query_rows(20, search_k), "staged/whole/nq%d" % nq)
    from morna_amd import _lib
    from morna_amd._lib import lib, ptr
    ids = np.zeros((3, 5), np.int32)
    assert lib().morna_get_nns_prefix(big._h, None, None, 3, 5, -1, 3, ptr(ids), None, None) == _lib.E_INVALID   # 70 rows are staged


def test_range_and_state_errors():
    from morna_amd import _lib
    from morna_amd._lib import lib, ptr
    from morna_amd.annoy import AnnoyIndex
    a = index(3000, D, 8)
    Q, items = queries(3000, D, 3, seed=1)
    for t in (0, -1, 9):
        with pytest.raises(IndexError) as e:
            a.get_nns_by_vector_batch(Q, 5, -1, n_trees=t)
        assert str(t) in str(e.value) and "8" in str(e.value)
        with pytest.raises(IndexError):
            a.get_nns_by_item_batch(items, 5, -1, n_trees=t)
    with pytest.raises(IndexError):
        a.get_nns_by_item_batch(np.array([3000], np.int32), 5, -1, n_trees=3)
    with pytest.raises(ValueError):
        a.get_nns_by_item_batch(items, 0, -1, n_trees=3)
    ids, d, cnt = np.zeros((3, 5), np.int32), np.zeros((3, 5), np.float32), np.zeros(3, np.int32)
    call = lib().morna_get_nns_prefix
    assert call(a._h, ptr(Q), ptr(items), 3, 5, -1, 3, ptr(ids), ptr(d), ptr(cnt)) == _lib.E_INVALID   # both sources
    if getattr(a, "_qrows_n", 0) == 0:
        assert call(a._h, None, None, 3, 5, -1, 3, ptr(ids), ptr(d), ptr(cnt)) == _lib.E_STATE         # neither: no staged rows
    assert call(a._h, ptr(Q), None, 3, 5, -1, 3, None, ptr(d), ptr(cnt)) == _lib.E_INVALID             # no room for the ids
    assert call(a._h, ptr(Q), None, 3, 5, -1, 3, ptr(ids), None, None) == _lib.OK                      # optional outputs
    unbuilt = AnnoyIndex(D)
    unbuilt.add_items(rows(100, D))
    with pytest.raises(RuntimeError):
        unbuilt.get_nns_by_item_batch(items % 100, 5, -1, n_trees=1)
