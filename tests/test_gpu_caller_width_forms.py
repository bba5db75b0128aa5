"""The callers of the approximate search at every row-width form of their kernels, against oracle mode 1.  -m gpu

knn.hip compiles query_descend_restricted_kernel<BM, NV> for NV = 1, 2, 3, 4, 6, 8, 12, 16, 24, 32 and the register-free
form 0, and query_descend_sweep_kernel<BM, NV> and query_roots_batch_kernel<NV> up to 12 (with_row_nv; wider rows take
NV = 0 there, or lose the root margins by query groups: roots_by_groups_ok).  test_gpu_width_forms.py pins the plain
descent at every width; here the restricted search (allow-lists, leave-out groups), the (tree count, search_k) sweep and
the tree-prefix call run once per form.  A width has f + 300 rows and three trees, and a leaf holds f + 2 items, so
every root splits and every query crosses the root hyperplanes (test_callers_at_width_vs_oracle); the children of
those roots are leaves, so a second, smaller case per width has 2 f + 300 rows in one tree and a split node below the
root, where the descents take hyperplane dots of their own (test_descents_below_the_roots_at_width).  The forest is
compared with the oracle's node for node first, so every answer below stands on the oracle's forest;
width_forms.descent_nv restates the dispatch (by hand-written widths in test_width_forms_cpu.py) and every case asserts
that its width takes the form it is here for.
"""
import numpy as np
import pytest

import width_forms as wf
from test_gpu_restrict import _approx_expected, _cases, _eligible, _query_groups, _same

pytestmark = pytest.mark.gpu

T = 3
# f, float4 per lane, the form of the restricted descent (built up to 32), of the sweep descent and root margins (up to 12)
_WIDTHS = [(500, 2, 2, 2), (641, 3, 3, 3), (1000, 4, 4, 4),
           (1100, 5, 0, 0),          # no register form of five: the restricted one-wave descent on wave_dot, the fused traversal
           (1500, 6, 6, 6), (2000, 8, 8, 8), (3000, 12, 12, 12),
           (4096, 16, 16, 0),        # the widest forms are the descent's alone: no root margins by query groups
           (5900, 24, 24, 0),        # ragged: the last float4 of the last lanes is padding
           (8192, 32, 32, 0)]


@pytest.fixture(scope="module")
def capi():
    from oracle import capi as c
    c.lib()
    return c


class _Oracle(object):
    """The oracle's whole candidate list of a stored row (n = every row), asked for once per (item, search_k)."""

    def __init__(self, o, N):
        self.o, self.N, self.made = o, N, {}

    def full(self, item, search_k):
        key = (int(item), int(search_k))
        if key not in self.made:
            ids, d = self.o.get_nns_by_item(key[0], self.N, key[1], include_distances=True)
            self.made[key] = (np.array(ids, np.int32), np.array(d, np.float32))
        return self.made[key]


def _equals_oracle(got, q, ids, d, label):
    """Answer q of `got` (ids, distances, counts) is the list (ids, d): the ids, and the fp32 distances as bytes."""
    m = int(got[2][q])
    assert m == len(ids), (label, m, len(ids))
    assert got[0][q, :m].tolist() == ids.tolist(), label
    assert got[1][q, :m].tobytes() == d.tobytes(), label


def _restricted(a, orc, N, f, items_all, Q_all, nqs=(5, 70), search_ks=None, ks=(1, 20),
                names=("half", "none", "all", "half+groups", "groups"), n_oracle=4):
    """5 queries: the spread form, whose descent is query_descend_restricted_kernel<BM, NV> at every width.  70: root margins
    by query groups and the same descent where the width has them, the fused restricted traversal elsewhere."""
    for nq in nqs:
        items, Q = items_all[:nq], Q_all[:nq]
        cases = [c for c in _cases(np.random.default_rng(f + nq), N) if c[0] in names]
        assert [c[0] for c in cases] == [n for n in ("half", "none", "all", "half+groups", "groups") if n in names]
        qg_all, no_group = _query_groups(nq), np.full(nq, -1, np.int32)
        for search_k in search_ks or (10, 2 * N):
            full = dict(item=a.get_nns_by_item_batch(items, N, search_k), vector=a.get_nns_by_vector_batch(Q, N, search_k))
            for name, allow, groups in cases:
                r = a.restriction(allow, groups)
                qg = qg_all if groups is not None else None
                want_g = qg_all if groups is not None else no_group
                for k in ks:
                    for src, kw in (("item", dict(items=items)), ("vector", dict(Q=Q))):
                        label = "restricted/f%d/nq%d/sk%d/%s/k%d/%s" % (f, nq, search_k, name, k, src)
                        got = a.get_nns_restricted(r, k, search_k, query_groups=qg, **kw)
                        _same(got, _approx_expected(full[src], N, allow, groups, want_g, k), label)
                        if src != "item":
                            continue
                        for q in range(n_oracle):                            # from the oracle alone
                            oi, od = orc.full(items[q], search_k)
                            keep = np.nonzero(_eligible(N, allow, groups, int(want_g[q]))[oi])[0][:k]
                            _equals_oracle(got, q, oi[keep], od[keep], label + "/oracle/q%d" % q)


def _sweep(a, orc, N, f, items_all, Q_all, trees=(1, T), nqs=(3, 70), n_oracle=4):
    """3 queries: the root margins of query_roots_kernel; 70: by query groups where the width has them.  Every cell is what the
    prefix call answers (the assertion of test_gpu_search_sweep.test_every_cell_equals_the_prefix_call), and the cells of the
    whole forest are the oracle's answers.  Returns the hyperplane dots of the last call's cells."""
    K, k = f + 2, 20
    sks = (1, K, K + 1, 2 * N)                                              # K / K + 1: the sides of one full leaf
    for nq in nqs:
        items, Q = items_all[:nq], Q_all[:nq]
        for src, kw, prefix in (("item", dict(items=items), lambda kk, s, t: a.get_nns_by_item_batch(items, kk, s, n_trees=t)),
                                ("vector", dict(Q=Q), lambda kk, s, t: a.get_nns_by_vector_batch(Q, kk, s, n_trees=t))):
            out = a.search_sweep(k, trees, sks, **kw)
            assert out["ids"].shape == (len(trees), len(sks), nq, k)
            for i, t in enumerate(trees):
                for j, s in enumerate(sks):
                    label = "sweep/f%d/nq%d/%s/t%d/sk%d" % (f, nq, src, t, s)
                    ids, d, cnt = prefix(k, s, t)
                    assert out["count"][i, j].tolist() == cnt.tolist(), label
                    assert out["ids"][i, j].tolist() == ids.tolist(), label
                    assert out["dist"][i, j].tobytes() == d.tobytes(), label
                    assert out["ncand"][i, j].tolist() == prefix(N, s, t)[2].tolist(), label + "/ncand"
                    if src == "item" and t == trees[-1]:
                        for q in range(min(nq, n_oracle)):                  # from the oracle alone
                            oi, od = orc.full(items[q], s)
                            _equals_oracle((out["ids"][i, j], out["dist"][i, j], out["count"][i, j]), q, oi[:k], od[:k],
                                           label + "/oracle/q%d" % q)
                            assert out["ncand"][i, j, q] == len(oi), label + "/oracle ncand/q%d" % q
    return out["ndots"]


def _prefix(a, X, N, f, items_all, Q_all):
    """n_trees = 1 on the three-tree forest is the plain call on a forest of one tree from the same rows and seed."""
    from morna_amd.annoy import AnnoyIndex
    one = AnnoyIndex(f)
    one.add_items(X)
    one.build(1)
    for nq in (3, 70):
        items, Q = items_all[:nq], Q_all[:nq]
        for search_k in (10, 2 * N):
            label = "prefix/f%d/nq%d/sk%d" % (f, nq, search_k)
            _same(a.get_nns_by_item_batch(items, 20, search_k, n_trees=1), one.get_nns_by_item_batch(items, 20, search_k), label + "/item")
            _same(a.get_nns_by_vector_batch(Q, 20, search_k, n_trees=1), one.get_nns_by_vector_batch(Q, 20, search_k), label + "/vector")


@pytest.mark.parametrize("f,per_lane,nv_restricted,nv_sweep", _WIDTHS)
def test_callers_at_width_vs_oracle(capi, f, per_lane, nv_restricted, nv_sweep):
    from morna_amd.annoy import AnnoyIndex
    # the width takes the forms it is here for
    assert (f + 255) // 256 == per_lane
    assert wf.descent_nv(f, 32) == nv_restricted and wf.descent_nv(f, 12) == nv_sweep
    N = f + 300
    rng = np.random.default_rng(31337 + f)
    X = wf.rows(rng, N, f)
    X[17] = 0.0                       # a zero row: norm == 0 paths, margin == 0 coin flips
    X[18] = X[19]                     # a duplicate pair
    o = capi.AnnoyOracle(f, mode=1)
    o.set_items(X)
    o.build(T)
    a = AnnoyIndex(f)
    a.add_items(X)
    a.build(T)
    assert a.forest_stats()["n_split"] >= T                                  # every root splits
    assert wf.compare_forest(a, o) == a.forest_stats()["n_split"]
    items_all = wf.query_items(N, n_all=70)                                  # 0, the zero row, a duplicate and the last row first
    Q_all = rng.standard_normal((70, f), dtype=np.float32)
    orc = _Oracle(o, N)
    _restricted(a, orc, N, f, items_all, Q_all)
    _sweep(a, orc, N, f, items_all, Q_all)
    _prefix(a, X, N, f, items_all, Q_all)


@pytest.mark.parametrize("f,per_lane,nv_restricted,nv_sweep", _WIDTHS)
def test_descents_below_the_roots_at_width(capi, f, per_lane, nv_restricted, nv_sweep):
    """The shape above ends at the roots' children: with f + 300 rows both children of a root are leaves, the descents pop
    leaves only, and the one piece of them that is compiled per width -- the hyperplane dot against the query held in
    registers (wave_dot_held<NV>) -- does not run.  2 f + 300 rows in one tree: the larger child of the root holds more than
    K = f + 2 rows and splits, so the restricted and the sweep descent take dots of their own, at search_k = 1 on the way
    to the first leaf and at 2 N for every split node of the tree."""
    from morna_amd.annoy import AnnoyIndex
    assert wf.descent_nv(f, 32) == nv_restricted and wf.descent_nv(f, 12) == nv_sweep
    N = 2 * f + 300
    rng = np.random.default_rng(41337 + f)
    X = wf.rows(rng, N, f)
    X[17] = 0.0
    X[18] = X[19]
    o = capi.AnnoyOracle(f, mode=1)
    o.set_items(X)
    o.build(1)
    _, n_split, below = wf.level_census(o)
    assert below >= 1 and n_split >= 2, (n_split, below)                     # a split node below the root
    a = AnnoyIndex(f)
    a.add_items(X)
    a.build(1)
    assert wf.compare_forest(a, o) == n_split
    items = wf.query_items(N, n_all=5)
    Q = rng.standard_normal((5, f), dtype=np.float32)
    orc = _Oracle(o, N)
    _restricted(a, orc, N, f, items, Q, nqs=(5,), search_ks=(1, 2 * N), ks=(20,), names=("half", "half+groups", "groups"),
                n_oracle=2)                                                  # (the oracle: 0.4 s a list at 16684 x 8192)
    ndots = _sweep(a, orc, N, f, items, Q, trees=(1,), nqs=(3,), n_oracle=2)
    assert (ndots[0, -1] == n_split).all(), (ndots[0, -1].tolist(), n_split)  # search_k = 2 N: every hyperplane of the tree
