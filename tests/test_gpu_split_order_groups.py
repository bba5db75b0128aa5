"""The order of the split contraction's rows by groups of like root-side codes (splitmm.hip, split_mm_order_rows).  -m gpu

The order only chooses which (row tile, task) products the contraction computes, so the forest must not depend on it; the
order itself is specified in integers ("the order of the rows") and is compared here, element for element,
with a numpy restatement of that text fed the root sides read back from the forest:

  code(item)  the side of the item at the root of trees 0 .. n_bits - 1, tree 0 most significant, n_bits = min(T, 24);
  sort        by (code, id);
  cores       runs of equal codes with at least thr = max(16, ceil(N / 2048)) rows, ascending by code (at most N / thr <= 2048);
  components  cores whose codes differ in at most 2 bits are linked; a component's id is its smallest core;
  assignment  every row to the core nearest in Hamming distance, ties to the lower core;
  final       (component, core, code, id); no core: (code, id).
  MORNA_SPLIT_ORDER_GROUPS=0: n_bits = min(T, 12) and (code, id).

One process per switch setting (the switches are read once), each building every case; the shapes are the smallest at which
the path runs at all: the order is made from 8192 rows up, the per-tile lists need 512 tasks in a level with at most 256 per
tree, and D = 64 (leaves of 66 rows) gives 160 trees 640 tasks at the third level.
"""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

TILE = 256
MAX_CORES = 2048
D = 64

# name -> (matrix, rows, trees)
CASES = {
    "clustered": ("clustered", 9000, 160),
    "unclustered": ("gauss", 9000, 160),
    "three_rows": ("copies", 9000, 160),
    "two_trees": ("clustered", 9000, 2),
    "thirteen_trees": ("clustered", 9000, 13),
    "n8192": ("clustered", 8192, 160),
    "n8191": ("clustered", 8191, 160),
}
RUNS = (("default", {"MORNA_DEBUG_OPEN": "1"}), ("groups_off", {"MORNA_SPLIT_ORDER_GROUPS": "0", "MORNA_DEBUG_OPEN": "1"}),
        ("no_order", {"MORNA_SPLIT_ORDER": "0"}), ("no_lists", {"MORNA_SPLIT_LISTS": "0"}))
_ORDER_LINE = re.compile(r"^\[morna\] split order: bits=(\d+) cores=(\d+) components=(\d+) rows_in_cores=(\d+)$")

# sizes of the mixture's clusters for 9000 rows (fewer rows: the last ones shrink): one below thr = 16, one above 1024
_SIZES = (12, 2600, 1500, 1300, 1200, 1000, 800, 588)


def make_matrix(kind, n):
    rng = np.random.default_rng(20261020)
    if kind == "gauss":
        return rng.standard_normal((n, D)).astype(np.float32)
    if kind == "copies":
        return rng.standard_normal((3, D)).astype(np.float32)[rng.integers(0, 3, n)]
    assert kind == "clustered"
    C = rng.standard_normal((len(_SIZES), D))
    C[2] = C[1] + 0.5 * rng.standard_normal(D)   # two centres close to each other: root hyperplanes cut through the pair
    lab = np.repeat(np.arange(len(_SIZES)), _SIZES)
    noise = rng.standard_normal((len(lab), D))
    X = (C[lab] + noise).astype(np.float32)
    return X[rng.permutation(len(lab))][:n]   # scrambled: the id order says nothing about the clusters


# ---- the numpy restatement ---------------------------------------------------------------------------------------------
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def popcount(x):
    x = np.asarray(x, np.uint32)
    return _POP8[x & 255] + _POP8[(x >> 8) & 255] + _POP8[(x >> 16) & 255] + _POP8[(x >> 24) & 255]


def root_sides(node_rec, perm, n_bits):
    """sides[t][item] of the first n_bits trees: 1 for the items of the root's second child (roots are nodes 0 .. T - 1)."""
    n = perm.shape[1]
    sides = np.zeros((n_bits, n), np.uint8)
    for t in range(n_bits):
        kind, tree, start, count, c0, c1 = node_rec[t]
        assert kind == 0 and tree == t and start == 0 and count == n
        s1, n1 = node_rec[c1][2], node_rec[c1][3]
        assert node_rec[c0][2] == 0 and node_rec[c0][3] == s1 and s1 + n1 == n
        sides[t, perm[t, s1:s1 + n1]] = 1
    return sides


def restate_order(sides, groups=True, d_merge=2):
    """(item_at, cores, components, rows_in_cores) by the rule in the module docstring; sides: [>= n_bits][N] of 0 / 1."""
    n = sides.shape[1]
    n_bits = min(sides.shape[0], 24 if groups else 12)
    code = np.zeros(n, np.int64)
    for t in range(n_bits):
        code = code * 2 + sides[t]
    ids = np.arange(n)
    by_code = np.lexsort((ids, code))
    if not groups:
        return by_code.astype(np.int32), 0, 0, 0
    thr = max(16, -(-n // 2048))
    ucodes, counts = np.unique(code, return_counts=True)
    cores = ucodes[counts >= thr]   # ascending by code
    assert len(cores) <= MAX_CORES   # follows from thr
    if len(cores) == 0:
        return by_code.astype(np.int32), 0, 0, 0
    linked = popcount(cores[:, None] ^ cores[None, :]) <= d_merge
    comp = np.arange(len(cores))
    while True:   # minimum label over neighbours until nothing changes
        new = np.where(linked, comp[None, :], len(cores)).min(axis=1)
        if (new == comp).all():
            break
        comp = new
    near = popcount(code[:, None] ^ cores[None, :]).argmin(axis=1)   # the first minimum: ties to the lower core
    item_at = np.lexsort((ids, code, near, comp[near]))
    return item_at.astype(np.int32), len(cores), int((comp == np.arange(len(cores))).sum()), int(counts[counts >= thr].sum())


def level_nodes(node_rec):
    """level of every node (roots: the nodes nobody's child)."""
    kind, c0, c1 = node_rec[:, 0], node_rec[:, 4], node_rec[:, 5]
    level = np.full(len(node_rec), -1, np.int32)
    is_child = np.zeros(len(node_rec), bool)
    is_child[c0[kind == 0]] = True
    is_child[c1[kind == 0]] = True
    frontier, lv = np.nonzero(~is_child)[0], 0
    while len(frontier):
        level[frontier] = lv
        sp = frontier[kind[frontier] == 0]
        frontier, lv = np.concatenate([c0[sp], c1[sp]]), lv + 1
    return level


def active_pairs(node_rec, perm, item_at):
    """{level: (tile of 256 rows, split node) pairs that hold a row} for the levels that use the per-tile lists (from the third
    on, at least 512 split nodes, at most 256 per tree), as scripts/active_pairs_probe.py counts them."""
    T, n = perm.shape
    rank = np.empty(n, np.int64)
    rank[item_at] = np.arange(n)
    level = level_nodes(node_rec)
    out = {}
    for L in range(2, int(level.max()) + 1):
        nodes = np.nonzero((level == L) & (node_rec[:, 0] == 0))[0]
        if len(nodes) < 512 or np.bincount(node_rec[nodes, 1], minlength=T).max() > 256:
            continue
        pairs = 0
        for nd in nodes:
            _, t, start, count = node_rec[nd][:4]
            pairs += len(np.unique(rank[perm[t, start:start + count]] // TILE))
        out[L] = pairs
    return out


# ---- one process per switch setting --------------------------------------------------------------------------------------
def _child(out_dir):
    from morna_amd.annoy import AnnoyIndex
    for name, (kind, n, trees) in CASES.items():
        a = AnnoyIndex(D)
        a.add_items(make_matrix(kind, n))
        a.build(trees)
        f = a.get_forest()
        h = hashlib.sha256()
        for k in ("perm", "node_rec", "hyperplanes", "hp_node"):
            h.update(np.ascontiguousarray(f[k]).tobytes())
        order = a.split_order()
        np.savez(os.path.join(out_dir, name + ".npz"), perm=f["perm"], node_rec=f["node_rec"],
                 order=np.zeros(0, np.int32) if order is None else order, has_order=order is not None)
        sys.stderr.flush()
        print("CASE", name, h.hexdigest(), flush=True)
        sys.stderr.write("[test] end of %s\n" % name)
        sys.stderr.flush()
        del a


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{run: {case: dict(digest, perm, node_rec, order or None, lines)}}"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    here = os.path.dirname(os.path.abspath(__file__))
    out = {}
    for run, extra in RUNS:
        d = str(tmp_path_factory.mktemp(run))
        code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_split_order_groups as m; m._child(%r)" % (root, here, d)
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        digests = dict(ln.split()[1:3] for ln in r.stdout.splitlines() if ln.startswith("CASE"))
        lines, cur = {}, []
        for ln in r.stderr.splitlines():   # the library's lines of each build, up to the child's marker
            if ln.startswith("[test] end of "):
                lines[ln[len("[test] end of "):]] = cur
                cur = []
            else:
                cur.append(ln)
        out[run] = {}
        for name in CASES:
            z = np.load(os.path.join(d, name + ".npz"))
            out[run][name] = dict(digest=digests[name], perm=z["perm"], node_rec=z["node_rec"],
                                  order=z["order"] if bool(z["has_order"]) else None, lines=lines[name])
    return out


pytestmark_gpu = pytest.mark.gpu


def _order_lines(lines):
    return [tuple(int(x) for x in m.groups()) for m in (_ORDER_LINE.match(ln) for ln in lines) if m]


@pytestmark_gpu
@pytest.mark.parametrize("case", list(CASES))
def test_forest_does_not_depend_on_the_order(runs, case):
    d = {run: runs[run][case]["digest"] for run, _ in RUNS}
    assert d["default"] == d["groups_off"] == d["no_order"] == d["no_lists"], d


@pytestmark_gpu
@pytest.mark.parametrize("case", list(CASES))
def test_order_is_the_restated_rule(runs, case):
    kind, n, trees = CASES[case]
    assert runs["no_order"][case]["order"] is None
    for run, groups in (("default", True), ("groups_off", False)):
        r = runs[run][case]
        if n < 8192:   # no order job
            assert r["order"] is None and not _order_lines(r["lines"])
            continue
        assert r["order"] is not None
        assert np.array_equal(np.sort(r["order"]), np.arange(n))
        sides = root_sides(r["node_rec"], r["perm"], min(trees, 24))
        want, cores, comps, in_cores = restate_order(sides, groups=groups)
        got = _order_lines(r["lines"])
        print(case, run, got)
        assert got == [(min(trees, 24 if groups else 12), cores, comps, in_cores)], (got, cores, comps, in_cores)
        assert np.array_equal(r["order"], want), np.nonzero(r["order"] != want)[0][:10]
        if groups and kind == "clustered" and trees >= 13:
            assert cores > 0 and comps > 0   # the case is about groups: the mixture must have some
        if kind == "gauss":
            assert cores == 0                # ... and this one about the fallback
    # the lists' level ran with each order (lists need 512 tasks)
    if n >= 8192 and trees == 160:
        assert any("lists=ahead" in ln and "rows=ordered" in ln for ln in runs["default"][case]["lines"])


@pytestmark_gpu
def test_fewer_pairs_on_clustered_rows(runs):
    """A property of the rule, not of the kernels: under the restated grouped order every level that uses the lists has
    fewer (tile, task) pairs than under the restated 12-bit order.  The mixture was chosen so on the CPU, with a forest from the
    oracle: there the grouped order has 0.80 - 0.98 of the 12-bit order's pairs at the levels 2 .. 10 (32 cores, 3 components;
    with a tenth of the noise the clusters never share a leading bit and the two orders differ by 1 % at most)."""
    r = runs["default"]["clustered"]
    sides = root_sides(r["node_rec"], r["perm"], 24)
    new = active_pairs(r["node_rec"], r["perm"], restate_order(sides, True)[0])
    old = active_pairs(r["node_rec"], r["perm"], restate_order(sides, False)[0])
    print("pairs by level, grouped order:", new, "12-bit order:", old)
    assert len(new) >= 2 and sorted(new) == sorted(old)
    for L in new:
        assert new[L] < old[L], (L, new[L], old[L])


# ---- host only -------------------------------------------------------------------------------------------------------------
def test_ctypes_signature_matches_the_header():
    import ctypes as C
    from morna_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "morna_hip.h")) as fh:
        src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+morna_debug_split_order\s*\(([^)]*)\)\s*;", src)
    assert m
    assert m.group(1) == "int"
    args = [a.strip() for a in m.group(2).split(",")]
    assert [re.sub(r"\s+", " ", a) for a in args] == ["morna_index *h", "int32_t *item_at"]
    res, argtypes = _lib.SIGNATURES["morna_debug_split_order"]
    assert res is C.c_int and len(argtypes) == 2 and all(t is C.c_void_p for t in argtypes)
    assert re.search(r"#define\s+MORNA_E_STATE\s+-3\b", src) and _lib.E_STATE == -3
