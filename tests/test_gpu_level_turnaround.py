"""The turn-around between two forest levels: `inv` off the partition, rebuilt beside the next two_means.  -m gpu

partition_kernel no longer keeps inv[tree][row] (the position of every row in every tree) current; split_inv_kernel
(splitmm.hip) rewrites it on the side stream, under the next level's two_means, for everything the level's partitions
moved -- only in front of a level that takes the matrix-core form.  The contraction's epilogue decides a row's node by
position alone, so a stale position (a row that landed in a leaf beside a split sibling, a retry, a rebuild on a used
handle) would change sides and with them the forest.  The forest must therefore be the same, bit for bit, with
MORNA_PARTITION_INV=1 (the partition's upkeep, as before), without the order of the rows, without the per-tile lists, with
the lists behind two_means, and on the all-fp32 path (MORNA_SPLIT_MM=0, which never reads `inv`) -- one process per
setting: the switches are read once.  The default process and the MORNA_PARTITION_INV=1 one also rebuild on their handle
(build(T) twice, then build(T // 2)) and compare with fresh handles: no `inv` of an earlier build may survive.

The test asserts that the cases were reached (MORNA_DEBUG_OPEN=1 makes the library say how every level went): a level
with inv=side behind ordered rows and lists where the shape has them, a split node with one leaf child and one split
child in front of a level that went through the contraction, and retries and fallback nodes for the shape with
duplicated rows.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, {root!r})
from morna_amd.annoy import AnnoyIndex
N, D, T, DUP = {N}, {D}, {T}, {DUP}
rng = np.random.default_rng(2027 + D)
nc = 5
C = rng.standard_normal((nc, D)).astype(np.float32)
lab = rng.integers(0, nc, N)
X = C[lab] + np.float32(0.25) * rng.standard_normal((N, D), dtype=np.float32)
X *= (10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
if DUP:   # a third of the rows are exact copies of a few rows: nodes no hyperplane can cut
    src = rng.integers(0, 4, N // 3)
    X[rng.choice(N, N // 3, replace=False)] = X[src]

def digest(a):
    f = a.get_forest()
    h = hashlib.sha256()
    for k in ("perm", "node_rec", "hyperplanes", "hp_node"):
        h.update(np.ascontiguousarray(f[k]).tobytes())
    st = a.forest_stats()
    h.update(repr(sorted(st.items())).encode())
    return h.hexdigest(), f, st

a = AnnoyIndex(D)
a.add_items(X)
if {REBUILD}:
    a.save({rows!r})   # the rows alone: loading them puts the handle back in front of its build, scratch buffers and all
a.build(T)
d1, f, st = digest(a)
print("DIGEST", d1, st["n_split"], st["max_depth"], st["split_attempts"], st["fallback_nodes"])
np.save({rec!r}, f["node_rec"])
if {REBUILD}:
    a.load({rows!r})
    a.build(T)
    d2 = digest(a)[0]
    a.load({rows!r})
    a.build(T // 2)
    d3 = digest(a)[0]
    b = AnnoyIndex(D)
    b.add_items(X)
    b.build(T // 2)
    d4 = digest(b)[0]
    print("REBUILD", d2, d3, d4)
"""

_RUNS = (("default", {}),   # (this one and the next also rebuild on their handle)
         ("partition_inv", {"MORNA_PARTITION_INV": "1"}),
         ("no_order", {"MORNA_SPLIT_ORDER": "0"}),
         ("no_lists", {"MORNA_SPLIT_LISTS": "0"}),
         ("lists_behind", {"MORNA_SPLIT_LISTS_AHEAD": "0"}),
         ("no_mm", {"MORNA_SPLIT_MM": "0"}))
_SWITCHES = ("MORNA_PARTITION_INV", "MORNA_SPLIT_ORDER", "MORNA_SPLIT_LISTS", "MORNA_SPLIT_LISTS_AHEAD", "MORNA_SPLIT_MM",
             "MORNA_DEBUG_TURN")

_PATH = re.compile(r"^\[morna\] split_mm path: split nodes=(\d+) tiles=(\d+) lists=(\w+) image=(\w+) inv=(\w+) rows=(\w+) level=(\d+)")


def _run(script, extra, rebuild):
    """(DIGEST fields, REBUILD fields, [(level, tiles, lists, inv, rows)] per attempt that went through the contraction)"""
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    r = subprocess.run([sys.executable, script], env=dict(env, MORNA_DEBUG_OPEN="1", **extra), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()[1:]
    reb = [ln for ln in r.stdout.splitlines() if ln.startswith("REBUILD")][0].split()[1:] if rebuild else None
    levels = []
    for ln in r.stderr.splitlines():
        m = _PATH.match(ln)
        if m:
            levels.append((int(m.group(7)), int(m.group(2)), m.group(3), m.group(5), m.group(6)))
    return out, reb, levels


def _leaf_beside_split(rec):
    """depths d such that some split node of depth d has one leaf child and one split child (node_rec rows: leaf, tree,
    start, count, child 0, child 1; ids are breadth-first, so a child's id is above its parent's)"""
    depth = np.zeros(len(rec), np.int64)
    found = set()
    for i in range(len(rec)):
        if rec[i, 0]:
            continue
        c0, c1 = int(rec[i, 4]), int(rec[i, 5])
        depth[c0] = depth[c1] = depth[i] + 1
        if bool(rec[c0, 0]) != bool(rec[c1, 0]):
            found.add(int(depth[i]))
    return found


# D, N, T, duplicated rows, ordered rows and lists expected, a leaf beside a split sibling in front of a contraction expected
_SHAPES = [(256, 9000, 150, False, True, True),     # many levels, ordered rows, lists, 256 x 256 tiles, leaves beside split siblings
           (1000, 9000, 150, False, True, True),    # strip levels, then one-wave levels
           (3000, 16000, 6, False, False, False),   # the benchmark's row length; dense 128 x 128 form only (its trees are
                                                    # full to the last level: no leaf has a split sibling)
           (64, 3000, 8, True, False, True)]        # retries and fallback nodes


@pytest.mark.parametrize("D,N,T,dup,lists,beside_expected", _SHAPES)
def test_level_turnaround_switches_change_nothing(tmp_path, D, N, T, dup, lists, beside_expected):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec_path = str(tmp_path / "node_rec.npy")
    out, reb, levels = {}, {}, {}
    for name, extra in _RUNS:
        rebuild = name in ("default", "partition_inv")
        script = str(tmp_path / ("digest_%s.py" % name))
        with open(script, "w") as fh:
            fh.write(_SCRIPT.format(root=root, N=N, D=D, T=T, DUP=dup, rec=rec_path, rows=str(tmp_path / "rows.bin"), REBUILD=rebuild))
        out[name], reb[name], levels[name] = _run(script, extra, rebuild)
        print(D, name, out[name][1:], levels[name])
        if name == "default":
            rec = np.load(rec_path)
    for name, _ in _RUNS:
        assert out[name] == out["default"], (name, out)
        if reb[name]:   # build(T) again on the used handle = the first build; build(T // 2) on it = a fresh handle's
            assert reb[name][0] == out[name][0], (name, reb[name], out[name])
            assert reb[name][1] == reb[name][2], (name, reb[name])
    dflt, part = levels["default"], levels["partition_inv"]
    assert dflt, "the matrix-core split did not run"
    assert not levels["no_mm"]
    # who made `inv`: the roots' identity at level 0, the side stream below it; under MORNA_PARTITION_INV=1 the partition
    # (but for the level that orders the rows, whose `inv` by row is written by the side stream in both)
    assert all(lv[3] == ("iota" if lv[0] == 0 else "side") for lv in dflt), dflt
    assert any(lv[3] == "side" for lv in dflt), dflt
    assert all(lv[3] == ("iota" if lv[0] == 0 else "side" if lv[0] == 1 and lv[4] == "ordered" else "partition") for lv in part), part
    assert any(lv[3] == "partition" for lv in part), part
    if lists:
        assert any(lv[3] == "side" and lv[4] == "ordered" and lv[2] == "ahead" and lv[1] == 256 for lv in dflt), dflt
        assert all(lv[4] == "ids" for lv in levels["no_order"]), levels["no_order"]
        assert all(lv[2] == "none" for lv in levels["no_lists"]), levels["no_lists"]
        assert any(lv[2] == "inline" for lv in levels["lists_behind"]), levels["lists_behind"]
    else:
        assert all(lv[2] == "none" for lv in dflt), dflt
    # a leaf beside a split sibling, children of a node of depth d: their positions are read by the contraction of level d + 1
    mm_levels = {lv[0] for lv in dflt}
    beside = _leaf_beside_split(rec)
    print(D, "leaf beside a split sibling below depths", sorted(beside), "contraction at levels", sorted(mm_levels))
    if beside_expected:
        assert any(d + 1 in mm_levels for d in beside), (sorted(beside), sorted(mm_levels))
    if dup:
        n_split, attempts, fallback = int(out["default"][1]), int(out["default"][3]), int(out["default"][4])
        assert fallback > 0 and attempts > n_split, out["default"]
