"""The forms of the forest build's partition give one forest.  -m gpu

A level's stable partition runs in the streaming form by default (forest.hip, partition_stream_kernel): 16 positions per
thread, chunks of 4096 positions that start where the node's items are 16-byte aligned in their image, one workgroup per
chunk behind a counting pass wherever a node of the attempt may span more than two chunks (more than 8189 positions), one
workgroup per node otherwise.
MORNA_PARTITION_FORM=0 is the earlier kernel, MORNA_PARTITION_FORM=2 the streaming form with one workgroup per node at every
level (a node's chunks one after the other), MORNA_PARTITION_INV=1 the earlier kernel keeping `inv`.  The switches are read
once per process: one child process per setting builds every shape below and prints a digest of the forest bytes (perm,
node_rec, hp_node, hyperplanes) and forest_stats(); the settings must agree shape by shape, and the default build is also
compared node for node with CPU oracle mode 1 on the shapes marked so.

Shapes, D = 64 (leaf capacity 66), 4 to 8 trees; a root holds all N rows, so its size is N:
  4095, 4096, 4097      one chunk less one, exactly, plus one (4097: the second chunk holds one position, or four at m = 3);
                        one workgroup per node, which walks both chunks
  8191, 8192, 8193      two chunks less one, exactly, plus one, or three where the image's alignment m shifts them; one
                        workgroup per chunk (the children, of about 4096 rows, are back at one workgroup per node)
  20000                 five chunks to a root: several workgroups share a node and sum the counts in front of theirs
  50                    the roots are leaves: no partition runs
  3000, a third of the rows copies of four rows   attempts fail, retries run, the random sides of `attempt` 3 are partitioned;
                        a node whose sides do not stand must be left as it was for the next attempt to read (oracle)
  6000, 301 rows in a second cluster   the roots split 5699 : 301, imbalance 0.94983 < 0.95: as lopsided as a first attempt
                        may stand (oracle)
Odd N put the images of the trees at every alignment (m = 0..3), and from the second level on segment starts are no
multiples of 4: asserted from node_rec.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 64
# name, N, trees, rows ("clusters", "dup", "lopsided"), compared with the oracle
_SHAPES = [("n4095", 4095, 4, "clusters", False),
           ("n4096", 4096, 4, "clusters", False),
           ("n4097", 4097, 4, "clusters", False),
           ("n8191", 8191, 4, "clusters", False),
           ("n8192", 8192, 4, "clusters", False),
           ("n8193", 8193, 4, "clusters", False),
           ("n20000", 20000, 4, "clusters", False),
           ("n50", 50, 4, "clusters", False),
           ("dup3000", 3000, 8, "dup", True),
           ("lopsided6000", 6000, 4, "lopsided", True)]
_SETTINGS = (("default", {}),
             ("form0", {"MORNA_PARTITION_FORM": "0"}),
             ("form2", {"MORNA_PARTITION_FORM": "2"}),
             ("inv", {"MORNA_PARTITION_INV": "1"}))
_SWITCHES = ("MORNA_PARTITION_FORM", "MORNA_PARTITION_INV", "MORNA_SPLIT_ORDER", "MORNA_SPLIT_LISTS", "MORNA_SPLIT_LISTS_AHEAD",
             "MORNA_SPLIT_MM", "MORNA_BUILD_TAIL", "MORNA_DEBUG_TURN", "MORNA_DEBUG_OPEN")

_SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, @ROOT@)
sys.path.insert(0, @TESTS@)
from morna_amd.annoy import AnnoyIndex
D = @D@

def rows(kind, N):
    rng = np.random.default_rng(2027 + D + (0 if kind == "dup" else N))   # dup: the rows of tests/test_gpu_level_turnaround.py
    if kind == "lopsided":   # two tight clusters, 301 rows in the second
        C = rng.standard_normal((2, D)).astype(np.float32)
        lab = np.zeros(N, np.int64)
        lab[rng.choice(N, 301, replace=False)] = 1
        return C[lab] + np.float32(0.05) * rng.standard_normal((N, D), dtype=np.float32)
    C = rng.standard_normal((5, D)).astype(np.float32)
    X = C[rng.integers(0, 5, N)] + np.float32(0.25) * rng.standard_normal((N, D), dtype=np.float32)
    X *= (10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
    if kind == "dup":   # a third of the rows are exact copies of a few rows: nodes no hyperplane can cut
        src = rng.integers(0, 4, N // 3)
        X[rng.choice(N, N // 3, replace=False)] = X[src]
    return X

for name, N, T, kind, with_oracle in @SHAPES@:
    X = rows(kind, N)
    a = AnnoyIndex(D)
    a.add_items(X)
    a.build(T)
    f = a.get_forest()
    st = a.forest_stats()
    h = hashlib.sha256()
    for k in ("perm", "node_rec", "hp_node", "hyperplanes"):
        h.update(np.ascontiguousarray(f[k]).tobytes())
    h.update(repr(sorted(st.items())).encode())
    if @ORACLE@ and with_oracle:
        import width_forms as wf
        from oracle import capi
        o = capi.AnnoyOracle(D, mode=1)
        o.set_items(X)
        o.build(T)
        assert wf.compare_forest(a, o) == st["n_split"], name
        print("ORACLE", name, flush=True)
    if @REC@:
        np.save(@REC@ + name + ".npy", f["node_rec"])
    print("SHAPE", name, h.hexdigest(), st["n_split"], st["max_depth"], st["split_attempts"], st["fallback_nodes"], flush=True)
"""


def _run(tmp, name, extra, shapes, oracle, rec_prefix):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = _SCRIPT
    for key, value in (("ROOT", root), ("TESTS", os.path.join(root, "tests")), ("D", D), ("SHAPES", shapes), ("ORACLE", oracle),
                       ("REC", rec_prefix)):
        text = text.replace("@%s@" % key, repr(value))
    script = str(tmp / ("forms_%s.py" % name))
    with open(script, "w") as fh:
        fh.write(text)
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    r = subprocess.run([sys.executable, script], env=dict(env, **extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (name, r.stdout[-1000:], r.stderr[-2000:])
    out = {ln.split()[1]: ln.split()[2:] for ln in r.stdout.splitlines() if ln.startswith("SHAPE")}
    checked = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("ORACLE")]
    return out, checked


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: {shape: [digest, n_split, max_depth, split_attempts, fallback_nodes]}}, the shapes the oracle confirmed, and
    where the default build left each shape's node_rec.  MORNA_PARTITION_INV=1 builds three shapes only."""
    tmp = tmp_path_factory.mktemp("partition_forms")
    prefix = str(tmp / "rec_")
    out, checked = {}, []
    for name, extra in _SETTINGS:
        shapes = [s for s in _SHAPES if name != "inv" or s[0] in ("n8193", "dup3000", "n20000")]
        out[name], c = _run(tmp, name, extra, shapes, name == "default", prefix if name == "default" else "")
        checked += c
    return out, checked, prefix


def _depths(rec):
    """depth of every node (node_rec rows: leaf, tree, start, count, child 0, child 1; breadth-first ids)"""
    depth = np.zeros(len(rec), np.int64)
    for i in range(len(rec)):
        if not rec[i, 0]:
            depth[int(rec[i, 4])] = depth[int(rec[i, 5])] = depth[i] + 1
    return depth


@pytest.mark.parametrize("name,N,T,kind,with_oracle", _SHAPES)
def test_partition_forms_give_one_forest(runs, name, N, T, kind, with_oracle):
    out, checked, prefix = runs
    ref = out["default"][name]
    print(name, ref[1:], {s: out[s].get(name, ["-"])[0][:12] for s in out})
    for setting in out:
        if name in out[setting]:
            assert out[setting][name] == ref, (setting, name, out[setting][name], ref)
    assert name in out["form0"] and name in out["form2"]
    assert (name in checked) == with_oracle
    n_split, max_depth, attempts, fallback = (int(x) for x in ref[1:])
    rec = np.load(prefix + name + ".npy")
    split = rec[rec[:, 0] == 0]
    assert len(split) == n_split
    if N <= D + 2:   # the roots are leaves
        assert n_split == 0 and len(rec) == T
        return
    assert n_split >= T and int(split[:, 3].max()) == N     # every root splits: a node of exactly N positions was partitioned
    # a split node below the roots starts where its parent's left child ended: somewhere
    depth = _depths(rec)
    deep = rec[(rec[:, 0] == 0) & (depth >= 1)]
    assert len(deep) and (deep[:, 2] % 4 != 0).any(), name
    if kind == "dup":
        assert attempts > n_split and fallback > 0, ref
    if kind == "lopsided":   # 5699 : 301 at every root
        kids = np.sort(rec[rec[:T, 4:6].astype(np.int64), 3], axis=1)
        assert (kids == [301, N - 301]).all(), kids


def test_inv_form_ran_on_its_shapes(runs):
    out = runs[0]
    assert sorted(out["inv"]) == ["dup3000", "n20000", "n8193"]
