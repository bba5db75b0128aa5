"""The forest build's tail: the last narrow levels run behind build()'s return, beside the next batch's contraction.  -m gpu

build() returns once the first attempt of a narrow level (at most n_cus / 8 split nodes, level >= 1) has been enqueued;
whatever touches the handle next runs the rest (finish_build, forest.hip), and the first dense query batch starts its
whole-batch contraction on a stream of its own before it does (knn.hip).  Same kernels, same tasks, same order: the forest
(perm, node_rec, hyperplanes, hp_node, stats) and the answers of the first search must be equal, bit for bit, to those of
MORNA_BUILD_TAIL=0, which completes the build before it returns -- one process per setting (the switch is read once),
the data of tests/test_gpu_level_turnaround.py.

Shapes (N, D, T; split nodes per level as the CPU oracle, mode 1, counted them -- what to expect, asserted only through what
the library says and the forest holds):
  16640, 256, 40   40, 80, 160, 318, 605, 952, 965, 577, 179, 27, 3   a two-level tail
  9000, 256, 150   ..., 294, 33, 2                                     a one-level tail, just past the threshold
  6000, 256, 64, a third of the rows duplicated   ..., 133, 24, 2      a tail on data with retries and fallback nodes
  2000, 256, 64    64, 128, 256, 195, 49                               no tail
  200, 256, 8      none (N <= K)                                       no split at all
MORNA_DEBUG_OPEN=1 makes the library say where it deferred and who finished the tail; the expected depth is read off the
forest itself: the first level >= 1 with at most 32 split nodes (256 CUs).

On the first shape the first call after build() is varied (fresh handle each, one process): the dense by-item and
by-vector batches (1024 queries: 256 x 256 tiles over 64 row tiles, the 128 x 128 form behind them), an 8-query batch,
get_forest, forest_stats, save (file bytes equal) + load into a fresh handle, an exact search, a restricted search,
synchronize; a rebuild with another tree count on a used handle against a fresh one; and a handle dropped straight
after build().
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_level_turnaround import _SCRIPT as _TURNAROUND_SCRIPT

pytestmark = pytest.mark.gpu

# the rows: the generator of the level turn-around test, as it stands there
_DATA = _TURNAROUND_SCRIPT[_TURNAROUND_SCRIPT.index("rng = np.random.default_rng"):_TURNAROUND_SCRIPT.index("def digest(a):")]

_HEAD = r"""
import hashlib, os, sys
import numpy as np
sys.path.insert(0, @ROOT@)
from morna_amd.annoy import AnnoyIndex
N, D, T, DUP, NQ = @N@, @D@, @T@, @DUP@, @NQ@
K_NN, SEARCH_K = 10, 100
""" + _DATA + r"""
items = np.linspace(0, N - 1, NQ).astype(np.int32)

def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()

def digest(a):
    f = a.get_forest()
    st = a.forest_stats()
    return sha(f["perm"], f["node_rec"], f["hyperplanes"], f["hp_node"], repr(sorted(st.items())).encode()), f, st

def fresh():
    a = AnnoyIndex(D)
    a.add_items(X)
    return a

def say(*words):
    print(*words, flush=True)

def mark(name):   # between the library's own lines on stderr
    sys.stderr.write("VARIANT %s\n" % name)
    sys.stderr.flush()
"""

# one shape, one setting: build, the first search, then the forest
_SHAPE = _HEAD + r"""
a = fresh()
a.build(T)
ans = sha(*a.get_nns_by_item_batch(items, K_NN, SEARCH_K))
d, f, st = digest(a)
np.save(@REC@, f["node_rec"])
say("RESULT", d, ans, st["n_split"], st["max_depth"], st["split_attempts"], st["fallback_nodes"])
"""

# the first shape: what the first call after build() is, a fresh handle per variant
_VARIANTS = _HEAD + r"""
Q = X[items]
allow = (np.arange(N) % 3) != 0
ex_items = items[:16]
few = items[:8]

def after(name, a, *first):   # the first call's own answer (if it has one), then the forest and the standard search
    d = digest(a)[0]
    ans = sha(*a.get_nns_by_item_batch(items, K_NN, SEARCH_K))
    say("VARIANT", name, d, ans, sha(*first) if first else "-")

mark("by_item"); a = fresh(); a.build(T); after("by_item", a, *a.get_nns_by_item_batch(items, K_NN, SEARCH_K))
mark("by_vector"); a = fresh(); a.build(T); after("by_vector", a, *a.get_nns_by_vector_batch(Q, K_NN, SEARCH_K))
mark("few"); a = fresh(); a.build(T); after("few", a, *a.get_nns_by_item_batch(few, K_NN, SEARCH_K))
mark("get_forest"); a = fresh(); a.build(T); f = a.get_forest(); after("get_forest", a, f["perm"], f["node_rec"], f["hyperplanes"], f["hp_node"])
mark("forest_stats"); a = fresh(); a.build(T); st = a.forest_stats(); after("forest_stats", a, repr(sorted(st.items())).encode())
mark("save"); a = fresh(); a.build(T); a.save(@SAVE@)
b = AnnoyIndex(D); b.load(@SAVE@); after("save", b, open(@SAVE@, "rb").read())
after("saved_handle", a)
mark("exact"); a = fresh(); a.build(T); after("exact", a, *a.exact_search_by_item_batch(ex_items, K_NN))
mark("restricted"); a = fresh(); r = a.restriction(allow=allow); a.build(T); after("restricted", a, *a.get_nns_restricted(r, K_NN, SEARCH_K, items=items))
mark("synchronize"); a = fresh(); a.build(T); a.synchronize(); after("synchronize", a)
# a used handle: rows loaded, build(T), the rows loaded again, build(T // 2) -- against a fresh handle's build(T // 2)
mark("rebuild"); a = fresh(); a.save(@ROWS@); a.build(T); a.load(@ROWS@); a.build(T // 2); after("rebuild", a)
mark("fresh_half"); b = fresh(); b.build(T // 2); after("fresh_half", b)
mark("end")
"""

# a handle dropped straight after build(), nothing else called
_DROP = _HEAD + r"""
a = fresh()
a.build(T)
del a
say("DROPPED")
"""

_SWITCHES = ("MORNA_BUILD_TAIL", "MORNA_PARTITION_INV", "MORNA_SPLIT_ORDER", "MORNA_SPLIT_LISTS", "MORNA_SPLIT_LISTS_AHEAD",
             "MORNA_SPLIT_MM", "MORNA_DEBUG_TURN", "MORNA_QUERY_DENSE", "MORNA_QUERY_FILTER", "MORNA_QUERY_BIG")
_DEFER = re.compile(r"^\[morna\] build tail: deferred at level=(\d+) tasks=(\d+)")
_DONE = re.compile(r"^\[morna\] build tail: finished by (.+): levels=(\d+) attempts=(\d+)$")
_MARK = re.compile(r"^VARIANT (\w+)$")


def _write(tmp_path, name, text, **fields):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = dict(fields, ROOT=root)
    for key, value in fields.items():
        text = text.replace("@%s@" % key, repr(value))
    path = str(tmp_path / name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def _run(script, tail_off):
    """(stdout lines, [(variant, 'defer', level, tasks) | (variant, 'done', who, levels, attempts)] as stderr has them)"""
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env["MORNA_DEBUG_OPEN"] = "1"
    if tail_off:
        env["MORNA_BUILD_TAIL"] = "0"
    r = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    events, variant = [], None
    for ln in r.stderr.splitlines():
        m = _MARK.match(ln)
        if m:
            variant = m.group(1)
        m = _DEFER.match(ln)
        if m:
            events.append((variant, "defer", int(m.group(1)), int(m.group(2))))
        m = _DONE.match(ln)
        if m:
            events.append((variant, "done", m.group(1), int(m.group(2)), int(m.group(3))))
    return r.stdout.splitlines(), events


def _splits_per_level(rec):
    """split nodes per depth (node_rec rows: leaf, tree, start, count, child 0, child 1; breadth-first ids)"""
    depth = np.zeros(len(rec), np.int64)
    counts = {}
    for i in range(len(rec)):
        if rec[i, 0]:
            continue
        depth[int(rec[i, 4])] = depth[int(rec[i, 5])] = depth[i] + 1
        counts[int(depth[i])] = counts.get(int(depth[i]), 0) + 1
    return [counts[d] for d in range(len(counts))]


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# N, D, T, duplicated rows, queries, levels the tail is expected to have at least (0: no deferral)
_SHAPES = [(16640, 256, 40, False, 1024, 2),
           (9000, 256, 150, False, 256, 1),
           (6000, 256, 64, True, 256, 1),
           (2000, 256, 64, False, 256, 0),
           (200, 256, 8, False, 64, 0)]


@pytest.mark.parametrize("N,D,T,dup,nq,tail_levels", _SHAPES)
def test_build_tail_changes_nothing(tmp_path, N, D, T, dup, nq, tail_levels):
    rec_path = str(tmp_path / "node_rec.npy")
    script = _write(tmp_path, "shape.py", _SHAPE, N=N, D=D, T=T, DUP=dup, NQ=nq, REC=rec_path)
    out, ev = {}, {}
    for name, off in (("default", False), ("tail_off", True)):
        lines, ev[name] = _run(script, off)
        out[name] = [ln for ln in lines if ln.startswith("RESULT")][0].split()[1:]
        print(N, name, out[name][2:], ev[name])
    assert out["default"] == out["tail_off"], out   # forest digest, answers of the first search, stats
    assert not ev["tail_off"], ev["tail_off"]        # MORNA_BUILD_TAIL=0: the build completes before it returns
    per_level = _splits_per_level(np.load(rec_path))
    max_depth = int(out["default"][3])
    print(N, "split nodes per level", per_level)
    narrow = _cus() // 8
    expected = [lv for lv in range(1, len(per_level)) if per_level[lv] <= narrow]
    if tail_levels == 0:
        assert not ev["default"], ev["default"]
        assert not expected, per_level
        if N <= D + 2:
            assert per_level == [] and int(out["default"][2]) == 0, out["default"]
        return
    # one deferral, at the first level >= 1 whose split nodes are few, with that level's nodes as its tasks; the first search
    # (dense, by item) finished it behind its own contraction
    assert [e[1] for e in ev["default"]] == ["defer", "done"], ev["default"]
    (_, _, level, tasks), (_, _, who, levels, attempts) = ev["default"]
    assert expected and level == expected[0] and tasks == per_level[level], (level, tasks, per_level)
    assert who == "query_batch, beside its contraction", who
    assert level + levels == max_depth and levels == len(per_level) - level, (level, levels, max_depth, per_level)
    assert levels >= tail_levels and attempts >= levels, (levels, attempts)
    if dup:   # retries and fallback nodes inside or before the tail
        n_split, split_attempts, fallback = int(out["default"][2]), int(out["default"][4]), int(out["default"][5])
        assert fallback > 0 and split_attempts > n_split, out["default"]


def test_first_call_after_build(tmp_path):
    N, D, T, nq = _SHAPES[0][:3] + (_SHAPES[0][4],)
    fields = dict(N=N, D=D, T=T, DUP=False, NQ=nq, SAVE=str(tmp_path / "index.mor"), ROWS=str(tmp_path / "rows.mor"))
    script = _write(tmp_path, "variants.py", _VARIANTS, **fields)
    res, ev = {}, {}
    for name, off in (("default", False), ("tail_off", True)):
        lines, ev[name] = _run(script, off)
        res[name] = {ln.split()[1]: ln.split()[2:] for ln in lines if ln.startswith("VARIANT")}
    ref = res["tail_off"]
    assert not ev["tail_off"], ev["tail_off"]
    full = ("by_item", "by_vector", "few", "get_forest", "forest_stats", "save", "saved_handle", "exact", "restricted", "synchronize")
    assert set(res["default"]) == set(ref) == set(full + ("rebuild", "fresh_half"))
    for name in full:   # the same forest and the same answers whatever came first, and the first call's own answer
        assert res["default"][name] == ref[name], (name, res["default"][name], ref[name])
        assert ref[name][:2] == ref["by_item"][:2], (name, ref[name], ref["by_item"])
    for r in (res["default"], ref):   # nothing of the first build survives in the second
        assert r["rebuild"] == r["fresh_half"] and r["rebuild"][:2] != r["by_item"][:2], (r["rebuild"], r["fresh_half"])
    assert res["default"]["rebuild"] == ref["rebuild"]
    # who finished the tail (every build of this shape defers)
    done = {}
    for e in ev["default"]:
        if e[1] == "done":
            done.setdefault(e[0], []).append(e[2])
    defers = [e[0] for e in ev["default"] if e[1] == "defer"]
    assert sorted(defers) == sorted(sum(([v] * len(w) for v, w in done.items()), [])), (defers, done)
    beside = "query_batch, beside its contraction"
    assert done["by_item"] == [beside] and done["by_vector"] == [beside], done
    assert done["few"] == ["query_batch"], done
    assert done["get_forest"][0] in ("morna_get_forest_stats", "morna_get_forest"), done
    assert done["forest_stats"] == ["morna_get_forest_stats"], done
    assert done["save"] == ["morna_save"], done
    assert done["exact"] == ["morna_exact_search_by_item"], done
    assert done["restricted"] == ["morna_get_nns_restricted"], done
    assert done["synchronize"] == ["morna_synchronize"], done
    assert done["rebuild"][0] == "morna_load", done   # the second load ends the first build; the second build's tail: the digest


def test_handle_dropped_after_build(tmp_path):
    N, D, T, nq = _SHAPES[0][:3] + (_SHAPES[0][4],)
    script = _write(tmp_path, "drop.py", _DROP, N=N, D=D, T=T, DUP=False, NQ=nq)
    lines, ev = _run(script, False)
    assert "DROPPED" in lines
    assert [e[1] for e in ev] == ["defer", "done"] and ev[1][2] == "morna_index_destroy", ev
