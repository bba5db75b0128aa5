"""A forest level's chain: the per-tile task lists built beside two_means, the fp16 image of the level's hyperplanes
written by the two_means kernel that made them.  -m gpu

Both only move work: the lists (splitmm.hip, split_mm_level_lists) read nothing two_means makes, and the image a
two_means epilogue writes (forest.hip; devutil.hpp half_*) has the bits rows_to_half_kernel gives the same hyperplane.
So the forest must not change with MORNA_SPLIT_LISTS_AHEAD=0 (lists in front of the contraction),
MORNA_TM_HALF_EPILOGUE=0 (a conversion launch behind two_means), both, or MORNA_SPLIT_MM=0 (the all-fp32 path) --
one process per setting: the switches are read once.  Shapes: the smallest that reach each form
(MORNA_DEBUG_OPEN=1 makes the library say which way every level went).

The image's two norm bounds are sums of squares, widened by 0.2 %.  The one-wave form adds them up in the conversion
kernel's own order: the filter leaves the same pairs open, level by level.  The strip and wide forms (four waves per
node) add in another order, so a bound may differ in its last digits and a pair whose |C| lies that close to it can
change sides of the filter -- never its side of the hyperplane.  Measured on the shapes below (MI355X), open pairs
per level, epilogue against conversion (levels in order; s = strip, w = wave, x = wide; the counts were the same in both
processes at every level):
  D = 256:  56w 31w 16663w 27139w 23670w 16057w 6755w      D = 1000: 0s 75s 43002w 52640w
  D = 3000: 0s 0s 6902s                                    D = 8448: 0x          (D = 1280: conversion in both)
Largest difference at a strip / wide level: 0 pairs; the margin allowed there is twice that.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, {root!r})
from morna_amd.annoy import AnnoyIndex
N, D, T = {N}, {D}, {T}
rng = np.random.default_rng(2027 + D)
nc = 5
C = rng.standard_normal((nc, D)).astype(np.float32)
lab = rng.integers(0, nc, N)
X = C[lab] + np.float32(0.25) * rng.standard_normal((N, D), dtype=np.float32)
X *= (10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
a = AnnoyIndex(D)
a.add_items(X)
a.build(T)
f = a.get_forest()
h = hashlib.sha256()
for k in ("perm", "node_rec", "hyperplanes", "hp_node"):
    h.update(np.ascontiguousarray(f[k]).tobytes())
st = a.forest_stats()
print("DIGEST", h.hexdigest(), st["n_split"], st["max_depth"])
"""

_RUNS = (("default", {"MORNA_DEBUG_OPEN": "1"}),
         ("lists_behind", {"MORNA_SPLIT_LISTS_AHEAD": "0"}),
         ("converted", {"MORNA_TM_HALF_EPILOGUE": "0", "MORNA_DEBUG_OPEN": "1"}),
         ("both_off", {"MORNA_SPLIT_LISTS_AHEAD": "0", "MORNA_TM_HALF_EPILOGUE": "0"}),
         ("no_mm", {"MORNA_SPLIT_MM": "0"}))

_MARGIN = 2 * 0   # open pairs a strip / wide level may leave beyond the conversion's: twice the largest difference measured

_LEVEL = re.compile(r"^\[morna\] split_mm level: D=\d+ split nodes=(\d+) .* open=(\d+) ")
_PATH = re.compile(r"^\[morna\] split_mm path: split nodes=(\d+) tiles=(\d+) lists=(\w+) image=(\w+)")


def _run(script, extra):
    """(digest fields, [(split nodes, open pairs, tiles, lists, image)] per level that went through the contraction)"""
    r = subprocess.run([sys.executable, script], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()[1:]
    levels, opened = [], None
    for ln in r.stderr.splitlines():
        m = _LEVEL.match(ln)
        if m:
            opened = (int(m.group(1)), int(m.group(2)))
            continue
        m = _PATH.match(ln)
        if m and opened is not None:
            assert int(m.group(1)) == opened[0], ln
            levels.append(opened + (int(m.group(2)), m.group(3), m.group(4)))
            opened = None
    return out, levels


# D, N, T, forms of two_means the default process must have taken the image from, lists expected
_SHAPES = [(256, 9000, 150, {"wave"}, True),              # one float4 per lane; 600 / 1200 / 2400 tasks: ordered rows, lists, 256 x 256
           (1000, 9000, 150, {"strip", "wave"}, True),    # dpad 1024: strips at levels 0-1, one wave below, lists from 600 tasks
           (3000, 16000, 6, {"strip"}, False),            # the benchmark's row length; dense 128 x 128 form only
           (1280, 9000, 6, {"converted"}, False),         # no register form (two_means_kernel): the conversion kernel still runs
           (8448, 9000, 4, {"wide"}, False)]              # two_means_wide_kernel's epilogue


@pytest.mark.parametrize("D,N,T,forms,lists", _SHAPES)
def test_level_chain_switches_change_nothing(tmp_path, D, N, T, forms, lists):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = str(tmp_path / "digest.py")
    with open(script, "w") as fh:
        fh.write(_SCRIPT.format(root=root, N=N, D=D, T=T))
    out, levels = {}, {}
    for name, extra in _RUNS:
        out[name], levels[name] = _run(script, extra)
    for name, _ in _RUNS:
        assert out[name] == out["default"], (name, out)
    dflt, conv = levels["default"], levels["converted"]
    for row in zip(dflt, conv):
        print(D, "epilogue", row[0], "conversion", row[1])
    assert dflt, "the matrix-core split did not run"
    assert {lv[4] for lv in dflt} >= forms, dflt                     # the forms this shape is here for wrote the image
    assert {lv[4] for lv in conv} == {"converted"}, conv
    if lists:
        assert any(lv[3] == "ahead" and lv[2] == 256 for lv in dflt), dflt   # the list path was taken, beside two_means
    else:
        assert all(lv[3] == "none" for lv in dflt), dflt
    # the image: the same levels, and the filter leaves (nearly) the same pairs open
    assert [lv[0] for lv in dflt] == [lv[0] for lv in conv], (dflt, conv)
    for e, c in zip(dflt, conv):
        if e[4] in ("wave", "converted"):
            assert e[1] == c[1], (e, c)                              # same summation order: the same bounds, bit for bit
        else:
            assert e[1] <= c[1] + _MARGIN, (e, c)
