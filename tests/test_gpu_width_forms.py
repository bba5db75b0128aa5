"""Every row-width form of two_means, and the searches at those widths, against oracle mode 1.  -m gpu

The forest build launches a differently compiled two_means kernel for every row width (forest_host.hpp, fb_attempt) and
the approximate search a differently compiled descent and root-margin kernel (knn.hip, with_row_nv).  Each shape below
is the smallest that splits below its roots at a width whose form no other oracle comparison reaches; width_forms.py
holds the comparison and a restatement of the dispatch (tested by hand-written widths in test_width_forms_cpu.py), and
the handle's tm_strip / tm_wave timers say which form the build did launch -- a form added or a threshold moved shows
as a failed expectation here, not as lost coverage.
"""
import os
import subprocess
import sys

import pytest

import width_forms as wf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from oracle import capi as c
    c.lib()
    return c


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# f, N, T, the form the default build must take at the roots
_WIDTHS = [(641, 2600, 8, ("wave", 3)),          # odd ragged width
           (1500, 6200, 4, ("wave", 6)),
           (1100, 4600, 4, ("lds", None)),       # 5 float4 per lane
           (2303, 9400, 2, ("lds", None)),       # 9, odd ragged
           (7800, 15800, 2, ("lds", None)),      # 31: the longest rows of the LDS form
           (4096, 16600, 2, ("strip", 16)),
           (5900, 12000, 3, ("strip", 24)),      # ragged
           (7000, 14200, 2, ("strip", 28)),
           (17500, 18000, 2, ("wide", 24))]      # 69 k-steps: 17 groups of four and one tail k-step


@pytest.mark.parametrize("f,N,T,form", _WIDTHS)
def test_width_form_vs_oracle(capi, f, N, T, form):
    """Forest node for node, split counters, searches in batches of 96 / 24 / 1, and the launch counts of the form."""
    wide = f > 8192
    got = wf.check_width(capi, f, N, T, _cus(), n_oracle=4 if wide else 24, wide=wide)   # (the oracle: 0.5 s a query at 17500)
    assert got == form


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
from oracle import capi
import width_forms as wf
capi.lib()
for f, N, T in {shapes!r}:
    form = wf.check_width(capi, f, N, T, {n_cus}, strip_on=False)
    print("WIDTH_OK", f, form[0], form[1], flush=True)
"""

# f, N, T, the form MORNA_TM_STRIP=0 puts in the place of the strips
_ONE_WAVE = [(1000, 4100, 4, ("wave", 4)), (2000, 8200, 2, ("wave", 8)), (3000, 12200, 2, ("wave", 12)),
             (4096, 16600, 2, ("lds", None))]


def test_one_wave_forms_vs_oracle_where_strips_run(tmp_path):
    """MORNA_TM_STRIP=0 (read once per process: a child): the one-wave forms of 4, 8 and 12 float4 per lane and the LDS
    form at 16, against the oracle as above.  check_width asserts that no strip launch was counted."""
    script = str(tmp_path / "one_wave.py")
    with open(script, "w") as fh:
        fh.write(_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), shapes=[s[:3] for s in _ONE_WAVE], n_cus=_cus()))
    r = subprocess.run([sys.executable, script], env=dict(os.environ, MORNA_TM_STRIP="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    done = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("WIDTH_OK")]
    assert done == [[str(f), form[0], str(form[1])] for f, N, T, form in _ONE_WAVE], r.stdout


_HANDOVER = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, {root!r})
from morna_amd.annoy import AnnoyIndex
N, D, T = 9000, 1000, 150
rng = np.random.default_rng(2027 + D)
nc = 5
C = rng.standard_normal((nc, D)).astype(np.float32)
lab = rng.integers(0, nc, N)
X = C[lab] + np.float32(0.25) * rng.standard_normal((N, D), dtype=np.float32)
X *= (10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
a = AnnoyIndex(D)
a.timer_enable(only=["tm_strip", "tm_wave"])
a.add_items(X)
a.build(T)
f = a.get_forest()
h = hashlib.sha256()
for k in ("perm", "node_rec", "hyperplanes", "hp_node"):
    h.update(np.ascontiguousarray(f[k]).tobytes())
items = (np.arange(64, dtype=np.int32) * 131) % N
g = hashlib.sha256()
for n, sk in ((10, -1), (20, 100), (5, 1)):
    ids, d, cnt = a.get_nns_by_item_batch(items, n, sk)
    g.update(ids.tobytes()); g.update(d.tobytes()); g.update(cnt.tobytes())
t = a.timers()
st = a.forest_stats()
print("DIGEST", h.hexdigest(), g.hexdigest(), st["n_split"], st["max_depth"], t["tm_strip"]["launches"], t["tm_wave"]["launches"])
"""


def test_strip_to_wave_handover_inside_one_build(tmp_path):
    """1000 floats, 150 trees: 150 and 300 nodes at the two shallowest levels (strips), 600 and more below (one wave per
    node) -- the shape test_gpu_level_chain.py measures.  The oracle would take 19 s here; the one-wave form alone is
    pinned to it above, so the same forest and the same 64 answers from a MORNA_TM_STRIP=0 process pin the hand-over."""
    script = str(tmp_path / "handover.py")
    with open(script, "w") as fh:
        fh.write(_HANDOVER.format(root=ROOT))
    out = {}
    for name, extra in (("default", {}), ("one_wave", {"MORNA_TM_STRIP": "0"})):
        r = subprocess.run([sys.executable, script], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stderr[-3000:])
        out[name] = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()[1:]
    assert out["default"][:4] == out["one_wave"][:4], out
    assert int(out["default"][3]) >= 3, out                              # levels below the strips exist
    assert int(out["default"][4]) > 0 and int(out["default"][5]) > 0, out   # both forms ran in the default build
    assert int(out["one_wave"][4]) == 0 and int(out["one_wave"][5]) > 0, out
