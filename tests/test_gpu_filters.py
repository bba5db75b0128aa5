"""The fp16 matrix-core filters at the row widths that ship (D = 3000: the bench; D = 8192: configs[4]) and past them
(12000, not a multiple of 256; 32768, the widest row) on rows built to defeat them.  -m gpu

The split of a level (splitmm.hip) and the candidate filter of the approximate search decide from fp16 copies only
what they can PROVE and hand everything else to the canonical fp32 arithmetic, so switching them off must change
nothing: whole-forest and search digests are compared across MORNA_SPLIT_MM = 0 / 1, MORNA_QUERY_FILTER = 0 / 1 and
MORNA_QUERY_DENSE = 0 / 1 (the filter dots of a whole batch as one contraction, or candidate by candidate),
MORNA_SPLIT_BIG = 0 / 1 and MORNA_QUERY_BIG = 0 / 1 (the contractions' tile shapes, each with its own accumulation
bound: the query filter's 256 x 256 form takes rows from 512 queries up only, so the digest holds a by-item batch of the
4096 items 356 .. 4451 -- every family below -- and, where N >= 16384, a by-vector batch of 1024 perturbed rows; the
library's "[morna] query contraction:" lines (MORNA_DEBUG_OPEN=1) must show large tiles in the default process, by the
rule of launch_contraction, and none with MORNA_QUERY_BIG=0; tests/test_gpu_query_big.py compares that form with the
CPU oracle), and across
MORNA_QUERY_SPLIT_TRAVERSE = 0 / 1 and MORNA_QUERY_SPREAD = 0 / 1 (how a batch's, and a small batch's, traversal is dealt out),
MORNA_SPLIT_ORDER = 0 / 1 and MORNA_SPLIT_LISTS = 0 / 1 (the order of the rows of the split contraction, and the per-tile
task lists: both only choose which products are computed; the 256-wide case with 150 trees has levels with enough split
nodes for the lists) -- separate processes: the switches are read once.  The rows:

  * midpoints  s (a / |a| + b / |b|) of rows a, b from two different clusters: against the hyperplane that separates
    those clusters (the normalised difference of their centroids) the dot product cancels to ~1e-7 of |row| |h|, so
    the side is decided by the rounding of the canonical fp32 dot;
  * near-mirror pairs  x, -x (1 + 1e-6 noise);
  * spikes: one element 1e9 times larger than the rest -- the fp16 copy keeps the spike alone, the sign of the dot
    is in what it dropped whenever the hyperplane is small at the spike;
  * rows at the edges of the fp16 scaling: largest element exactly a power of two, and one ulp below one;
  * norms from 1e-18 to 1e18, a zero row, exact duplicates, exact scaled duplicates, near-duplicates in the 5th digit.
"""
import os
import subprocess
import sys

import pytest

from test_gpu_query_big import _CONTRACTION, _big_tiles, _cus

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, {root!r})
from morna_amd.annoy import AnnoyIndex
N, D, T = {N}, {D}, {T}
rng = np.random.default_rng(2026 + D)
nc = 5
C = rng.standard_normal((nc, D)).astype(np.float32)
lab = rng.integers(0, nc, N)
X = np.empty((N, D), np.float32)   # made in chunks of rows: at 34000 x 32768 one fp64 temporary would be 9 GB
for c0 in range(0, N, 2048):
    c1 = min(N, c0 + 2048)
    X[c0:c1] = C[lab[c0:c1]] + np.float32(0.25) * rng.standard_normal((c1 - c0, D), dtype=np.float32)
X *= (10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
# midpoints of rows from different clusters (a, b among the first m0 rows)
m0 = 2000
unit = X[:m0] / np.linalg.norm(X[:m0].astype(np.float64), axis=1, keepdims=True).astype(np.float32)
for i in range(m0, m0 + 1500):
    a, b = rng.integers(0, m0, 2)
    while lab[a] == lab[b]:
        b = rng.integers(0, m0)
    X[i] = (unit[a] + unit[b]) * np.float32(10.0 ** rng.uniform(-2, 2))
# exact midpoints of the cluster centres themselves, at many scales
for i in range(3500, 3600):
    a, b = rng.choice(nc, 2, replace=False)
    ca, cb = C[a] / np.linalg.norm(C[a]), C[b] / np.linalg.norm(C[b])
    X[i] = (ca + cb) * np.float32(2.0 ** rng.integers(-20, 20))
# near-mirror pairs
for i in range(3600, 4000, 2):
    X[i + 1] = -X[i] * (1.0 + 1e-6 * rng.standard_normal(D)).astype(np.float32)
# spikes
for i in range(4000, 4200):
    X[i] = (1e-9 * rng.standard_normal(D)).astype(np.float32)
    X[i, rng.integers(0, D)] = np.float32(rng.choice([-1.0, 1.0]))
    X[i] *= np.float32(10.0 ** rng.uniform(-3, 3))
# fp16 scaling edges
for i in range(4200, 4300):
    j = rng.integers(0, D)
    X[i] = np.clip(X[i], -1, 1) * np.float32(0.4)
    X[i, j] = np.float32(1.0) if i % 2 else np.nextafter(np.float32(2.0), np.float32(0.0))
    X[i] *= np.float32(2.0 ** rng.integers(-30, 30))
X[4300] = 0.0
X[4301] = X[4302]
X[4303:4400] = X[50] * (1.0 + 1e-5 * rng.standard_normal((97, D))).astype(np.float32)
X[4400:4450] = X[50] * np.float32(4.0)
X[4450] *= np.float32(1e-18)
X[4451] *= np.float32(1e15)
a = AnnoyIndex(D)
a.add_items(X)
a.build(T)
f = a.get_forest()
h = hashlib.sha256()
for k in ("perm", "node_rec", "hyperplanes", "hp_node"):
    h.update(np.ascontiguousarray(f[k]).tobytes())
items = np.concatenate([np.arange(40), np.arange(2000, 2040), np.arange(3500, 3520), np.arange(3600, 3640),
                        np.arange(4000, 4020), np.arange(4200, 4220), np.arange(4300, 4320), np.arange(4400, 4410),
                        [4450, 4451]]).astype(np.int32)
for n, sk in ((20, 100), (10, -1), (50, 4000)):
    ids, d, cnt = a.get_nns_by_item_batch(items, n, sk)
    h.update(ids.tobytes()); h.update(d.tobytes()); h.update(cnt.tobytes())
Q = (X[items[:32]].astype(np.float64) * (1 + 1e-3 * rng.standard_normal((32, D)))).astype(np.float32)
ids, d, cnt = a.get_nns_by_vector_batch(Q, 20, 100)
h.update(ids.tobytes()); h.update(d.tobytes()); h.update(cnt.tobytes())
# batches wide enough for the 256 x 256 form of the whole-batch contraction (512 queries): every adversarial family by item ...
ids, d, cnt = a.get_nns_by_item_batch(np.arange(356, 4452).astype(np.int32), 20, 100)
h.update(ids.tobytes()); h.update(d.tobytes()); h.update(cnt.tobytes())
if N >= 16384:   # ... and 1024 perturbed rows by vector: the midpoints' tail and everything behind them
    Q = (X[3428:4452].astype(np.float64) * (1 + 1e-3 * rng.standard_normal((1024, D)))).astype(np.float32)
    ids, d, cnt = a.get_nns_by_vector_batch(Q, 20, 100)
    h.update(ids.tobytes()); h.update(d.tobytes()); h.update(cnt.tobytes())
st = a.forest_stats()
print("DIGEST", h.hexdigest(), st["n_split"], st["max_depth"])
"""


# one process per switch (they are read once per process); the default one also prints the open-pair share per level and
# which form of the query contraction took which rows, the no_query_big one the latter
_RUNS = (("default", {"MORNA_DEBUG_OPEN": "1"}), ("no_mm", {"MORNA_SPLIT_MM": "0"}),
         ("no_qf", {"MORNA_QUERY_FILTER": "0"}), ("no_dense", {"MORNA_QUERY_DENSE": "0"}),
         ("no_order", {"MORNA_SPLIT_ORDER": "0"}), ("no_lists", {"MORNA_SPLIT_LISTS": "0", "MORNA_SPLIT_ORDER": "0"}),
         # round 3: the traversal of a batch as root margins by query groups + one-wave descents, or fused (one
         # workgroup per query); small batches dealt out over the chip, or one workgroup per query
         ("fused_traverse", {"MORNA_QUERY_SPLIT_TRAVERSE": "0"}), ("no_spread", {"MORNA_QUERY_SPREAD": "0"}),
         # one accumulation bound or the other: 128 x 128 contraction tiles only (split, query filter)
         ("no_split_big", {"MORNA_SPLIT_BIG": "0"}), ("no_query_big", {"MORNA_QUERY_BIG": "0", "MORNA_DEBUG_OPEN": "1"}))


def _digest(script, extra):
    """(digest fields, split_mm open-pair lines, query contraction lines as dicts) of one process."""
    r = subprocess.run([sys.executable, script], env=dict(os.environ, **extra), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()[1:]
    contractions = [_CONTRACTION.match(ln) for ln in r.stderr.splitlines() if ln.startswith("[morna] query contraction:")]
    assert all(contractions), r.stderr[-2000:]
    contractions = [dict(queries=int(m.group(2)), rows=int(m.group(3)), big_tiles=int(m.group(4)), rem_rows=int(m.group(5)),
                         by=m.group(7)) for m in contractions]
    return out, [ln for ln in r.stderr.splitlines() if ln.startswith("[morna] split_mm level")], contractions


def _check_query_forms(N, default, no_big):
    """The large form of the query contraction took rows in the default process (by item; by vector too where the digest has
    that batch), as many as launch_contraction's rule says, and none with MORNA_QUERY_BIG=0.  Either list may be None."""
    if default is not None:
        n_cus = _cus()
        print(default)
        for c in default:
            assert c["rows"] == N and c["big_tiles"] == _big_tiles(n_cus, N, c["queries"]) and c["rem_rows"] == N - 256 * c["big_tiles"], c
        assert any(c["big_tiles"] > 0 and c["by"] == "by_item" for c in default), default
        if N >= 16384:
            assert any(c["big_tiles"] > 0 and c["by"] == "by_vector" for c in default), default
    if no_big is not None:
        assert no_big and all(c["big_tiles"] == 0 and c["rem_rows"] == N for c in no_big), no_big
        assert any(c["queries"] >= 512 for c in no_big), no_big   # batches the large form would have taken


def _check_default(out, open_lines):
    assert int(out[2]) >= 2                                  # at least two levels went through the contraction
    assert open_lines, "the matrix-core split did not run"
    print("\n".join(open_lines))                             # pytest -s: the open-pair share per level
    # the filter must have left pairs open (the rows above) and still decided most
    shares = [float(ln.split("(")[-1].split("%")[0]) for ln in open_lines]
    assert max(shares) > 0.0 and min(shares) < 50.0, open_lines


def _write_script(path, D, N, T):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(path, "w") as fh:
        fh.write(_SCRIPT.format(root=root, N=N, D=D, T=T))
    return path


@pytest.mark.parametrize("D,N,T", [(3000, 16000, 6), (8192, 34000, 3), (256, 40000, 150), (12000, 34000, 3)])
def test_adversarial_rows_filters_change_nothing(tmp_path, D, N, T):
    script = _write_script(str(tmp_path / "digest.py"), D, N, T)
    out, forms = {}, {}
    for name, extra in _RUNS:
        out[name], lines, forms[name] = _digest(script, extra)
        if name == "default":
            open_lines = lines
    assert out["default"] == out["no_mm"] == out["no_qf"] == out["no_dense"] == out["no_order"] == out["no_lists"], out
    assert out["default"] == out["fused_traverse"] == out["no_spread"], out
    assert out["default"] == out["no_split_big"] == out["no_query_big"], out
    _check_default(out["default"], open_lines)
    _check_query_forms(N, forms["default"], forms["no_query_big"])


# The widest row: 70000 rows of 32768 floats, past twice annoy's leaf of D + 2 rows, so the forest splits below its root
# (9 GB of rows per process: one test per switch, each against the default process's digest, made once)
_WIDEST = (32768, 70000, 2)


@pytest.fixture(scope="module")
def widest(tmp_path_factory):
    script = _write_script(str(tmp_path_factory.mktemp("widest") / "digest.py"), *_WIDEST)
    out, open_lines, forms = _digest(script, dict(_RUNS)["default"])
    return script, out, open_lines, forms


def test_widest_row_adversarial_rows_default(widest):
    _check_default(widest[1], widest[2])
    _check_query_forms(_WIDEST[1], widest[3], None)


@pytest.mark.parametrize("name", [n for n, _ in _RUNS if n != "default"])
def test_widest_row_filters_change_nothing(widest, name):
    script, default = widest[:2]
    out, _, forms = _digest(script, dict(_RUNS)[name])
    assert out == default, name
    if name == "no_query_big":
        _check_query_forms(_WIDEST[1], None, forms)
