"""The 256 x 256 form of the whole-batch filter contraction (query_scores_big_kernel, knn.hip) on rows built to defeat it.  -m gpu

From 512 queries up a dense batch's filter scores come from two launches: 256 x 256 tiles (one accumulation chain of dpad
products) for as many 256-row tiles as fill the chip in whole rounds, 128 x 128 tiles for the rows behind them, and
query_refine_kernel<2> picks the accumulation bound per candidate by its id.  A candidate whose lower bound lies above the
k-th upper bound gets no canonical dot: the one place where the approximate search can lose a true neighbour silently.

One process per case (MORNA_DEBUG_OPEN=1 is read once): it builds one index and asks every batch four ways --
  big       all queries at once: the form under test;
  spread    the same handle in slices of 32 queries: canonical dots for every candidate, no contraction, no filter;
  dense128  the same handle in slices of 256 queries: dense, the 128 x 128 form alone;
  oracle    the CPU oracle (mode 1) for every anchor query and 8 others --
and prints what it compared as one CALL line per batch; the library's witness lines ("[morna] query contraction:",
"[morna] query refine:") say which form took which rows and how many candidates survived the filter.  Asserted here:
ids, fp32 distances and counts equal byte for byte among big, spread, dense128 and the oracle; every distance reported for
an anchor within 2e-5 of the fp64 angular distance of the returned id (the tolerance of test_gpu_configs.py); and what
keeps the comparison from going vacuous: the expected large tiles (> 0) and rows behind them (the rule of
launch_contraction restated from the CU count), 0 large tiles in the dense128 slices, no contraction in the spread ones,
k * nq <= survivors < candidates, every anchor's k results rows of its own ladder, a tie group across the cut
(d[k-1] == d[k] when an anchor is asked for 2k), and ladder rows on both sides of big_rows among one anchor's results.

Rows: clustered (as _clustered of test_gpu_parity.py) with norms over 10^+-3; at random ids
  * 12 ladders: an anchor row a and 256 rows at angular distance (2 - 2 cos) d0 (1 + 1e-6 j), d0 = 0.01, j = 0 .. 255:
    c a / |a| + sqrt(1 - c^2) u_j with c = 1 - d_j / 2, u_j a random unit vector orthogonal to a, times 10^-2 .. 10^2.
    Half of the anchors are Gaussian, half have all elements in [0.5, 1] (every product of a chain has one sign).  A third
    of the ladders have u_j on columns [0, 64) only, a third on [dim - 64, dim) only: a lost or repeated first or last
    K-step moves them across the threshold.  The steps of a ladder (1e-8) lie below the rounding of the canonical fp32 dot
    (1e-7 of the distance), so the top 20 is decided by that rounding, and the fp16 images alone rank the rows wrongly: a
    filter with no slack fails here.  (The last step of the canonical distance is taken in fp64, so near rows seldom tie
    exactly; the exact ties, ranked by id, come from 80 copies of ladder 0's nearest row scaled by powers of two.)
    Rows j = 0, 2, 4, .. of every ladder lie at ids >= big_rows (B), as many as fit behind it, rows j = 1 below it; ladder
    rows are forced onto ids 0, 255, 256, B - 1, B, B + 1, B + 127, B + 128, N - 1 (those that exist).
    (Case f holds 1074 rows: its ladders have 48 rows, 12 x 256 do not fit.)
  * the families of test_gpu_filters.py that bear on the query filter: spikes, the fp16 scaling edges, near-mirror pairs,
    exact and scaled duplicates, a zero row, rows of norm 1e-18 and 1e15 (no fp16 image: never filtered).  All finite.
Queries: the anchors at positions 0, 255, 256, 511, nq - 1 and elsewhere, the rest any other rows (ids repeat), by vector
perturbed by 1e-3 (the anchors and the 8 others of the oracle as they are stored).
"""
import json
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import json, math, sys
import numpy as np
sys.path.insert(0, @ROOT@)
from morna_amd.annoy import AnnoyIndex
from oracle import capi
D, N, T, NQ, B, L, A = @D@, @N@, @T@, @NQ@, @B@, @L@, 12
MODES, CALLS = @MODES@, @CALLS@
D0 = 0.01
rng = np.random.default_rng(77000 + D + N)

def mark(call, phase):   # between the library's own lines on stderr
    sys.stderr.write("MARK %s %s\n" % (call, phase))
    sys.stderr.flush()

# ---- rows: clustered, norms over 10^+-3 (in chunks: no fp64 temporary of the whole matrix)
centers = rng.standard_normal((12, D)).astype(np.float32)
lab = rng.integers(0, 12, N)
X = np.empty((N, D), np.float32)
for c0 in range(0, N, 1024):
    c1 = min(N, c0 + 1024)
    X[c0:c1] = centers[lab[c0:c1]] + np.float32(0.3) * rng.standard_normal((c1 - c0, D), dtype=np.float32)
X *= (10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)

# ---- ids: the forced ones first in their pool, the rest of each pool in random order
forced = sorted(set(i for i in (0, 255, 256, B - 1, B, B + 1, B + 127, B + 128, N - 1) if 0 <= i < N))
lo_forced, hi_forced = [i for i in forced if i < B], [i for i in forced if i >= B]
lo_pool = lo_forced + [int(i) for i in rng.permutation(B) if int(i) not in lo_forced]
hi_pool = hi_forced + [int(i) for i in rng.permutation(np.arange(B, N)) if int(i) not in hi_forced]
behind = N - B
n_hi = min(L // 2, max(0, behind - 5) // A)   # rows j = 0, 2, .. 2 (n_hi - 1) of every ladder lie behind B
assert n_hi * A >= len(hi_forced), (n_hi, hi_forced)
ladder_id = np.empty((A, L), np.int64)
placed = np.zeros((A, L), bool)
for jj in range(n_hi):
    for a in range(A):
        ladder_id[a, 2 * jj] = hi_pool.pop(0)
        placed[a, 2 * jj] = True
for a in range(A):                            # j = 1 of every ladder below B: ladders 0 .. 3 take 0, 255, 256, B - 1
    ladder_id[a, 1] = lo_pool.pop(0)
    placed[a, 1] = True
rest = [int(i) for i in rng.permutation(np.array(lo_pool + hi_pool, np.int64))]
for a in range(A):
    for j in range(L):
        if not placed[a, j]:
            ladder_id[a, j] = rest.pop()
anchor_id = np.array([rest.pop() for _ in range(A)], np.int64)

# ---- ladders
ladder_set = []
for a in range(A):
    av = rng.standard_normal(D) if a % 2 == 0 else rng.uniform(0.5, 1.0, D)
    an = av / np.linalg.norm(av)
    sup = (slice(0, D), slice(0, 64), slice(D - 64, D))[(a // 2) % 3]   # full, first columns, last columns: 4 ladders each
    a_s = an[sup]
    R = rng.standard_normal((L, a_s.shape[0]))
    R -= np.outer(R @ a_s, a_s) / (a_s @ a_s)                           # orthogonal to a, inside the support
    R /= np.linalg.norm(R, axis=1, keepdims=True)
    dj = D0 * (1.0 + 1e-6 * np.arange(L))
    c = 1.0 - dj / 2.0
    rows = np.outer(c, an)
    rows[:, sup] += np.sqrt(1.0 - c * c)[:, None] * R
    rows *= 10.0 ** rng.uniform(-2, 2, (L, 1))
    X[ladder_id[a]] = rows.astype(np.float32)
    X[anchor_id[a]] = (an * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
    ladder_set.append(set(ladder_id[a].tolist()) | {int(anchor_id[a])})
for ids in forced:
    assert any(ids in s for s in ladder_set), ("a forced id holds no ladder row", ids)

# ---- the families of test_gpu_filters.py that bear on the query filter, at random ids
def take(n):
    return np.array([rest.pop() for _ in range(n)], np.int64)

others = take(8)                  # ordinary rows, left as they are: the oracle's 8 other queries
for i in take(16):                # spikes
    X[i] = (1e-9 * rng.standard_normal(D)).astype(np.float32)
    X[i, rng.integers(0, D)] = np.float32(rng.choice([-1.0, 1.0]))
    X[i] *= np.float32(10.0 ** rng.uniform(-3, 3))
for n, i in enumerate(take(16)):  # fp16 scaling edges: largest element a power of two, and one ulp below one
    X[i] = np.clip(X[i], -1, 1) * np.float32(0.4)
    X[i, rng.integers(0, D)] = np.float32(1.0) if n % 2 else np.nextafter(np.float32(2.0), np.float32(0.0))
    X[i] *= np.float32(2.0 ** rng.integers(-30, 30))
mir = take(16)                    # near-mirror pairs
for i, j in zip(mir[0::2], mir[1::2]):
    X[j] = -X[i] * (1.0 + 1e-6 * rng.standard_normal(D)).astype(np.float32)
dup = take(10)                    # exact and scaled duplicates of a query row and of a ladder row
X[dup[0]] = X[others[0]]
X[dup[1:5]] = X[others[0]] * np.float32(4.0)
X[dup[5]] = X[ladder_id[0, 3]]
X[dup[6:10]] = X[ladder_id[0, 3]] * np.float32(0.25)
ladder_set[0] |= set(dup[5:10].tolist())
# a tie group wide enough to cross the cut at k = 20 and at k = 50: the nearest row of ladder 0 (it lies at id B, or at B - 1
# when nothing lies behind B) times powers of two -- the same canonical distance bit for bit, ranked by id alone
tie = take(80)
X[tie] = X[ladder_id[0, 0]][None, :] * (2.0 ** rng.integers(-3, 4, (80, 1))).astype(np.float32)
ladder_set[0] |= set(tie.tolist())
zero, tiny, huge = take(3)
X[zero] = 0.0
for i, s in ((tiny, 1e-18), (huge, 1e15)):
    v = X[i].astype(np.float64)
    X[i] = (v / np.linalg.norm(v) * s).astype(np.float32)
assert np.isfinite(X).all()

# ---- queries
pos = [p for p in (0, 255, 256, 511, NQ - 1)]
free = [int(p) for p in rng.permutation(NQ) if int(p) not in pos]
anchor_pos = np.array(pos + free[:A - len(pos)], np.int64)
other_pos = np.array(free[A:A + 8], np.int64)
not_anchor = np.setdiff1d(np.arange(N), anchor_id)
items = rng.choice(not_anchor, NQ).astype(np.int32)      # ids repeat
items[anchor_pos] = anchor_id
items[other_pos] = others
checked = np.concatenate([anchor_pos, other_pos])
Q = None
if "vector" in MODES:
    Q = X[items]
    for c0 in range(0, NQ, 512):
        Q[c0:c0 + 512] = (Q[c0:c0 + 512].astype(np.float64) * (1 + 1e-3 * rng.standard_normal((len(Q[c0:c0 + 512]), D)))).astype(np.float32)
    Q[checked] = X[items[checked]]

a = AnnoyIndex(D)
a.add_items(X)
a.build(T)
o = capi.AnnoyOracle(D, mode=1)
o.set_items(X)
o.build(T)

def unit64(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)

def ask(mode, sel, k, sk):
    return a.get_nns_by_item_batch(items[sel], k, sk) if mode == "item" else a.get_nns_by_vector_batch(Q[sel], k, sk)

def sliced(mode, step, k, sk):
    parts = [ask(mode, slice(q0, min(NQ, q0 + step)), k, sk) for q0 in range(0, NQ, step)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))

def differing(x, y):   # queries whose ids, distance bits or counts differ
    return np.nonzero((x[0] != y[0]).any(1) | (x[1].view(np.uint32) != y[1].view(np.uint32)).any(1) | (x[2] != y[2]))[0]

def describe(big, ref, bad):   # the first differing queries: position, query tile, row asked, ids lost and gained and their side of B
    out = []
    for q in bad[:4]:
        lost = sorted(set(ref[0][q].tolist()) - set(big[0][q].tolist()))
        gained = sorted(set(big[0][q].tolist()) - set(ref[0][q].tolist()))
        out.append(dict(q=int(q), tile=int(q) // 256, item=int(items[q]), lost=lost, gained=gained,
                        lost_behind_B=[int(i >= B) for i in lost], gained_behind_B=[int(i >= B) for i in gained]))
    return out

for mode in MODES:
    for k, sk in CALLS:
        call = "%s_k%d_sk%d" % (mode, k, sk)
        mark(call, "big")
        big = ask(mode, slice(0, NQ), k, sk)
        mark(call, "spread")
        spread = sliced(mode, 32, k, sk)
        mark(call, "dense128")
        dense128 = sliced(mode, 256, k, sk)
        mark(call, "done")
        rep = dict(call=call, mode=mode, k=k, search_k=sk, nq=NQ)
        bad = differing(big, spread)
        rep["spread_differ"], rep["spread_first"] = int(len(bad)), describe(big, spread, bad)
        bad = differing(big, dense128)
        rep["dense128_differ"], rep["dense128_first"] = int(len(bad)), describe(big, dense128, bad)
        # the CPU oracle: ids, distance bits, counts
        oracle_bad = []
        ref_ans = {}
        for q in checked:
            if mode == "item":
                rid, rd = o.get_nns_by_item(int(items[q]), k, sk, include_distances=True)
            else:
                rid, rd = o.get_nns_by_vector(Q[q], k, sk, include_distances=True)
            ref_ans[int(q)] = rid
            m = int(big[2][q])
            if not (m == len(rid) and big[0][q, :m].tolist() == rid and
                    big[1][q, :m].tobytes() == np.array(rd, np.float32).tobytes()):
                lost = sorted(set(rid) - set(big[0][q].tolist()))
                oracle_bad.append(dict(q=int(q), tile=int(q) // 256, item=int(items[q]), lost=lost,
                                       lost_behind_B=[int(i >= B) for i in lost]))
        rep["oracle_checked"], rep["oracle_differ"] = int(len(checked)), oracle_bad
        # the anchors: fp64 distances of the returned ids, their own ladders, both sides of B, a tie group across the cut
        dev, own, both, ties = 0.0, 0, 0, 0
        for n, q in enumerate(anchor_pos):
            qv = unit64(X[anchor_id[n]])
            m = int(big[2][q])
            for r in range(m):
                i = int(big[0][q, r])
                true = math.sqrt(max(0.0, 2.0 - 2.0 * float(unit64(X[i]) @ qv)))
                dev = max(dev, abs(float(big[1][q, r]) - true))
            rid = ref_ans[int(q)]
            own += int(len(rid) == k and all(i in ladder_set[n] for i in rid))
            both += int(any(i < B for i in rid) and any(i >= B for i in rid))
        for n, q in enumerate(anchor_pos):
            if mode == "item":
                _, rd = o.get_nns_by_item(int(items[q]), 2 * k, sk, include_distances=True)
            else:
                _, rd = o.get_nns_by_vector(Q[q], 2 * k, sk, include_distances=True)
            if len(rd) > k and np.float32(rd[k - 1]) == np.float32(rd[k]):
                ties += 1
                break
        rep.update(anchors=int(A), anchor_fp64_dev=dev, anchors_own_ladder=own, anchors_both_sides=both, tie_across_cut=ties)
        print("CALL", json.dumps(rep), flush=True)
print("DONE", flush=True)
"""

_SWITCHES = ("MORNA_QUERY_BIG", "MORNA_QUERY_DENSE", "MORNA_QUERY_FILTER", "MORNA_QUERY_SPREAD", "MORNA_QUERY_SPLIT_TRAVERSE",
             "MORNA_BUILD_TAIL", "MORNA_SPLIT_MM")
_MARK = re.compile(r"^MARK (\S+) (\S+)$")
_CONTRACTION = re.compile(r"^\[morna\] query contraction: site=(\S+) queries=(\d+) rows=(\d+) big_tiles=(\d+) rem_rows=(\d+) "
                          r"query_tiles=(\d+) (by_item|by_vector)$")
_REFINE = re.compile(r"^\[morna\] query refine: queries=(\d+) candidates=(\d+) survivors=(\d+)$")


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _big_tiles(n_cus, N, nq):
    """The rule of launch_contraction (knn.hip): whole rounds of the chip, one 256 x 256 workgroup per CU; from 512 queries up."""
    if nq < 512:
        return 0
    per_round = n_cus // math.gcd(n_cus, (nq + 255) // 256)
    return (N // 256) // per_round * per_round


# name, D, N, T, nq, by, ((k, search_k), ..), ladder rows, large tiles at 256 CUs, ladder rows expected on both sides of big_rows
_CASES = [
    ("a", 256, 16384 + 77, 4, 1024, ("item", "vector"), ((20, 100), (50, 4000)), 256, 64, True),   # 77 rows behind; k > KTH_MAX_K
    ("b", 256, 16384, 4, 1000, ("vector",), ((20, 100),), 256, 64, False),       # big_rows == N; a ragged last query tile
    ("c", 3000, 8192 + 300, 2, 2048, ("item", "vector"), ((20, 100),), 256, 32, True),   # the bench's width; the forest splits
    ("d", 12000, 4096 + 130, 2, 4096, ("vector",), ((20, -1),), 256, 16, False),  # dpad 12032; one leaf: 4226 > 4096 candidates
    ("e", 32768, 4096 + 130, 2, 4096, ("item",), ((20, -1),), 256, 16, True),     # the widest row: one chain of 32768 products
    ("f", 256, 1024 + 50, 2, 16384, ("item",), ((20, 100),), 48, 4, True),        # 4 large tiles: half an XCD group returns early
]


@pytest.mark.parametrize("name,D,N,T,nq,modes,calls,ladder,tiles_256cu,both_sides", _CASES, ids=[c[0] for c in _CASES])
def test_large_form_on_adversarial_rows(tmp_path, name, D, N, T, nq, modes, calls, ladder, tiles_256cu, both_sides):
    n_cus = _cus()
    tiles = _big_tiles(n_cus, N, nq)
    if n_cus == 256:
        assert tiles == tiles_256cu, (tiles, tiles_256cu)
    assert tiles > 0, "no large tiles at %d CUs: the case does not reach the form under test" % n_cus
    B = tiles * 256
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = _SCRIPT
    for key, value in dict(ROOT=root, D=D, N=N, T=T, NQ=nq, B=B, L=ladder, MODES=tuple(modes), CALLS=tuple(calls)).items():
        text = text.replace("@%s@" % key, repr(value))
    script = str(tmp_path / "case.py")
    with open(script, "w") as fh:
        fh.write(text)
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env["MORNA_DEBUG_OPEN"] = "1"
    r = subprocess.run([sys.executable, script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stderr[-3000:]

    # the library's witness lines, by call and phase
    seen, where = {}, None
    for ln in r.stderr.splitlines():
        m = _MARK.match(ln)
        if m:
            where = (m.group(1), m.group(2))
            continue
        m = _CONTRACTION.match(ln)
        if m:
            seen.setdefault(where, {"contraction": [], "refine": []})["contraction"].append(
                dict(site=m.group(1), queries=int(m.group(2)), rows=int(m.group(3)), big_tiles=int(m.group(4)),
                     rem_rows=int(m.group(5)), query_tiles=int(m.group(6)), by=m.group(7)))
            continue
        m = _REFINE.match(ln)
        if m:
            seen.setdefault(where, {"contraction": [], "refine": []})["refine"].append(
                dict(queries=int(m.group(1)), candidates=int(m.group(2)), survivors=int(m.group(3))))
    reports = [json.loads(ln[5:]) for ln in r.stdout.splitlines() if ln.startswith("CALL ")]
    assert len(reports) == len(modes) * len(calls), r.stdout[-2000:]

    none = {"contraction": [], "refine": []}
    for rep in reports:
        call, k = rep["call"], rep["k"]
        big, spread, dense128 = (seen.get((call, ph), none) for ph in ("big", "spread", "dense128"))
        print(name, call, "big:", big, "dense128:", dense128["contraction"][:1], len(dense128["contraction"]),
              {key: rep[key] for key in ("spread_differ", "dense128_differ", "oracle_checked", "anchor_fp64_dev",
                                         "anchors_own_ladder", "anchors_both_sides", "tie_across_cut")})
        # the form under test ran: one batch, one contraction, the expected tiles and rows behind them
        assert len(big["contraction"]) == 1 and len(big["refine"]) == 1, big
        line = big["contraction"][0]
        assert line["queries"] == nq and line["rows"] == N and line["by"] == "by_" + rep["mode"], line
        assert line["big_tiles"] == tiles and line["rem_rows"] == N - B and line["query_tiles"] == (nq + 255) // 256, (line, tiles, B)
        assert (line["rem_rows"] == 0) == (name == "b"), line
        ref = big["refine"][0]
        assert ref["queries"] == nq and k * nq <= ref["survivors"] < ref["candidates"], ref
        # the references ran as what they are: no contraction at all; the 128 x 128 form alone, one per slice
        assert not spread["contraction"] and not spread["refine"], spread
        assert len(dense128["contraction"]) == (nq + 255) // 256 == len(dense128["refine"]), dense128
        assert all(c["big_tiles"] == 0 and c["rem_rows"] == N for c in dense128["contraction"]), dense128
        # the rows did what they were built for
        assert rep["anchors_own_ladder"] == rep["anchors"], rep
        assert rep["tie_across_cut"] >= 1, rep
        if both_sides:
            assert rep["anchors_both_sides"] >= 1, rep
        # the answers
        assert rep["oracle_checked"] == rep["anchors"] + 8 and not rep["oracle_differ"], rep["oracle_differ"]
        assert rep["spread_differ"] == 0, rep["spread_first"]
        assert rep["dense128_differ"] == 0, rep["dense128_first"]
        assert rep["anchor_fp64_dev"] <= 2e-5, rep["anchor_fp64_dev"]
