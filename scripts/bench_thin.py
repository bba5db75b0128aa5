#!/usr/bin/env python3
"""Depth thinning over the junction store (morna_jstore_thin) at the data set of scripts/bench_junctions.py
(synth.synthetic_intropolis, 50k samples, 70k junctions, ~1e8 entries).  Reports, as one JSON line and as the text kept in
profiles/thin.txt, for 1, 64 and 1000 jobs at keep 0.1 (consecutive sample ids), and for one heavy job -- a row of the store
with three of its coverages set near 2^24, in a store of its own:

  kernel ms    HIP-event time of both passes and the scan: the best of three calls after a warm-up, and the spread
  bytes        read (16 per entry of every named row) and written (4 per entry, 8 per surviving line), and the rate they make
  draws        the summed coverage of the named rows: hashes made, and the rate
  whole call   wall clock of JunctionStore.thin, the copies back and the numpy views included
  numpy        the same contract restated with numpy on the host image of the rows (handed over ready made), on as many of
               the first jobs as make at most --numpy-draws draws; its draws per second, and whether the answers are equal

    python3 scripts/bench_thin.py [--samples 50000] [--junctions 70000] [--json out.json] [--text out.txt]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morna_amd._lib import check, lib, ptr  # noqa: E402
from morna_amd.index import ParsedLines  # noqa: E402
from morna_amd.junctions import JunctionStore  # noqa: E402
from morna_amd.synth import synthetic_intropolis  # noqa: E402

SEED, KEEP = 8675309, int(round(0.1 * 4294967296.0))
M32 = np.uint64(0xffffffff)


def fmix32(h):
    h = np.array(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & M32
    h ^= h >> np.uint64(16)
    return h


def numpy_thin(ext, line, cov, keep, seed, block=1 << 24):
    """(lines, thinned coverages) of one job by the contract of include/morna_hip.h, the draws made in blocks."""
    e = int(ext) & (2**64 - 1)
    s = int(fmix32(seed & 0xffffffff))
    u = int(fmix32((e & 0xffffffff) ^ int(fmix32((e >> 32) ^ s))))
    v = fmix32(np.uint64(u) ^ (np.asarray(line, np.int64).astype(np.uint64) & M32))
    cov = np.asarray(cov, np.int64)
    kept = np.zeros(len(cov), np.int64)
    ends = np.cumsum(cov)
    lo = 0
    while lo < len(cov):                                       # whole entries, about `block` draws at a time
        hi = max(lo + 1, int(np.searchsorted(ends, (ends[lo] - cov[lo]) + block, side="right")))
        c = cov[lo:hi]
        if len(c) == 1 and c[0] > block:                       # one entry deeper than a block: its draws in slices
            for first in range(0, int(c[0]), block):
                i = np.arange(first, min(first + block, int(c[0])), dtype=np.uint64)
                h = fmix32((v[lo] + np.uint64(0x9e3779b9) * (i + np.uint64(1))) & M32)
                kept[lo] += int((h < np.uint64(keep)).sum())
        else:
            i = np.arange(int(c.sum()), dtype=np.uint64) - np.repeat(np.cumsum(c) - c, c).astype(np.uint64)
            h = fmix32((np.repeat(v[lo:hi], c) + np.uint64(0x9e3779b9) * (i + np.uint64(1))) & M32)
            kept[lo:hi] = np.bincount(np.repeat(np.arange(len(c)), c)[h < np.uint64(keep)], minlength=len(c))
        lo = hi
    on = kept >= 1
    return np.asarray(line, np.int32)[on], kept[on].astype(np.int32)


def render(res):
    """The lines kept in profiles/thin.txt, from the results of a run."""
    text = ["depth thinning over the junction store at keep 0.1, %d samples x %d lines, %d entries (scripts/bench_thin.py)" %
            (res["n_samples"], res["n_lines"], res["nnz"])]
    for name in res["shapes"]:
        r = res[name]
        text.append("thin %5s jobs   kernels %.3f ms (three calls: %.3f to %.3f) for %.3f MB read + %.3f MB written: %.4g GB/s; %d draws: "
                    "%.3f Gdraws/s; %d workgroups per pass; whole call %.2f ms; %d lines keep %d reads; numpy on %d jobs, %d draws: "
                    "%.2f ms, %.4f Gdraws/s, answers equal: %s" %
                    (name, r["kernel_ms"], r["kernel_ms_min"], r["kernel_ms_max"], r["bytes_read"] / 1e6, r["bytes_written"] / 1e6,
                     r["GBps"], r["draws"], r["Gdraws_per_s"], r["workgroups"], r["wall_ms"], r["kept_lines"], r["kept_reads"],
                     r["numpy_jobs"], r["numpy_draws"], r["numpy_ms"], r["numpy_Gdraws_per_s"], r["equals_numpy"]))
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--numpy-draws", type=int, default=60_000_000)
    ap.add_argument("--json", default=None)
    ap.add_argument("--text", default=None)
    args = ap.parse_args()
    res = dict(samples=args.samples, junctions=args.junctions)

    def note(what):
        sys.stderr.write("[bench_thin] %s\n" % what)
        sys.stderr.flush()

    note("making the data set")
    d = synthetic_intropolis(args.samples, J=args.junctions)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "index.tsv")
        keys = [k.encode("ascii") for k in d["keys"]]
        key_off = np.zeros(len(keys) + 1, np.int64)
        key_off[1:] = np.cumsum([len(k) for k in keys])
        key_bytes = np.frombuffer(b"".join(keys), np.uint8)
        check(lib().morna_write_intropolis(path.encode(), ptr(key_bytes), ptr(key_off), len(keys), ptr(d["row_ptr"]),
                                           ptr(np.ascontiguousarray(d["samples"], np.int64)),
                                           ptr(np.ascontiguousarray(d["cov"], np.int32))))
        note("parsing it")
        parsed = ParsedLines(path, sample_count=args.samples, sample_threshold=0)
    note("building the store")
    store = JunctionStore.build(parsed)
    del parsed, d
    res.update(n_samples=store.n_samples, n_lines=store.n_lines, nnz=store.nnz)
    ids = np.sort(store.sample_ids())
    shapes = [("%d" % n, store, ids[:n].tolist()) for n in (1, 64, min(1000, len(ids)))]
    line, cov = store.sample(int(ids[0]))
    cov = cov.copy()
    at = [len(cov) // 4, len(cov) // 2, len(cov) - 1]
    cov[at] = [2**24, 2**24 - 1, 2**24 - 4097]
    heavy = JunctionStore.from_arrays([int(ids[0])], [0, len(line)], line, cov, store.n_lines)
    shapes.append(("heavy", heavy, [int(ids[0])]))
    res["shapes"] = [name for name, _, _ in shapes]
    for name, st, jobs in shapes:
        note("thin " + name)
        st.thin(jobs, KEEP, SEED)                               # warm-up
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            thinned = st.thin(jobs, KEEP, SEED)
            wall = (time.perf_counter() - t0) * 1e3
            runs.append((st.thin_stats(), wall))
        best = min(runs, key=lambda r: r[0]["kernel_ms"])
        ms = [r[0]["kernel_ms"] for r in runs]
        moved = best[0]["bytes_read"] + best[0]["bytes_written"]
        note("numpy " + name)
        host_rows, draws = [], 0
        for s in jobs:                                          # the first jobs, up to the draw budget (one at the least)
            row = st.sample(s)
            if host_rows and draws + int(row[1].sum()) > args.numpy_draws:
                break
            host_rows.append(row)
            draws += int(row[1].sum())
        t0 = time.perf_counter()
        answers = [numpy_thin(s, row[0], row[1], KEEP, SEED) for s, row in zip(jobs, host_rows)]
        host_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(a[0], t.lines) and np.array_equal(a[1], t.cov) for a, t in zip(answers, thinned))
        res[name] = dict(kernel_ms=best[0]["kernel_ms"], kernel_ms_min=min(ms), kernel_ms_max=max(ms), bytes_read=best[0]["bytes_read"],
                         bytes_written=best[0]["bytes_written"], GBps=moved / best[0]["kernel_ms"] / 1e6, draws=best[0]["draws"],
                         Gdraws_per_s=best[0]["draws"] / best[0]["kernel_ms"] / 1e6, wall_ms=best[1], workgroups=best[0]["workgroups"],
                         kept_lines=int(sum(len(t) for t in thinned)), kept_reads=int(sum(int(t.cov.sum()) for t in thinned)),
                         numpy_jobs=len(host_rows), numpy_draws=draws, numpy_ms=host_ms,
                         numpy_Gdraws_per_s=draws / max(host_ms, 1e-9) / 1e6, equals_numpy=bool(same))
    out = json.dumps(res, sort_keys=True)
    print(out)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(out + "\n")
    text = render(res)
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
