#!/usr/bin/env python3
"""The junction store and its filter at configs[2]'s data set (synth.synthetic_intropolis, 50k samples, 70k junctions,
~1e8 entries).  Reports, as one JSON line and as the text kept in profiles/junctions.txt:

  build        morna_jstore_build: HIP-event time of its kernels (count, two scans, place), the algorithmic bytes
               2 x 8 B x nnz, and the rate they make; wall clock of the whole call (upload and host image included)
  retain_N     morna_jstore_retain for N = 1, 64 and 1000 result lists of k = 20: kernel time (both passes and the tile
               scan), the bytes of the k lists each query must read, the wall clock of the call
  host_N       the same retentions by the tests' Python restatement of morna.py:1539-1569 (tests/test_junctions_cpu.py,
               ref_retain) on the host, its tables handed over ready made, and that its answer is the GPU's

A result list is 20 samples of one latent cluster of the data set (what a neighbour search returns: the members of a
cluster are contiguous sample ids), filter .05,5.

    python3 scripts/bench_junctions.py [--samples 50000] [--junctions 70000] [--json out.json] [--text out.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from morna_amd._lib import check, lib, ptr  # noqa: E402
from morna_amd.index import ParsedLines  # noqa: E402
from morna_amd.junctions import JunctionStore  # noqa: E402
from morna_amd.synth import synthetic_intropolis  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--host-lists", type=int, default=1000, help="largest batch the host restatement is timed on")
    ap.add_argument("--json", default=None)
    ap.add_argument("--text", default=None)
    args = ap.parse_args()
    res = dict(samples=args.samples, junctions=args.junctions, k=args.k, filter=".05,5")
    t0 = time.perf_counter()
    d = synthetic_intropolis(args.samples, J=args.junctions)
    res["synth_s"] = time.perf_counter() - t0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "index.tsv")
        keys = [k.encode("ascii") for k in d["keys"]]
        key_off = np.zeros(len(keys) + 1, np.int64)
        key_off[1:] = np.cumsum([len(k) for k in keys])
        key_bytes = np.frombuffer(b"".join(keys), np.uint8)
        check(lib().morna_write_intropolis(path.encode(), ptr(key_bytes), ptr(key_off), len(keys), ptr(d["row_ptr"]),
                                           ptr(np.ascontiguousarray(d["samples"], np.int64)),
                                           ptr(np.ascontiguousarray(d["cov"], np.int32))))
        t0 = time.perf_counter()
        parsed = ParsedLines(path, sample_count=args.samples, sample_threshold=0)
        res["parse_s"] = time.perf_counter() - t0
    JunctionStore.build(parsed)                                 # warm-up: the first launch of every kernel
    t0 = time.perf_counter()
    store = JunctionStore.build(parsed)
    res["build_wall_ms"] = (time.perf_counter() - t0) * 1e3
    ms, nbytes = store.timers()["build"]
    res.update(n_samples=store.n_samples, n_lines=store.n_lines, nnz=store.nnz, build_kernel_ms=ms, build_bytes=nbytes,
               build_GBps=nbytes / ms / 1e6)
    del parsed
    # result lists: 20 consecutive sample ids (one cluster) starting at seeded places
    rng = np.random.Generator(np.random.PCG64(20))
    ids = np.sort(store.sample_ids())
    starts = rng.integers(0, len(ids) - args.k, size=1000)
    lists = [ids[s:s + args.k].tolist() for s in starts.tolist()]
    from test_junctions_cpu import ref_retain
    for n in (1, 64, 1000):
        batch = lists[:n]
        store.retain(batch, .05, 5)                             # warm-up
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            kept = store.retain(batch, .05, 5)
            wall = (time.perf_counter() - t0) * 1e3
            ms, nbytes = store.timers()["retain"]
            if best is None or ms < best[0]:
                best = (ms, nbytes, wall)
        res["retain_%d" % n] = dict(kernel_ms=best[0], list_bytes=best[1], list_GBps=best[1] / best[0] / 1e6, wall_ms=best[2],
                                    retained=int(sum(len(r) for r in kept)))
        if n <= args.host_lists:
            tables = {}
            for s in set(x for lst in batch for x in lst):
                line, cov = store.sample(s)
                tables[s] = (line.tolist(), [str(c) for c in cov.tolist()])     # the reference's coverages are strings
            t0 = time.perf_counter()
            answers = [ref_retain([tables[s][0] for s in lst], [tables[s][1] for s in lst], .05, 5) for lst in batch]
            host_ms = (time.perf_counter() - t0) * 1e3
            same = all(sorted(a[0]) == r.lines.tolist() for a, r in zip(answers, kept))
            same = same and all([a[1][j] for j in r.lines.tolist()] == r.found_in for a, r in list(zip(answers, kept))[:4])
            res["host_%d" % n] = dict(ms=host_ms, equals_gpu=bool(same))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    text = ["junction store and filter, %d samples x %d lines, %d entries (scripts/bench_junctions.py)" %
            (res["n_samples"], res["n_lines"], res["nnz"]),
            "store build   kernels %.2f ms for %.0f MB algorithmic (2 x 8 B x nnz): %.0f GB/s; whole call %.0f ms" %
            (res["build_kernel_ms"], res["build_bytes"] / 1e6, res["build_GBps"], res["build_wall_ms"])]
    for n in (1, 64, 1000):
        r = res["retain_%d" % n]
        h = res.get("host_%d" % n)
        text.append("retain %4d x k=%d   kernels %.3f ms for %.1f MB of lists: %.1f GB/s; whole call %.2f ms; %d lines retained%s" %
                    (n, args.k, r["kernel_ms"], r["list_bytes"] / 1e6, r["list_GBps"], r["wall_ms"], r["retained"],
                     "; host restatement %.0f ms, answers equal: %s" % (h["ms"], h["equals_gpu"]) if h else ""))
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
