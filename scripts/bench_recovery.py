#!/usr/bin/env python3
"""The recovery tables (`morna recovery`) at the data set of scripts/bench_junctions.py
(synth.synthetic_intropolis, 50k samples, 70k junctions, ~1e8 entries).  Reports, as one JSON line and as the text kept
in profiles/recovery.txt:

  recovery_N   morna_jstore_recovery_by_sample for N = 1, 64 and 1000 result lists of k = 20 over the default grid of
               8 frequencies x 8 coverages: kernel time (the memset of the histogram and the one kernel), the bytes of
               the k + 1 rows each query reads and the rate they make, and the wall clock of the whole call with the 64
               cells derived on the host (junctions.recovery_rows)
  retain_N     the same table by the route there was before: one morna_jstore_retain per cell, then a host intersection
               of every retained list with the truth.  For N = 1 and 64 all 64 cells are run; for N = 1000 ONE cell
               (.05,5) is run and its time multiplied by 64 -- the line says so
  equal        that the cells both routes computed hold the same retrieved and true-positive counts
  sweep_N      morna_jstore_recovery_sweep_by_sample (N7) for N lists of 64 consecutive sample ids and the prefixes 5, 10, 20,
               40, 64: kernel time, row bytes and rate of the one call, from recovery_stats; and the route there was before,
               five recovery_by_sample calls on the lists cut to those lengths: the sum of their kernel times and of their
               bytes.  Both best of three repeats after a warm-up, with the spread (largest minus smallest) of the three;
               and whether the five slices equal the five histograms

A result list is 20 consecutive sample ids (one latent cluster of the data set, what a neighbour search returns), the
query the sample just before them: leave one out, its own junctions the truth.

    python3 scripts/bench_recovery.py [--samples 50000] [--junctions 70000] [--sweep 5,10,20,40,64] [--json out.json] [--text out.txt]
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
from morna_amd.junctions import JunctionStore, parse_recovery_grid, parse_results_sweep, recovery_rows  # noqa: E402
from morna_amd.synth import synthetic_intropolis  # noqa: E402


def by_retain(store, lists, truths, frequency, coverage):
    """(retrieved, true positives) of every list under one cell, by the filter and a host intersection."""
    kept = store.retain(lists, float(frequency), coverage)
    return [(len(r), len(np.intersect1d(r.lines, t, assume_unique=True))) for r, t in zip(kept, truths)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--sweep", default="5,10,20,40,64", help="the prefixes of the sweep case")
    ap.add_argument("--json", default=None)
    ap.add_argument("--text", default=None)
    args = ap.parse_args()
    frequencies, coverages = parse_recovery_grid()
    cells = [(f, c) for f in frequencies for c in coverages]
    res = dict(samples=args.samples, junctions=args.junctions, k=args.k, cells=len(cells))
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
        parsed = ParsedLines(path, sample_count=args.samples, sample_threshold=0)
    store = JunctionStore.build(parsed)
    del parsed, d
    res.update(n_samples=store.n_samples, n_lines=store.n_lines, nnz=store.nnz)
    rng = np.random.Generator(np.random.PCG64(20))
    ids = np.sort(store.sample_ids())
    starts = rng.integers(0, len(ids) - args.k - 1, size=1000)
    queries = [int(ids[s]) for s in starts.tolist()]
    lists = [ids[s + 1:s + 1 + args.k].tolist() for s in starts.tolist()]
    truths = [store.sample(q)[0] for q in queries]
    equal = True
    for n in (1, 64, 1000):
        batch, who, truth = lists[:n], queries[:n], truths[:n]
        store.recovery_by_sample(batch, who, coverages)        # warm-up
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            hist = store.recovery_by_sample(batch, who, coverages)
            tables = [recovery_rows(hist[q], len(batch[q]), frequencies, coverages) for q in range(n)]
            wall = (time.perf_counter() - t0) * 1e3
            stats = store.recovery_stats()
            if best is None or stats["kernel_ms"] < best[0]["kernel_ms"]:
                best = (stats, wall)
        stats, wall = best
        res["recovery_%d" % n] = dict(kernel_ms=stats["kernel_ms"], row_bytes=stats["bytes"], workgroups=stats["workgroups"],
                                      row_GBps=stats["bytes"] / stats["kernel_ms"] / 1e6, wall_ms=wall,
                                      hist_bytes=int(hist.size) * 4)
        run = cells if n < 1000 else [(".05", 5)]
        by_retain(store, batch, truth, *run[0])                # warm-up
        t0 = time.perf_counter()
        answers = {cell: by_retain(store, batch, truth, *cell) for cell in run}
        retain_ms = (time.perf_counter() - t0) * 1e3
        for cell, counts in answers.items():
            at = cells.index(cell)
            equal = equal and counts == [(tables[q][at]["retrieved"], tables[q][at]["true_positive"]) for q in range(n)]
        res["retain_%d" % n] = dict(cells_run=len(run), ms_run=retain_ms, ms_all_cells=retain_ms * len(cells) / len(run))
    prefixes = parse_results_sweep(args.sweep)
    deep = [ids[min(s, len(ids) - prefixes[-1] - 1) + 1:][:prefixes[-1]].tolist() for s in starts.tolist()]
    for n in (1, 64, 1000):
        batch, who = deep[:n], queries[:n]
        cuts = [[lst[:p] for lst in batch] for p in prefixes]

        def one_call():
            hist = store.recovery_sweep_by_sample(batch, who, coverages, prefixes)
            return hist, store.recovery_stats()

        def five_calls():
            hists, ms, nbytes = [], 0.0, 0
            for cut in cuts:
                hists.append(store.recovery_by_sample(cut, who, coverages))
                stats = store.recovery_stats()
                ms, nbytes = ms + stats["kernel_ms"], nbytes + stats["bytes"]
            return hists, ms, nbytes
        one_call()                                             # warm-up
        five_calls()
        sweep_ms, five_ms = [], []
        for _ in range(3):
            hist, stats = one_call()
            sweep_ms.append(stats["kernel_ms"])
            hists, ms, five_bytes = five_calls()
            five_ms.append(ms)
        same = all(np.array_equal(hist[:, i], hists[i]) for i in range(len(prefixes)))
        equal = equal and same
        res["sweep_%d" % n] = dict(prefixes=prefixes, kernel_ms=min(sweep_ms), kernel_ms_spread=max(sweep_ms) - min(sweep_ms),
                                   row_bytes=stats["bytes"], row_GBps=stats["bytes"] / min(sweep_ms) / 1e6,
                                   workgroups=stats["workgroups"], five_calls_kernel_ms=min(five_ms),
                                   five_calls_kernel_ms_spread=max(five_ms) - min(five_ms), five_calls_row_bytes=five_bytes,
                                   five_calls_row_GBps=five_bytes / min(five_ms) / 1e6, equal=bool(same))
    res["equal"] = bool(equal)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    text = ["recovery tables, %d samples x %d lines, %d entries, grid of %d frequencies x %d coverages (scripts/bench_recovery.py)" %
            (res["n_samples"], res["n_lines"], res["nnz"], len(frequencies), len(coverages))]
    for n in (1, 64, 1000):
        r, o = res["recovery_%d" % n], res["retain_%d" % n]
        text.append("recovery %4d x k=%d   kernel %.3f ms for %.1f MB of rows: %.1f GB/s, %d workgroups; whole call with its %d cells "
                    "%.2f ms, %.1f MB copied back; one retain per cell and a host intersection: %.0f ms%s" %
                    (n, args.k, r["kernel_ms"], r["row_bytes"] / 1e6, r["row_GBps"], r["workgroups"], len(cells), r["wall_ms"],
                     r["hist_bytes"] / 1e6, o["ms_all_cells"],
                     "" if o["cells_run"] == len(cells) else " (%d cell timed, %.0f ms, times %d)" % (o["cells_run"], o["ms_run"], len(cells))))
    for n in (1, 64, 1000):
        r = res["sweep_%d" % n]
        text.append("sweep    %4d x -r %s   one call: kernel %.3f ms (spread %.3f) for %.1f MB of rows: %.1f GB/s, %d workgroups; "
                    "%d recovery calls on the cut lists: kernel %.3f ms in all (spread %.3f) for %.1f MB: %.1f GB/s; slices equal: %s" %
                    (n, ",".join(str(p) for p in r["prefixes"]), r["kernel_ms"], r["kernel_ms_spread"], r["row_bytes"] / 1e6,
                     r["row_GBps"], r["workgroups"], len(r["prefixes"]), r["five_calls_kernel_ms"], r["five_calls_kernel_ms_spread"],
                     r["five_calls_row_bytes"] / 1e6, r["five_calls_row_GBps"], r["equal"]))
    r = res["sweep_1000"]
    spread = max(r["kernel_ms_spread"], r["five_calls_kernel_ms_spread"])
    text.append("sweep at 1000 lists: %.3f ms against %.3f ms of the separate calls, spread of the three repeats %.3f ms: the sweep "
                "is %s" % (r["kernel_ms"], r["five_calls_kernel_ms"], spread,
                           "no slower" if r["kernel_ms"] <= r["five_calls_kernel_ms"] + spread else "SLOWER"))
    text.append("equal: %s (the retain route's cells and the sweep's slices)" % res["equal"])
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
