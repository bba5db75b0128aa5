#!/usr/bin/env python3
"""Pooling groups of samples over the junction store (morna_jstore_pool) at the data set of
scripts/bench_junctions.py (synth.synthetic_intropolis, 50k samples, 70k junctions, ~1e8 entries).  Reports, as one JSON
line and as the text kept in profiles/pool.txt, for 1 group of 20 samples, 1 group of 1000 and 50 disjoint groups of 1000
(the whole store):

  kernel ms    HIP-event time of both passes and the tile scan: the best of three calls after a warm-up, and the spread
  bytes        read (8 per entry of every member row, per pass) and written (16 per held line), and the rate they make
  whole call   wall clock of JunctionStore.pool, the copies back and the numpy views included
  numpy        the same sums by np.add.at over the host image of the member rows (handed over ready made), and whether
               the answers are equal

A group is consecutive sample ids (the members of a latent cluster are contiguous): a tissue or a study.

    python3 scripts/bench_pool.py [--samples 50000] [--junctions 70000] [--json out.json] [--text out.txt]
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


def numpy_pool(rows, n_lines):
    """(lines, sums, holders) of one group from its members' (lines, coverages) arrays."""
    line = np.concatenate([r[0] for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    cov = np.concatenate([r[1] for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    sums, holders = np.zeros(n_lines, np.int64), np.zeros(n_lines, np.int32)
    np.add.at(sums, line, cov)
    np.add.at(holders, line, 1)
    held = np.nonzero(holders)[0]
    return held.astype(np.int32), sums[held], holders[held]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--json", default=None)
    ap.add_argument("--text", default=None)
    args = ap.parse_args()
    res = dict(samples=args.samples, junctions=args.junctions)

    def note(what):
        sys.stderr.write("[bench_pool] %s\n" % what)
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
    per = min(1000, len(ids))
    shapes = [("1x20", [ids[:20].tolist()]), ("1x%d" % per, [ids[:per].tolist()]),
              ("%dx%d" % (len(ids) // per, per), [ids[g * per:(g + 1) * per].tolist() for g in range(len(ids) // per)])]
    res["shapes"] = [name for name, _ in shapes]
    for name, groups in shapes:
        note("pool " + name)
        store.pool(groups)                                      # warm-up
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            pooled = store.pool(groups)
            wall = (time.perf_counter() - t0) * 1e3
            runs.append((store.pool_stats(), wall))
        best = min(runs, key=lambda r: r[0]["kernel_ms"])
        ms = [r[0]["kernel_ms"] for r in runs]
        moved = best[0]["bytes_read"] + best[0]["bytes_written"]
        note("numpy " + name)
        host_rows = [[store.sample(s) for s in grp] for grp in groups]
        t0 = time.perf_counter()
        answers = [numpy_pool(rows, store.n_lines) for rows in host_rows]
        host_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(a[0], p.lines) and np.array_equal(a[1], p.sums) and np.array_equal(a[2], p.holders)
                   for a, p in zip(answers, pooled))
        res[name] = dict(kernel_ms=best[0]["kernel_ms"], kernel_ms_min=min(ms), kernel_ms_max=max(ms), bytes_read=best[0]["bytes_read"],
                         bytes_written=best[0]["bytes_written"], GBps=moved / best[0]["kernel_ms"] / 1e6, wall_ms=best[1],
                         workgroups=best[0]["workgroups"], held=int(sum(len(p) for p in pooled)), numpy_ms=host_ms,
                         equals_numpy=bool(same))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    text = ["pooled samples over the junction store, %d samples x %d lines, %d entries (scripts/bench_pool.py)" %
            (res["n_samples"], res["n_lines"], res["nnz"])]
    for name in res["shapes"]:
        r = res[name]
        text.append("pool %9s   kernels %.3f ms (three calls: %.3f to %.3f) for %.1f MB read in two passes + %.1f MB written: %.1f GB/s; "
                    "%d workgroups per pass; whole call %.2f ms; %d lines held; numpy np.add.at %.0f ms, answers equal: %s" %
                    (name, r["kernel_ms"], r["kernel_ms_min"], r["kernel_ms_max"], r["bytes_read"] / 1e6, r["bytes_written"] / 1e6,
                     r["GBps"], r["workgroups"], r["wall_ms"], r["held"], r["numpy_ms"], r["equals_numpy"]))
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
