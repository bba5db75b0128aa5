#!/usr/bin/env python3
"""Hashed rows from store rows and `morna hashing` at bench_junctions.py's data set
(synth.synthetic_intropolis, 50k samples, 70k junctions, ~1e8 entries).  Reports, as one JSON line and as text (kept in
profiles/hashing.txt):

  rows_D       morna_add_items_from_store for all items of the index at D = 500, 3000, 8192, 32768: kernel time (HIP events,
               the best of three calls), its statistics' bytes over that time, and whether the rows and norms are those of
               build_features
  features_D   MORNA_T_FEATURES of build_features on the same data at the same D, in the same session (the best of three)
  hashing      the whole MornaSearch.hashing_sweep call for 100 queries at the widths 500,1000,3000,8192,index on an index of
               16384 features, and the share of it the --junction-file parse (junctions.line_hashes) takes

    python3 scripts/bench_hashing.py [--samples 50000] [--junctions 70000] [--threshold 100] [--text out.txt]
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
from morna_amd.annoy import AnnoyIndex  # noqa: E402
from morna_amd.index import ParsedLines, go_index_native  # noqa: E402
from morna_amd.junctions import JunctionStore, line_hashes, line_weights  # noqa: E402
from morna_amd.synth import synthetic_intropolis  # noqa: E402

DIMS = [500, 3000, 8192, 32768]
SWEEP = [500, 1000, 3000, 8192, 16384]      # "500,1000,3000,8192,index" on the index below
INDEX_DIM = 16384


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--threshold", type=int, default=100)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--no-sweep", action="store_true", help="skip the index build and the whole hashing call")
    ap.add_argument("--json", default=None)
    ap.add_argument("--text", default=None)
    args = ap.parse_args()
    res = dict(samples=args.samples, junctions=args.junctions, threshold=args.threshold, k=args.k, queries=args.queries)
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
        del d
        whole = ParsedLines(path, sample_count=args.samples, sample_threshold=0)
        w = line_weights(whole, args.threshold)
        if w is None:
            raise SystemExit("the synthetic file repeats a junction: no weights")
        store = JunctionStore.build(whole)
        store.set_weights(w)
        a = whole.arrays()
        line_hash = AnnoyIndex(8).hash_keys(a["key_bytes"], a["key_off"])[0]
        del whole, a
        kept = ParsedLines(path, sample_count=args.samples, sample_threshold=args.threshold)
        items = np.array(kept.arrays()["ext_ids"], np.int64)
        res.update(n_samples=store.n_samples, n_lines=store.n_lines, nnz=store.nnz, items=len(items))
        for D in DIMS:
            f = AnnoyIndex(D)
            f.timer_enable(True, only=["features"])
            kept.stage(f)
            best = None
            for _ in range(3):
                f.timer_reset()
                f.build_features(kept.n_items)
                f.synchronize()
                t = f.timers()["features"]
                if best is None or t["ms"] < best["ms"]:
                    best = t
            res["features_%d" % D] = dict(ms=best["ms"], bytes=best["bytes"], GBps=best["bytes"] / best["ms"] / 1e6)
            f.unstage_junctions()
            h = AnnoyIndex(D)
            best = None
            for _ in range(3):
                h.add_items_from_store(store, items, line_hash)
                st = store.hash_rows_stats()
                if best is None or st["kernel_ms"] < best["kernel_ms"]:
                    best = st
            same = h.get_norms2().tobytes() == f.get_norms2().tobytes()
            if D <= 3000:
                same = same and h.get_items().tobytes() == f.get_items().tobytes()
            res["rows_%d" % D] = dict(kernel_ms=best["kernel_ms"], bytes_read=best["bytes_read"], bytes_written=best["bytes_written"],
                                      GBps=(best["bytes_read"] + best["bytes_written"]) / best["kernel_ms"] / 1e6,
                                      workgroups=best["workgroups"], same_as_build_features=bool(same))
            del f, h
        del kept
        if not args.no_sweep:
            from morna_amd.search import MornaSearch
            base = os.path.join(tmp, "idx")
            go_index_native(path, base, INDEX_DIM, 1, args.samples, args.threshold, 1024, False, None, junction_store=True)
            searcher = MornaSearch(base)
            rng = np.random.Generator(np.random.PCG64(21))
            queries = [int(x) for x in items[rng.permutation(len(items))[:args.queries]]]
            store2, _ = searcher.unhashed_store()
            t0 = time.perf_counter()
            line_hashes(path, store2.n_lines, searcher.annoy_index)
            parse_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            table = searcher.hashing_sweep(queries, args.k, SWEEP, path)
            whole_ms = (time.perf_counter() - t0) * 1e3
            res["hashing"] = dict(whole_ms=whole_ms, parse_ms=parse_ms, parse_share=parse_ms / whole_ms, kernel_ms=table.kernel_ms,
                                  summary=[list(r) for r in table.summary()])
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    text = ["hashed rows from store rows, %d samples x %d lines, %d entries; the %d items of the index at threshold %d "
            "(scripts/bench_hashing.py)" % (res["n_samples"], res["n_lines"], res["nnz"], res["items"], args.threshold)]
    for D in DIMS:
        r, f = res["rows_%d" % D], res["features_%d" % D]
        text.append("D = %5d   add_items_from_store kernels %.2f ms, %.1f MB read + %.1f MB written: %.0f GB/s, %d workgroups; rows and norms "
                    "%s build_features'; build_features (MORNA_T_FEATURES) %.2f ms, %.1f MB algorithmic: %.0f GB/s" %
                    (D, r["kernel_ms"], r["bytes_read"] / 1e6, r["bytes_written"] / 1e6, r["GBps"], r["workgroups"],
                     "are" if r["same_as_build_features"] else "ARE NOT", f["ms"], f["bytes"] / 1e6, f["GBps"]))
    if "hashing" in res:
        r = res["hashing"]
        text.append("hashing    %d queries, r = %d, --features %s on an index of %d features: whole call %.0f ms, of which the "
                    "--junction-file parse %.0f ms (%.0f %%); row kernels %s ms" %
                    (args.queries, args.k, ",".join(map(str, SWEEP)), INDEX_DIM, r["whole_ms"], r["parse_ms"], 100 * r["parse_share"],
                     " / ".join("%.2f" % x for x in r["kernel_ms"])))
        for row in r["summary"]:
            text.append("           " + "\t".join("-" if v is None else ("%.6f" % v if isinstance(v, float) else str(v)) for v in row))
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
