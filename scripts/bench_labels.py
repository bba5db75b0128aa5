#!/usr/bin/env python3
"""Label distance sums at bench.py's data set: synthetic intropolis 50k samples x 3000 features.  For
L = 2, 64 and 4096 labels (uniformly random, one item in 20 unlabelled) and 1, 64, 1000 and all by-item queries: the scan and
the sums kernel by HIP events (morna_label_sums_stats) and the whole call on the host clock, each the best of three after a
warm-up call, with the spread (max - min) / min of the three; the sums kernel beside its byte floor, 4 N nq bytes of scan values
at the HBM rate measured for a streaming read (6.3 TB/s); and the whole call beside morna_exact_search_by_item of the same
queries at k = 20.  With --exact-only only that yardstick is timed, and --tree DIR imports the package of another checkout
(the parent commit's, whose library lacks the new call).  One JSON line, and text (kept in profiles/labels.txt).

    python3 scripts/bench_labels.py [--samples 50000] [--features 3000] [--text out.txt] [--exact-only] [--tree DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HBM_TBS = 6.3


def best(values):
    return min(values), (max(values) - min(values)) / min(values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--text", default=None)
    ap.add_argument("--exact-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.index import prepare_csr
    from morna_amd.synth import SEED, synthetic_intropolis
    data = synthetic_intropolis(args.samples, J=args.junctions, seed=SEED)
    prep = prepare_csr(data["keys"], data["row_ptr"], data["samples"], data["cov"], data["sample_count"], 100)
    a = AnnoyIndex(args.features)
    a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
    a.stage_item_order(prep["ext_ids"])
    a.build_features(prep["n_items"])
    a.unstage_junctions()
    n = a.get_n_items()
    rng = np.random.Generator(np.random.PCG64(13))
    items_all = rng.permutation(n).astype(np.int32)
    res = dict(samples=n, features=args.features, k=args.k, tree=os.path.abspath(args.tree), cases={})
    text = ["label distance sums, %d samples x %d features, by-item queries (scripts/bench_labels.py%s)"
            % (n, args.features, ", package of %s" % args.tree if args.exact_only else ""),
            "ms, best of 3 after a warm-up (spread = (max - min) / min); floor = 4 N nq bytes at %.1f TB/s" % HBM_TBS]
    for nq in (1, 64, 1000, n):
        items = items_all[:nq]
        a.exact_search_by_item_batch(items, args.k)
        a.synchronize()
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            a.exact_search_by_item_batch(items, args.k)
            wall.append((time.perf_counter() - t0) * 1e3)
        ex, ex_spread = best(wall)
        res["cases"]["exact/%d" % nq] = dict(wall_ms=ex, wall_spread=ex_spread)
        text.append("%6d queries  exact search, k = %d        call %10.3f ms (spread %5.1f %%)" % (nq, args.k, ex, 100 * ex_spread))
        if args.exact_only:
            continue
        floor = 4.0 * n * nq / (HBM_TBS * 1e12) * 1e3
        for L in (2, 64, 4096):
            labels = rng.integers(0, L, size=n).astype(np.int32)
            labels[rng.random(n) < 0.05] = -1
            a.label_sums(labels, L, items=items)
            scan, sums, wall = [], [], []
            for _ in range(3):
                t0 = time.perf_counter()
                a.label_sums(labels, L, items=items)
                wall.append((time.perf_counter() - t0) * 1e3)
                stats = a.label_sums_stats()
                scan.append(stats["scan_ms"])
                sums.append(stats["sums_ms"])
            (sc, sc_s), (su, su_s), (wa, wa_s) = best(scan), best(sums), best(wall)
            res["cases"]["labels/%d/%d" % (nq, L)] = dict(scan_ms=sc, scan_spread=sc_s, sums_ms=su, sums_spread=su_s, wall_ms=wa,
                                                         wall_spread=wa_s, floor_ms=floor, batches=stats["batches"])
            text.append("%6d queries  L = %-4d  scan %9.3f ms (%4.1f %%)  sums kernel %9.4f ms (%4.1f %%; floor %8.4f ms, x%.2f)  "
                        "call %10.3f ms (%4.1f %%; x%.2f of the exact search)"
                        % (nq, L, sc, 100 * sc_s, su, 100 * su_s, floor, su / floor, wa, 100 * wa_s, wa / ex))
    print(json.dumps(res, sort_keys=True))
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
