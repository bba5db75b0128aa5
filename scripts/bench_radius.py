#!/usr/bin/env python3
"""Radius search at bench.py's data set: synthetic intropolis 50k samples x 3000 features, by-item queries,
1 / 64 / 1000 / all of them.  The radii are quantiles of a first exact search (200 queries, 1024 deep): the median distance
of the 2nd, 21st and 1001st entry, so that an answer averages about 1, 20 and 1000 samples beside the query itself; they are
recorded.  Per case: the scan, the selection (count, offsets, write) and the distance pass with the device ordering by HIP
events (morna_exact_radius_stats) and the whole call on the host clock, each the best of three after a warm-up call, with
the spread (max - min) / min of the three; the candidates and results.  Beside it morna_exact_search_by_item of the same
queries at k = 20: the call, and from the library's timers the scan kernel and the rest of the `exact` group (selection and
re-rank).  With --exact-only only that yardstick is timed, and --tree DIR imports the package of another checkout (the
parent commit's, whose library lacks the new call).  One JSON line, and text (kept in profiles/radius.txt).

    python3 scripts/bench_radius.py [--samples 50000] [--features 3000] [--text out.txt] [--exact-only] [--tree DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def best(values):
    return min(values), (max(values) - min(values)) / max(min(values), 1e-12)


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
    rng = np.random.Generator(np.random.PCG64(14))
    items_all = rng.permutation(n).astype(np.int32)
    depth = min(1024, n)
    _, d, cnt = a.exact_search_by_item_batch(items_all[:200], depth)
    ok = cnt == depth
    radii = [float(np.median(d[ok, min(m, depth - 1)])) for m in (1, 20, 1000)]
    res = dict(samples=n, features=args.features, k=args.k, tree=os.path.abspath(args.tree), radii=radii, cases={})
    text = ["radius search, %d samples x %d features, by-item queries (scripts/bench_radius.py%s)"
            % (n, args.features, ", package of %s" % args.tree if args.exact_only else ""),
            "radii (median distance of entry 2 / 21 / 1001 of 200 exact lists): %r" % (radii,),
            "ms, best of 3 after a warm-up (spread = (max - min) / min)"]
    for nq in (1, 64, 1000, n):
        items = items_all[:nq]
        a.exact_search_by_item_batch(items, args.k)
        a.synchronize()
        wall, scan, rest = [], [], []
        for _ in range(3):
            a.timer_enable(True)
            a.timer_reset()
            t0 = time.perf_counter()
            a.exact_search_by_item_batch(items, args.k)
            wall.append((time.perf_counter() - t0) * 1e3)
            t = a.timers()
            a.timer_enable(False)
            scan.append(t["exact_scan"]["ms"])
            rest.append(t["exact"]["ms"] - t["exact_scan"]["ms"])
        (ex, ex_s), (es, es_s), (er, er_s) = best(wall), best(scan), best(rest)
        res["cases"]["exact/%d" % nq] = dict(wall_ms=ex, wall_spread=ex_s, scan_ms=es, scan_spread=es_s, select_rerank_ms=er,
                                             select_rerank_spread=er_s, select_rerank_runs=rest)
        text.append("%6d queries  exact search, k = %d   scan %9.3f ms (%4.1f %%)  selection + re-rank %9.3f ms (%4.1f %%; runs %s)  "
                    "call %10.3f ms (%4.1f %%)" % (nq, args.k, es, 100 * es_s, er, 100 * er_s,
                                                   " ".join("%.3f" % v for v in rest), ex, 100 * ex_s))
        if args.exact_only:
            continue
        for r in radii:
            a.exact_radius(r, items=items)
            scan, sel, dist, wall = [], [], [], []
            for _ in range(3):
                t0 = time.perf_counter()
                a.exact_radius(r, items=items)
                wall.append((time.perf_counter() - t0) * 1e3)
                st = a.exact_radius_stats()
                scan.append(st["scan_ms"])
                sel.append(st["select_ms"])
                dist.append(st["dist_ms"])
            (sc, sc_s), (se, se_s), (di, di_s), (wa, wa_s) = best(scan), best(sel), best(dist), best(wall)
            res["cases"]["radius/%d/%.6f" % (nq, r)] = dict(
                scan_ms=sc, scan_spread=sc_s, select_ms=se, select_spread=se_s, dist_ms=di, dist_spread=di_s, wall_ms=wa,
                wall_spread=wa_s, candidates=st["candidates"], results=st["results"], batches=st["batches"], window=st["window"])
            text.append("%6d queries  r = %.6f  scan %9.3f ms (%4.1f %%)  selection %8.3f ms (%4.1f %%)  distances %9.3f ms (%4.1f %%)  "
                        "sel + dist %9.3f ms (x%.2f of selection + re-rank)  call %10.3f ms (%4.1f %%)  results / query %9.2f  "
                        "candidates beyond the answer %d"
                        % (nq, r, sc, 100 * sc_s, se, 100 * se_s, di, 100 * di_s, se + di, (se + di) / max(er, 1e-9), wa, 100 * wa_s,
                           st["results"] / nq, st["candidates"] - st["results"]))
    print(json.dumps(res, sort_keys=True))
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
