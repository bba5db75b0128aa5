#!/usr/bin/env python3
"""Spherical k-means at bench.py's data set: synthetic intropolis 50k samples x 3000 features, k = 8 / 64 /
1024, the seeds drawn as `morna cluster --seed 0` draws them, at most --iterations assignments.  Per case, by HIP events
(morna_kmeans_stats) and divided by the iterations run: the scan, the pick (pick, offsets, list), the resolve (fp64 chains and
the minimum) and the update (member lists and sums); the share of open rows, the chains per row, and the whole call on the
host clock -- each the best of three calls after a warm-up call, with the spread (max - min) / min of the three.  Last, the
one-giant-cluster case: k = 1, whose update is one dependent chain over all rows per column.  One JSON line, and text (kept
in profiles/kmeans.txt).

    python3 scripts/bench_kmeans.py [--samples 50000] [--features 3000] [--iterations 10] [--text out.txt]
"""
import argparse
import json
import os
import sys
import time


def best(values):
    return min(values), (max(values) - min(values)) / max(min(values), 1e-12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--text", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.index import prepare_csr
    from morna_amd.search import cluster_seed_items
    from morna_amd.synth import SEED, synthetic_intropolis
    data = synthetic_intropolis(args.samples, J=args.junctions, seed=SEED)
    prep = prepare_csr(data["keys"], data["row_ptr"], data["samples"], data["cov"], data["sample_count"], 100)
    a = AnnoyIndex(args.features)
    a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
    a.stage_item_order(prep["ext_ids"])
    a.build_features(prep["n_items"])
    a.unstage_junctions()
    n = a.get_n_items()
    res = dict(samples=n, features=args.features, max_iterations=args.iterations, cases={})
    text = ["spherical k-means, %d samples x %d features, at most %d assignments (scripts/bench_kmeans.py)" % (n, args.features, args.iterations),
            "ms per iteration by HIP events and the whole call on the host clock, best of 3 after a warm-up (spread = (max - min) / min)"]
    for k in (8, 64, 1024, 1):
        seeds = cluster_seed_items(range(n), k, 0)
        a.kmeans(seeds, args.iterations)                      # warm-up: workspace, code objects
        runs = []
        for _ in range(3):
            a.synchronize()
            t0 = time.perf_counter()
            out = a.kmeans(seeds, args.iterations)
            wall = (time.perf_counter() - t0) * 1e3
            runs.append((wall, a.kmeans_stats(), out))
        it = runs[0][1]["iterations"]
        case = dict(iterations=it, converged=bool(runs[0][2]["converged"]), largest=runs[0][1]["largest"],
                    open_share=runs[0][1]["open_rows"] / float(it * n), chains_per_row=runs[0][1]["chains"] / float(it * n))
        line = "k = %4d  iterations %3d%s  largest cluster %5d" % (k, it, " (converged)" if case["converged"] else "", case["largest"])
        for key in ("scan_ms", "pick_ms", "resolve_ms", "update_ms"):
            v, spread = best([r[1][key] / it for r in runs])
            case[key + "_per_iteration"], case[key + "_spread"] = v, spread
            line += "  %s %8.3f ms (%4.1f %%)" % (key[:-3], v, 100 * spread)
        v, spread = best([r[0] for r in runs])
        case["call_ms"], case["call_spread"] = v, spread
        line += "  call %9.3f ms (%4.1f %%)  open rows %5.2f %%  chains / row %.3f" % (
            v, 100 * spread, 100 * case["open_share"], case["chains_per_row"])
        assert all(r[2]["assign"].tobytes() == runs[0][2]["assign"].tobytes() and r[2]["centroids"].tobytes() == runs[0][2]["centroids"].tobytes()
                   for r in runs), "two calls differ"
        res["cases"]["k%d" % k] = case
        text.append(line)
    giant = res["cases"]["k1"]
    text.append("k = 1 is the one-giant-cluster case: every column's sum is one dependent fp64 chain over all %d rows; member lists and "
                "update of the call: %.1f ms" % (n, giant["update_ms_per_iteration"] * giant["iterations"]))
    print(json.dumps(res))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")
    else:
        sys.stderr.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
