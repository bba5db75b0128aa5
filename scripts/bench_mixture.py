#!/usr/bin/env python3
"""The label mixture at bench.py's data set: synthetic intropolis 50k samples x 3000 features, the labels the
clusters of `morna cluster --seed 0` (k = 2 / 64 / 128, at most 5 assignments), 1 / 64 / 1000 / all by-item queries.  Per case,
by HIP events (morna_mixture_stats): the centroid step (member lists and sums), the Gram (transpose, Gram, normalisation), the
query dots (staging and dots) and the solver; the sweeps (mean and largest), the queries that did not converge, and the whole
call on the host clock -- each the best of three calls after a warm-up call, with the spread (max - min) / min of the three.
The rate of the dots kernel is given in multiply-add pairs per second against the fp64 vector peak.  For scale: numpy
(BLAS dots) plus scipy.optimize.nnls on the host over a bounded sample of the same queries.  One JSON line, and text (kept in
profiles/mixture.txt).

    python3 scripts/bench_mixture.py [--samples 50000] [--features 3000] [--host-queries 64] [--text out.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

FP64_VECTOR_PEAK = 78.6e12      # flop/s of the MI355X's vector ALUs in fp64, a fused multiply-add counted as two


def best(values):
    return min(values), (max(values) - min(values)) / max(min(values), 1e-12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--host-queries", type=int, default=64)
    ap.add_argument("--tolerance", type=float, default=1e-9)
    ap.add_argument("--max-sweeps", type=int, default=10000)
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
    n, D = a.get_n_items(), args.features
    res = dict(samples=n, features=D, tolerance=args.tolerance, max_sweeps=args.max_sweeps, cases={})
    text = ["label mixture, %d samples x %d features, tol %g, at most %d sweeps (scripts/bench_mixture.py)" % (n, D, args.tolerance, args.max_sweeps),
            "labels: the clusters of k-means from `cluster --seed 0` seeds after at most 5 assignments; queries by item",
            "ms by HIP events and the whole call on the host clock, best of 3 after a warm-up (spread = (max - min) / min)"]
    X = None
    for L in (2, 64, 128):
        lab = a.kmeans(cluster_seed_items(range(n), L, 0), 5)["assign"]
        for nq in (1, 64, 1000, n):
            items = np.arange(n, dtype=np.int32) if nq == n else np.random.RandomState(nq).choice(n, nq, replace=False).astype(np.int32)
            a.mixture(lab, L, items=items, tol=args.tolerance, max_sweeps=args.max_sweeps)       # warm-up: workspace, code objects
            runs = []
            for _ in range(3):
                a.synchronize()
                t0 = time.perf_counter()
                w, info, _ = a.mixture(lab, L, items=items, tol=args.tolerance, max_sweeps=args.max_sweeps)
                runs.append(((time.perf_counter() - t0) * 1e3, a.mixture_stats()))
            case = dict(mean_sweeps=float(info[:, 2].mean()), max_sweeps=int(info[:, 2].max()), open=int((info[:, 3] != 1).sum()),
                        mixed_share=float(np.mean([(np.sort(x)[-2] if L > 1 else 0.0) >= 0.1 * x.sum() > 0 for x in w])))
            line = "L = %3d  queries %5d  sweeps mean %.1f max %d  not converged %d" % (L, nq, case["mean_sweeps"], case["max_sweeps"], case["open"])
            for key in ("centroids_ms", "gram_ms", "dots_ms", "solve_ms"):
                case[key], case[key + "_spread"] = best([r[1][key] for r in runs])
                line += "  %s %.3f (%.0f%%)" % (key[:-3], case[key], 100 * case[key + "_spread"])
            case["call_ms"], case["call_spread"] = best([r[0] for r in runs])
            case["dots_pairs_per_s"] = nq * float(D) * L / (case["dots_ms"] * 1e-3)
            line += "  call %.2f (%.0f%%)  dots %.3g pairs/s = %.2f%% of the fp64 vector peak" % (
                case["call_ms"], 100 * case["call_spread"], case["dots_pairs_per_s"], 100 * 2 * case["dots_pairs_per_s"] / FP64_VECTOR_PEAK)
            res["cases"]["L%d_q%d" % (L, nq)] = case
            text.append(line)
            print(line, file=sys.stderr, flush=True)            # (progress: the cases of 50 000 queries take their time)
        # the host, for scale: the same fit of a bounded sample of queries with numpy and scipy.optimize.nnls
        from scipy.optimize import nnls
        if X is None:
            X = a.get_items().astype(np.float64)
        hq = np.random.RandomState(7).choice(n, min(args.host_queries, n), replace=False)
        t0 = time.perf_counter()
        unit = X / np.sqrt((X * X).sum(axis=1))[:, None]
        cent = np.stack([unit[lab == l].sum(axis=0) for l in range(L)])
        t_cent = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for i in hq:
            c = cent.copy()
            c[lab[i]] -= unit[i]
            norm = np.sqrt((c * c).sum(axis=1))
            nnls((c / np.where(norm > 0, norm, 1.0)[:, None]).T, unit[i], maxiter=30 * L)
        t_fit = (time.perf_counter() - t0) * 1e3 / len(hq)
        res["cases"]["L%d_host" % L] = dict(centroids_ms=t_cent, per_query_ms=t_fit, queries=len(hq))
        text.append("L = %3d  host (numpy + scipy.optimize.nnls, %d queries): centroids %.1f ms, %.3f ms per query" % (L, len(hq), t_cent, t_fit))
    print(json.dumps(res))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")
    else:
        print("\n".join(text))


if __name__ == "__main__":
    main()
