#!/usr/bin/env python3
"""Principal axes at bench.py's data set: synthetic intropolis 50k samples x 3000 features, p = 2 / 10 /
32 with 8 extra columns, tol 1e-9.  Per case, by HIP events (morna_pca_stats) and divided by the iterations run: the T pass,
the Y pass, the orthonormalisation, the small products and the host's eigen step; the iterations, the whole call on the host
clock and the bytes of rows read per second of the two row passes -- each the best of three calls after a warm-up call, with
the spread (max - min) / min of the three.  One line at --wide-features (random rows of --wide-samples x 16384: the widest
form of the row kernels).  Beside them the host route: morna_get_items, then numpy.linalg.eigh of the fp64 covariance of the
same unit rows -- its time and the largest |theta_j - lambda_j| / lambda_0 against the GPU's values.  One JSON line, and text
(kept in profiles/pca.txt).

    python3 scripts/bench_pca.py [--samples 50000] [--features 3000] [--max-iterations 500] [--text out.txt]
"""
import argparse
import json
import os
import sys
import time


def best(values):
    return min(values), (max(values) - min(values)) / max(min(values), 1e-12)


def run_case(a, p, extra, max_iterations):
    a.pca(p, extra=extra, max_iterations=2)                  # warm-up: workspace, code objects
    runs = []
    for _ in range(3):
        a.synchronize()
        t0 = time.perf_counter()
        out = a.pca(p, extra=extra, tol=1e-9, max_iterations=max_iterations)
        wall = (time.perf_counter() - t0) * 1e3
        runs.append((wall, a.pca_stats(), out))
    assert all(r[2]["axes"].tobytes() == runs[0][2]["axes"].tobytes() and r[2]["values"].tobytes() == runs[0][2]["values"].tobytes()
               for r in runs), "two calls differ"
    it = runs[0][1]["iterations"]
    case = dict(iterations=it, converged=bool(runs[0][2]["converged"]), fitted=runs[0][1]["fitted"])
    line = "p = %2d  b = %2d  iterations %3d%s" % (p, p + extra, it, " (converged)" if case["converged"] else "")
    for key in ("t_ms", "y_ms", "orth_ms", "small_ms", "eig_ms"):
        v, spread = best([r[1][key] / it for r in runs])
        case[key + "_per_iteration"], case[key + "_spread"] = v, spread
        line += "  %s %7.3f ms (%4.1f %%)" % (key[:-3], v, 100 * spread)
    v, spread = best([r[0] for r in runs])
    case["call_ms"], case["call_spread"] = v, spread
    pass_bytes = 4.0 * a.f * case["fitted"] * 2                # T and Y of one iteration
    case["row_gb_per_s"] = pass_bytes / ((case["t_ms_per_iteration"] + case["y_ms_per_iteration"]) * 1e-3) / 1e9
    line += "  call %9.3f ms (%4.1f %%)  rows read %7.1f GB/s" % (v, 100 * spread, case["row_gb_per_s"])
    return case, line, runs[0][2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--max-iterations", type=int, default=500)
    ap.add_argument("--wide-samples", type=int, default=50_000)
    ap.add_argument("--wide-features", type=int, default=16384)
    ap.add_argument("--wide-iterations", type=int, default=5)
    ap.add_argument("--text", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
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
    res = dict(samples=n, features=args.features, max_iterations=args.max_iterations, cases={})
    text = ["principal axes, %d samples x %d features, 8 extra columns, tol 1e-9 (scripts/bench_pca.py)" % (n, args.features),
            "ms per iteration by HIP events and the whole call on the host clock, best of 3 after a warm-up (spread = (max - min) / min)"]
    values = {}
    for p in (2, 10, 32):
        case, line, out = run_case(a, p, 8, args.max_iterations)
        res["cases"]["p%d" % p] = case
        values[p] = out["values"]
        text.append(line)
        sys.stderr.write(line + "\n")
    # the host route: the rows back, the covariance of the unit rows and its eigenvalues
    t0 = time.perf_counter()
    X = a.get_items().astype(np.float64)
    t1 = time.perf_counter()
    pp = (X * X).sum(axis=1)
    ok = (pp > 0) & np.isfinite(pp)
    Uf = X[ok] / np.sqrt(pp[ok])[:, None]
    dev = Uf - Uf.mean(axis=0)
    lam = np.linalg.eigh(dev.T @ dev / len(Uf))[0][::-1]
    t2 = time.perf_counter()
    host = dict(get_items_ms=(t1 - t0) * 1e3, eigh_ms=(t2 - t1) * 1e3)
    for p in (2, 10, 32):
        host["disagreement_p%d" % p] = float(np.max(np.abs(values[p] - lam[:p])) / lam[0])
    res["host"] = host
    sys.stderr.write("host route done\n")
    text.append("host route: morna_get_items %.1f ms, covariance and numpy.linalg.eigh %.1f ms; max |theta - lambda| / lambda_0: "
                "p = 2 %.2e, p = 10 %.2e, p = 32 %.2e" % (host["get_items_ms"], host["eigh_ms"], host["disagreement_p2"],
                                                          host["disagreement_p10"], host["disagreement_p32"]))
    del a, X, Uf, dev
    # the widest form: random rows, a fixed number of iterations
    rng = np.random.default_rng(SEED)
    wide = AnnoyIndex(args.wide_features)
    step = 4096
    for i0 in range(0, args.wide_samples, step):
        rows = rng.standard_normal((min(step, args.wide_samples - i0), args.wide_features)).astype(np.float32)
        rows[:, :16] += 3.0 * (np.arange(i0, i0 + len(rows)) % 4 == 0)[:, None]
        wide.add_items(rows, first_id=i0)
    case, line, _ = run_case(wide, 10, 8, args.wide_iterations)
    res["cases"]["wide"] = dict(case, samples=args.wide_samples, features=args.wide_features)
    text.append("%d random samples x %d features, at most %d iterations:" % (args.wide_samples, args.wide_features, args.wide_iterations))
    text.append(line)
    print(json.dumps(res))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")
    else:
        sys.stderr.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
