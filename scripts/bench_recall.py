#!/usr/bin/env python3
"""`morna recall`'s sweep at bench.py's data set: synthetic intropolis 50k samples x 3000 features, 200
trees, k = 20.  Batches of 1, 64 and 1000 by-item queries over the grid trees 10,20,50,100,200 x search_k
100,200,500,1000,4000.  Per batch size, each figure the median of `--repeats` calls after a warm-up call, with the spread
(max - min) / median, kernel time by HIP events (the library's `query` and `exact` timer groups) and the whole call on the
host clock:

  (a) the sweep, and recall_sweep (the exact search included); the sweep also with MORNA_SWEEP_FILTER=0, which takes the
      canonical dot of every candidate where the default filters on the fp16 scores of one whole-batch contraction;
  (b) the 25 separate tree-prefix calls, summed, for information;
  (c) the sweep of the column trees = 200 alone against the five plain get_nns_by_item_batch calls at those search_k, summed.

--baseline-only times only the five plain calls of (c) and needs none of the sweep's symbols, so that the parent commit's
library can be timed by the same script (MORNA_LIB=<its libmorna_hip.so>).  One JSON line, and text (profiles/recall.txt
is put together from the text of both).

    python3 scripts/bench_recall.py [--samples 50000] [--features 3000] [--trees 200] [--text out.txt] [--baseline-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("morna_get_nns_prefix", "morna_search_sweep", "morna_recall_sweep", "morna_search_sweep_stats")


def timed(a, groups, fn, repeats):
    """(median kernel ms, its spread, median wall ms, its spread) of `repeats` calls after one warm-up."""
    fn()
    a.synchronize()
    kernel, wall = [], []
    for _ in range(repeats):
        a.timer_reset()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        t = a.timers()
        kernel.append(sum(t[g]["ms"] for g in groups))
    km, wm = float(np.median(kernel)), float(np.median(wall))
    return km, (max(kernel) - min(kernel)) / km, wm, (max(wall) - min(wall)) / wm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--trees", type=int, default=200)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--grid-trees", default="10,20,50,100,200")
    ap.add_argument("--grid-search-ks", default="100,200,500,1000,4000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--text", default=None)
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    from morna_amd import _lib
    if args.baseline_only:   # a library from before the sweep: bind only what it exports
        import ctypes
        exported = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW_SYMBOLS:
            if name in _lib.SIGNATURES and not hasattr(exported, name):
                del _lib.SIGNATURES[name]
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
    a.build(args.trees, seed=0)
    n, k = a.get_n_items(), args.k
    trees = sorted(set(min(int(t), args.trees) for t in args.grid_trees.split(",")))
    sks = [int(s) for s in args.grid_search_ks.split(",")]
    items_all = np.random.Generator(np.random.PCG64(10)).permutation(n).astype(np.int32)[:1000]
    a.timer_enable(True, only=["query", "exact"])
    res = dict(samples=n, features=args.features, trees=args.trees, k=k, grid_trees=trees, grid_search_ks=sks,
               repeats=args.repeats, library=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
               baseline_only=args.baseline_only, cases={})
    text = ["recall sweep, %d samples x %d features, %d trees, k = %d, by-item queries; trees %s x search_k %s "
            "(scripts/bench_recall.py%s)" % (n, args.features, args.trees, k, args.grid_trees, args.grid_search_ks,
                                             " --baseline-only" if args.baseline_only else ""),
            "kernel ms by HIP events / whole call on the host clock, median of %d after a warm-up (spread = (max - min) / median)"
            % args.repeats]

    def report(nq, name, fn, groups=("query",)):
        km, ks, wm, ws = timed(a, groups, fn, args.repeats)
        res["cases"]["%d/%s" % (nq, name)] = dict(kernel_ms=km, kernel_spread=ks, wall_ms=wm, wall_spread=ws)
        text.append("%4d queries  %-46s kernels %10.4f ms (spread %5.1f %%)   call %10.4f ms (spread %5.1f %%)"
                    % (nq, name, km, 100 * ks, wm, 100 * ws))
        return km, wm

    for nq in (1, 64, 1000):
        items = items_all[:nq]
        report(nq, "(c) five plain calls, all %d trees, summed" % args.trees,
               lambda: [a.get_nns_by_item_batch(items, k, s) for s in sks])
        if args.baseline_only:
            continue
        report(nq, "(c) sweep of the column trees = %d alone" % args.trees, lambda: a.search_sweep(k, trees[-1:], sks, items=items))
        def unfiltered(fn):   # canonical dots for every candidate, whatever the batch (read per call by the library)
            os.environ["MORNA_SWEEP_FILTER"] = "0"
            try:
                return fn()
            finally:
                del os.environ["MORNA_SWEEP_FILTER"]
        report(nq, "(c) the same, MORNA_SWEEP_FILTER=0", lambda: unfiltered(lambda: a.search_sweep(k, trees[-1:], sks, items=items)))
        report(nq, "(a) sweep, MORNA_SWEEP_FILTER=0", lambda: unfiltered(lambda: a.search_sweep(k, trees, sks, items=items)))
        st0 = a.sweep_stats()
        text.append("              rows read by canonical dots per query: %.0f; contraction %d" % (st0["rows_canonical"] / float(nq), st0["contraction"]))
        report(nq, "(a) sweep, %d x %d cells" % (len(trees), len(sks)), lambda: a.search_sweep(k, trees, sks, items=items))
        st = a.sweep_stats()
        text.append("              rows read by canonical dots per query: %.0f; descents %d, cells %d, contraction %d"
                    % (st["rows_canonical"] / float(nq), st["descents"], st["cells"], st["contraction"]))
        res["cases"]["%d/stats" % nq] = st
        report(nq, "(a) recall_sweep (exact search included)", lambda: a.recall_sweep(k, trees, sks, items=items),
               groups=("query", "exact"))
        report(nq, "(b) %d separate tree-prefix calls, summed" % (len(trees) * len(sks)),
               lambda: [a.get_nns_by_item_batch(items, k, s, n_trees=t) for t in trees for s in sks])
        out = a.recall_sweep(k, trees, sks, items=items)
        ok = out["exact_count"] > 0
        recall = (out["hits"][:, :, ok] / out["exact_count"][ok].astype(np.float64)).mean(axis=2) if ok.any() else None
        if recall is not None:
            text.append("              mean recall (rows: trees %s; columns: search_k %s):" % (args.grid_trees, args.grid_search_ks))
            for i, t in enumerate(trees):
                text.append("              %5d  " % t + "  ".join("%.3f" % r for r in recall[i]))
    print(json.dumps(res, sort_keys=True))
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
