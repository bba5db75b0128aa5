#!/usr/bin/env python3
"""Restricted search at bench.py's data set: synthetic intropolis 50k samples x 3000 features, 200 trees,
k = 20 (BASELINE.json configs[2]).  Times 1, 64 and 1000 by-item queries, approximate (search_k = 100, bench.py's) and exact,
for: the unrestricted call; an all-ones allow-list; allow fractions 0.5, 0.1 and 0.01; and 1000 leave-out groups of 50, every
query carrying its own sample's group.  Per case: the kernel time of the call by HIP events (the library's `query` / `exact`
timer groups) and the whole call on the host clock, each the best of three after a warm-up call, with the spread
(max - min) / min of the three.  The all-ones case against the unrestricted one is the cost of the mechanism: its ratio is
printed beside the unrestricted case's own spread; the lone approximate query is timed once more at a search_k the first
leaf does not end, where neither call takes the uncopied first leaf.  One JSON line, and text (kept in profiles/restricted.txt).

    python3 scripts/bench_restricted.py [--samples 50000] [--features 3000] [--trees 200] [--text out.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morna_amd.annoy import AnnoyIndex  # noqa: E402
from morna_amd.index import prepare_csr  # noqa: E402
from morna_amd.synth import SEED, synthetic_intropolis  # noqa: E402


def timed(a, group, fn, repeats=3):
    """(best kernel ms, its spread, best wall ms, its spread) of `repeats` calls after one warm-up."""
    fn()
    a.synchronize()
    kernel, wall = [], []
    for _ in range(repeats):
        a.timer_reset()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(a.timers()[group]["ms"])
    return min(kernel), (max(kernel) - min(kernel)) / min(kernel), min(wall), (max(wall) - min(wall)) / min(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--trees", type=int, default=200)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--search-k", type=int, default=100)
    ap.add_argument("--text", default=None)
    args = ap.parse_args()
    data = synthetic_intropolis(args.samples, J=args.junctions, seed=SEED)
    prep = prepare_csr(data["keys"], data["row_ptr"], data["samples"], data["cov"], data["sample_count"], 100)
    a = AnnoyIndex(args.features)
    a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
    a.stage_item_order(prep["ext_ids"])
    a.build_features(prep["n_items"])
    a.unstage_junctions()
    a.build(args.trees, seed=0)
    n, k = a.get_n_items(), args.k
    rng = np.random.Generator(np.random.PCG64(10))
    items_all = rng.permutation(n).astype(np.int32)[:1000]
    group = (rng.permutation(n) // 50).astype(np.int32)          # n / 50 groups of 50 (1000 at 50k)
    cases = [("unrestricted", None, False), ("allow all", a.restriction(np.ones(n, bool)), False)]
    for frac in (0.5, 0.1, 0.01):
        cases.append(("allow %g" % frac, a.restriction(rng.random(n) < frac), False))
    cases.append(("%d groups of 50" % (n // 50), a.restriction(None, group), True))
    a.timer_enable(True, only=["query", "exact"])
    res = dict(samples=n, features=args.features, trees=args.trees, k=k, search_k=args.search_k, cases={})
    text = ["restricted search, %d samples x %d features, %d trees, k = %d, by-item queries; approximate search_k = %d "
            "(scripts/bench_restricted.py)" % (n, args.features, args.trees, k, args.search_k),
            "kernel ms by HIP events / whole call on the host clock, best of 3 after a warm-up (spread = (max - min) / min)"]
    for kind, timer in (("approximate", "query"), ("exact", "exact")):
        for nq in (1, 64, 1000):
            items = items_all[:nq]
            base = None
            for name, r, own in cases:
                qg = group[items] if own else None
                if kind == "approximate":
                    fn = ((lambda: a.get_nns_by_item_batch(items, k, args.search_k)) if r is None else
                          (lambda: a.get_nns_restricted(r, k, args.search_k, items=items, query_groups=qg)))
                else:
                    fn = ((lambda: a.exact_search_by_item_batch(items, k)) if r is None else
                          (lambda: a.exact_search_restricted(r, k, items=items, query_groups=qg)))
                km, ks, wm, ws = timed(a, timer, fn)
                if r is None:
                    base = (km, wm)
                res["cases"]["%s/%d/%s" % (kind, nq, name)] = dict(kernel_ms=km, kernel_spread=ks, wall_ms=wm, wall_spread=ws)
                text.append("%-11s %4d queries  %-18s kernels %9.4f ms (spread %5.1f %%, x%.3f of unrestricted)   call %9.4f ms "
                            "(spread %5.1f %%, x%.3f)" % (kind, nq, name, km, 100 * ks, km / base[0], wm, 100 * ws, wm / base[1]))
    # the lone query again at a search_k the first leaf does not end: no call takes the uncopied first leaf, so the all-ones
    # case against the unrestricted one is the seeding of the bitmap alone
    deep = 2 * (args.features + 2) + args.search_k
    items = items_all[:1]
    base = None
    for name, r, _ in cases[:2]:
        fn = ((lambda: a.get_nns_by_item_batch(items, k, deep)) if r is None else
              (lambda: a.get_nns_restricted(r, k, deep, items=items)))
        km, ks, wm, ws = timed(a, "query", fn)
        base = base or (km, wm)
        res["cases"]["approximate_deep/1/%s" % name] = dict(kernel_ms=km, kernel_spread=ks, wall_ms=wm, wall_spread=ws, search_k=deep)
        text.append("approximate    1 queries  %-18s kernels %9.4f ms (spread %5.1f %%, x%.3f of unrestricted)   call %9.4f ms "
                    "(spread %5.1f %%, x%.3f)   search_k = %d: past the first leaf" % (name, km, 100 * ks, km / base[0], wm, 100 * ws,
                                                                                       wm / base[1], deep))
    print(json.dumps(res, sort_keys=True))
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
