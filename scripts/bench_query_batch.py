#!/usr/bin/env python3
"""Batch search of new query samples from an intropolis file at C3 scale: one seeded synthetic data set cut into a
50k-sample index (3000 features, 200 trees) and 1000 new query samples (synth.index_and_query_files).  Reports

  prepass_ms      host pre-pass: parse of the query file + morna_lines_query_terms (wall clock)
  features_ms     morna_build_query_rows on the GPU (HIP events, MORNA_T_FEATURES) and its wall clock
  approx_ms       morna_get_nns_by_query_rows, k=20, search_k=100, all queries in one call (device synchronised)
  exact_ms        morna_exact_search_query_rows, k=20, all queries in one call (device synchronised)
  one_by_one_*    the same 1000 queries as 1000 one-query calls in one process (get_nns_by_vector / exact_search)

    python3 scripts/bench_query_batch.py [--queries 1000] [--json out.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morna_amd.annoy import AnnoyIndex  # noqa: E402
from morna_amd.index import ParsedLines, pack_vocab, prepare_csr  # noqa: E402
from morna_amd.synth import index_and_query_files  # noqa: E402


def timed(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--dim", type=int, default=3000)
    ap.add_argument("--trees", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    res = dict(samples=args.samples, queries=args.queries, junctions=args.junctions, dim=args.dim, trees=args.trees)
    with tempfile.TemporaryDirectory() as tmp:
        qpath = os.path.join(tmp, "queries.tsv.gz")
        t0 = time.perf_counter()
        cut = index_and_query_files(None, qpath, args.samples, args.queries, J=args.junctions)
        res["synth_s"] = time.perf_counter() - t0
        d = cut["index"]
        prep = prepare_csr(d["keys"], d["row_ptr"], d["samples"], d["cov"], d["sample_count"], 100)
        a = AnnoyIndex(args.dim)
        a.stage_junctions(prep["key_bytes"], prep["key_off"], prep["row_ptr"], prep["ids"], prep["cov"], prep["idf"])
        a.stage_item_order(prep["ext_ids"])
        a.build_features(prep["n_items"])
        a.build(args.trees)
        a.unstage_junctions()
        a.synchronize()
        res["index_items"] = int(prep["n_items"])
        vocab = pack_vocab(prep["freq"])
        sc = int(d["sample_count"])

        def prepass():
            return ParsedLines(qpath, sample_count=sc, sample_threshold=0).query_terms(vocab, sc)
        res["prepass_ms"], T = timed(prepass, 3)
        res["query_lines"], res["query_nnz"] = T.n_lines, T.nnz
        res["query_samples"] = T.n_items
        a.build_query_rows(T)                                   # warm-up (allocations)
        a.timer_enable(True, only=["features"])
        a.timer_reset()
        res["features_wall_ms"], _ = timed(lambda: a.build_query_rows(T), 5)
        res["features_ms"] = a.timers()["features"]["ms"] / max(a.timers()["features"]["launches"], 1)
        a.timer_enable(False)
        r64, r32 = a.get_query_rows()
        a.get_nns_by_query_rows(20, 100)
        a.exact_search_query_rows(20)

        def approx():
            out = a.get_nns_by_query_rows(20, 100)
            a.synchronize()
            return out
        res["approx_ms"], batch_approx = timed(approx, 5)

        def exact():
            out = a.exact_search_query_rows(20)
            a.synchronize()
            return out
        res["exact_ms"], batch_exact = timed(exact, 5)

        # the same queries one call each, in one process (what a loop over `morna search` would do minus the process starts)
        def one_by_one_approx():
            for q in range(len(r32)):
                a.get_nns_by_vector_batch(r32[q:q + 1], 20, 100)
        res["one_by_one_approx_ms"], _ = timed(one_by_one_approx, 1)

        def one_by_one_exact():
            for q in range(len(r64)):
                a.exact_search_batch(r64[q:q + 1], 20)
        res["one_by_one_exact_ms"], _ = timed(one_by_one_exact, 1)
        # the batch answers are the one-query answers
        ids1 = np.stack([a.get_nns_by_vector_batch(r32[q:q + 1], 20, 100)[0][0] for q in range(0, len(r32), 50)])
        res["approx_matches_one_by_one"] = bool((ids1 == batch_approx[0][::50]).all())
        ide = np.stack([a.exact_search_batch(r64[q:q + 1], 20)[0][0] for q in range(0, len(r64), 50)])
        res["exact_matches_one_by_one"] = bool((ide == batch_exact[0][::50]).all())
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
