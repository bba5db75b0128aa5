#!/usr/bin/env python3
"""What the feature hashing costs in neighbours: recall@k of the approximate search (forest, --search-k) and of the exact
search in the hashed space against the unhashed TF-IDF answer, on synth.synthetic_intropolis data,
by-item queries.  The query itself (distance ~0 in every space) is left out of both lists.

    python3 scripts/recall_vs_unhashed.py [--samples 5000] [--junctions 20000] [--features 3000] [--queries 1000] [--text out.txt]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from morna_amd._lib import check, lib, ptr  # noqa: E402
from morna_amd.index import go_index  # noqa: E402
from morna_amd.search import MornaSearch  # noqa: E402
from morna_amd.synth import query_items, synthetic_intropolis  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--junctions", type=int, default=20_000)
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--trees", type=int, default=200)
    ap.add_argument("--threshold", type=int, default=100)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--search-k", type=int, default=100)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--text", default=None)
    args = ap.parse_args()
    d = synthetic_intropolis(args.samples, J=args.junctions)
    with tempfile.TemporaryDirectory() as tmp:
        path, base = os.path.join(tmp, "index.tsv"), os.path.join(tmp, "idx")
        keys = [k.encode("ascii") for k in d["keys"]]
        key_off = np.zeros(len(keys) + 1, np.int64)
        key_off[1:] = np.cumsum([len(k) for k in keys])
        check(lib().morna_write_intropolis(path.encode(), ptr(np.frombuffer(b"".join(keys), np.uint8)), ptr(key_off), len(keys),
                                           ptr(d["row_ptr"]), ptr(np.ascontiguousarray(d["samples"], np.int64)),
                                           ptr(np.ascontiguousarray(d["cov"], np.int32))))
        go_index(path, base, args.features, args.trees, args.samples, args.threshold, 1024, False, None, native=True,
                 junction_store=True)
        s = MornaSearch(base)
        inv = s._inverse_map()
        items = query_items(s.index_size, args.queries)
        k1 = args.k + 1
        approx, _, _ = s.annoy_index.get_nns_by_item_batch(items, k1, args.search_k)
        exact, _, _ = s.annoy_index.exact_search_by_item_batch(items, k1)
        unhashed = s.unhashed_search_member_n_batch([inv[int(i)] for i in items], k1, include_distances=False)

    def others(row, me):
        return [int(x) for x in row if int(x) != me and int(x) >= 0][:args.k]

    hits = {"approximate": 0, "exact": 0}
    total = 0
    for q, me in enumerate(items.tolist()):
        truth = set(others(unhashed[q][0], me))
        total += len(truth)
        hits["approximate"] += len(truth & set(others(approx[q], me)))
        hits["exact"] += len(truth & set(others(exact[q], me)))
    res = dict(samples=args.samples, junctions=args.junctions, features=args.features, trees=args.trees, search_k=args.search_k,
               k=args.k, queries=len(items), threshold=args.threshold,
               recall_approximate=hits["approximate"] / total, recall_exact_hashed=hits["exact"] / total)
    print(json.dumps(res, sort_keys=True))
    text = ["recall@%d against the unhashed TF-IDF neighbours, %d by-item queries, %d samples x %d junctions (threshold %d), "
            "%d features, %d trees (scripts/recall_vs_unhashed.py)" % (args.k, len(items), args.samples, args.junctions, args.threshold,
                                                                      args.features, args.trees),
            "approximate search (--search-k %d)   %.4f" % (args.search_k, res["recall_approximate"]),
            "exact search in the hashed space      %.4f" % res["recall_exact_hashed"]]
    print("\n".join(text))
    if args.text:
        with open(args.text, "w") as fh:
            fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
