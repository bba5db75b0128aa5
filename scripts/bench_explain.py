#!/usr/bin/env python3
"""`morna explain`'s library call at bench_junctions.py's data set (synth.synthetic_intropolis, 50k samples,
70k junctions, ~1e8 entries).  Reports, as one JSON line and as text (kept in profiles/explain.txt):

  explain_N    morna_jstore_explain_by_sample for N = 1, 64, 1000 by-sample queries, each against its 20 unhashed neighbours,
               top 10: kernel time (HIP events; warm, the median of --repeats calls), pairs, store entries streamed, the
               algorithmic bytes (8 B per entry streamed) over kernel time, and the wall clock of the whole Python call
  longest      one query against the one row of the longest length the store has
  top_T        the 1000-query case at top = 1 and 64: what the list costs
  yardstick 1  morna_jstore_nearest_by_sample for the same queries with the same 20 results as each query's population, k = 20,
               a call per query: the re-rank's ordered sums for the same pairs, without the lists (kernel time: the search's
               and the row-norm pass's).  --parent-lib runs it in a process of its own on that build of the library (the
               parent commit's), else on this one: no kernel of nearest.hip differs between the two
  yardstick 2  the plain-Python restatement of the contract (tests/explain_ref.py) on the host for the pairs of one query and
               for the longest row, and whether the GPU's bytes are its bytes

    python3 scripts/bench_explain.py [--samples 50000] [--junctions 70000] [--parent-lib libmorna_hip.so] [--text out.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from morna_amd._lib import check, lib, ptr  # noqa: E402
from morna_amd.junctions import JunctionStore, line_weights, load_weights, save_weights  # noqa: E402

K, TOP = 20, 10


def say(what):
    sys.stderr.write("[bench_explain] %s\n" % what)
    sys.stderr.flush()


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def yardstick_nearest(store, queries, lists, repeats):
    """A call of nearest_by_sample per query, its results as the population: (kernel ms, wall ms), summed over the queries,
    the median of `repeats` rounds after a warm round."""
    kernel, wall = [], []
    for rnd in range(repeats + 1):
        k_ms, t0 = 0.0, time.perf_counter()
        for q, lst in zip(queries, lists):
            store.nearest_by_sample(np.asarray(lst, np.int64), [int(q)], len(lst))
            st = store.nearest_stats()
            k_ms += st["kernel_ms"] + st["norms_ms"]
        if rnd:
            kernel.append(k_ms)
            wall.append((time.perf_counter() - t0) * 1e3)
    return median(kernel), median(wall)


def yardstick_main(args):
    """The child of --parent-lib: the store and weights of the parent process, yardstick 1 on the library MORNA_LIB names."""
    import ctypes
    from morna_amd import _lib
    older = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(older, n)]:       # the parent's build lacks this commit's symbols
        del _lib.SIGNATURES[name]
    store = JunctionStore.load(args.yardstick_store)
    w, _, _ = load_weights(args.yardstick_store + ".w")
    store.set_weights(w)
    job = np.load(args.yardstick_store + ".npz")
    out = {}
    for n in (1, 64, 1000):
        n = min(n, len(job["queries"]))
        say("yardstick 1 at %d queries" % n)
        out[str(n)] = yardstick_nearest(store, job["queries"][:n], job["lists"][:n], args.repeats)
    out["longest"] = yardstick_nearest(store, job["queries"][:1], [[int(job["longest"])]], args.repeats)
    print("YARDSTICK " + json.dumps(out))


def render(res):
    """The text of a result (profiles/explain.txt)."""
    sizes = sorted(int(name.split("_")[1]) for name in res if name.startswith("explain_"))
    text = ["explain, %d samples x %d lines (%d with weight), %d entries, %d results per query, top %d; medians of %d warm calls "
            "(scripts/bench_explain.py)" % (res["n_samples"], res["n_lines"], res["weighted_lines"], res["nnz"], res["k"], res["top"],
                                            res["repeats"])]
    names = {"longest": "longest row (%d entries), 1 pair" % res["longest_row"], "top_1": "%d queries, top 1" % sizes[-1],
             "top_64": "%d queries, top 64" % sizes[-1]}
    names.update(("explain_%d" % n, "%d queries" % n) for n in sizes)
    for name in ["explain_%d" % n for n in sizes] + ["longest", "top_1", "top_64"]:
        r = res[name]
        text.append("%-34s kernels %.3f ms (%.3f to %.3f), %d pairs, %d passes of %d queries, %.1f MB streamed: %.1f GB/s, "
                    "%.2f us per pair; whole call %.1f ms" % (names[name], r["kernel_ms"], r["kernel_min_ms"], r["kernel_max_ms"], r["pairs"],
                                                              r["passes"], r["queries_per_pass"], 8 * r["entries"] / 1e6, r["GBps"],
                                                              1e3 * r["kernel_ms"] / max(r["pairs"], 1), r["wall_ms"]))
    for name in [str(n) for n in sizes] + ["longest"]:
        r, mine = res["nearest_%s" % name], res["longest" if name == "longest" else "explain_%s" % name]
        text.append("yardstick 1, %-21s nearest_by_sample per query, its results the population (%s): kernels %.3f ms, calls %.1f ms; "
                    "explain's kernels are %.2f x that" % (name + (" queries" if name != "longest" else " row"), res["yardstick_library"],
                                                           r["kernel_ms"], r["wall_ms"], mine["kernel_ms"] / r["kernel_ms"]))
    for name, what in (("host_1", "the %d pairs of one query" % res["host_1"]["pairs"]), ("host_longest", "the longest row")):
        h = res[name]
        text.append("yardstick 2, %-21s the Python restatement on the host %.1f ms; the GPU's bytes are its bytes: %s"
                    % (what, h["ms"], h["same_bytes"]))
    return "\n".join(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50_000)
    ap.add_argument("--junctions", type=int, default=70_000)
    ap.add_argument("--threshold", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="a build of libmorna_hip.so at the parent commit, for yardstick 1")
    ap.add_argument("--yardstick-store", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None)
    ap.add_argument("--text", default=None)
    ap.add_argument("--render", default=None, help="print the text of this earlier --json result and stop (no GPU)")
    args = ap.parse_args()
    if args.render is not None:
        with open(args.render) as fh:
            print(render(json.loads(fh.read())))
        return
    if args.yardstick_store is not None:
        return yardstick_main(args)
    from explain_ref import SUMS, bits, explain_pair
    from morna_amd.index import ParsedLines
    from morna_amd.synth import synthetic_intropolis
    res = dict(samples=args.samples, junctions=args.junctions, k=K, top=TOP, threshold=args.threshold, repeats=args.repeats)
    say("making the data set")
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
        parsed = ParsedLines(path, sample_count=args.samples, sample_threshold=0)
    w = line_weights(parsed, args.threshold)
    if w is None:
        raise SystemExit("the synthetic file repeats a junction: no weights")
    say("building the store")
    store = JunctionStore.build(parsed)
    del parsed, d
    store.set_weights(w)
    pop = store.sample_ids()
    res.update(n_samples=store.n_samples, n_lines=store.n_lines, nnz=store.nnz, weighted_lines=int((w != 0).sum()))
    rng = np.random.Generator(np.random.PCG64(21))
    n_most = min(1000, len(pop))
    queries = pop[rng.permutation(len(pop))][:n_most]
    say("searching the lists")
    ids, _, cnt = store.nearest_by_sample(pop, queries, K)                   # the lists: every query's unhashed neighbours
    lists = [pop[ids[q, :cnt[q]]].tolist() for q in range(n_most)]
    longest, longest_len = max(((int(s), len(store.sample(int(s))[0])) for s in pop.tolist()), key=lambda t: t[1])
    res["longest_row"] = longest_len
    sizes = sorted(set(min(n, n_most) for n in (1, 64, 1000)))

    def timed(q, lst, top):
        kernel, wall, got = [], [], None
        for rnd in range(args.repeats + 1):                                   # the first round warms this shape up
            t0 = time.perf_counter()
            got = store.explain_by_sample(q, lst, top)
            if rnd:
                wall.append((time.perf_counter() - t0) * 1e3)
                kernel.append(store.explain_stats()["kernel_ms"])
        st = store.explain_stats()
        return dict(kernel_ms=median(kernel), kernel_min_ms=min(kernel), kernel_max_ms=max(kernel), wall_ms=median(wall),
                    pairs=st["pairs"], entries=st["entries"], passes=st["passes"], queries_per_pass=st["queries_per_pass"],
                    GBps=st["bytes"] / median(kernel) / 1e6), got

    answers = {}
    say("explain")
    for n in sizes:
        res["explain_%d" % n], answers[n] = timed(queries[:n], lists[:n], TOP)
    res["longest"], answers["longest"] = timed(queries[:1], [[longest]], TOP)
    for top in (1, 64):
        res["top_%d" % top], _ = timed(queries[:sizes[-1]], lists[:sizes[-1]], top)

    # yardstick 1: the re-rank's ordered sums for the same pairs
    say("yardstick 1")
    if args.parent_lib:
        with tempfile.TemporaryDirectory() as tmp:
            base = os.path.join(tmp, "store.junc.mor")
            store.save(base)
            save_weights(base + ".w", w, args.samples, args.threshold)
            np.savez(base + ".npz", queries=queries, lists=np.array([lst + [lst[-1]] * (K - len(lst)) for lst in lists], np.int64),
                     longest=longest)
            env = dict(os.environ, MORNA_LIB=os.path.abspath(args.parent_lib))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--yardstick-store", base, "--repeats", str(args.repeats)],
                                 env=env, stdout=subprocess.PIPE, text=True, check=True, timeout=1500).stdout
        y = json.loads([t for t in out.splitlines() if t.startswith("YARDSTICK ")][0][len("YARDSTICK "):])
        res["yardstick_library"] = "parent build"
    else:
        y = {str(n): yardstick_nearest(store, queries[:n], lists[:n], args.repeats) for n in sizes}
        y["longest"] = yardstick_nearest(store, queries[:1], [[longest]], args.repeats)
        res["yardstick_library"] = "this build"
    for name, (k_ms, wall) in y.items():
        res["nearest_%s" % name] = dict(kernel_ms=k_ms, wall_ms=wall)

    # yardstick 2: the restatement on the host, and that the GPU's bytes are its bytes
    def host(q, lst, got):
        q_row = store.sample(int(q))
        rows = [store.sample(int(s)) for s in lst]
        t0 = time.perf_counter()
        want = [explain_pair(q_row[0], q_row[1], r[0], r[1], w, TOP) for r in rows]
        ms = (time.perf_counter() - t0) * 1e3
        same = all(all(bits(getattr(g, n)) == bits(x[n]) for n in SUMS) and g.lines.tolist() == x["lines"]
                   and [bits(t) for t in g.terms] == [bits(t) for t in x["terms"]] and g.cov_r.tolist() == x["cov_r"]
                   and (g.shared, g.n_q, g.n_r) == (x["shared"], x["n_q"], x["n_r"]) for g, x in zip(got, want))
        return dict(ms=ms, pairs=len(rows), same_bytes=bool(same))
    say("yardstick 2")
    res["host_1"] = host(queries[0], lists[0], answers[sizes[0]][0])
    res["host_longest"] = host(queries[0], [longest], answers["longest"][0])

    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    text = render(res)
    print(text)
    if args.text:
        with open(args.text, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
