#!/usr/bin/env python3
"""The kernels every form of the approximate search launches, call by call, for comparing two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d out -o p -- python3 scripts/query_launch_order.py
    python3 scripts/query_launch_order.py --compare parent/.../p_kernel_trace.csv branch/.../p_kernel_trace.csv

One process, one call of each form on 16640 rows x 256 features, 40 trees (the first shape of tests/test_gpu_build_tail.py,
whose build returns with its last levels pending): 1024 queries by vector as the first call after build() (the contraction
beside the build's tail; MORNA_DEBUG_OPEN=1 makes the library say so), then 1 and 8 by item and 8 by vector (the spread
form), 100 by item (the gather filter), 1024 by item (the whole-batch contraction with the large tiles), one restricted
call and one sweep of 200 queries.  A small torch kernel separates the calls in the trace.  --compare prints, per call,
the (kernel, grid, workgroup, LDS) sequence in dispatch order of both traces and whether they agree.
"""
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CALLS = ["build", "1024 by vector, first call after build()", "1 by item", "8 by item", "8 by vector", "100 by item, search_k 100",
         "1024 by item", "making the restriction", "100 by item, restricted", "sweep of 200 by item"]


def name_of(raw):
    n = raw.split("(")[0].replace("void ", "")
    if n.startswith("_ZN5morna"):   # a name rocprofv3 left mangled: _ZN5morna<len><name>...
        rest = n[len("_ZN5morna"):]
        digits = "".join(ch for ch in rest[:3] if ch.isdigit())
        n = "morna::" + rest[len(digits):len(digits) + int(digits)]
    return n


def launches(path):
    """[[(name, grid, workgroup, lds), ...] per call] of a rocprofv3 kernel trace, in dispatch order."""
    rows = list(csv.DictReader(open(path)))
    order = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[order]))

    def dims(r, what):
        return tuple(int(r[what + "_" + ax]) for ax in "XYZ") if what + "_X" in r else (int(r[what]),)

    calls = [[]]
    for r in rows:
        name = name_of(r["Kernel_Name"])
        if "morna" not in name:
            if "FunctorOnSelf_add" in name:   # the separator
                calls.append([])
            continue
        calls[-1].append((name.replace("morna::", ""), dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), int(r["LDS_Block_Size"])))
    return calls


def compare(a_path, b_path):
    a, b = launches(a_path), launches(b_path)
    print("calls: %d and %d" % (len(a), len(b)))
    same_all = len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        label = CALLS[i] if i < len(CALLS) else "after the last call"
        queries = [t for t in x if t[0].startswith(("query_", "sweep_", "pack_topk"))] if i > 0 else []
        verdict = "same" if x == y else ("same launches, another order" if sorted(x) == sorted(y) else "DIFFERENT")
        same_all = same_all and x == y
        print("%-45s %4d and %4d launches: %s" % (label, len(x), len(y), verdict))
        for t in queries:
            print("    %-50s grid %-18s workgroup %-14s LDS %6d" % (t[0][:50], "x".join(map(str, t[1])), "x".join(map(str, t[2])), t[3]))
        if x != y:
            for t, u in zip(x, y):
                if t != u:
                    print("    first difference: %r / %r" % (t, u))
                    break
    print("every call launches the same sequence" if same_all else "the traces differ")
    return 0 if same_all else 1


def main():
    import torch
    from morna_amd.annoy import AnnoyIndex
    N, D, T = 16640, 256, 40
    rng = np.random.default_rng(2027 + D)   # the rows of tests/test_gpu_level_turnaround.py
    C = rng.standard_normal((5, D)).astype(np.float32)
    X = C[rng.integers(0, 5, N)] + np.float32(0.25) * rng.standard_normal((N, D), dtype=np.float32)
    X *= (10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
    items = np.linspace(0, N - 1, 1024).astype(np.int32)
    Q = np.ascontiguousarray(X[items])
    mark = torch.zeros(64, device="cuda")

    def separate(a):
        a.synchronize()
        torch.cuda.synchronize()
        mark.add_(1.0)
        torch.cuda.synchronize()

    a = AnnoyIndex(D)
    a.add_items(X)
    a.build(T)
    torch.cuda.synchronize()   # (not the handle: its synchronize() would finish the pending tail)
    mark.add_(1.0)
    torch.cuda.synchronize()
    a.get_nns_by_vector_batch(Q, 10, 100)
    separate(a)
    for call in (lambda: a.get_nns_by_item_batch(items[:1], 20, 100), lambda: a.get_nns_by_item_batch(items[:8], 20, 100),
                 lambda: a.get_nns_by_vector_batch(Q[:8], 20, 100), lambda: a.get_nns_by_item_batch(items[:100], 20, 100),
                 lambda: a.get_nns_by_item_batch(items, 20, 100)):
        call()
        separate(a)
    r = a.restriction((np.arange(N) % 3) != 0, (np.arange(N) % 7).astype(np.int32))
    separate(a)   # (whatever making the restriction launches: a segment of its own)
    a.get_nns_restricted(r, 20, 100, items=items[:100], query_groups=(np.arange(100) % 7).astype(np.int32))
    separate(a)
    a.search_sweep(20, (10, 40), (100, 1000), items=items[:200])
    separate(a)
    print("query_launch_order: done")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
