#!/usr/bin/env python3
"""The kernels every form of the exact family launches (exact.hip), call by call, for comparing two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d out -o p -- python3 scripts/exact_launch_order.py
    python3 scripts/exact_launch_order.py --compare parent/.../p_kernel_trace.csv branch/.../p_kernel_trace.csv

One process.  On 9000 rows x 64 features (past the 8192 rows of the two-pass selection): the exact search of 1 query by
vector, 8 by item, 40 by vector (the matrix-core scan), the same 40 with MORNA_EXACT_SELECT2=0, 40 restricted with query
groups and 40 packed for the sharded merge; label_sums of 40 queries, 5 labels, plain and restricted; exact_radius of 40
queries plain, restricted, with `after`, and with MORNA_RADIUS_BATCH=7.  On 4096 rows: one exact search of 40 (the k-round
selection).  A small torch kernel separates the calls in the trace, as in query_launch_order.py, whose reader of the trace
this script uses.  --compare prints, per call, the (kernel, grid, workgroup, LDS) sequence of the first trace and whether the
second has the same.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import query_launch_order as qlo  # noqa: E402

CALLS = ["adding the rows", "exact, 1 by vector", "exact, 8 by item", "exact, 40 by vector", "exact, 40 by vector, SELECT2=0",
         "making the restriction", "exact, 40 restricted with query groups", "exact, 40 packed", "label_sums, 40", "label_sums, 40 restricted",
         "radius, 40", "radius, 40 restricted", "radius, 40 with after", "radius, 40, RADIUS_BATCH=7", "4096 rows: adding them",
         "4096 rows: exact, 40 by vector"]


def compare(a_path, b_path):
    """The sequence of every call of the first trace, then query_launch_order's verdict on the two, call by call."""
    for label, call in zip(CALLS + ["after the last call"], qlo.launches(a_path)):
        print(label)
        for t in call:
            print("    %-50s grid %-18s workgroup %-14s LDS %6d" % (t[0][:50], "x".join(map(str, t[1])), "x".join(map(str, t[2])), t[3]))
    qlo.CALLS = CALLS
    return qlo.compare(a_path, b_path)


def with_env(name, value, fn):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def main():
    import torch
    from morna_amd.annoy import AnnoyIndex
    N, D = 9000, 64
    rng = np.random.default_rng(950)
    X = rng.standard_normal((N, D)).astype(np.float32)
    items = np.linspace(0, N - 1, 40).astype(np.int32)
    X[5000:5040] = X[items] * (1 + np.float32(0.02) * rng.standard_normal((40, D)).astype(np.float32))   # (radius lists of two)
    Q = X[items].astype(np.float64)
    labels = (np.arange(N) % 5).astype(np.int32)
    q_groups = (items % 7).astype(np.int32)
    mark = torch.zeros(64, device="cuda")
    packed = torch.zeros(AnnoyIndex.exact_packed_bytes(40, 10), dtype=torch.uint8, device="cuda")

    def separate(a):
        a.synchronize()
        torch.cuda.synchronize()
        mark.add_(1.0)
        torch.cuda.synchronize()

    a = AnnoyIndex(D)
    a.add_items(X)
    separate(a)
    for call in (lambda: a.exact_search_batch(Q[:1], 10), lambda: a.exact_search_by_item_batch(items[:8], 10),
                 lambda: a.exact_search_batch(Q, 10), lambda: with_env("MORNA_EXACT_SELECT2", "0", lambda: a.exact_search_batch(Q, 10))):
        call()
        separate(a)
    r = a.restriction((np.arange(N) % 3) != 0, (np.arange(N) % 7).astype(np.int32))
    separate(a)
    for call in (lambda: a.exact_search_restricted(r, 10, Q=Q, query_groups=q_groups),
                 lambda: a.exact_search_packed(packed.data_ptr(), 10, 0, Q=Q),
                 lambda: a.label_sums(labels, 5, items=items),
                 lambda: a.label_sums(labels, 5, items=items, restriction=r, query_groups=q_groups),
                 lambda: a.exact_radius(0.5, items=items),
                 lambda: a.exact_radius(0.5, items=items, restriction=r, query_groups=q_groups),
                 lambda: a.exact_radius(0.5, items=items, after=items),
                 lambda: with_env("MORNA_RADIUS_BATCH", "7", lambda: a.exact_radius(0.5, items=items))):
        call()
        separate(a)
    b = AnnoyIndex(D)
    b.add_items(X[:4096])
    separate(b)
    b.exact_search_batch(Q, 10)
    separate(b)
    print("exact_launch_order: done")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main()
