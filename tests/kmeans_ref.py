"""numpy restatements of the k-means contract (include/morna_hip.h, "spherical k-means"), shared by
test_kmeans_cpu.py and the GPU tests.  Plain fp64: numpy multiplies and adds separately, so every product and every sum is
rounded once, as the contract says.  ref_assign loops sequentially over the columns (cosine_distance's order), vectorised
over (row, centroid); ref_kmeans adds a cluster's members sequentially in ascending id, vectorised over the columns."""
import numpy as np


def ref_distances(X, Cn):
    """d[i, j] = cosine_distance(x_i, c_j) (morna.py:101-114): fp64 [n, k], NaN where math.sqrt would raise."""
    XT = np.ascontiguousarray(np.asarray(X, dtype=np.float32).astype(np.float64).T)     # [D, n]: a column is contiguous
    CT = np.ascontiguousarray(np.asarray(Cn, dtype=np.float64).T)                      # [D, k]
    D, n = XT.shape
    k = CT.shape[1]
    pp, qq, pq, tmp = np.zeros(n), np.zeros(k), np.zeros((n, k)), np.empty((n, k))
    with np.errstate(all="ignore"):
        for z in range(D):
            i, j = XT[z], CT[z]
            pp = pp + i * i
            qq = qq + j * j
            np.multiply(i[:, None], j[None, :], out=tmp)
            np.add(pq, tmp, out=pq)
        pp, qq = pp[:, None], qq[None, :]
        ppqq = pp * qq
        safe = np.where(ppqq > 0.0, ppqq, 1.0)
        distance = np.where(ppqq > 0.0, 2.0 - (2.0 * pq) / np.sqrt(safe), 2.0)
        return np.sqrt(distance)


def assign_from_distances(d, allow=None):
    """(assign int32 [n], dist fp64 [n]) from d [n, k]: the lowest j of the smallest distance, a NaN behind every number (all
    NaN: j = 0, the canonical NaN); -1 and -1.0 for a row that `allow` (booleans [n]) leaves out."""
    key = np.where(np.isnan(d), np.inf, d)
    a = np.argmin(key, axis=1).astype(np.int32)          # the first of equal keys
    dist = d[np.arange(len(a)), a]
    dist = np.where(np.isnan(dist), np.nan, dist)        # one NaN for all
    if allow is not None:
        allow = np.asarray(allow, bool)
        a = np.where(allow, a, -1).astype(np.int32)
        dist = np.where(allow, dist, -1.0)
    return a, dist


def ref_assign(X, Cn, allow=None):
    """One assignment of the contract: assign_from_distances(ref_distances(X, Cn), allow)."""
    return assign_from_distances(ref_distances(X, Cn), allow)


def ref_scales(X):
    """(ok, s): s_i = 1 / sqrt(pp_i) with pp_i the sequential sum of squares; ok_i: the member is not skipped."""
    Xd = np.asarray(X, dtype=np.float32).astype(np.float64)
    pp = np.zeros(Xd.shape[0])
    with np.errstate(all="ignore"):
        for z in range(Xd.shape[1]):
            pp = pp + Xd[:, z] * Xd[:, z]
        ok = (pp > 0.0) & (pp < np.inf)
        s = 1.0 / np.sqrt(np.where(ok, pp, 1.0))
    return ok, s


def ref_kmeans(X, seeds, max_iter, allow=None):
    """dict(assign, dist, centroids, sizes, iterations, converged) of the contract's loop."""
    Xd = np.asarray(X, dtype=np.float32).astype(np.float64)
    ok, s = ref_scales(X)
    Cn = Xd[np.asarray(seeds, np.int64)].copy()
    k = Cn.shape[0]
    prev, converged, t = None, False, 0
    while True:
        t += 1
        a, d = ref_assign(X, Cn, allow)
        if t > 1 and np.array_equal(a, prev):
            converged = True
            break
        if t == max_iter:
            break
        new = Cn.copy()
        with np.errstate(all="ignore"):
            for j in range(k):
                acc, any_member = np.zeros(Xd.shape[1]), False
                for i in np.nonzero(a == j)[0]:
                    if ok[i]:
                        acc = acc + Xd[i] * s[i]
                        any_member = True
                if any_member:
                    new[j] = acc
        prev, Cn = a, new
    sizes = np.array([(a == j).sum() for j in range(k)], np.int32)
    return dict(assign=a, dist=d, centroids=Cn, sizes=sizes, iterations=t, converged=converged)
