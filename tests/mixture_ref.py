"""numpy restatement of the label mixture contract (include/morna_hip.h, "label mixture"), shared by
test_mixture_cpu.py and the GPU tests.  Plain fp64: numpy multiplies and adds separately, so every product and every sum is
rounded once.  Where the order matters the loop is sequential in Python (over the columns for yy, t and S, over a label's
members for the sums, over the labels inside a sweep and inside the report) and numpy only vectorises across what is
independent: the queries, and the labels m that a step updates.  pp, sigma and the member sums come from kmeans_ref."""
import numpy as np

from kmeans_ref import ref_scales


def ref_pp(X):
    """pp_i: the sequential fp64 sum of squares of row i (the sum ref_scales takes its scales from)."""
    Xd = np.asarray(X, dtype=np.float32).astype(np.float64)
    pp = np.zeros(Xd.shape[0])
    with np.errstate(all="ignore"):
        for z in range(Xd.shape[1]):
            pp = pp + Xd[:, z] * Xd[:, z]
    return pp


def ref_label_centroids(X, item_label, L, allow=None):
    """(sums [L, D], counts int32 [L], S [L, L]): kmeans' update over the eligible members of every label, the unskipped
    members counted, and the Gram matrix summed over the columns in ascending order."""
    Xd = np.asarray(X, dtype=np.float32).astype(np.float64)
    item_label = np.asarray(item_label)
    ok, s = ref_scales(X)
    elig = np.ones(len(Xd), bool) if allow is None else np.asarray(allow, bool)
    sums, counts = np.zeros((L, Xd.shape[1])), np.zeros(L, np.int32)
    with np.errstate(all="ignore"):
        for l in range(L):
            acc = np.zeros(Xd.shape[1])
            for i in np.nonzero((item_label == l) & elig)[0]:
                if ok[i]:
                    acc = acc + Xd[i] * s[i]
                    counts[l] += 1
            sums[l] = acc
        S = np.zeros((L, L))
        for z in range(Xd.shape[1]):
            S = S + sums[:, z][:, None] * sums[:, z][None, :]
    return sums, counts, S


def ref_problem(X, item_label, L, Y=None, items=None, allow=None):
    """Everything of the contract in front of the solver, per query: dict(sums, counts, S, yy, t (unpatched), own (-1: no
    label is left out), Sq [nq, L, L], tq, mq, active, d, G [nq, L, L], b, valid)."""
    Xd = np.asarray(X, dtype=np.float32).astype(np.float64)
    item_label = np.asarray(item_label)
    sums, counts, S = ref_label_centroids(X, item_label, L, allow)
    ok, sig = ref_scales(X)
    pp = ref_pp(X)
    elig = np.ones(len(Xd), bool) if allow is None else np.asarray(allow, bool)
    if items is not None:
        items = np.asarray(items, np.int64)
        Y = Xd[items]
    Y = np.asarray(Y, dtype=np.float64)
    nq, D = Y.shape
    yy, t = np.zeros(nq), np.zeros((nq, L))
    with np.errstate(all="ignore"):
        for z in range(D):
            yy = yy + Y[:, z] * Y[:, z]
            t = t + sums[:, z][None, :] * Y[:, z][:, None]
        Sq = np.broadcast_to(S, (nq, L, L)).copy()
        tq, mq = t.copy(), np.broadcast_to(counts, (nq, L)).copy()
        own = np.full(nq, -1, np.int64)
        if items is not None:
            for q, i in enumerate(items):
                o = int(item_label[i])
                if o < 0 or not elig[i] or not ok[i]:
                    continue
                own[q] = o
                tau = t[q] * sig[i]
                row = S[o] - tau
                row[o] = (S[o, o] - 2.0 * tau[o]) + 1.0
                Sq[q, o, :] = row
                Sq[q, :, o] = row
                tq[q, o] = t[q, o] - pp[i] * sig[i]
                mq[q, o] -= 1
        diag = Sq[:, np.arange(L), np.arange(L)]
        active = (mq >= 1) & (diag > 0.0) & (diag < np.inf)
        d = np.sqrt(np.where(active, diag, 1.0))
        G = Sq / (d[:, :, None] * d[:, None, :])
        G[:, np.arange(L), np.arange(L)] = 1.0
        fit = (yy > 0.0) & (yy < np.inf)
        b = np.where(active, tq / (d * np.sqrt(np.where(fit, yy, 1.0))[:, None]), 0.0)
    return dict(sums=sums, counts=counts, S=S, yy=yy, t=t, own=own, Sq=Sq, tq=tq, mq=mq, active=active, d=d, G=G, b=b,
                valid=fit & active.any(axis=1))


def ref_solve(G, b, active, valid, tol, max_sweeps):
    """The solver and the report: (weights [nq, L], info [nq, 4] = rr, kkt, sweeps, status)."""
    nq, L = b.shape
    a, g = np.zeros((nq, L)), b.copy()
    running = valid.copy()
    sweeps, status = np.zeros(nq), np.where(valid, 0.0, -1.0)
    with np.errstate(all="ignore"):
        for s in range(1, int(max_sweeps) + 1):
            if not running.any():
                break
            mx = np.zeros(nq)
            for l in range(L):
                idx = np.nonzero(running & active[:, l])[0]
                if not len(idx):
                    continue
                delta = g[idx, l]
                lo = -a[idx, l]
                delta = np.where(delta < lo, lo, delta)
                step = np.abs(delta)
                mx[idx] = np.where(step > mx[idx], step, mx[idx])
                nz = delta != 0.0
                idx, delta = idx[nz], delta[nz]
                if len(idx):
                    a[idx, l] = a[idx, l] + delta
                    g[idx] = g[idx] - delta[:, None] * G[idx, l, :]     # (G is symmetric: row l is column l)
            sweeps[running] = s
            done = running & (mx <= tol)
            status[done] = 1.0
            running &= ~done
        h = np.zeros((nq, L))
        for m in range(L):
            on = active[:, m]
            h[on] = h[on] + G[on, m, :] * a[on, m][:, None]
        w = b - h
        k = np.where(a > 0.0, np.abs(w), np.where(w > 0.0, w, 0.0))
        kkt = np.max(np.where(active, k, 0.0), axis=1)
        u, v = np.zeros(nq), np.zeros(nq)
        for l in range(L):
            on = active[:, l]
            u[on] = u[on] + a[on, l] * h[on, l]
            v[on] = v[on] + a[on, l] * b[on, l]
        rr = (1.0 - 2.0 * v) + u
    weights = np.where(active & valid[:, None], a, 0.0)
    info = np.stack([np.where(valid, rr, 0.0), np.where(valid, kkt, 0.0), np.where(valid, sweeps, 0.0), status], axis=1)
    return weights, info


def ref_mixture(X, item_label, L, Y=None, items=None, allow=None, tol=1e-9, max_sweeps=10000):
    """The whole contract: (weights float64 [nq, L], info float64 [nq, 4], active bool [nq, L])."""
    P = ref_problem(X, item_label, L, Y=Y, items=items, allow=allow)
    weights, info = ref_solve(P["G"], P["b"], P["active"], P["valid"], tol, max_sweeps)
    return weights, info, P["active"]
