"""numpy restatement of the principal-axes contract (include/morna_hip.h, "principal axes"), shared by
test_pca_cpu.py and the GPU tests.  Plain fp64: numpy multiplies and adds separately, so every product and every sum is
rounded once, as the contract says.  Every sum is BS, the blocked ascending sum: bs() walks the 256 places of a block one by
one, vectorised over the blocks and over every other axis, then adds the blocks' partials one by one."""
import numpy as np

from kmeans_ref import ref_scales

BLOCK = 256
MAX_COMPONENTS = 32
MAX_BLOCK = 64
JACOBI_SWEEPS = 64
MASK64 = (1 << 64) - 1


class PcaRefused(ValueError):
    """The calls the contract answers with MORNA_E_INVALID."""


def bs(terms, axis=-1):
    """BS of `terms` along `axis`: per block of 256 indices the terms added in ascending order from 0.0, then the blocks'
    partials added in ascending order from 0.0."""
    t = np.moveaxis(np.asarray(terms, dtype=np.float64), axis, 0)
    n = t.shape[0]
    nblk = (n + BLOCK - 1) // BLOCK
    part = np.zeros((nblk,) + t.shape[1:])
    for k in range(min(BLOCK, n)):
        sl = t[k::BLOCK]
        part[:sl.shape[0]] = part[:sl.shape[0]] + sl
    out = np.zeros(t.shape[1:])
    for blk in range(nblk):
        out = out + part[blk]
    return out


def bs_dot(A, B):
    """BS_z(A[z][j] * B[z][k]) -> [ja, kb], without the [dim, ja, kb] array of terms."""
    dim, ja = A.shape
    kb = B.shape[1]
    nblk = (dim + BLOCK - 1) // BLOCK
    part = np.zeros((nblk, ja, kb))
    for k in range(min(BLOCK, dim)):
        a, b = A[k::BLOCK], B[k::BLOCK]
        part[:a.shape[0]] = part[:a.shape[0]] + a[:, :, None] * b[:, None, :]
    out = np.zeros((ja, kb))
    for blk in range(nblk):
        out = out + part[blk]
    return out


def mix(x):
    """The splitmix64 finaliser, on a Python int below 2^64."""
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK64
    x ^= x >> 31
    return x


def start_matrix(dim, b, seed):
    """G[z][j] of the contract."""
    base = (int(seed) * 0x9E3779B97F4A7C15) & MASK64
    G = np.empty((dim, b))
    for z in range(dim):
        for j in range(b):
            G[z, j] = float(mix((base + 64 * z + j) & MASK64) >> 11) * 2.0 ** -53 - 0.5
    return G


def orth(A):
    """Orth(A): classical Gram-Schmidt applied twice, column by column."""
    dim, b = A.shape
    Q = np.zeros((dim, b))
    for j in range(b):
        a = A[:, j].copy()
        if j > 0:
            for _ in range(2):
                r = bs_dot(Q[:, :j], a[:, None])[:, 0]
                for k in range(j):
                    a = a - r[k] * Q[:, k]
        nn = bs(a * a)
        if not (0.0 < nn < np.inf):
            raise PcaRefused("column %d has no direction of its own left: fewer than b = %d independent directions" % (j, b))
        Q[:, j] = a / np.sqrt(nn)
    return Q


def jacobi(B):
    """Eig(B): (theta descending with equal values in ascending index, W with its columns in that order)."""
    A = np.array(B, dtype=np.float64)
    b = A.shape[0]
    R = np.eye(b)
    tiny = 2.0 ** -54
    for _ in range(JACOBI_SWEEPS):
        rotated = False
        for p in range(b - 1):
            for q in range(p + 1, b):
                apq, app, aqq = A[p, q], A[p, p], A[q, q]
                if apq == 0.0 or abs(apq) <= tiny * (abs(app) + abs(aqq)):
                    continue
                rotated = True
                with np.errstate(over="ignore"):
                    tau = (aqq - app) / (2.0 * apq)
                    t = 1.0 / (abs(tau) + np.sqrt(1.0 + tau * tau))
                if tau < 0.0:
                    t = -t
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                x, y = A[:, p].copy(), A[:, q].copy()
                A[:, p] = c * x - s * y
                A[:, q] = s * x + c * y
                x, y = A[p, :].copy(), A[q, :].copy()
                A[p, :] = c * x - s * y
                A[q, :] = s * x + c * y
                A[p, q] = 0.0
                A[q, p] = 0.0
                x, y = R[:, p].copy(), R[:, q].copy()
                R[:, p] = c * x - s * y
                R[:, q] = s * x + c * y
        if not rotated:
            break
    diag = np.diag(A).copy()
    order = np.argsort(-diag, kind="stable")
    return diag[order], R[:, order]


def small_product(A, W, bo=None):
    """M[z][j] = the sum over k ascending of A[z][k] * W[k][j] from 0.0, j < bo."""
    b = W.shape[0]
    bo = b if bo is None else bo
    M = np.zeros((A.shape[0], bo))
    for k in range(b):
        M = M + A[:, k:k + 1] * W[k:k + 1, :bo]
    return M


def fix_signs(V):
    """Every column negated when its element of largest magnitude (lowest z among equals) is negative."""
    V = V.copy()
    for j in range(V.shape[1]):
        z = int(np.argmax(np.abs(V[:, j])))
        if V[z, j] < 0.0:
            V[:, j] = -V[:, j]
    return V


def unit_rows(X):
    """(ok, U): the skip rule and u_i[z] = (double) x_i[z] * s_i (rows that are skipped: zeros)."""
    Xd = np.asarray(X, dtype=np.float32).astype(np.float64)
    ok, s = ref_scales(X)
    with np.errstate(all="ignore"):
        U = np.where(ok[:, None], Xd * s[:, None], 0.0)
    return ok, U


def row_sum(terms, F):
    """BS over the rows (axis 0) of `terms`, the rows outside F adding no term (0.0 in their place adds nothing: a partial
    starts at +0.0 and never becomes -0.0)."""
    shape = (len(F),) + (1,) * (terms.ndim - 1)
    return bs(np.where(F.reshape(shape), terms, 0.0), axis=0)


def ref_pca(X, p, extra=8, center=True, seed=0, tol=1e-9, max_iter=500, allow=None):
    """dict(axes [p, dim], mean [dim], values [p], iterations, converged, fitted, total_variance) of the contract."""
    ok, U = unit_rows(X)
    n, dim = U.shape
    F = ok if allow is None else ok & np.asarray(allow, bool)
    m = int(F.sum())
    if not (1 <= p <= MAX_COMPONENTS) or extra < 0 or p + extra > MAX_BLOCK:
        raise PcaRefused("p or the block outside its limits")
    if m < 2:
        raise PcaRefused("fewer than 2 rows to fit")
    b = p + extra
    if b > min(dim, m - 1):
        raise PcaRefused("the block is wider than min(dim, m - 1)")
    fm = float(m)
    mu = row_sum(U, F) / fm if center else np.zeros(dim)
    Q = orth(start_matrix(dim, b, seed))
    UF = U[F]                                   # (rows outside F add no term: taking them out of T changes nothing)
    rows = np.nonzero(F)[0]
    prev, converged, t = None, False, 0
    while True:
        t += 1
        c = bs_dot(mu[:, None], Q)[0]
        T = np.zeros((n, b))
        T[rows] = _row_dots(UF, Q) - c[None, :]
        S = row_sum(T, F)
        Y = _rows_outer(U, T, F)
        Z = (Y - mu[:, None] * S[None, :]) / fm
        B = bs_dot(Q, Z)
        B = np.where(np.tri(b, k=-1, dtype=bool), B.T, B)   # B_kj := B_jk for j <= k
        theta, W = jacobi(B)
        if not np.all(np.isfinite(theta)):
            raise PcaRefused("a non-finite variance")
        if t >= 2 and np.max(np.abs(theta[:p] - prev[:p])) <= tol * theta[0]:
            converged = True
            break
        if t == max_iter:
            break
        prev = theta
        Q = orth(small_product(Z, W))
    V = fix_signs(small_product(Q, W, p))
    dev = bs((U - mu[None, :]) * (U - mu[None, :]), axis=1)
    tv = row_sum(dev, F) / fm
    return dict(axes=np.ascontiguousarray(V.T), mean=mu, values=theta[:p].copy(), iterations=t, converged=converged, fitted=m,
                total_variance=float(tv))


def _row_dots(U, Q):
    """BS_z(u_i[z] * Q[z][j]) -> [n, b]."""
    n, dim = U.shape
    b = Q.shape[1]
    nblk = (dim + BLOCK - 1) // BLOCK
    part = np.zeros((n, nblk, b))
    for k in range(min(BLOCK, dim)):
        u, q = U[:, k::BLOCK], Q[k::BLOCK]
        part[:, :u.shape[1]] = part[:, :u.shape[1]] + u[:, :, None] * q[None, :, :]
    out = np.zeros((n, b))
    for blk in range(nblk):
        out = out + part[:, blk]
    return out


def _rows_outer(U, T, F):
    """BS_{i in F}(u_i[z] * T[i][j]) -> [dim, b]."""
    n, dim = U.shape
    b = T.shape[1]
    nrb = (n + BLOCK - 1) // BLOCK
    part = np.zeros((nrb, dim, b))
    Tm = np.where(F[:, None], T, 0.0)
    Um = np.where(F[:, None], U, 0.0)
    for k in range(min(BLOCK, n)):
        u, tt = Um[k::BLOCK], Tm[k::BLOCK]
        part[:u.shape[0]] = part[:u.shape[0]] + u[:, :, None] * tt[:, None, :]
    out = np.zeros((dim, b))
    for blk in range(nrb):
        out = out + part[blk]
    return out


def ref_project(axes, mean, Y):
    """coords [nq, p] of the fp64 queries Y [nq, dim] (a stored row: its fp32 elements widened): NaN for a query with not
    (0 < pp < inf)."""
    Y = np.asarray(Y, dtype=np.float64)
    V = np.ascontiguousarray(np.asarray(axes, dtype=np.float64).T)
    mean = np.asarray(mean, dtype=np.float64)
    pp = np.zeros(Y.shape[0])
    with np.errstate(all="ignore"):
        for z in range(Y.shape[1]):
            pp = pp + Y[:, z] * Y[:, z]
        ok = (pp > 0.0) & (pp < np.inf)
        s = 1.0 / np.sqrt(np.where(ok, pp, 1.0))
        U = np.where(ok[:, None], Y * s[:, None], 0.0)
    c = bs_dot(mean[:, None], V)[0]
    coords = _row_dots(U, V) - c[None, :]
    coords[~ok] = np.nan
    return coords
