// pca.hip -- principal axes (include/morna_hip.h, "principal axes"): a block power iteration over the
// unit-scaled stored rows, and the coordinates of rows and queries on its axes.
//   (exact.hip)            the rows' scales (kmeans_row_scales), the queries checked and staged as fp64 rows
//                          (exact_check_queries, exact_stage_queries)
//   pca_fitted_kernel      fs[i] = s_i for the rows of F, -1 for every other row: the one array that says what is fitted
//   pca_t_kernel           the T pass, and the projection: a wave per PCA_TR rows; a lane owns one component of one column
//                          block, so the block partials of a row are independent chains across lanes, folded in block order
//   pca_y_kernel           the Y pass, and the mean: lanes along z (coalesced fp32 reads), PCA_YJ components in registers,
//                          one workgroup per row block; the partial of every row block of a slice goes to P[slot][dim][b]
//   pca_fold_kernel        partials added in slot order to the running sum: Y, S, c, B
//   pca_colsum_kernel      the row-block partials of S_j
//   pca_gram_kernel        the column-block partials of BS_z(A[z][j] * B[z][k]): c and B, and the projection's mean term
//   pca_scale_kernel, pca_z_kernel, pca_matmul_kernel, pca_rowdev_kernel   mu, Z, Z W and Q W, the rows' squared deviations
//   pca_orth_kernel        Orth in one workgroup: a column's dots in parallel over (earlier column, block) pairs
// The b x b eigenproblem is plain C++ on the host (pca_jacobi).  Every sum is BS as the header defines it: a partial is one
// dependent chain of at most 256 terms in ascending index, partials are added in ascending block; nothing is summed in
// another order, and no atomic is used: the bytes of the answer do not depend on the grid, the wave or the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "devutil.hpp"
#include "search_common.hpp"

namespace morna {

#define PCA_THREADS 256
#define PCA_BLOCK 256                          // terms of a BS block
#define PCA_TR 4                               // rows a wave of pca_t_kernel carries
#define PCA_T_WAVES (PCA_THREADS / WAVE)
#define PCA_YJ 8                               // components a thread of pca_y_kernel keeps in registers
#define PCA_ORTH_THREADS 1024
#define PCA_SLICE_VALUES ((int64_t)1 << 24)    // fp64 partials of a slice of row blocks (128 MiB)
#define PCA_BATCH_VALUES ((int64_t)1 << 26)    // fp64 query elements staged per batch of a projection (512 MiB)
#define PCA_JACOBI_SWEEPS 64

__device__ __forceinline__ double pca_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(PCA_THREADS) void pca_fitted_kernel(const double *__restrict__ scale, const uint32_t *__restrict__ deny,
                                                                 int64_t n_items, double *__restrict__ fs)
{
    const int64_t i = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
    if (i >= n_items) return;
    const bool denied = deny && ((deny[i >> 5] >> (i & 31)) & 1u);
    const double s = scale[i];
    fs[i] = !denied && s > 0.0 ? s : -1.0;
}

// scale[q] of staged fp64 queries, as kmeans_norms_kernel makes it of stored rows
__global__ __launch_bounds__(PCA_THREADS) void pca_qnorms_kernel(const double *__restrict__ Qd, int64_t nb, int32_t dim, double *__restrict__ scale)
{
    const int64_t q = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
    if (q >= nb) return;
    const double *row = Qd + q * dim;
    double pp = 0.0;
    for (int z = 0; z < dim; z++) pp = __dadd_rn(pp, __dmul_rn(row[z], row[z]));
    scale[q] = pp > 0.0 && pp < INFINITY ? __ddiv_rn(1.0, __dsqrt_rn(pp)) : -1.0;
}

// out[i][j] = BS_z((double) X[i][z] * scale[i] * Q[z][j]) - c[j] for j < b and the rows with scale[i] > 0; the canonical NaN
// for the others.  X: n rows, `stride` elements apart.  bp: b rounded up to a power of two; lane = g * bp + j carries
// component j of the column blocks g, g + 64 / bp, ..; after every round the partials are added in block order.
template <class E>
__global__ __launch_bounds__(PCA_THREADS) void pca_t_kernel(const E *__restrict__ X, int64_t stride, const double *__restrict__ scale,
                                                            int64_t n, int32_t dim, const double *__restrict__ Q, int32_t b, int32_t bp,
                                                            const double *__restrict__ c, double *__restrict__ out)
{
    const int lane = threadIdx.x & (WAVE - 1), w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int64_t r0 = ((int64_t)blockIdx.x * PCA_T_WAVES + w) * PCA_TR;
    if (r0 >= n) return;
    const int j = lane & (bp - 1), g = lane / bp, G = WAVE / bp;
    const int nblk = (dim + PCA_BLOCK - 1) / PCA_BLOCK;
    const E *row[PCA_TR];
    double s[PCA_TR], tot[PCA_TR];
#pragma unroll
    for (int u = 0; u < PCA_TR; u++) {
        const int64_t i = r0 + u < n ? r0 + u : n - 1;   // (a row past the end is read as the last one and not written)
        row[u] = X + i * stride;
        s[u] = scale[i];
        tot[u] = 0.0;
    }
    for (int b0 = 0; b0 < nblk; b0 += G) {
        const int blk = b0 + g;
        double part[PCA_TR];
#pragma unroll
        for (int u = 0; u < PCA_TR; u++) part[u] = 0.0;
        if (blk < nblk && j < b) {
            const int z0 = blk * PCA_BLOCK, z1 = z0 + PCA_BLOCK < dim ? z0 + PCA_BLOCK : dim;
            for (int z = z0; z < z1; z++) {
                const double qv = Q[(int64_t)z * b + j];
#pragma unroll
                for (int u = 0; u < PCA_TR; u++)
                    part[u] = __dadd_rn(part[u], __dmul_rn(__dmul_rn((double)row[u][z], s[u]), qv));
            }
        }
        for (int gg = 0; gg < G && b0 + gg < nblk; gg++)
#pragma unroll
            for (int u = 0; u < PCA_TR; u++) tot[u] = __dadd_rn(tot[u], __shfl(part[u], gg * bp + j, WAVE));
    }
    if (g == 0 && j < b) {
        const double cj = c[j];
#pragma unroll
        for (int u = 0; u < PCA_TR; u++)
            if (r0 + u < n) out[(r0 + u) * b + j] = s[u] > 0.0 ? __dsub_rn(tot[u], cj) : pca_nan();
    }
}

// P[blockIdx.z][z][j] = the partial of row block rb0 + blockIdx.z of BS_{i: fs[i] > 0}((double) X[i][z] * fs[i] * T[i][j]),
// j in [PCA_YJ blockIdx.y, + PCA_YJ); T null: every T[i][j] is 1.0 (the mean's sum, b = 1)
__global__ __launch_bounds__(PCA_THREADS) void pca_y_kernel(const float *__restrict__ X, int64_t n_items, int32_t dim, int32_t dpad,
                                                            const double *__restrict__ fs, const double *__restrict__ T, int32_t b,
                                                            int64_t rb0, double *__restrict__ P)
{
    const int z = blockIdx.x * PCA_THREADS + threadIdx.x, j0 = blockIdx.y * PCA_YJ;
    const int64_t rb = rb0 + blockIdx.z;
    const int64_t i0 = rb * PCA_BLOCK, i1 = i0 + PCA_BLOCK < n_items ? i0 + PCA_BLOCK : n_items;
    const bool live = z < dim;
    double part[PCA_YJ];
#pragma unroll
    for (int jj = 0; jj < PCA_YJ; jj++) part[jj] = 0.0;
    for (int64_t i = i0; i < i1; i++) {
        const double s = fs[i];
        if (!(s > 0.0)) continue;
        const double u = live ? __dmul_rn((double)X[i * dpad + z], s) : 0.0;
#pragma unroll
        for (int jj = 0; jj < PCA_YJ; jj++) {
            const double t = j0 + jj < b ? (T ? T[i * b + j0 + jj] : 1.0) : 0.0;
            part[jj] = __dadd_rn(part[jj], __dmul_rn(u, t));
        }
    }
    if (!live) return;
    double *out = P + ((int64_t)blockIdx.z * dim + z) * b;
#pragma unroll
    for (int jj = 0; jj < PCA_YJ; jj++)
        if (j0 + jj < b) out[j0 + jj] = part[jj];
}

// acc[e] = (first ? 0.0 : acc[e]) + P[0][e] + P[1][e] + .. in that order, e < count
__global__ __launch_bounds__(PCA_THREADS) void pca_fold_kernel(const double *__restrict__ P, int64_t slots, int64_t count, int first,
                                                               double *__restrict__ acc)
{
    const int64_t e = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
    if (e >= count) return;
    double a = first ? 0.0 : acc[e];
    for (int64_t sl = 0; sl < slots; sl++) a = __dadd_rn(a, P[sl * count + e]);
    acc[e] = a;
}

// P[rb][j] = the partial of row block rb of BS_{i: fs[i] > 0}(T[i][j])
__global__ __launch_bounds__(WAVE) void pca_colsum_kernel(const double *__restrict__ T, const double *__restrict__ fs, int64_t n_items,
                                                          int32_t b, double *__restrict__ P)
{
    const int j = threadIdx.x;
    if (j >= b) return;
    const int64_t i0 = (int64_t)blockIdx.x * PCA_BLOCK, i1 = i0 + PCA_BLOCK < n_items ? i0 + PCA_BLOCK : n_items;
    double a = 0.0;
    for (int64_t i = i0; i < i1; i++)
        if (fs[i] > 0.0) a = __dadd_rn(a, T[i * b + j]);
    P[(int64_t)blockIdx.x * b + j] = a;
}

// P[blk][j][k] = the partial of column block blk of BS_z(A[z][j] * B[z][k]), j < ja, k < kb
__global__ __launch_bounds__(PCA_THREADS) void pca_gram_kernel(const double *__restrict__ A, int32_t ja, const double *__restrict__ B,
                                                               int32_t kb, int32_t dim, double *__restrict__ P)
{
    const int z0 = blockIdx.x * PCA_BLOCK, z1 = z0 + PCA_BLOCK < dim ? z0 + PCA_BLOCK : dim;
    for (int pr = threadIdx.x; pr < ja * kb; pr += PCA_THREADS) {
        const int j = pr / kb, k = pr % kb;
        double a = 0.0;
        for (int z = z0; z < z1; z++) a = __dadd_rn(a, __dmul_rn(A[(int64_t)z * ja + j], B[(int64_t)z * kb + k]));
        P[(int64_t)blockIdx.x * ja * kb + pr] = a;
    }
}

// v[e] = v[e] / m
__global__ __launch_bounds__(PCA_THREADS) void pca_scale_kernel(double *__restrict__ v, int64_t count, double m)
{
    const int64_t e = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
    if (e < count) v[e] = __ddiv_rn(v[e], m);
}

// Z[z][j] = (Y[z][j] - mu[z] * S[j]) / m
__global__ __launch_bounds__(PCA_THREADS) void pca_z_kernel(const double *__restrict__ Y, const double *__restrict__ mu,
                                                            const double *__restrict__ S, int32_t dim, int32_t b, double m,
                                                            double *__restrict__ Z)
{
    const int64_t e = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
    if (e >= (int64_t)dim * b) return;
    const int64_t z = e / b;
    const int j = (int)(e % b);
    Z[e] = __ddiv_rn(__dsub_rn(Y[e], __dmul_rn(mu[z], S[j])), m);
}

// M[z][j] = the sum over k ascending of A[z][k] * W[k][j] from 0.0, j < bo (W [b][b])
__global__ __launch_bounds__(PCA_THREADS) void pca_matmul_kernel(const double *__restrict__ A, const double *__restrict__ W, int32_t dim,
                                                                 int32_t b, int32_t bo, double *__restrict__ M)
{
    const int64_t e = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
    if (e >= (int64_t)dim * bo) return;
    const int64_t z = e / bo;
    const int j = (int)(e % bo);
    double a = 0.0;
    for (int k = 0; k < b; k++) a = __dadd_rn(a, __dmul_rn(A[z * b + k], W[k * b + j]));
    M[e] = a;
}

// dev[i] = BS_z((u_i[z] - mu[z])^2) for the rows with fs[i] > 0, 0.0 for the others.  A wave per row; lane l carries the
// column blocks l, l + 64, ..
__global__ __launch_bounds__(PCA_THREADS) void pca_rowdev_kernel(const float *__restrict__ X, int64_t n_items, int32_t dim, int32_t dpad,
                                                                 const double *__restrict__ fs, const double *__restrict__ mu,
                                                                 double *__restrict__ dev)
{
    const int lane = threadIdx.x & (WAVE - 1), w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int64_t i = (int64_t)blockIdx.x * PCA_T_WAVES + w;
    if (i >= n_items) return;
    const double s = fs[i];
    if (!(s > 0.0)) {
        if (lane == 0) dev[i] = 0.0;
        return;
    }
    const float *row = X + i * dpad;
    const int nblk = (dim + PCA_BLOCK - 1) / PCA_BLOCK;
    double tot = 0.0;
    for (int b0 = 0; b0 < nblk; b0 += WAVE) {
        const int blk = b0 + lane;
        double part = 0.0;
        if (blk < nblk) {
            const int z0 = blk * PCA_BLOCK, z1 = z0 + PCA_BLOCK < dim ? z0 + PCA_BLOCK : dim;
            for (int z = z0; z < z1; z++) {
                const double d = __dsub_rn(__dmul_rn((double)row[z], s), mu[z]);
                part = __dadd_rn(part, __dmul_rn(d, d));
            }
        }
        for (int gg = 0; gg < WAVE && b0 + gg < nblk; gg++) tot = __dadd_rn(tot, __shfl(part, gg, WAVE));
    }
    if (lane == 0) dev[i] = tot;
}

// Q = Orth(A), both [dim][b]; one workgroup.  status[0] = 0, or 1 + the column whose nn was not in (0, inf): Q is then
// unfinished.  s_part holds a column's (earlier column, block) partials: (b - 1) * blocks <= 63 * 128 values.
__global__ __launch_bounds__(PCA_ORTH_THREADS) void pca_orth_kernel(const double *__restrict__ A, int32_t dim, int32_t b,
                                                                    double *__restrict__ Q, int32_t *__restrict__ status)
{
    __shared__ double s_part[(MORNA_PCA_MAX_BLOCK - 1) * (Q_MAX_DPAD / PCA_BLOCK)];
    __shared__ double s_r[MORNA_PCA_MAX_BLOCK];
    __shared__ double s_nn;
    const int tid = threadIdx.x;
    const int nblk = (dim + PCA_BLOCK - 1) / PCA_BLOCK;
    for (int64_t e = tid; e < (int64_t)dim * b; e += PCA_ORTH_THREADS) Q[e] = A[e];
    __syncthreads();
    for (int j = 0; j < b; j++) {
        for (int pass = 0; pass < 2 && j > 0; pass++) {
            for (int pr = tid; pr < j * nblk; pr += PCA_ORTH_THREADS) {
                const int k = pr / nblk, blk = pr % nblk;
                const int z0 = blk * PCA_BLOCK, z1 = z0 + PCA_BLOCK < dim ? z0 + PCA_BLOCK : dim;
                double a = 0.0;
                for (int z = z0; z < z1; z++) a = __dadd_rn(a, __dmul_rn(Q[(int64_t)z * b + k], Q[(int64_t)z * b + j]));
                s_part[pr] = a;
            }
            __syncthreads();
            if (tid < j) {
                double a = 0.0;
                for (int blk = 0; blk < nblk; blk++) a = __dadd_rn(a, s_part[tid * nblk + blk]);
                s_r[tid] = a;
            }
            __syncthreads();
            for (int z = tid; z < dim; z += PCA_ORTH_THREADS) {
                double a = Q[(int64_t)z * b + j];
                for (int k = 0; k < j; k++) a = __dsub_rn(a, __dmul_rn(s_r[k], Q[(int64_t)z * b + k]));
                Q[(int64_t)z * b + j] = a;
            }
            __syncthreads();
        }
        for (int blk = tid; blk < nblk; blk += PCA_ORTH_THREADS) {
            const int z0 = blk * PCA_BLOCK, z1 = z0 + PCA_BLOCK < dim ? z0 + PCA_BLOCK : dim;
            double a = 0.0;
            for (int z = z0; z < z1; z++) {
                const double v = Q[(int64_t)z * b + j];
                a = __dadd_rn(a, __dmul_rn(v, v));
            }
            s_part[blk] = a;
        }
        __syncthreads();
        if (tid == 0) {
            double a = 0.0;
            for (int blk = 0; blk < nblk; blk++) a = __dadd_rn(a, s_part[blk]);
            s_nn = a;
        }
        __syncthreads();
        const double nn = s_nn;
        if (!(nn > 0.0 && nn < INFINITY)) {
            if (tid == 0) status[0] = j + 1;
            return;
        }
        const double root = __dsqrt_rn(nn);
        for (int z = tid; z < dim; z += PCA_ORTH_THREADS) Q[(int64_t)z * b + j] = __ddiv_rn(Q[(int64_t)z * b + j], root);
        __syncthreads();
    }
    if (tid == 0) status[0] = 0;
}

// Eig(B) of the header: A[b][b] symmetric in, its diagonal out; W[b][b] the rotations; then theta descending (equal values in
// ascending index) with W's columns in that order.  Plain IEEE operations (the build passes -ffp-contract=off).
// False, with nothing ordered: a diagonal element is not finite.
static bool pca_jacobi(std::vector<double> &A, int b, std::vector<double> &theta, std::vector<double> &W)
{
    std::vector<double> R((size_t)b * b, 0.0);
    for (int i = 0; i < b; i++) R[(size_t)i * b + i] = 1.0;
    const double tiny = std::ldexp(1.0, -54);
    for (int sweep = 0; sweep < PCA_JACOBI_SWEEPS; sweep++) {
        bool rotated = false;
        for (int p = 0; p + 1 < b; p++)
            for (int q = p + 1; q < b; q++) {
                const double apq = A[(size_t)p * b + q], app = A[(size_t)p * b + p], aqq = A[(size_t)q * b + q];
                if (apq == 0.0 || std::fabs(apq) <= tiny * (std::fabs(app) + std::fabs(aqq))) continue;
                rotated = true;
                const double tau = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                if (tau < 0.0) t = -t;
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < b; k++) {
                    const double x = A[(size_t)k * b + p], y = A[(size_t)k * b + q];
                    A[(size_t)k * b + p] = c * x - s * y;
                    A[(size_t)k * b + q] = s * x + c * y;
                }
                for (int k = 0; k < b; k++) {
                    const double x = A[(size_t)p * b + k], y = A[(size_t)q * b + k];
                    A[(size_t)p * b + k] = c * x - s * y;
                    A[(size_t)q * b + k] = s * x + c * y;
                }
                A[(size_t)p * b + q] = 0.0;
                A[(size_t)q * b + p] = 0.0;
                for (int k = 0; k < b; k++) {
                    const double x = R[(size_t)k * b + p], y = R[(size_t)k * b + q];
                    R[(size_t)k * b + p] = c * x - s * y;
                    R[(size_t)k * b + q] = s * x + c * y;
                }
            }
        if (!rotated) break;
    }
    for (int i = 0; i < b; i++)
        if (!(std::fabs(A[(size_t)i * b + i]) < INFINITY)) return false;
    std::vector<int> order((size_t)b);
    for (int i = 0; i < b; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return A[(size_t)x * b + x] > A[(size_t)y * b + y]; });
    theta.assign((size_t)b, 0.0);
    W.assign((size_t)b * b, 0.0);
    for (int j = 0; j < b; j++) {
        theta[(size_t)j] = A[(size_t)order[(size_t)j] * b + order[(size_t)j]];
        for (int k = 0; k < b; k++) W[(size_t)k * b + j] = R[(size_t)k * b + order[(size_t)j]];
    }
    return true;
}

static inline uint64_t pca_mix(uint64_t x)
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

static inline unsigned pca_grid(int64_t count) { return (unsigned)((count + PCA_THREADS - 1) / PCA_THREADS); }

// out[ja][kb] = BS_z(A[z][j] * B[z][k]) on the stream: the column blocks' partials into P, then their fold
static int pca_gram(morna_index *h, const double *A, int32_t ja, const double *B, int32_t kb, int32_t dim, double *P, double *out)
{
    const int nblk = (dim + PCA_BLOCK - 1) / PCA_BLOCK;
    hipLaunchKernelGGL(pca_gram_kernel, dim3((unsigned)nblk), dim3(PCA_THREADS), 0, h->stream, A, ja, B, kb, dim, P);
    hipLaunchKernelGGL(pca_fold_kernel, dim3(pca_grid((int64_t)ja * kb)), dim3(PCA_THREADS), 0, h->stream, P, (int64_t)nblk, (int64_t)ja * kb,
                       1, out);
    HIP_TRY(hipGetLastError());
    return MORNA_OK;
}

// Y[dim][b] = BS_{i in F}(u_i[z] * T[i][j]) on the stream, a slice of `slice` row blocks at a time through P[slice][dim][b]
static int pca_row_sums(morna_index *h, const double *fs, const double *T, int32_t b, int64_t slice, double *P, double *Y)
{
    const int64_t N = h->n_items, nrb = (N + PCA_BLOCK - 1) / PCA_BLOCK;
    const int32_t D = h->dim;
    for (int64_t rb0 = 0; rb0 < nrb; rb0 += slice) {
        const int64_t ns = std::min(slice, nrb - rb0);
        const dim3 grid(pca_grid(D), (unsigned)((b + PCA_YJ - 1) / PCA_YJ), (unsigned)ns);
        hipLaunchKernelGGL(pca_y_kernel, grid, dim3(PCA_THREADS), 0, h->stream, h->X.p, N, D, h->dpad, fs, T, b, rb0, P);
        hipLaunchKernelGGL(pca_fold_kernel, dim3(pca_grid((int64_t)D * b)), dim3(PCA_THREADS), 0, h->stream, P, ns, (int64_t)D * b,
                           rb0 == 0 ? 1 : 0, Y);
    }
    HIP_TRY(hipGetLastError());
    return MORNA_OK;
}

static inline int32_t pca_pow2(int32_t b)
{
    int32_t bp = 1;
    while (bp < b) bp *= 2;
    return bp;
}

template <class E>
static int pca_dots(morna_index *h, const E *X, int64_t stride, const double *scale, int64_t n, const double *Q, int32_t b, const double *c,
                    double *out)
{
    const int64_t per = (int64_t)PCA_T_WAVES * PCA_TR;
    hipLaunchKernelGGL(pca_t_kernel<E>, dim3((unsigned)((n + per - 1) / per)), dim3(PCA_THREADS), 0, h->stream, X, stride, scale, n, h->dim, Q,
                       b, pca_pow2(b), c, out);
    HIP_TRY(hipGetLastError());
    return MORNA_OK;
}

static int pca_orth(morna_index *h, const double *A, int32_t b, double *Q, int32_t *d_status, const char *what)
{
    hipLaunchKernelGGL(pca_orth_kernel, dim3(1), dim3(PCA_ORTH_THREADS), 0, h->stream, A, h->dim, b, Q, d_status);
    HIP_TRY(hipGetLastError());
    int32_t st = 0;
    HIP_TRY(hipMemcpyAsync(&st, d_status, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (st != 0) {
        set_error("pca: column %d of %s has no direction of its own left: the rows hold fewer than b = %d independent directions", st - 1,
                  what, b);
        return MORNA_E_INVALID;
    }
    return MORNA_OK;
}

int pca(morna_index *h, const morna_restriction *rst, int32_t p, int32_t extra, bool center, uint64_t seed, double tol, int32_t max_iter,
        double *axes_out, double *mean_out, double *values_out, double *info_out)
{
    MORNA_TRY(finish_build(h, "pca"));
    MORNA_TRY(upload_host_rows(h));
    if (rst) MORNA_TRY(restriction_usable(h, rst));
    if (h->n_items <= 0) {
        set_error("pca on an empty index");
        return MORNA_E_EMPTY;
    }
    const int64_t N = h->n_items, nrb = (N + PCA_BLOCK - 1) / PCA_BLOCK;
    const int32_t D = h->dim;
    const int32_t nblk = (D + PCA_BLOCK - 1) / PCA_BLOCK;
    if (rst && rst->has_group) {
        set_error("pca: a restriction that holds groups is not taken, only an allow-list");
        return MORNA_E_INVALID;
    }
    if (p < 1 || p > MORNA_PCA_MAX_COMPONENTS) {
        set_error("pca: %d components, 1 to %d are taken", p, MORNA_PCA_MAX_COMPONENTS);
        return MORNA_E_INVALID;
    }
    if (extra < 0 || extra > MORNA_PCA_MAX_BLOCK - p) {
        set_error("pca: %d components and %d extra columns, a block of at most %d columns is taken", p, extra, MORNA_PCA_MAX_BLOCK);
        return MORNA_E_INVALID;
    }
    if (!(tol >= 0.0) || !(tol < INFINITY)) {
        set_error("pca: tol = %g, a finite value of at least 0 is taken", tol);
        return MORNA_E_INVALID;
    }
    if (max_iter < 1) {
        set_error("pca: max_iter = %d, at least 1 is taken", max_iter);
        return MORNA_E_INVALID;
    }
    if (h->dpad > Q_MAX_DPAD) {
        set_error("pca: dimension %d is above the supported %d", D, Q_MAX_DPAD);
        return MORNA_E_INVALID;
    }
    const int32_t b = p + extra;
    // row blocks per slice of the Y pass: its partials within PCA_SLICE_VALUES, its grid within the z limit
    const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nrb, 32768), PCA_SLICE_VALUES / ((int64_t)D * b)));
    const size_t n_part = (size_t)std::max<int64_t>(std::max<int64_t>(slice * D * b, (int64_t)nblk * b * b), nrb * b);
    double *d_scale = nullptr, *d_fs = nullptr, *d_mu = nullptr, *d_G = nullptr, *d_Q = nullptr, *d_T = nullptr, *d_Y = nullptr, *d_Z = nullptr;
    double *d_P = nullptr, *d_c = nullptr, *d_S = nullptr, *d_B = nullptr, *d_W = nullptr, *d_dev = nullptr;
    int32_t *d_status = nullptr;
    MORNA_TRY(carve_workspace(h->pca_ws, [&](Carver &c) {
        d_scale = c.take<double>((size_t)N);
        d_fs = c.take<double>((size_t)N);
        d_dev = c.take<double>((size_t)N);
        d_mu = c.take<double>((size_t)D);
        d_G = c.take<double>((size_t)D * b);
        d_Q = c.take<double>((size_t)D * b);
        d_Y = c.take<double>((size_t)D * b);
        d_Z = c.take<double>((size_t)D * b);
        d_T = c.take<double>((size_t)N * b);
        d_P = c.take<double>(n_part);
        d_c = c.take<double>((size_t)b);
        d_S = c.take<double>((size_t)b);
        d_B = c.take<double>((size_t)b * b);
        d_W = c.take<double>((size_t)b * b);
        d_status = c.take<int32_t>(1);
    }));
    // ---- F and m
    MORNA_TRY(kmeans_row_scales(h, d_scale));
    hipLaunchKernelGGL(pca_fitted_kernel, dim3(pca_grid(N)), dim3(PCA_THREADS), 0, h->stream, d_scale, rst ? rst->deny.p : nullptr, N, d_fs);
    HIP_TRY(hipGetLastError());
    std::vector<double> fs((size_t)N);
    HIP_TRY(hipMemcpyAsync(fs.data(), d_fs, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int64_t m = 0;
    for (int64_t i = 0; i < N; i++) m += fs[(size_t)i] > 0.0 ? 1 : 0;
    if (m < 2) {
        set_error("pca: %lld rows to fit (eligible with a positive finite sum of squares), at least 2 are taken", (long long)m);
        return MORNA_E_INVALID;
    }
    if (b > std::min<int64_t>(D, m - 1)) {
        set_error("pca: a block of %d columns, at most min(dim, rows fitted - 1) = %lld are taken", b, (long long)std::min<int64_t>(D, m - 1));
        return MORNA_E_INVALID;
    }
    HipEvents ev;
    MORNA_TRY(ev.create(8));
    double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // T, Y, Orth, small products, Eig
    // ---- the mean
    if (center) {
        MORNA_TRY(pca_row_sums(h, d_fs, nullptr, 1, slice, d_P, d_mu));
        hipLaunchKernelGGL(pca_scale_kernel, dim3(pca_grid(D)), dim3(PCA_THREADS), 0, h->stream, d_mu, (int64_t)D, (double)m);
        HIP_TRY(hipGetLastError());
    } else HIP_TRY(hipMemsetAsync(d_mu, 0, (size_t)D * 8, h->stream));
    // ---- the start
    {
        std::vector<double> G((size_t)D * b);
        const uint64_t base = seed * 0x9E3779B97F4A7C15ull;
        for (int64_t z = 0; z < D; z++)
            for (int j = 0; j < b; j++)
                G[(size_t)(z * b + j)] = (double)(pca_mix(base + 64ull * (uint64_t)z + (uint64_t)j) >> 11) * 0x1p-53 - 0.5;
        HIP_TRY(hipMemcpyAsync(d_G, G.data(), (size_t)D * b * 8, hipMemcpyHostToDevice, h->stream));
        MORNA_TRY(ev.record(0, h->stream));
        MORNA_TRY(pca_orth(h, d_G, b, d_Q, d_status, "the start"));   // (waits for the stream: G may go)
        MORNA_TRY(ev.record(1, h->stream));
    }
    std::vector<double> B((size_t)b * b), theta, prev, W;
    int32_t t = 0;
    bool converged = false;
    for (t = 1;; t++) {
        MORNA_TRY(ev.record(2, h->stream));
        MORNA_TRY(pca_gram(h, d_mu, 1, d_Q, b, D, d_P, d_c));
        MORNA_TRY(ev.record(3, h->stream));
        MORNA_TRY(pca_dots<float>(h, h->X.p, (int64_t)h->dpad, d_fs, N, d_Q, b, d_c, d_T));
        MORNA_TRY(ev.record(4, h->stream));
        hipLaunchKernelGGL(pca_colsum_kernel, dim3((unsigned)nrb), dim3(WAVE), 0, h->stream, d_T, d_fs, N, b, d_P);
        hipLaunchKernelGGL(pca_fold_kernel, dim3(pca_grid(b)), dim3(PCA_THREADS), 0, h->stream, d_P, nrb, (int64_t)b, 1, d_S);
        MORNA_TRY(pca_row_sums(h, d_fs, d_T, b, slice, d_P, d_Y));
        hipLaunchKernelGGL(pca_z_kernel, dim3(pca_grid((int64_t)D * b)), dim3(PCA_THREADS), 0, h->stream, d_Y, d_mu, d_S, D, b, (double)m, d_Z);
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(5, h->stream));
        MORNA_TRY(pca_gram(h, d_Q, b, d_Z, b, D, d_P, d_B));
        MORNA_TRY(ev.record(6, h->stream));
        HIP_TRY(hipMemcpyAsync(B.data(), d_B, (size_t)b * b * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (t == 1) MORNA_TRY(ev.elapsed(0, 1, &ms[2]));
        MORNA_TRY(ev.elapsed(2, 3, &ms[3]));
        MORNA_TRY(ev.elapsed(3, 4, &ms[0]));
        MORNA_TRY(ev.elapsed(4, 5, &ms[1]));
        MORNA_TRY(ev.elapsed(5, 6, &ms[3]));
        const auto e0 = std::chrono::steady_clock::now();
        for (int j = 0; j < b; j++)
            for (int k = 0; k < j; k++) B[(size_t)j * b + k] = B[(size_t)k * b + j];
        prev = theta;
        const bool finite = pca_jacobi(B, b, theta, W);
        ms[4] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - e0).count();
        if (!finite) {
            set_error("pca: iteration %d gave a non-finite variance", t);
            return MORNA_E_INVALID;
        }
        if (t >= 2) {
            double worst = 0.0;
            for (int j = 0; j < p; j++) worst = std::max(worst, std::fabs(theta[(size_t)j] - prev[(size_t)j]));
            converged = worst <= tol * theta[0];
        }
        HIP_TRY(hipMemcpyAsync(d_W, W.data(), (size_t)b * b * 8, hipMemcpyHostToDevice, h->stream));
        if (converged || t == max_iter) break;
        MORNA_TRY(ev.record(2, h->stream));
        hipLaunchKernelGGL(pca_matmul_kernel, dim3(pca_grid((int64_t)D * b)), dim3(PCA_THREADS), 0, h->stream, d_Z, d_W, D, b, b, d_G);
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(3, h->stream));
        MORNA_TRY(pca_orth(h, d_G, b, d_Q, d_status, "Z W"));
        MORNA_TRY(ev.record(4, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        MORNA_TRY(ev.elapsed(2, 3, &ms[3]));
        MORNA_TRY(ev.elapsed(3, 4, &ms[2]));
    }
    // ---- the result: V = Q W with the sign rule, the total variance
    MORNA_TRY(ev.record(2, h->stream));
    hipLaunchKernelGGL(pca_matmul_kernel, dim3(pca_grid((int64_t)D * b)), dim3(PCA_THREADS), 0, h->stream, d_Q, d_W, D, b, b, d_G);
    MORNA_TRY(ev.record(3, h->stream));
    hipLaunchKernelGGL(pca_rowdev_kernel, dim3((unsigned)((N + PCA_T_WAVES - 1) / PCA_T_WAVES)), dim3(PCA_THREADS), 0, h->stream, h->X.p, N, D,
                       h->dpad, d_fs, d_mu, d_dev);
    HIP_TRY(hipGetLastError());
    std::vector<double> V((size_t)D * b), dev((size_t)N);
    HIP_TRY(hipMemcpyAsync(V.data(), d_G, (size_t)D * b * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(dev.data(), d_dev, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(mean_out, d_mu, (size_t)D * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    MORNA_TRY(ev.elapsed(2, 3, &ms[3]));
    for (int j = 0; j < p; j++) {
        int64_t zbig = 0;
        for (int64_t z = 1; z < D; z++)
            if (std::fabs(V[(size_t)(z * b + j)]) > std::fabs(V[(size_t)(zbig * b + j)])) zbig = z;
        const bool flip = V[(size_t)(zbig * b + j)] < 0.0;
        for (int64_t z = 0; z < D; z++) axes_out[(int64_t)j * D + z] = flip ? -V[(size_t)(z * b + j)] : V[(size_t)(z * b + j)];
        values_out[j] = theta[(size_t)j];
    }
    double tv = 0.0;
    for (int64_t rb = 0; rb < nrb; rb++) {
        double part = 0.0;
        for (int64_t i = rb * PCA_BLOCK; i < std::min<int64_t>(N, (rb + 1) * PCA_BLOCK); i++)
            if (fs[(size_t)i] > 0.0) part = part + dev[(size_t)i];
        tv = tv + part;
    }
    info_out[0] = (double)t;
    info_out[1] = converged ? 1.0 : 0.0;
    info_out[2] = (double)m;
    info_out[3] = tv / (double)m;
    h->pca_stats[0] = ms[0];
    h->pca_stats[1] = ms[1];
    h->pca_stats[2] = ms[2];
    h->pca_stats[3] = ms[3];
    h->pca_stats[4] = ms[4];
    h->pca_stats[5] = (double)t;
    h->pca_stats[6] = (double)m;
    h->pca_stats[7] = 4.0 * (double)D * ((double)N + (double)m * (2.0 + 2.0 * (double)t));
    return MORNA_OK;
}

int pca_project(morna_index *h, const double *axes_host, const double *mean_host, int32_t p, const ExactQueries &Q, int64_t nq,
                double *coords_out)
{
    MORNA_TRY(finish_build(h, "pca_project"));
    MORNA_TRY(upload_host_rows(h));
    if (h->n_items <= 0) {
        set_error("pca_project on an empty index");
        return MORNA_E_EMPTY;
    }
    const int32_t D = h->dim;
    const int32_t nblk = (D + PCA_BLOCK - 1) / PCA_BLOCK;
    if (p < 1 || p > MORNA_PCA_MAX_COMPONENTS) {
        set_error("pca_project: %d components, 1 to %d are taken", p, MORNA_PCA_MAX_COMPONENTS);
        return MORNA_E_INVALID;
    }
    if (nq < 0) {
        set_error("pca_project: a negative number of queries");
        return MORNA_E_INVALID;
    }
    for (int64_t e = 0; e < (int64_t)p * D; e++)
        if (!(std::fabs(axes_host[e]) < INFINITY)) {
            set_error("pca_project: axis %lld has a non-finite element", (long long)(e / D));
            return MORNA_E_INVALID;
        }
    for (int64_t z = 0; z < D; z++)
        if (!(std::fabs(mean_host[z]) < INFINITY)) {
            set_error("pca_project: the mean has a non-finite element");
            return MORNA_E_INVALID;
        }
    int qt = 0;
    MORNA_TRY(exact_check_queries(h, "pca_project", Q, nq, &qt));
    if (nq == 0) return MORNA_OK;
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(nq, PCA_BATCH_VALUES / D));
    double *d_V = nullptr, *d_mu = nullptr, *d_P = nullptr, *d_c = nullptr, *d_Qd = nullptr, *d_scale = nullptr, *d_out = nullptr;
    int32_t *d_items = nullptr;
    MORNA_TRY(carve_workspace(h->pca_ws, [&](Carver &c) {
        d_V = c.take<double>((size_t)D * p);
        d_mu = c.take<double>((size_t)D);
        d_P = c.take<double>((size_t)nblk * p);
        d_c = c.take<double>((size_t)p);
        d_Qd = c.take<double>((size_t)batch * D);
        d_scale = c.take<double>((size_t)batch);
        d_out = c.take<double>((size_t)batch * p);
        d_items = c.take<int32_t>(Q.items() ? (size_t)batch : 0);
    }));
    std::vector<double> V((size_t)D * p);
    for (int j = 0; j < p; j++)
        for (int64_t z = 0; z < D; z++) V[(size_t)(z * p + j)] = axes_host[(int64_t)j * D + z];
    HIP_TRY(hipMemcpyAsync(d_V, V.data(), (size_t)D * p * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_mu, mean_host, (size_t)D * 8, hipMemcpyHostToDevice, h->stream));
    MORNA_TRY(pca_gram(h, d_mu, 1, d_V, p, D, d_P, d_c));
    for (int64_t q0 = 0; q0 < nq; q0 += batch) {
        const int64_t nb = std::min(batch, nq - q0);
        MORNA_TRY(exact_stage_queries(h, Q, q0, nb, d_items, d_Qd));
        hipLaunchKernelGGL(pca_qnorms_kernel, dim3(pca_grid(nb)), dim3(PCA_THREADS), 0, h->stream, d_Qd, nb, D, d_scale);
        MORNA_TRY(pca_dots<double>(h, d_Qd, (int64_t)D, d_scale, nb, d_V, p, d_c, d_out));
        HIP_TRY(hipMemcpyAsync(coords_out + q0 * p, d_out, (size_t)nb * p * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // (V on the host and the batch's arrays may go)
    }
    return MORNA_OK;
}

}  // namespace morna
