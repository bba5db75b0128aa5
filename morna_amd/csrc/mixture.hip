// mixture.hip -- label mixture (include/morna_hip.h, "label mixture"): every query as a non-negative
// combination of the label centroids.
//   (exact.hip)              the centroid sums: the scales, member lists and update of k-means for the given labelling
//                            (kmeans_label_sums), the queries staged as fp64 rows (exact_stage_queries)
//   mixture_labels_kernel    the labelling of the eligible rows: -1 where the allow-list leaves a row out
//   mixture_counts_kernel    per label its unskipped members
//   mixture_transpose_kernel s[L][dim] -> sT[dim][LP], LP = L rounded up to 64, zeros behind L: lanes over labels read one line
//   mixture_gram_kernel      one thread per pair l <= m: S_lm, one sequential chain over the columns
//   mixture_norm_kernel      d_l, the active labels and G of the queries that leave no label out
//   mixture_dots_kernel      t[q][l] and yy[q]: lanes over labels, MX_DOT_Q queries per wave in registers, the query
//                            elements of a tile of columns in LDS (wave-uniform reads), sT from L2
//   mixture_solve_kernel     persistent workgroups, G in LDS; a wave per query: the own label's patch, the cyclic coordinate
//                            descent, the report
// Every sum is one dependent chain in ascending index with one rounding per multiply and per add; nothing is summed across
// lanes, and no atomic is used: the bytes of the answer do not depend on the grid, the wave or the batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "devutil.hpp"
#include "search_common.hpp"

namespace morna {

#define MX_THREADS 256
#define MX_DOT_Q 8                             // queries a wave of mixture_dots_kernel keeps in registers
#define MX_DOT_WAVES (MX_THREADS / WAVE)
#define MX_DOT_QB (MX_DOT_Q * MX_DOT_WAVES)    // queries of a workgroup: sT is read from L2 once per that many
#define MX_DOT_Z 64                            // columns of a tile
#define MX_SOLVE_THREADS 512
#define MX_SOLVE_WAVES (MX_SOLVE_THREADS / WAVE)
#define MX_BATCH_VALUES ((int64_t)1 << 27)     // fp64 query elements staged per batch (1 GiB)

__global__ __launch_bounds__(MX_THREADS) void mixture_labels_kernel(const int32_t *__restrict__ label, const uint32_t *__restrict__ deny,
                                                                    int64_t n_items, int32_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x;
    if (i >= n_items) return;
    const bool denied = deny && ((deny[i >> 5] >> (i & 31)) & 1u);
    out[i] = denied ? -1 : label[i];
}

// m_l: the members of label l that the update did not skip
__global__ __launch_bounds__(MX_THREADS) void mixture_counts_kernel(const int32_t *__restrict__ member, const int32_t *__restrict__ start,
                                                                    const int32_t *__restrict__ sizes, const double *__restrict__ scale,
                                                                    int32_t L, int32_t *__restrict__ counts)
{
    const int l = blockIdx.x * MX_THREADS + threadIdx.x;
    if (l >= L) return;
    const int32_t *mem = member + start[l];
    int c = 0;
    for (int u = 0; u < sizes[l]; u++) c += scale[mem[u]] > 0.0 ? 1 : 0;
    counts[l] = c;
}

__global__ __launch_bounds__(MX_THREADS) void mixture_transpose_kernel(const double *__restrict__ sums, int32_t L, int32_t LP, int32_t dim,
                                                                       double *__restrict__ sT)
{
    const int64_t t = (int64_t)blockIdx.x * MX_THREADS + threadIdx.x;
    if (t >= (int64_t)dim * LP) return;
    const int l = (int)(t % LP);
    const int64_t z = t / LP;
    sT[t] = l < L ? sums[(int64_t)l * dim + z] : 0.0;
}

// S_lm = S_ml = the sum over z of s_l[z] * s_m[z] from 0.0 in ascending z, for l <= m
__global__ __launch_bounds__(MX_THREADS) void mixture_gram_kernel(const double *__restrict__ sT, int32_t dim, int32_t LP, int32_t L,
                                                                  double *__restrict__ S)
{
    const int t = blockIdx.x * MX_THREADS + threadIdx.x;
    if (t >= L * L) return;
    const int l = t / L, m = t % L;
    if (l > m) return;
    double acc = 0.0;
    for (int z = 0; z < dim; z++) acc = __dadd_rn(acc, __dmul_rn(sT[(int64_t)z * LP + l], sT[(int64_t)z * LP + m]));
    S[l * L + m] = acc;
    S[m * L + l] = acc;
}

// one workgroup: d_l = sqrt(S_ll), act_l = (m_l >= 1 and 0 < S_ll < inf), G_lm = S_lm / (d_l d_m) between active labels
// (1.0 on the diagonal, 0.0 where either is inactive: never read)
__global__ __launch_bounds__(MX_THREADS) void mixture_norm_kernel(const double *__restrict__ S, const int32_t *__restrict__ counts, int32_t L,
                                                                  double *__restrict__ d, int32_t *__restrict__ act, double *__restrict__ G)
{
    __shared__ double s_d[MORNA_MIXTURE_LABELS_MAX];
    __shared__ int s_act[MORNA_MIXTURE_LABELS_MAX];
    const int tid = threadIdx.x;
    for (int l = tid; l < L; l += MX_THREADS) {
        const double sll = S[l * L + l];
        const bool on = counts[l] >= 1 && sll > 0.0 && sll < INFINITY;
        s_act[l] = on ? 1 : 0;
        s_d[l] = on ? __dsqrt_rn(sll) : 0.0;
        act[l] = s_act[l];
        d[l] = s_d[l];
    }
    __syncthreads();
    for (int t = tid; t < L * L; t += MX_THREADS) {
        const int l = t / L, m = t % L;
        double g = 0.0;
        if (l == m) g = 1.0;
        else if (s_act[l] && s_act[m]) g = __ddiv_rn(S[t], __dmul_rn(s_d[l], s_d[m]));
        G[t] = g;
    }
}

// t[q][l] = the sum over z of s_l[z] * y_q[z], yy[q] = the sum of y_q[z]^2, from 0.0 in ascending z.  A lane owns labels
// lane + 64 v (v < NL) of MX_DOT_Q queries; the queries' elements of MX_DOT_Z columns are brought to LDS by the whole
// workgroup and read back wave-uniformly.  Thread u < MX_DOT_QB of the workgroup carries yy of its query u.
template <int NL>
__global__ __launch_bounds__(MX_THREADS) void mixture_dots_kernel(const double *__restrict__ Qd, int64_t nb, int32_t dim,
                                                                  const double *__restrict__ sT, int32_t LP, double *__restrict__ t,
                                                                  double *__restrict__ yy)
{
    __shared__ double s_y[MX_DOT_QB][MX_DOT_Z + 1];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int64_t q0 = (int64_t)blockIdx.x * MX_DOT_QB;
    double acc[MX_DOT_Q][NL];
#pragma unroll
    for (int u = 0; u < MX_DOT_Q; u++)
#pragma unroll
        for (int v = 0; v < NL; v++) acc[u][v] = 0.0;
    double yq = 0.0;
    for (int z0 = 0; z0 < dim; z0 += MX_DOT_Z) {
        const int zc = dim - z0 < MX_DOT_Z ? dim - z0 : MX_DOT_Z;
        __syncthreads();   // the tile before this one has been read
#pragma unroll
        for (int u = 0; u < MX_DOT_QB / MX_DOT_WAVES; u++) {
            const int qq = w + MX_DOT_WAVES * u;
            const int64_t q = q0 + qq;
            s_y[qq][lane] = q < nb && lane < zc ? Qd[q * dim + z0 + lane] : 0.0;
        }
        __syncthreads();
        if (tid < MX_DOT_QB)
            for (int zz = 0; zz < zc; zz++) {
                const double y = s_y[tid][zz];
                yq = __dadd_rn(yq, __dmul_rn(y, y));
            }
        const double *sz = sT + (int64_t)z0 * LP + lane;
#pragma unroll 4
        for (int zz = 0; zz < zc; zz++) {
            double s[NL];
#pragma unroll
            for (int v = 0; v < NL; v++) s[v] = sz[(int64_t)zz * LP + WAVE * v];
#pragma unroll
            for (int u = 0; u < MX_DOT_Q; u++) {
                const double y = s_y[w * MX_DOT_Q + u][zz];
#pragma unroll
                for (int v = 0; v < NL; v++) acc[u][v] = __dadd_rn(acc[u][v], __dmul_rn(s[v], y));
            }
        }
    }
#pragma unroll
    for (int u = 0; u < MX_DOT_Q; u++) {
        const int64_t q = q0 + w * MX_DOT_Q + u;
        if (q < nb)
#pragma unroll
            for (int v = 0; v < NL; v++) t[q * LP + lane + WAVE * v] = acc[u][v];
    }
    if (tid < MX_DOT_QB && q0 + tid < nb) yy[q0 + tid] = yq;
}

// lane l of a wave-resident fp64 value, l wave-uniform
__device__ __forceinline__ double mx_lane_read(double v, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// label l's value: slot l / 64 of lane l % 64
__device__ __forceinline__ double mx_label_read(double v0, double v1, int l)
{
    return l < WAVE ? mx_lane_read(v0, l) : mx_lane_read(v1, l - WAVE);
}

struct MixtureSolveArgs {
    const double *G, *d, *S;       // [L][L], [L], [L][L]: mixture_norm_kernel, mixture_gram_kernel
    const int32_t *act, *counts;   // [L]
    const double *t, *yy;          // [nb][LP], [nb]: mixture_dots_kernel
    const int32_t *items;          // [nb] the queries' rows, or null: no query leaves a label out
    const int32_t *label;          // [n_items] as given
    const uint32_t *deny;          // the allow-list's complement, or null
    const double *scale;           // [n_items]
    int64_t nb;
    int32_t L, LP, max_sweeps;
    double tol;
    double *weights, *info;        // [nb][L], [nb][4]
    uint8_t *active;               // [nb][L]
};

// A wave per query, taken in turn by the waves of a grid that follows the CU count.  Lane `lane` owns labels lane and
// lane + 64: their a, g and b stay in registers.  delta of a step is read from the owning lane and is the same for all lanes;
// every lane then updates its own g.  The query that leaves its own label o out reads row and column o from the wave's
// vector s_go in place of G.
__global__ __launch_bounds__(MX_SOLVE_THREADS) void mixture_solve_kernel(MixtureSolveArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int L = A.L;
    double *s_G = (double *)smem;                                  // [L][L]
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = __builtin_amdgcn_readfirstlane(tid / WAVE);
    double *s_go = s_G + L * L + w * L;                            // [L] of this wave
    for (int i = tid; i < L * L; i += MX_SOLVE_THREADS) s_G[i] = A.G[i];
    __syncthreads();
    const bool two = L > WAVE;
    const int m0 = lane, m1 = lane + WAVE;
    const bool in0 = m0 < L, in1 = m1 < L;
    for (int64_t q = (int64_t)blockIdx.x * MX_SOLVE_WAVES + w; q < A.nb; q += (int64_t)gridDim.x * MX_SOLVE_WAVES) {
        // ---- the query's own label, when it leaves one out
        int o = -1;
        double sig = 0.0;
        if (A.items) {
            const int64_t i = A.items[q];
            const int32_t lab = A.label[i];
            const double sc = A.scale[i];
            const bool denied = A.deny && ((A.deny[i >> 5] >> (i & 31)) & 1u);
            if (lab >= 0 && !denied && sc > 0.0) {
                o = lab;
                sig = sc;
            }
        }
        const double y2 = A.yy[q];
        double t0 = in0 ? A.t[q * A.LP + m0] : 0.0, t1 = in1 ? A.t[q * A.LP + m1] : 0.0;
        double d0 = in0 ? A.d[m0] : 0.0, d1 = in1 ? A.d[m1] : 0.0;
        bool act0 = in0 && A.act[m0] != 0, act1 = in1 && A.act[m1] != 0;
        if (o >= 0) {
            const double tau0 = __dmul_rn(t0, sig), tau1 = __dmul_rn(t1, sig);
            double sp0 = in0 ? __dsub_rn(A.S[o * L + m0], tau0) : 0.0, sp1 = in1 ? __dsub_rn(A.S[o * L + m1], tau1) : 0.0;
            const double drop = __dmul_rn(y2, sig);   // pp_i sigma_i: the query's sum of squares is pp_i
            if (m0 == o) {
                sp0 = __dadd_rn(__dsub_rn(A.S[o * L + o], __dmul_rn(2.0, tau0)), 1.0);
                t0 = __dsub_rn(t0, drop);
            }
            if (m1 == o) {
                sp1 = __dadd_rn(__dsub_rn(A.S[o * L + o], __dmul_rn(2.0, tau1)), 1.0);
                t1 = __dsub_rn(t1, drop);
            }
            const double soo = mx_label_read(sp0, sp1, o);
            const bool on = A.counts[o] - 1 >= 1 && soo > 0.0 && soo < INFINITY;
            const double dn = on ? __dsqrt_rn(soo) : 0.0;
            if (m0 == o) {
                act0 = on;
                d0 = dn;
            }
            if (m1 == o) {
                act1 = on;
                d1 = dn;
            }
            if (in0) s_go[m0] = m0 == o ? 1.0 : __ddiv_rn(sp0, __dmul_rn(dn, d0));
            if (in1) s_go[m1] = m1 == o ? 1.0 : __ddiv_rn(sp1, __dmul_rn(dn, d1));
            __builtin_amdgcn_wave_barrier();   // (the wave reads what its lanes wrote: LDS keeps a wave's accesses in order)
        }
        const unsigned long long mask0 = __ballot(act0), mask1 = __ballot(act1);
        const double sq = __dsqrt_rn(y2);
        const double b0 = act0 ? __ddiv_rn(t0, __dmul_rn(d0, sq)) : 0.0, b1 = act1 ? __ddiv_rn(t1, __dmul_rn(d1, sq)) : 0.0;
        const bool valid = y2 > 0.0 && y2 < INFINITY && (mask0 | mask1) != 0ull;
        double a0 = 0.0, a1 = 0.0, g0 = b0, g1 = b1;
        double rr = 0.0, kkt = 0.0;
        int sweeps = 0, status = -1;
        if (valid) {
            status = 0;
            for (int s = 1; s <= A.max_sweeps; s++) {
                double mx = 0.0;
                for (int l = 0; l < L; l++) {
                    if (!(((l < WAVE ? mask0 >> l : mask1 >> (l - WAVE))) & 1ull)) continue;
                    const double gl = mx_label_read(g0, g1, l), al = mx_label_read(a0, a1, l);
                    double delta = gl;
                    if (delta < -al) delta = -al;
                    if (delta != 0.0) {
                        if (m0 == l) a0 = __dadd_rn(a0, delta);
                        if (m1 == l) a1 = __dadd_rn(a1, delta);
                        const double *row = l == o ? s_go : s_G + l * L;
                        double G0 = in0 ? row[m0] : 0.0;
                        if (m0 == o && l != o) G0 = s_go[l];
                        g0 = __dsub_rn(g0, __dmul_rn(delta, G0));
                        if (two) {
                            double G1 = in1 ? row[m1] : 0.0;
                            if (m1 == o && l != o) G1 = s_go[l];
                            g1 = __dsub_rn(g1, __dmul_rn(delta, G1));
                        }
                    }
                    if (fabs(delta) > mx) mx = fabs(delta);
                }
                sweeps = s;
                if (mx <= A.tol) {
                    status = 1;
                    break;
                }
            }
            // ---- the report
            double h0 = 0.0, h1 = 0.0;
            for (int m = 0; m < L; m++) {
                if (!(((m < WAVE ? mask0 >> m : mask1 >> (m - WAVE))) & 1ull)) continue;
                const double am = mx_label_read(a0, a1, m);
                const double *row = m == o ? s_go : s_G + m * L;
                double G0 = in0 ? row[m0] : 0.0, G1 = in1 ? row[m1] : 0.0;
                if (m0 == o && m != o) G0 = s_go[m];
                if (m1 == o && m != o) G1 = s_go[m];
                h0 = __dadd_rn(h0, __dmul_rn(G0, am));
                h1 = __dadd_rn(h1, __dmul_rn(G1, am));
            }
            const double w0 = __dsub_rn(b0, h0), w1 = __dsub_rn(b1, h1);
            const double k0 = a0 > 0.0 ? fabs(w0) : (w0 > 0.0 ? w0 : 0.0), k1 = a1 > 0.0 ? fabs(w1) : (w1 > 0.0 ? w1 : 0.0);
            const double u0 = __dmul_rn(a0, h0), u1 = __dmul_rn(a1, h1), v0 = __dmul_rn(a0, b0), v1 = __dmul_rn(a1, b1);
            double u = 0.0, v = 0.0;
            for (int l = 0; l < L; l++) {
                if (!(((l < WAVE ? mask0 >> l : mask1 >> (l - WAVE))) & 1ull)) continue;
                const double kl = mx_label_read(k0, k1, l);
                if (kl > kkt) kkt = kl;
                u = __dadd_rn(u, mx_label_read(u0, u1, l));
                v = __dadd_rn(v, mx_label_read(v0, v1, l));
            }
            rr = __dadd_rn(__dsub_rn(1.0, __dmul_rn(2.0, v)), u);
        }
        if (in0) {
            A.weights[q * L + m0] = valid && act0 ? a0 : 0.0;
            A.active[q * L + m0] = act0 ? 1 : 0;
        }
        if (in1) {
            A.weights[q * L + m1] = valid && act1 ? a1 : 0.0;
            A.active[q * L + m1] = act1 ? 1 : 0;
        }
        if (lane < 4) A.info[q * 4 + lane] = lane == 0 ? rr : lane == 1 ? kkt : lane == 2 ? (double)sweeps : (double)status;
    }
}

int mixture(morna_index *h, const morna_restriction *rst, const ExactQueries &Q, int64_t nq, const int32_t *item_label_host, int32_t L,
            double tol, int32_t max_sweeps, double *sums_out, int32_t *counts_out, double *gram_out, double *weights_out,
            double *info_out, uint8_t *active_out)
{
    const bool solve = weights_out != nullptr;
    const char *who = solve ? "mixture" : "label_centroids";
    MORNA_TRY(finish_build(h, who));
    MORNA_TRY(upload_host_rows(h));
    if (rst) MORNA_TRY(restriction_usable(h, rst));
    if (h->n_items <= 0) {
        set_error("%s on an empty index", who);
        return MORNA_E_EMPTY;
    }
    const int64_t N = h->n_items;
    const int32_t D = h->dim;
    if (rst && rst->has_group) {
        set_error("%s: a restriction that holds groups is not taken, only an allow-list", who);
        return MORNA_E_INVALID;
    }
    if (L < 1 || L > MORNA_MIXTURE_LABELS_MAX) {
        set_error("%s: %d labels, 1 to %d are taken", who, L, MORNA_MIXTURE_LABELS_MAX);
        return MORNA_E_INVALID;
    }
    for (int64_t i = 0; i < N; i++)
        if (item_label_host[i] < -1 || item_label_host[i] >= L) {
            set_error("%s: item %lld has the label %d, outside [-1, %d)", who, (long long)i, item_label_host[i], L);
            return MORNA_E_INVALID;
        }
    if (solve) {
        if (nq < 0) {
            set_error("mixture: a negative number of queries");
            return MORNA_E_INVALID;
        }
        if (!(tol >= 0.0) || !(tol < INFINITY)) {
            set_error("mixture: tol = %g, a finite value of at least 0 is taken", tol);
            return MORNA_E_INVALID;
        }
        if (max_sweeps < 1) {
            set_error("mixture: max_sweeps = %d, at least 1 is taken", max_sweeps);
            return MORNA_E_INVALID;
        }
        int qt = 0;
        MORNA_TRY(exact_check_queries(h, who, Q, nq, &qt));
        if (nq == 0) return MORNA_OK;
    }
    const int32_t LP = (L + WAVE - 1) / WAVE * WAVE;
    const int64_t chunks = kmeans_lists_chunks(N), nblk = (N + MX_THREADS - 1) / MX_THREADS;
    const int64_t batch = solve ? std::max<int64_t>(1, std::min<int64_t>(nq, MX_BATCH_VALUES / D)) : 0;
    KmeansLists W;
    int32_t *d_label = nullptr, *d_elig = nullptr, *d_counts = nullptr, *d_act = nullptr, *d_items = nullptr;
    double *d_sums = nullptr, *d_sT = nullptr, *d_S = nullptr, *d_G = nullptr, *d_d = nullptr;
    double *d_Qd = nullptr, *d_t = nullptr, *d_yy = nullptr, *d_w = nullptr, *d_info = nullptr;
    uint8_t *d_active = nullptr;
    MORNA_TRY(carve_workspace(h->mx_ws, [&](Carver &c) {
        const size_t b = (size_t)batch;
        d_label = c.take<int32_t>((size_t)N);
        d_elig = c.take<int32_t>((size_t)N);
        W.scale = c.take<double>((size_t)N);
        W.chunk_cnt = c.take<int32_t>((size_t)chunks * L);
        W.sizes = c.take<int32_t>((size_t)L);
        W.start = c.take<int32_t>((size_t)L);
        W.member = c.take<int32_t>((size_t)N);
        W.totals = c.take<int32_t>(4);
        d_counts = c.take<int32_t>((size_t)L);
        d_act = c.take<int32_t>((size_t)L);
        d_sums = c.take<double>((size_t)L * D);
        d_sT = c.take<double>((size_t)LP * D);
        d_S = c.take<double>((size_t)L * L);
        d_G = c.take<double>((size_t)L * L);
        d_d = c.take<double>((size_t)L);
        d_Qd = c.take<double>(b * D);
        d_items = c.take<int32_t>(Q.items() && solve ? b : 0);
        d_t = c.take<double>(b * LP);
        d_yy = c.take<double>(b);
        d_w = c.take<double>(b * L);
        d_info = c.take<double>(b * 4);
        d_active = c.take<uint8_t>(b * L);
    }));
    HipEvents ev;
    MORNA_TRY(ev.create(6));
    // ---- the centroid sums and their counts
    MORNA_TRY(ev.record(0, h->stream));
    HIP_TRY(hipMemcpyAsync(d_label, item_label_host, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(W.totals, 0, 16, h->stream));
    HIP_TRY(hipMemsetAsync(d_sums, 0, (size_t)L * D * 8, h->stream));   // a label without an unskipped member: the zero vector
    hipLaunchKernelGGL(mixture_labels_kernel, dim3((unsigned)nblk), dim3(MX_THREADS), 0, h->stream, d_label, rst ? rst->deny.p : nullptr, N,
                       d_elig);
    MORNA_TRY(kmeans_label_sums(h, d_elig, L, W, d_sums));
    hipLaunchKernelGGL(mixture_counts_kernel, dim3(1), dim3(MX_THREADS), 0, h->stream, W.member, W.start, W.sizes, W.scale, L, d_counts);
    HIP_TRY(hipGetLastError());
    MORNA_TRY(ev.record(1, h->stream));
    // ---- the Gram matrix, normalised for the queries that leave no label out
    hipLaunchKernelGGL(mixture_transpose_kernel, dim3((unsigned)(((int64_t)D * LP + MX_THREADS - 1) / MX_THREADS)), dim3(MX_THREADS), 0,
                       h->stream, d_sums, L, LP, D, d_sT);
    hipLaunchKernelGGL(mixture_gram_kernel, dim3((unsigned)((L * L + MX_THREADS - 1) / MX_THREADS)), dim3(MX_THREADS), 0, h->stream, d_sT, D,
                       LP, L, d_S);
    hipLaunchKernelGGL(mixture_norm_kernel, dim3(1), dim3(MX_THREADS), 0, h->stream, d_S, d_counts, L, d_d, d_act, d_G);
    HIP_TRY(hipGetLastError());
    MORNA_TRY(ev.record(2, h->stream));
    if (sums_out) HIP_TRY(hipMemcpyAsync(sums_out, d_sums, (size_t)L * D * 8, hipMemcpyDeviceToHost, h->stream));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, d_counts, (size_t)L * 4, hipMemcpyDeviceToHost, h->stream));
    if (gram_out) HIP_TRY(hipMemcpyAsync(gram_out, d_S, (size_t)L * L * 8, hipMemcpyDeviceToHost, h->stream));
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t q0 = 0; solve && q0 < nq; q0 += batch) {
        const int64_t nb = std::min(batch, nq - q0);
        MORNA_TRY(ev.record(3, h->stream));
        MORNA_TRY(exact_stage_queries(h, Q, q0, nb, d_items, d_Qd));
        const dim3 dgrid((unsigned)((nb + MX_DOT_QB - 1) / MX_DOT_QB));
        if (L > WAVE) hipLaunchKernelGGL(mixture_dots_kernel<2>, dgrid, dim3(MX_THREADS), 0, h->stream, d_Qd, nb, D, d_sT, LP, d_t, d_yy);
        else hipLaunchKernelGGL(mixture_dots_kernel<1>, dgrid, dim3(MX_THREADS), 0, h->stream, d_Qd, nb, D, d_sT, LP, d_t, d_yy);
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(4, h->stream));
        MixtureSolveArgs A;
        A.G = d_G;
        A.d = d_d;
        A.S = d_S;
        A.act = d_act;
        A.counts = d_counts;
        A.t = d_t;
        A.yy = d_yy;
        A.items = Q.items() ? d_items : nullptr;
        A.label = d_label;
        A.deny = rst ? rst->deny.p : nullptr;
        A.scale = W.scale;
        A.nb = nb;
        A.L = L;
        A.LP = LP;
        A.max_sweeps = max_sweeps;
        A.tol = tol;
        A.weights = d_w;
        A.info = d_info;
        A.active = d_active;
        const int64_t groups = (nb + MX_SOLVE_WAVES - 1) / MX_SOLVE_WAVES;
        const dim3 sgrid((unsigned)std::max<int64_t>(1, std::min<int64_t>(groups, h->n_cus)));
        const size_t lds = ((size_t)L * L + (size_t)MX_SOLVE_WAVES * L) * 8;
        MORNA_TRY(launch_lds(mixture_solve_kernel, sgrid, dim3(MX_SOLVE_THREADS), lds, LDS_DEFAULT, h->stream, A));
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(5, h->stream));
        HIP_TRY(hipMemcpyAsync(weights_out + q0 * L, d_w, (size_t)nb * L * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(info_out + q0 * 4, d_info, (size_t)nb * 32, hipMemcpyDeviceToHost, h->stream));
        if (active_out) HIP_TRY(hipMemcpyAsync(active_out + q0 * L, d_active, (size_t)nb * L, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        MORNA_TRY(ev.elapsed(3, 4, &ms[2]));
        MORNA_TRY(ev.elapsed(4, 5, &ms[3]));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    MORNA_TRY(ev.elapsed(0, 1, &ms[0]));
    MORNA_TRY(ev.elapsed(1, 2, &ms[1]));
    for (int i = 0; i < 4; i++) h->mixture_stats[i] = ms[i];
    if (solve) {
        double total = 0.0, largest = 0.0, open = 0.0;
        for (int64_t q = 0; q < nq; q++) {
            total += info_out[q * 4 + 2];
            largest = std::max(largest, info_out[q * 4 + 2]);
            open += info_out[q * 4 + 3] != 1.0 ? 1.0 : 0.0;
        }
        h->mixture_stats[4] = (double)nq;
        h->mixture_stats[5] = total;
        h->mixture_stats[6] = largest;
        h->mixture_stats[7] = open;
    }
    return MORNA_OK;
}

}  // namespace morna
