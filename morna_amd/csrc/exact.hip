// exact.hip -- the searches that read every row, on gfx950.
//
// exact_*_kernel : MornaSearch.exact_search_nn + cosine_distance (morna.py:
//                  681-716, 101-114) -- an fp32 scan of all rows picks every row
//                  that can be in the top k, then those rows are re-evaluated in
//                  the reference's sequential fp64 order and ranked with the
//                  bisect_left tie rule, so ids and distances are bit-exact.
// label_sums_kernel : per query and label, the integer sum of the scan's distances
//                  (morna_hip.h, "label distance sums").
// radius_*_kernel : every row within an fp64 distance of a query, from the same scan
//                  and the same fp64 chain (morna_hip.h, "radius search").
//                  The host side of the three (exact_search_any, label_sums,
//                  exact_radius; "the exact family, host side" below) is one front
//                  per call -- checks, the rows outside the scan's domain, the batch
//                  size, the workspace -- and per batch of queries
//                    front     the queries staged and widened, their fp32 images,
//                              the scan (exact_scan_mfma_kernel from 32 queries,
//                              exact_scan_kernel<qt> below), [exact_mask_kernel]
//                    select    the call's own kernels over the scan values
//                    deliver   the call's own copies
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "common.hpp"
#include "devutil.hpp"
#include "search_common.hpp"

namespace morna {

// =============================================================== exact search

#define E_ROWS 64       // rows per workgroup
// the domain of the scan's window (exact_scan_eps): rows by their fp32 norm2, queries by their fp64 sum of squares
#define EX_N2_LO 1.2621774483536189e-29   // 2^-96, times dpad
#define EX_N2_HI 8.5070591730234616e37f   // 2^126
#define EX_QQ_LO 0x1p-900
#define EX_QQ_HI 0x1p890

// approx[q][row] = 2 - 2 cos in fp32 arithmetic (selection only, never returned)
template <int E_QT>   // queries sharing one pass over a block of rows
__global__ __launch_bounds__(256) void exact_scan_kernel(const float *__restrict__ X, const float *__restrict__ norm2,
                                                         int64_t n_items, int32_t dpad,
                                                         const float *__restrict__ Qf /* [nq][dpad] */,
                                                         const float *__restrict__ qn2 /* [nq] */, int64_t nq,
                                                         float *__restrict__ approx /* [nq][n_items] */)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *qs = (float4 *)smem;   // [E_QT][nvec]
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int nvec = dpad / 4;
    const int64_t q0 = (int64_t)blockIdx.y * E_QT;
    const int nqt = (int)((nq - q0) < E_QT ? (nq - q0) : E_QT);
    for (int i = tid; i < E_QT * nvec; i += 256) {
        int qq = i / nvec, v = i - qq * nvec;
        qs[i] = qq < nqt ? ((const float4 *)(Qf + (q0 + qq) * dpad))[v] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * E_ROWS;
    for (int rr = w; rr < E_ROWS; rr += 4) {
        const int64_t r = r0 + rr;
        if (r >= n_items) break;
        const float4 *x = (const float4 *)(X + r * dpad);
        float acc[E_QT];
#pragma unroll
        for (int qq = 0; qq < E_QT; qq++) acc[qq] = 0.f;
        for (int i = lane; i < nvec; i += WAVE) {
            const float4 xv = x[i];
#pragma unroll
            for (int qq = 0; qq < E_QT; qq++) {
                const float4 qv = qs[qq * nvec + i];
                acc[qq] += xv.x * qv.x + xv.y * qv.y + xv.z * qv.z + xv.w * qv.w;
            }
        }
        const float rn = norm2[r];
#pragma unroll
        for (int qq = 0; qq < E_QT; qq++) {
            const float pq = wave_sum_xor(acc[qq]);
            if (lane == 0 && qq < nqt) {
                const double ppqq = (double)rn * (double)qn2[q0 + qq];
                approx[(q0 + qq) * n_items + r] = ppqq > 0.0 ? (float)(2.0 - 2.0 * (double)pq / sqrt(ppqq)) : 2.0f;
            }
        }
    }
}

// per query: threshold = k-th smallest approx value; candidates = everything within eps of it, and the rows outside the
// scan's domain (`outs`: their scan values are NaN, so they neither set the threshold nor pass it)
// RST: the restricted form.  A row that is not eligible for the query has the scan value NaN, as a row outside the domain
// has; the rows with a value are then counted per query (kk), and only the eligible rows of `outs` are appended.
template <bool RST>
__device__ __forceinline__ void exact_select_body(const float *__restrict__ approx, int64_t n_items,
                                                  int32_t k, float eps, int32_t cap,
                                                  const int32_t *__restrict__ outs, int32_t n_outs,
                                                  int32_t *__restrict__ cand /* [nq][cap] */,
                                                  int32_t *__restrict__ ncand_out /* [nq] */, const RestrictArgs &R)
{
    __shared__ uint64_t s_red[Q_WAVES];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const float *a = approx + qi * n_items;
    int32_t gq = -1;
    if constexpr (RST) gq = restrict_query_group(R, qi);
    auto value = [&](int64_t i) -> float {   // the scan value of row i as the selection sees it
        if constexpr (RST) return restrict_eligible(R, gq, i) ? a[i] : __builtin_nanf("");
        else return a[i];
    };
    int kk = (int)(k < n_items - n_outs ? k : n_items - n_outs);   // the k-th of the rows with a scan value
    if constexpr (RST) {
        __shared__ int s_valid;
        if (tid == 0) s_valid = 0;
        __syncthreads();
        int mine = 0;
        for (int64_t i = tid; i < n_items; i += 256) {
            const float v = value(i);
            mine += v == v ? 1 : 0;
        }
        atomicAdd(&s_valid, mine);
        __syncthreads();
        kk = k < s_valid ? k : s_valid;
    }
    uint64_t prev = 0;
    bool have_prev = false;
    constexpr int HELD = 32;   // a shard of up to 8192 rows: the scan values of the query stay in registers for all k rounds
    if (n_items <= 256 * HELD) {
        uint32_t key32[HELD];
#pragma unroll
        for (int u = 0; u < HELD; u++) {
            const int64_t i = tid + 256 * u;
            key32[u] = i < n_items ? f32_orderable(value(i)) : 0xffffffffu;
        }
        for (int r = 0; r < kk; r++) {
            uint64_t best = ~0ull;
#pragma unroll
            for (int u = 0; u < HELD; u++) {
                const uint64_t key = ((uint64_t)key32[u] << 32) | (uint32_t)(tid + 256 * u);
                if (tid + 256 * u < n_items && (!have_prev || key > prev) && key < best) best = key;
            }
            best = block_min_u64(best, s_red, tid);
            prev = best;
            have_prev = true;
        }
    } else {
        for (int r = 0; r < kk; r++) {
            uint64_t best = ~0ull;
            for (int64_t i = tid; i < n_items; i += 256) {
                const uint64_t key = ((uint64_t)f32_orderable(value(i)) << 32) | (uint32_t)i;
                if ((!have_prev || key > prev) && key < best) best = key;
            }
            best = block_min_u64(best, s_red, tid);
            prev = best;
            have_prev = true;
        }
    }
    const float thr = kk > 0 ? f32_from_orderable((uint32_t)(prev >> 32)) + eps : -INFINITY;
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int64_t i = tid; i < n_items; i += 256) {
        if (value(i) <= thr) {
            int slot = atomicAdd(&s_n, 1);
            if (slot < cap) cand[qi * cap + slot] = (int32_t)i;
        }
    }
    for (int j = tid; j < n_outs; j += 256) {
        if constexpr (RST) {
            if (!restrict_eligible(R, gq, outs[j])) continue;
        }
        const int slot = atomicAdd(&s_n, 1);
        if (slot < cap) cand[qi * cap + slot] = outs[j];
    }
    __syncthreads();
    if (tid == 0) ncand_out[qi] = s_n;   // may exceed cap: the host then retries with more room
}

__global__ __launch_bounds__(256) void exact_select_kernel(const float *__restrict__ approx, int64_t n_items,
                                                           int32_t k, float eps, int32_t cap,
                                                           const int32_t *__restrict__ outs, int32_t n_outs,
                                                           int32_t *__restrict__ cand /* [nq][cap] */,
                                                           int32_t *__restrict__ ncand_out /* [nq] */)
{
    exact_select_body<false>(approx, n_items, k, eps, cap, outs, n_outs, cand, ncand_out, RestrictArgs());
}

__global__ __launch_bounds__(256) void exact_select_restricted_kernel(const float *__restrict__ approx, int64_t n_items,
                                                                      int32_t k, float eps, int32_t cap,
                                                                      const int32_t *__restrict__ outs, int32_t n_outs,
                                                                      int32_t *__restrict__ cand /* [nq][cap] */,
                                                                      int32_t *__restrict__ ncand_out /* [nq] */, RestrictArgs R)
{
    exact_select_body<true>(approx, n_items, k, eps, cap, outs, n_outs, cand, ncand_out, R);
}

// cosine_distance in the reference's order (morna.py:101-114): one thread per candidate walks ITS row front to back in
// fp64 (pp += i*i; qq += j*j; pq += i*j), a 128-byte line of the row requested ahead of the one being consumed; the query
// is read through wave-uniform loads.  The pass is bound by the issue of its three dependent fp64 chains (8192 steps each
// at D = 8192), i.e. by the NUMBER of candidates: what keeps it short is the width of the scan's window (exact_scan_eps).
// Tried at configs[4]'s shard (6250 queries, ~100 candidates each when the window was 1e-3): rows staged through LDS by the
// whole workgroup 5.9 ms, a parallel-fp64 narrowing pass in front 4.4 ms, this form 3.4 ms.
#define RR_COLS 32
#define RR_THREADS 64   // one wave per query: the candidates are a few dozen, and a wave that waits for its chains leaves the SIMD to other queries
// The chain itself, one thread, one row: what exact_rerank_kernel and radius_dist_kernel both return.
__device__ __forceinline__ double exact_ref_distance(const float4 *__restrict__ row, const double *__restrict__ q, int32_t dim)
{
    double pp = 0.0, qq = 0.0, pq = 0.0;
    float4 cur[RR_COLS / 4], nxt[RR_COLS / 4];
#pragma unroll
    for (int u = 0; u < RR_COLS / 4; u++) cur[u] = row[u];   // (dpad is a multiple of 256: every line read exists)
    for (int z0 = 0; z0 < dim; z0 += RR_COLS) {
        const bool more = z0 + RR_COLS < dim;
#pragma unroll
        for (int u = 0; u < RR_COLS / 4; u++) nxt[u] = row[(more ? z0 + RR_COLS : z0) / 4 + u];
        const int zn = dim - z0 < RR_COLS ? dim - z0 : RR_COLS;
#pragma unroll
        for (int u = 0; u < RR_COLS / 4; u++) {
            const float e4[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
#pragma unroll
            for (int v = 0; v < 4; v++) {
                if (4 * u + v < zn) {
                    const double i = (double)e4[v], j = q[z0 + 4 * u + v];
                    pp = __dadd_rn(pp, __dmul_rn(i, i));
                    qq = __dadd_rn(qq, __dmul_rn(j, j));
                    pq = __dadd_rn(pq, __dmul_rn(i, j));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < RR_COLS / 4; u++) cur[u] = nxt[u];
    }
    const double ppqq = __dmul_rn(pp, qq);
    double distance = 2.0;
    if (ppqq > 0.0) distance = __dsub_rn(2.0, __ddiv_rn(__dmul_rn(2.0, pq), __dsqrt_rn(ppqq)));
    return __dsqrt_rn(distance);   // NaN where Python's math.sqrt raises
}

__global__ __launch_bounds__(RR_THREADS) void exact_rerank_kernel(const float *__restrict__ X, int32_t dim, int32_t dpad,
                                                           const double *__restrict__ Qd /* [nq][dim] */,
                                                           const int32_t *__restrict__ cand, const int32_t *__restrict__ ncand,
                                                           int32_t cap, int32_t k, double *__restrict__ cdist /* [nq][cap] */,
                                                           int32_t *__restrict__ ids_out, double *__restrict__ dist_out,
                                                           int32_t *__restrict__ count_out)
{
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const double *q = Qd + qi * dim;
    const int n = ncand[qi] < cap ? ncand[qi] : cap;
    const int32_t *c = cand + qi * cap;
    double *cd = cdist + qi * cap;
    for (int t = tid; t < n; t += RR_THREADS)
        cd[t] = exact_ref_distance((const float4 *)(X + (int64_t)c[t] * dpad), q, dim);
    // A NaN is a row for which Python's math.sqrt raises ValueError (negative radicand: the cosine rounded to more
    // than 1, i.e. a row all but parallel to the query).  The reference evaluates EVERY row, so one such row anywhere
    // fails the whole query; such a row has a scan distance of ~0 and is therefore always among the candidates.  The
    // query's count is reported as -1 and the caller raises (MornaSearch.exact_search_nn).
    __shared__ int s_nan;
    if (tid == 0) s_nan = 0;
    __syncthreads();
    {
        bool any_nan = false;
        for (int t = tid; t < n; t += RR_THREADS) any_nan |= cd[t] != cd[t];
        if (any_nan) s_nan = 1;
    }
    __syncthreads();
    // rank = number of candidates that bisect_left insertion leaves in front:
    // smaller distance, or equal distance and HIGHER id (inserted later, lands first).
    // NaN distances go last, by ascending id (the lists are still filled in, for diagnosis).
    for (int t = tid; t < n; t += RR_THREADS) {
        const double d = cd[t];
        const int32_t id = c[t];
        const bool dnan = d != d;
        int rank = 0;
        for (int u = 0; u < n; u++) {
            const double du = cd[u];
            const bool unan = du != du;
            bool before;
            if (dnan) before = !unan || c[u] < id;
            else before = (du < d) || (du == d && c[u] > id);
            rank += (before && u != t) ? 1 : 0;
        }
        if (rank < k) {
            ids_out[qi * k + rank] = id;
            dist_out[qi * k + rank] = d;
        }
    }
    const int kout = k < n ? k : n;
    for (int r = kout + tid; r < k; r += RR_THREADS) {
        ids_out[qi * k + r] = -1;
        dist_out[qi * k + r] = INFINITY;
    }
    if (tid == 0) count_out[qi] = s_nan ? -1 : kout;
}

// Selection for shards of more than 8192 rows: TWO passes over a query's scan values instead of k (the k rounds of
// exact_select_kernel read 4 * N * k bytes per query: 200 GB for configs[4]'s 50 000 queries x 50 000 rows, k = 20).
//   A  every thread takes the minimum of its strided share; the kk-th smallest of the 256 minima bounds the kk-th smallest
//      value from above (kk distinct elements lie at or below it);
//   B  everything within eps of that bound is collected as (key, id) pairs -- a superset of the candidates;
//   C  the kk-th smallest of the collected pairs, by counting, IS the kk-th smallest of all values: thr = it + eps;
//   D  the candidates are the collected pairs at or below thr -- the set exact_select_kernel produces.
// `pairs` is the memory of the re-rank's distance array (not yet in use).  More collected than `cap`: the count is reported
// and the host retries with room for all of them, as for the candidates themselves.  Needs k <= 256 (one minimum per thread).
// The rows outside the scan's domain (`outs`, scan value NaN) are appended to the candidates.  When they leave fewer than kk
// of the 256 minima a value, the bound of A is +inf (B collects every row with a value).
// RST: the restricted form, as in exact_select_body: a row that is not eligible has the value NaN, the rows with a value
// are counted in pass A (which reads every value anyway), and a thread's share without an eligible value is a share of NaNs.
template <bool RST>
__device__ __forceinline__ void exact_select2_body(const float *__restrict__ approx, int64_t n_items, int32_t k, float eps,
                                                   int32_t cap, const int32_t *__restrict__ outs, int32_t n_outs,
                                                   uint2 *__restrict__ pairs /* [nq][cap] */,
                                                   int32_t *__restrict__ cand /* [nq][cap] */,
                                                   int32_t *__restrict__ ncand_out /* [nq] */, const RestrictArgs &R)
{
    __shared__ uint64_t s_key[256];
    __shared__ int s_n;
    __shared__ uint32_t s_thr;
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const float *a = approx + qi * n_items;
    int32_t gq = -1;
    if constexpr (RST) gq = restrict_query_group(R, qi);
    auto value = [&](int64_t i) -> float {
        if constexpr (RST) return restrict_eligible(R, gq, i) ? a[i] : __builtin_nanf("");
        else return a[i];
    };
    auto append_outs = [&]() {
        for (int j = tid; j < n_outs; j += 256) {
            if constexpr (RST) {
                if (!restrict_eligible(R, gq, outs[j])) continue;
            }
            const int slot = atomicAdd(&s_n, 1);
            if (slot < cap) cand[qi * cap + slot] = outs[j];
        }
    };
    int kk = (int)(k < n_items - n_outs ? k : n_items - n_outs);
    uint64_t mine = ~0ull;
    if constexpr (!RST) {
        if (kk <= 0) {   // every row is outside the domain
            if (tid == 0) s_n = 0;
            __syncthreads();
            append_outs();
            __syncthreads();
            if (tid == 0) ncand_out[qi] = s_n;
            return;
        }
        for (int64_t i = tid; i < n_items; i += 256) {
            const uint64_t key = ((uint64_t)f32_orderable(a[i]) << 32) | (uint32_t)i;
            mine = key < mine ? key : mine;
        }
    } else {
        __shared__ int s_valid;
        if (tid == 0) s_valid = 0;
        __syncthreads();
        int valid = 0;
        for (int64_t i = tid; i < n_items; i += 256) {
            const float v = value(i);
            valid += v == v ? 1 : 0;
            const uint64_t key = ((uint64_t)f32_orderable(v) << 32) | (uint32_t)i;
            mine = key < mine ? key : mine;
        }
        atomicAdd(&s_valid, valid);
        __syncthreads();
        kk = k < s_valid ? k : s_valid;
        if (kk <= 0) {   // no eligible row has a scan value
            if (tid == 0) s_n = 0;
            __syncthreads();
            append_outs();
            __syncthreads();
            if (tid == 0) ncand_out[qi] = s_n;
            return;
        }
    }
    s_key[tid] = mine;
    if (tid == 0) s_n = 0;
    __syncthreads();
    {
        int below = 0;
        for (int j = 0; j < 256; j++) below += s_key[j] < mine ? 1 : 0;
        if (mine != ~0ull && below == kk - 1) s_thr = (uint32_t)(mine >> 32);
    }
    __syncthreads();
    float bound = f32_from_orderable(s_thr) + eps;
    if (bound != bound) bound = INFINITY;   // the kk-th minimum is a NaN: a thread's share held only rows outside the domain
    uint2 *pr = pairs + qi * cap;
    for (int64_t i = tid; i < n_items; i += 256) {
        const float v = value(i);
        if (v <= bound) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < cap) pr[slot] = make_uint2(f32_orderable(v), (uint32_t)i);
        }
    }
    __syncthreads();
    const int m = s_n;
    if (m > cap) {
        if (tid == 0) ncand_out[qi] = m + n_outs;
        return;
    }
    for (int t = tid; t < m; t += 256) {
        const uint2 p = pr[t];
        const uint64_t kt = ((uint64_t)p.x << 32) | p.y;
        int below = 0;
        for (int u = 0; u < m; u++) {
            const uint2 o = pr[u];
            below += (((uint64_t)o.x << 32) | o.y) < kt ? 1 : 0;
        }
        if (below == kk - 1) s_thr = p.x;
    }
    __syncthreads();
    const float thr = f32_from_orderable(s_thr) + eps;
    __syncthreads();
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int t = tid; t < m; t += 256) {
        const uint2 p = pr[t];
        if (f32_from_orderable(p.x) <= thr) cand[qi * cap + atomicAdd(&s_n, 1)] = (int32_t)p.y;
    }
    append_outs();
    __syncthreads();
    if (tid == 0) ncand_out[qi] = s_n;
}

__global__ __launch_bounds__(256) void exact_select2_kernel(const float *__restrict__ approx, int64_t n_items, int32_t k, float eps,
                                                            int32_t cap, const int32_t *__restrict__ outs, int32_t n_outs,
                                                            uint2 *__restrict__ pairs /* [nq][cap] */,
                                                            int32_t *__restrict__ cand /* [nq][cap] */,
                                                            int32_t *__restrict__ ncand_out /* [nq] */)
{
    exact_select2_body<false>(approx, n_items, k, eps, cap, outs, n_outs, pairs, cand, ncand_out, RestrictArgs());
}

__global__ __launch_bounds__(256) void exact_select2_restricted_kernel(const float *__restrict__ approx, int64_t n_items, int32_t k,
                                                                       float eps, int32_t cap, const int32_t *__restrict__ outs,
                                                                       int32_t n_outs, uint2 *__restrict__ pairs /* [nq][cap] */,
                                                                       int32_t *__restrict__ cand /* [nq][cap] */,
                                                                       int32_t *__restrict__ ncand_out /* [nq] */, RestrictArgs R)
{
    exact_select2_body<true>(approx, n_items, k, eps, cap, outs, n_outs, pairs, cand, ncand_out, R);
}

// The query of exact_search_nn when it is a STORED row (or an fp32 row handed over in device memory): the fp32 values
// widened to fp64 -- what `zip(self.annoy_index.get_item_vector(i), query)` sees when the query came out of the index
// (morna.py:697-703).  One workgroup per query; src_stride floats between rows, items == null: row q.
__global__ void exact_widen_kernel(const float *__restrict__ src, int64_t src_stride, const int32_t *__restrict__ items,
                                   int32_t dim, double *__restrict__ Qd)
{
    const int64_t q = blockIdx.x;
    const float *row = src + (items ? (int64_t)items[q] : q) * src_stride;
    for (int z = threadIdx.x; z < dim; z += blockDim.x) Qd[q * dim + z] = (double)row[z];
}

// a batch's exact answers -> their place in the message of the row-sharded exact search (global ids)
__global__ void exact_pack_kernel(const int32_t *__restrict__ ids, const double *__restrict__ dist, const int32_t *__restrict__ cnt,
                                  int64_t nb, int32_t k, int32_t id_offset, int32_t *__restrict__ m_ids, int32_t *__restrict__ m_cnt,
                                  double *__restrict__ m_dist)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb * k) {
        const int32_t id = ids[i];
        m_ids[i] = id >= 0 ? id + id_offset : -1;
        m_dist[i] = dist[i];
    }
    if (i < nb) m_cnt[i] = cnt[i];
}

// fp64 query -> fp32 image + its squared norm (selection pass only).  The image is of the query times 2^s, s chosen so that
// its largest |element| lies in [1, 2): cos does not change, no element of a finite query overflows fp32 and the norm is at
// least 1 (exact_scan_eps).  Where the unscaled image was normal and finite, the scan values are the unscaled ones bit for
// bit.  A query outside the domain -- its fp64 sum of squares qq outside [EX_QQ_LO, EX_QQ_HI], NaN and inf included (only
// fp32 queries in device memory are not checked on the host) -- gets a zero image: every row then ties at 2 and is
// re-ranked, as the reference evaluates it.
__global__ void exact_prep_kernel(const double *__restrict__ Qd, int64_t nq, int32_t dim, int32_t dpad,
                                  float *__restrict__ Qf, float *__restrict__ qn2)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    if (q >= nq) return;
    double mx = 0.0, qq = 0.0;
    for (int i = lane; i < dim; i += WAVE) {
        const double v = Qd[q * dim + i];
        mx = fmax(mx, fabs(v));   // (fmax drops a NaN: qq does not)
        qq += v * v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, off, WAVE));
        qq += __shfl_xor(qq, off, WAVE);
    }
    const bool inside = qq >= EX_QQ_LO && qq <= EX_QQ_HI;   // (any summation order: the bounds keep wide margins)
    int e = 0;
    if (mx > 0.0) (void)frexp(mx, &e);   // mx = f 2^e, f in [0.5, 1)
    float s = 0.f;
    for (int i = lane; i < dpad; i += WAVE) {
        float v = i < dim && inside ? (float)ldexp(Qd[q * dim + i], 1 - e) : 0.f;   // (exact where the result reaches fp32's range)
        Qf[q * dpad + i] = v;
        s += v * v;
    }
    s = wave_sum_xor(s);
    if (lane == 0) qn2[q] = s;
}

// ---- batched scan on the matrix cores ---------------------------------------------
// Many queries against all rows is a dense contraction C[q][r] = sum_d Q[q][d] X[r][d]
// (2*Q*N*D flop over 4*D*(Q+N) bytes per tile pass): the one GEMM-shaped piece of the
// path, so it runs on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate).
// 128 queries x 128 rows per workgroup, K stepped by 32 through LDS, each of the 4 waves
// owns a 64 x 64 quadrant as 2 x 2 MFMA tiles.  The result only SELECTS candidates; the
// returned distances are recomputed in the reference's fp64 order by exact_rerank_kernel.
#define MM_TILE 128
#define MM_BK 32
#define MM_LD (MM_BK + 4)   // padded LDS row (floats); 144-byte rows keep float4 accesses aligned
#define MM_FLUSH 128        // columns per accumulation chain of the scan (a multiple of MM_BK, a power of two)
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256, 2) void exact_scan_mfma_kernel(const float *__restrict__ X, const float *__restrict__ norm2,
                                                              int64_t n_items, int32_t dpad,
                                                              const float *__restrict__ Qf, const float *__restrict__ qn2,
                                                              int64_t nq, float *__restrict__ approx)
{
    __shared__ __attribute__((aligned(16))) float As[MM_TILE * MM_LD];   // queries  [128][36]
    __shared__ __attribute__((aligned(16))) float Bs[MM_TILE * MM_LD];   // rows     [128][36]
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int wm = w >> 1, wn = w & 1;                 // the wave's 64 x 64 quadrant
    const int64_t r0 = (int64_t)blockIdx.x * MM_TILE, q0 = (int64_t)blockIdx.y * MM_TILE;

    // global -> register staging: 4 float4 per operand per thread (row = idx / 8, 16-byte column = idx % 8)
    float4 ga[4], gb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int idx = tid + it * 256, row = idx >> 3, c4 = idx & 7;
            const int64_t q = q0 + row, r = r0 + row;
            ga[it] = q < nq ? *(const float4 *)(Qf + q * dpad + k0 + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            gb[it] = r < n_items ? *(const float4 *)(X + r * dpad + k0 + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int idx = tid + it * 256, row = idx >> 3, c4 = idx & 7;
            *(float4 *)(As + row * MM_LD + c4 * 4) = ga[it];
            *(float4 *)(Bs + row * MM_LD + c4 * 4) = gb[it];
        }
    };
    // Blocked accumulation: the running accumulator of a tile is added into a second one every MM_FLUSH columns and
    // cleared, so that a chain of fmaf is MM_FLUSH products long and the second level adds dpad / MM_FLUSH partial sums --
    // an error bound of (MM_FLUSH + dpad / MM_FLUSH) u instead of dpad / 2 u (one chain per half of the columns, as this
    // kernel first had it): the selection window of exact_scan_eps() is 12x narrower at D = 8192, and the fp64 re-rank,
    // whose time is the number of candidates, 3-4x shorter.
    f32x16 acc[2][2], acc_b[2][2];   // running chain; sum of the flushed chains
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[i][j][e] = acc_b[i][j][e] = 0.f;

    fetch(0);
    stash();
    __syncthreads();
    const int lr = lane & 31, lh = lane >> 5;
    for (int k0 = 0; k0 < dpad; k0 += MM_BK) {
        const bool more = k0 + MM_BK < dpad;
        if (more) fetch(k0 + MM_BK);                   // next K slab in flight under the MFMAs
#pragma unroll
        for (int blk = 0; blk < MM_BK / 8; blk++) {
            // lane half h supplies k = 8*blk + 4*h + j to MFMA j: any k order is a valid sum here
            float4 a4[2], b4[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                a4[t] = *(const float4 *)(As + (wm * 64 + t * 32 + lr) * MM_LD + blk * 8 + lh * 4);
                b4[t] = *(const float4 *)(Bs + (wn * 64 + t * 32 + lr) * MM_LD + blk * 8 + lh * 4);
            }
#pragma unroll
            for (int tm = 0; tm < 2; tm++)
#pragma unroll
                for (int tn = 0; tn < 2; tn++) {
                    f32x16 &c = acc[tm][tn];
                    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tm].x, b4[tn].x, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tm].y, b4[tn].y, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tm].z, b4[tn].z, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[tm].w, b4[tn].w, c, 0, 0, 0);
                }
        }
        if (((k0 + MM_BK) & (MM_FLUSH - 1)) == 0 || !more) {   // uniform: the chain ends here
#pragma unroll
            for (int tm = 0; tm < 2; tm++)
#pragma unroll
                for (int tn = 0; tn < 2; tn++) {
                    acc_b[tm][tn] = acc_b[tm][tn] + acc[tm][tn];
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[tm][tn][e] = 0.f;
                }
        }
        __syncthreads();
        if (more) stash();
        __syncthreads();
    }
#pragma unroll
    for (int tm = 0; tm < 2; tm++)
#pragma unroll
        for (int tn = 0; tn < 2; tn++) acc[tm][tn] = acc_b[tm][tn];
    // epilogue: C/D layout of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5).
    // A (queries) indexes the rows of the tile, B (matrix rows) its columns: 32 lanes write 32 consecutive r.
#pragma unroll
    for (int tm = 0; tm < 2; tm++)
#pragma unroll
        for (int tn = 0; tn < 2; tn++) {
            const int64_t r = r0 + wn * 64 + tn * 32 + lr;
            const float rn = r < n_items ? norm2[r] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int64_t q = q0 + wm * 64 + tm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (q < nq && r < n_items) {
                    const double ppqq = (double)rn * (double)qn2[q];
                    approx[q * n_items + r] = ppqq > 0.0 ? (float)(2.0 - 2.0 * (double)acc[tm][tn][e] / sqrt(ppqq)) : 2.0f;
                }
            }
        }
}

// How far the scan's 2 - 2 cos can be from the exact value, times two (the k-th smallest scan value that sets the
// threshold and the candidate itself can both be off): every row within this of the threshold is kept, so no row
// of the true top k is lost.  Unit roundoff u = 2^-24, errors relative to |x| |q| >= sum |x_i q_i|:
//   dot, vector-ALU scan : a lane adds dpad / 64 products in turn, then the 6-stage butterfly
//   dot, matrix-core scan: chains of MM_FLUSH products (v_mfma_f32_32x32x2_f32 is a chain of IEEE fmaf: measured bit for
//                          bit on MI355X by scripts/mfma_accum_probe.hip, profiles/r02_mfma_accum_probe.txt), their
//                          dpad / MM_FLUSH partial sums added one after the other
//   norms (norm2 of the row, qn2 of the query): sums of dpad / 64 squares per lane + butterfly; half of each enters cos
//   the fp32 image of the query and the rounding of the value itself: 2 u
//   underflow: u / 8 (below)
// Domain.  Relative error terms hold for normal numbers.  The query's image is scaled so that its largest |element| is in
// [1, 2) (exact_prep_kernel): |q| >= 1, nothing overflows, and an element lost to underflow costs at most 2^-126 |x_i|.
// A row is inside the domain when its fp32 norm2 lies in [dpad 2^-96, 2^126] (EX_N2_LO, EX_N2_HI).  Then every partial
// sum stays finite, and each of the <= dpad products or squares loses at most 2^-124 absolute to underflow (even with
// denormals flushed), i.e. at most 2^-28 of norm2 and sqrt(dpad) 2^-76 of |x| |q| -- inside the u / 8 term.  Rows outside
// the domain (norm2 of 0 for a non-zero row, subnormal, tiny, inf or NaN: a row with a non-finite element) are on the list
// of exact_outside_kernel: their scan values are NaN, they take no part in the threshold, and every query re-ranks them,
// which gives the reference's value whatever it is.  A zero row is inside: both give 2.
// The window bounds the error against the TRUE 2 - 2cos; the re-rank returns the reference's fp64 value, which is that
// only while its own arithmetic stays normal.  For a row inside the domain the fp64 pp lies in [2^-97, 2^127]; a query
// whose fp64 qq lies in [EX_QQ_LO, EX_QQ_HI] = [2^-900, 2^890] keeps pp qq in [2^-997, 2^1017], normal, and what pq and qq
// lose to fp64 underflow (<= 32768 2^-1075) is nothing beside sqrt(pp qq) or qq.  Outside those bounds cosine_distance can
// give 2 where the cosine is not 0 (pp qq underflows to 0 or overflows): such a query is compared with every row
// (exact_prep_kernel gives it a zero image), as the reference does.
static float exact_scan_eps(int32_t dpad, bool mfma)
{
    const double u = 5.9604644775390625e-8;
    const double e_dot = mfma ? (MM_FLUSH + dpad / MM_FLUSH + 8) * u : (dpad / 64 + 8) * u;
    const double e_norm = (dpad / 64 + 8) * u;
    return (float)(2.0 * 2.0 * (e_dot + e_norm + 2 * u + u / 8));
}

// The window of the radius search (morna_exact_radius): row i is a candidate iff its scan value
//     v <= fl_up((float)(r * r)) + eps,     eps = exact_scan_eps(dpad, which scan ran), the sum taken in fp64 (exact).
// Derivation.  Let t be the true 2 - 2cos and D the reference's fp64 radicand (exact_ref_distance returns sqrt(D)).  The row
// belongs to the answer iff sqrt(D) <= r in fp64.  Correctly rounded sqrt is monotone, so sqrt(D) <= r implies
// D <= r^2 (1 + 2^-52); the fp64 chain keeps |D - t| below dpad 2^-50, and the scan keeps |v - t| <= eps / 2 (eps is the
// bound above taken twice, for the two values the top-k threshold compares; here there is one).  So a row of the answer has
//     v <= t + eps / 2 <= r^2 + eps / 2 + (r^2 2^-52 + dpad 2^-50).
// w = (float)(r * r) is r^2 rounded twice to nearest, at worst a little under half an fp32 ulp below r^2; the next float up,
// fl_up(w), is at least r^2 (and +inf when r^2 overflows fp32: every row is then a candidate, which r >= 2 means anyway).
// The bracket is at most 2^-34 for r <= 2 and dpad <= 32768 while eps / 2 is at least 2^-19: the unused half of eps covers
// it.  Nothing more is added: every candidate costs one fp64 chain in radius_dist_kernel.
// NaN rows: the radicand is negative only when the fp64 cosine rounds above 1, so t < dpad 2^-50 and v <= eps / 2 + that:
// inside the window of every r >= 0.
static double exact_radius_window(double r, float eps)
{
    const float w = (float)(r * r);
    return (double)nextafterf(w, INFINITY) + (double)eps;
}

// The rows outside the scan's domain (exact_scan_eps): non-zero rows whose fp32 norm2 is below lo or above EX_N2_HI (NaN
// included: a row with a NaN or inf element is one of them).  out[0] counts them into out[1..].  Only those few rows are
// read.
__global__ void exact_outside_kernel(const float *__restrict__ X, const float *__restrict__ norm2, int64_t n_items, int32_t dim,
                                     int32_t dpad, float lo, int32_t *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_items) return;
    const float n = norm2[r];
    if (n >= lo && n <= EX_N2_HI) return;
    bool nonzero = false;
    const float *x = X + r * dpad;
    for (int z = 0; z < dim; z++) nonzero |= x[z] != 0.f;   // (a NaN is non-zero)
    if (nonzero) out[1 + atomicAdd(&out[0], 1)] = (int32_t)r;
}

// scan value NaN for the rows outside the domain, every query of the batch
__global__ void exact_mask_kernel(const int32_t *__restrict__ outs, int32_t n_outs, int64_t nb, int64_t n_items,
                                  float *__restrict__ approx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * n_outs) return;
    const int64_t q = i / n_outs;
    approx[q * n_items + outs[i - q * n_outs]] = __builtin_nanf("");
}

// made once per row set (invalidated wherever rows or norms change: compute_norms, the fused feature build, load).  Rows
// with a non-finite element are not refused: re-ranked like the others on the list, they get the reference's value (2
// for a NaN row, NaN -- count -1 -- for most inf rows), and every shard of a sharded search answers in the same way.
static int exact_outside_rows(morna_index *h)
{
    if (!h->ex_out_valid) {
        const int64_t N = h->n_items;
        MORNA_TRY(h->ex_out.alloc((size_t)N + 1));
        HIP_TRY(hipMemsetAsync(h->ex_out.p, 0, 4, h->stream));
        hipLaunchKernelGGL(exact_outside_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, h->X.p,
                           h->norm2.p, N, h->dim, h->dpad, (float)(EX_N2_LO * h->dpad), h->ex_out.p);
        HIP_TRY(hipGetLastError());
        int32_t got = 0;
        HIP_TRY(hipMemcpyAsync(&got, h->ex_out.p, 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->ex_out_n = got;
        h->ex_out_valid = true;
    }
    return MORNA_OK;
}

template <int QT>
static int launch_exact_scan(morna_index *h, int64_t N, int64_t nb, const float *Qf, const float *qn2, float *approx)
{
    dim3 grid((unsigned)((N + E_ROWS - 1) / E_ROWS), (unsigned)((nb + QT - 1) / QT));
    // (the limit is raised for one query image past 16384 floats)
    return launch_lds(exact_scan_kernel<QT>, grid, dim3(256), (size_t)QT * h->dpad * 4, LDS_64K, h->stream, h->X.p, h->norm2.p, N,
                      h->dpad, Qf, qn2, nb, approx);
}

// Message of the row-sharded exact search, nq queries: ids int32 [nq][k] (global, -1 = empty) | count int32 [nq] (-1: the
// reference raises for this query) | pad to 8 bytes | distances fp64 [nq][k]
size_t exact_msg_dist_offset(int64_t nq, int32_t k) { return align_up((size_t)nq * ((size_t)k + 1) * 4, 8); }
size_t exact_msg_bytes(int64_t nq, int32_t k) { return exact_msg_dist_offset(nq, k) + (size_t)nq * k * 8; }

// ---- the exact family, host side ---------------------------------------------------------------------------------------
// exact_search_any, label_sums and exact_radius read from top to bottom: the front (exact_front: the checks, the rows outside
// the scan's domain, the batch size, the workspace), then per batch the front's part (exact_front_batch: the queries' groups,
// the scan, the mask), the call's own selection and its own delivery, and last the call's statistics.

// What every caller of the scan checks first: host queries finite with a finite sum of squares in the reference's order
// (cosine_distance), stored rows in range, the row width within the scan's.  qt_out: the queries that share one pass of
// exact_scan_kernel (their fp32 images share 64 KiB of LDS).  who: the name the messages open with.
int exact_check_queries(morna_index *h, const char *who, const ExactQueries &Q, int64_t nq, int *qt_out)
{
    const int64_t N = h->n_items;
    const int32_t D = h->dim, dpad = h->dpad;
    if (const double *q_host = Q.host64())   // the contract: finite elements and a finite sum of squares in the reference's order (cosine_distance)
        for (int64_t i = 0; i < nq; i++) {
            double qq = 0.0;
            for (int32_t z = 0; z < D; z++) {
                const double j = q_host[i * D + z], jj = j * j;
                qq = qq + jj;
            }
            if (!(qq <= DBL_MAX)) {
                set_error("%s: query %lld has a non-finite element or sum of squares", who, (long long)i);
                return MORNA_E_INVALID;
            }
        }
    if (const int32_t *items_host = Q.items())
        for (int64_t i = 0; i < nq; i++)
            if (items_host[i] < 0 || items_host[i] >= N) {
                set_error("Item index %d out of range [0, %lld)", items_host[i], (long long)N);
                return MORNA_E_RANGE;
            }
    // queries resident per pass: their fp32 images share 64 KiB of LDS
    *qt_out = (size_t)dpad * 4 * 8 <= 65536 ? 8 : (size_t)dpad * 4 * 4 <= 65536 ? 4 : (size_t)dpad * 4 * 2 <= 65536 ? 2 : 1;
    if (dpad > Q_MAX_DPAD) {   // exact_scan_kernel<1> keeps the query's fp32 image in LDS (128 KiB at 32768)
        set_error("%s: dimension %d is above the supported %d", who, D, Q_MAX_DPAD);
        return MORNA_E_INVALID;
    }
    return MORNA_OK;
}

// What a call works out once, before its first batch.
struct ExactFront {
    ExactQueries Q;
    int64_t N;
    int32_t D, dpad;
    int qt;                        // queries that share one pass of exact_scan_kernel
    int32_t n_outs;                // the rows outside the scan's domain (exact_outside_rows): re-ranked, or refused, by the caller
    const int32_t *outs;
    int64_t batch;                 // queries per batch
    const int32_t *q_group_host;   // the queries' groups, when the call has them (else null: nothing is staged)
    RestrictArgs R;
    // a batch's pieces of h->ex_ws (the caller's own follow them)
    double *Qd;                    // [batch][D] the queries as the re-rank reads them
    float *Qf, *qn2;               // [batch][dpad], [batch] their fp32 images and norms
    int32_t *d_items;              // [batch] by item, else null
    int32_t *d_qg;                 // [batch] with q_group_host, else null
    float *approx;                 // [batch][N] the scan values
};

// The once-per-call part.  who: the entry point (its name in the messages too).  own_checks() -> int: the caller's argument
// checks, made after the common refusals and before anything is looked at on the device; with no queries the front returns
// behind them and leaves F unset.  batch_cap > 0: no more queries per batch than that.  own_layout(Carver &, batch): the
// caller's pieces of h->ex_ws, behind the common ones.  The workspace stays with the handle (a hipMalloc / hipFree pair per
// array and call cost more than a small search).
template <class Checks, class Layout>
static int exact_front(morna_index *h, const char *who, const char *name, const morna_restriction *rst, const ExactQueries &Q,
                       int64_t nq, const int32_t *q_group_host, int64_t batch_cap, Checks &&own_checks, Layout &&own_layout,
                       ExactFront &F)
{
    MORNA_TRY(finish_build(h, who));   // (shares the handle's stream and workspace with the tail of a pending build)
    MORNA_TRY(upload_host_rows(h));
    if (rst) MORNA_TRY(restriction_usable(h, rst));
    if (h->n_items <= 0) {
        set_error("%s on an empty index", name);
        return MORNA_E_EMPTY;
    }
    MORNA_TRY(own_checks());
    if (nq == 0) return MORNA_OK;
    F.Q = Q;
    F.N = h->n_items;
    F.D = h->dim;
    F.dpad = h->dpad;
    MORNA_TRY(exact_check_queries(h, "exact search", Q, nq, &F.qt));   // (the family's wording, whichever entry point)
    MORNA_TRY(exact_outside_rows(h));
    F.n_outs = h->ex_out_n;
    F.outs = h->ex_out.p + 1;
    // queries per batch: approx[nq][N] floats capped at 2 GiB
    F.batch = std::max<int64_t>(1, std::min<int64_t>(nq, ((int64_t)1 << 29) / std::max<int64_t>(F.N, 1)));
    if (batch_cap > 0) F.batch = std::min(F.batch, batch_cap);
    F.q_group_host = rst && rst->has_group ? q_group_host : nullptr;   // (the one condition under which groups are staged)
    MORNA_TRY(carve_workspace(h->ex_ws, [&](Carver &c) {
        const size_t b = (size_t)F.batch;
        F.Qd = c.take<double>(b * F.D);
        F.Qf = c.take<float>(b * F.dpad);
        F.qn2 = c.take<float>(b);
        F.d_items = Q.items() ? c.take<int32_t>(b) : nullptr;
        F.d_qg = F.q_group_host ? c.take<int32_t>(b) : nullptr;
        F.approx = c.take<float>(b * F.N);
        own_layout(c, F.batch);
    }));
    F.R = restrict_args(rst, F.d_qg);
    return MORNA_OK;
}

// queries q0 .. q0 + nb of a call staged as fp64 rows Qd[nb][dim] on the handle's stream, from any of the four sources; by
// item their ids go to d_items[nb] first
int exact_stage_queries(morna_index *h, const ExactQueries &Q, int64_t q0, int64_t nb, int32_t *d_items, double *Qd)
{
    const int32_t D = h->dim, dpad = h->dpad;
    switch (Q.source) {
    case ExactQueries::HOST_F64:
        HIP_TRY(hipMemcpyAsync(Qd, Q.host64() + q0 * D, (size_t)nb * D * 8, hipMemcpyHostToDevice, h->stream));
        break;
    case ExactQueries::DEV_F32:
        hipLaunchKernelGGL(exact_widen_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, Q.dev32() + q0 * D, (int64_t)D, nullptr, D, Qd);
        break;
    case ExactQueries::DEV_F64:
        HIP_TRY(hipMemcpyAsync(Qd, Q.dev64() + q0 * D, (size_t)nb * D * 8, hipMemcpyDeviceToDevice, h->stream));
        break;
    case ExactQueries::ITEMS:
        HIP_TRY(hipMemcpyAsync(d_items, Q.items() + q0, (size_t)nb * 4, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(exact_widen_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, h->X.p, (int64_t)dpad, d_items, D, Qd);
        break;
    }
    return MORNA_OK;
}

// queries q0 .. q0 + nb of the call staged as fp64 (Qd), their fp32 images and norms made, and the scan run over every row --
// approx[nb][N], nothing masked.  The MFMA scan for 32 queries or more, exact_scan_kernel<qt> below.
static int exact_scan_batch(morna_index *h, const ExactFront &F, int64_t q0, int64_t nb)
{
    const int64_t N = F.N;
    const int32_t D = F.D, dpad = F.dpad;
    MORNA_TRY(exact_stage_queries(h, F.Q, q0, nb, F.d_items, F.Qd));
    // one pass over the matrix per qt queries: 4*D*N bytes each
    const int64_t q_per_pass = nb >= 32 ? MM_TILE : F.qt;
    ScopedTimer tm(h, MORNA_T_EXACT, 4 * (int64_t)D * N * ((nb + q_per_pass - 1) / q_per_pass));
    hipLaunchKernelGGL(exact_prep_kernel, dim3((unsigned)((nb * WAVE + 255) / 256)), dim3(256), 0, h->stream,
                       F.Qd, nb, D, dpad, F.Qf, F.qn2);
    ScopedTimer ts(h, MORNA_T_EXACT_SCAN, nb >= 32 ? 2 * (int64_t)nb * N * dpad : 0);   // "bytes" = flops on the matrix cores
    if (nb >= 32) {   // enough queries to fill MFMA tiles: dense contraction on the matrix cores
        dim3 grid((unsigned)((N + MM_TILE - 1) / MM_TILE), (unsigned)((nb + MM_TILE - 1) / MM_TILE));
        hipLaunchKernelGGL(exact_scan_mfma_kernel, grid, dim3(256), 0, h->stream, h->X.p, h->norm2.p, N, dpad, F.Qf,
                           F.qn2, nb, F.approx);
    } else if (F.qt == 8) MORNA_TRY((launch_exact_scan<8>(h, N, nb, F.Qf, F.qn2, F.approx)));
    else if (F.qt == 4) MORNA_TRY((launch_exact_scan<4>(h, N, nb, F.Qf, F.qn2, F.approx)));
    else if (F.qt == 2) MORNA_TRY((launch_exact_scan<2>(h, N, nb, F.Qf, F.qn2, F.approx)));
    else MORNA_TRY((launch_exact_scan<1>(h, N, nb, F.Qf, F.qn2, F.approx)));
    return MORNA_OK;
}

// The front of a batch, queries q0 .. q0 + nb: their groups staged when the call has them, the scan, and with `mask` the
// scan values of the rows outside the domain made NaN.  ev (or null): event 0 is recorded in front of the scan, event 1
// behind it and the mask.  *eps: the window of the scan that ran (exact_scan_eps).
static int exact_front_batch(morna_index *h, const ExactFront &F, int64_t q0, int64_t nb, bool mask, HipEvents *ev, float *eps)
{
    if (F.d_qg) HIP_TRY(hipMemcpyAsync(F.d_qg, F.q_group_host + q0, (size_t)nb * 4, hipMemcpyHostToDevice, h->stream));
    if (ev) MORNA_TRY(ev->record(0, h->stream));
    MORNA_TRY(exact_scan_batch(h, F, q0, nb));
    if (mask && F.n_outs > 0)
        hipLaunchKernelGGL(exact_mask_kernel, dim3((unsigned)((nb * F.n_outs + 255) / 256)), dim3(256), 0, h->stream, F.outs,
                           F.n_outs, nb, F.N, F.approx);
    HIP_TRY(hipGetLastError());
    if (ev) MORNA_TRY(ev->record(1, h->stream));
    *eps = exact_scan_eps(F.dpad, nb >= 32);
    return MORNA_OK;
}

// A workgroup of `threads` per (query, chunk of rows): about 2048 workgroups when the batch is small, whole rows past that.
// Returns the chunks of a query; chunk_rows: the rows of a chunk, a multiple of `threads`.
static int32_t exact_row_chunks(int64_t N, int64_t nb, int threads, int64_t *chunk_rows)
{
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((2048 + nb - 1) / nb, (N + 2047) / 2048));
    *chunk_rows = ((N + chunks - 1) / chunks + threads - 1) / threads * threads;
    return (int32_t)((N + *chunk_rows - 1) / *chunk_rows);
}

// The answers: host arrays, and / or msg_dev (device memory, exact_msg_bytes(nq, k)) with global ids = local + id_offset --
// then only enqueued on the handle's stream behind the last selection.
int exact_search_any(morna_index *h, const ExactQueries &Q, int64_t nq, int32_t k, int32_t *ids_out, double *dist_out,
                     int32_t *count_out, uint8_t *msg_dev, int64_t id_offset, const morna_restriction *rst,
                     const int32_t *q_group_host)
{
    ExactFront F;
    int32_t *ncand = nullptr, *d_ids = nullptr, *d_cnt = nullptr;
    double *d_dist = nullptr;
    size_t s_ids = 0, s_dist = 0, s_out = 0;
    MORNA_TRY(exact_front(h, "exact_search", "exact search", rst, Q, nq, q_group_host, 0, [&]() -> int {
        if (k <= 0 || nq < 0) {
            set_error("exact search: k must be positive");
            return MORNA_E_INVALID;
        }
        return MORNA_OK;
    }, [&](Carver &c, int64_t batch) {
        ncand = c.take<int32_t>((size_t)batch);
        const size_t at = c.used;   // ids, distances, counts: one block, one copy to the host
        d_ids = c.take<int32_t>((size_t)batch * k);
        s_ids = c.used - at;
        d_dist = c.take<double>((size_t)batch * k);
        s_dist = c.used - at - s_ids;
        d_cnt = c.take<int32_t>((size_t)batch);
        s_out = c.used - at;
    }, F));
    if (nq == 0) return MORNA_OK;
    const int64_t N = F.N, batch = F.batch;
    std::vector<int32_t> h_ncand((size_t)batch);
    int32_t cap = std::max<int32_t>(std::max(64, 4 * k) + F.n_outs, h->ex_cap), need_max = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += batch) {
        const int64_t nb = std::min(batch, nq - q0);
        float eps = 0.f;
        MORNA_TRY(exact_front_batch(h, F, q0, nb, true, nullptr, &eps));
        ScopedTimer tm_sel(h, MORNA_T_EXACT, 0);            // selection + fp64 re-rank: the same group as the scan
        const bool select2_on = env_on("MORNA_EXACT_SELECT2");   // (read per call: a test switches it)
        for (;;) {
            MORNA_TRY(h->ex_cand.alloc((size_t)batch * cap));
            MORNA_TRY(h->ex_cdist.alloc((size_t)batch * cap));
            if (rst && N > 8192 && k <= 256 && select2_on)
                hipLaunchKernelGGL(exact_select2_restricted_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, F.approx, N, k, eps, cap,
                                   F.outs, F.n_outs, (uint2 *)h->ex_cdist.p, h->ex_cand.p, ncand, F.R);
            else if (rst)
                hipLaunchKernelGGL(exact_select_restricted_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, F.approx, N, k, eps,
                                   cap, F.outs, F.n_outs, h->ex_cand.p, ncand, F.R);
            else if (N > 8192 && k <= 256 && select2_on)
                hipLaunchKernelGGL(exact_select2_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, F.approx, N, k, eps, cap,
                                   F.outs, F.n_outs, (uint2 *)h->ex_cdist.p, h->ex_cand.p, ncand);
            else
                hipLaunchKernelGGL(exact_select_kernel, dim3((unsigned)nb), dim3(256), 0, h->stream, F.approx, N, k, eps,
                                   cap, F.outs, F.n_outs, h->ex_cand.p, ncand);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h_ncand.data(), ncand, (size_t)nb * 4, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            int32_t need = 0;
            for (int64_t i = 0; i < nb; i++) need = std::max(need, h_ncand[(size_t)i]);
            need_max = std::max(need_max, need);
            if (need <= cap) break;
            cap = need;   // huge tie groups at the boundary: make room for all of them
        }
        hipLaunchKernelGGL(exact_rerank_kernel, dim3((unsigned)nb), dim3(RR_THREADS), 0, h->stream, h->X.p, F.D, F.dpad,
                           F.Qd, h->ex_cand.p, ncand, cap, k, h->ex_cdist.p, d_ids, d_dist, d_cnt);
        HIP_TRY(hipGetLastError());
        if (msg_dev) {
            hipLaunchKernelGGL(exact_pack_kernel, dim3((unsigned)((nb * k + 255) / 256)), dim3(256), 0, h->stream, d_ids, d_dist, d_cnt,
                               nb, k, (int32_t)id_offset, (int32_t *)msg_dev + q0 * k, (int32_t *)msg_dev + nq * k + q0,
                               (double *)(msg_dev + exact_msg_dist_offset(nq, k)) + q0 * k);
            HIP_TRY(hipGetLastError());
            h->unsettled = true;
        }
        if (ids_out)
            MORNA_TRY(fetch_results(h, (const uint8_t *)d_ids, s_out, s_ids, s_dist, 8, nb, k, ids_out + q0 * k,
                                    dist_out ? dist_out + q0 * k : nullptr, count_out ? count_out + q0 : nullptr));
    }
    h->ex_cap = need_max;   // the next call starts with the room this one needed (no more: one query with a tie of thousands
                            // does not size every later call)
    return MORNA_OK;
}

int exact_search(morna_index *h, const double *q, int64_t nq, int32_t k, int32_t *ids_out, double *dist_out,
                 int32_t *count_out)
{
    return exact_search_any(h, ExactQueries::host(q), nq, k, ids_out, dist_out, count_out, nullptr, 0);
}

// =============================================================== label sums (morna_hip.h, "label distance sums")

#define LS_THREADS 256
#define LS_UNROLL 8
#define LS_LDS_SLOTS 2048   // (label, replica) accumulators of a workgroup while there is more than one replica: 12 bytes each, 24 KiB

// sums[q][g] += sum of D(q, r), counts[q][g] += 1 over the counted rows r of label g in the workgroup's chunk of rows
// (blockIdx.y; blockIdx.x is the query), D = (uint64)(sqrt((double)max(v, 0)) * 2^32 + 0.5) of the scan value v.  Integer
// sums: any order, grid and reduction shape give the same bits.
// The accumulators live in LDS as [L][R]: R replicas of every label's pair, R the largest power of two with L * R <=
// LS_LDS_SLOTS, at most LS_THREADS and at least 1; thread t adds into replica t & (R - 1).  With up to 8 labels every thread
// owns its pairs and no two adds meet; with 64 labels a replica is shared by 8 threads, which meet only on equal labels; only
// past 1024 labels is there one copy (48 KiB at 4096), and then the adds of a step spread over thousands of addresses.  The
// replicas are folded in log2(R) steps and the labels that counted a row added to the outputs (zeroed by the host) with
// integer atomics: several chunks of one query meet there.  counted_total: the rows counted by the whole launch.
template <bool RST>
__global__ __launch_bounds__(LS_THREADS) void label_sums_kernel(const float *__restrict__ approx, int64_t n_items, int64_t chunk_rows,
                                                                const int32_t *__restrict__ item_label, int32_t L, int32_t R,
                                                                const int32_t *__restrict__ items /* [nq] or null */,
                                                                RestrictArgs Rst, unsigned long long *__restrict__ sums,
                                                                int32_t *__restrict__ counts,
                                                                unsigned long long *__restrict__ counted_total)
{
    __shared__ int s_counted;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long *s_sum = (unsigned long long *)smem;   // [L][R]
    int32_t *s_cnt = (int32_t *)(s_sum + (size_t)L * R);       // [L][R]
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    for (int i = tid; i < L * R; i += LS_THREADS) {
        s_sum[i] = 0ull;
        s_cnt[i] = 0;
    }
    if (tid == 0) s_counted = 0;
    __syncthreads();
    const float *a = approx + qi * n_items;
    const int64_t r_begin = (int64_t)blockIdx.y * chunk_rows;
    const int64_t r_end = r_begin + chunk_rows < n_items ? r_begin + chunk_rows : n_items;
    const int64_t self = items ? (int64_t)items[qi] : -1;
    int32_t gq = -1;
    if constexpr (RST) gq = restrict_query_group(Rst, qi);
    const int rep = tid & (R - 1);
    for (int64_t base = r_begin; base < r_end; base += LS_THREADS * LS_UNROLL) {
        float v[LS_UNROLL];
        int32_t g[LS_UNROLL];
#pragma unroll
        for (int u = 0; u < LS_UNROLL; u++) {   // the loads of a step first: LS_UNROLL rows in flight per thread
            const int64_t r = base + u * LS_THREADS + tid;
            g[u] = r < r_end ? item_label[r] : -1;
            v[u] = r < r_end ? a[r] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < LS_UNROLL; u++) {
            const int64_t r = base + u * LS_THREADS + tid;
            bool counted = g[u] >= 0 && g[u] < L && r != self;   // (labels are checked on the host: the bound keeps LDS safe)
            if constexpr (RST) counted = counted && restrict_eligible(Rst, gq, r);
            if (!counted) continue;
            const double d = sqrt((double)fmaxf(v[u], 0.f));
            const unsigned long long fx = (unsigned long long)(d * 4294967296.0 + 0.5);
            atomicAdd(&s_sum[g[u] * R + rep], fx);
            atomicAdd(&s_cnt[g[u] * R + rep], 1);
        }
    }
    __syncthreads();
    for (int s = R >> 1; s >= 1; s >>= 1) {   // replica r += replica r + s, every label
        for (int i = tid; i < L * s; i += LS_THREADS) {
            const int lab = i / s, r = i - lab * s;
            s_sum[lab * R + r] += s_sum[lab * R + r + s];
            s_cnt[lab * R + r] += s_cnt[lab * R + r + s];
        }
        __syncthreads();
    }
    int mine = 0;
    for (int lab = tid; lab < L; lab += LS_THREADS) {
        const int32_t c = s_cnt[lab * R];
        if (c == 0) continue;
        atomicAdd(&sums[qi * L + lab], s_sum[lab * R]);
        atomicAdd(&counts[qi * L + lab], c);
        mine += c;
    }
    if (mine) atomicAdd(&s_counted, mine);
    __syncthreads();
    if (tid == 0 && s_counted) atomicAdd(counted_total, (unsigned long long)s_counted);
}

// morna_label_sums: the front, then label_sums_kernel over approx[nb][N].
int label_sums(morna_index *h, const morna_restriction *rst, const ExactQueries &Q, int64_t nq, const int32_t *q_group_host,
               const int32_t *item_label_host, int32_t L, uint64_t *sums_out, int32_t *counts_out)
{
    ExactFront F;
    MORNA_TRY(exact_front(h, "label_sums", "label_sums", rst, Q, nq, q_group_host, 0, [&]() -> int {
        if (nq < 0) {
            set_error("label_sums: a negative number of queries");
            return MORNA_E_INVALID;
        }
        for (int64_t i = 0; i < h->n_items; i++)
            if (item_label_host[i] < -1 || item_label_host[i] >= L) {
                set_error("label_sums: item %lld has the label %d, outside [-1, %d)", (long long)i, item_label_host[i], L);
                return MORNA_E_INVALID;
            }
        return MORNA_OK;
    }, [](Carver &, int64_t) {}, F));
    if (nq == 0) return MORNA_OK;
    if (F.n_outs > 0) {   // their scan values are NaN: the sums have no meaning with them
        std::vector<int32_t> outs((size_t)F.n_outs);
        HIP_TRY(hipMemcpy(outs.data(), F.outs, outs.size() * 4, hipMemcpyDeviceToHost));
        set_error("label_sums: row %d lies outside the domain of the scan (its squared norm underflows, overflows or is not "
                  "finite); %d such rows", *std::min_element(outs.begin(), outs.end()), F.n_outs);
        return MORNA_E_INVALID;
    }
    const int64_t N = F.N, batch = F.batch;
    int32_t R = 1;
    while (R * 2 <= LS_THREADS && (int64_t)L * R * 2 <= LS_LDS_SLOTS) R *= 2;   // (1 past LS_LDS_SLOTS / 2 labels)
    const size_t lds = (size_t)L * R * 12;
    const size_t s_sums = align_up((size_t)batch * L * 8, 256), s_cnts = align_up((size_t)batch * L * 4, 256);
    MORNA_TRY(h->lb_label.alloc((size_t)N));
    MORNA_TRY(h->lb_out.alloc(s_sums + s_cnts + 8));   // sums | counts | the rows counted by the launch
    unsigned long long *d_sums = (unsigned long long *)h->lb_out.p;
    int32_t *d_cnts = (int32_t *)(h->lb_out.p + s_sums);
    unsigned long long *d_counted = (unsigned long long *)(h->lb_out.p + s_sums + s_cnts);
    HIP_TRY(hipMemcpyAsync(h->lb_label.p, item_label_host, (size_t)N * 4, hipMemcpyHostToDevice, h->stream));
    HipEvents ev;
    MORNA_TRY(ev.create(3));
    double scan_ms = 0.0, sums_ms = 0.0, counted = 0.0, eps_half = 0.0;
    int64_t batches = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += batch) {
        const int64_t nb = std::min(batch, nq - q0);
        HIP_TRY(hipMemsetAsync(h->lb_out.p, 0, s_sums + s_cnts + 8, h->stream));
        float eps = 0.f;
        MORNA_TRY(exact_front_batch(h, F, q0, nb, false, &ev, &eps));   // (no row is outside the domain: nothing to mask)
        int64_t chunk_rows = 0;
        const dim3 grid((unsigned)nb, (unsigned)exact_row_chunks(N, nb, LS_THREADS, &chunk_rows));
        MORNA_TRY(with_flag(rst != nullptr, [&](auto restricted) {
            hipLaunchKernelGGL(label_sums_kernel<decltype(restricted)::value>, grid, dim3(LS_THREADS), lds, h->stream, F.approx, N,
                               chunk_rows, h->lb_label.p, L, R, F.d_items, F.R, d_sums, d_cnts, d_counted);
            return MORNA_OK;
        }));
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(2, h->stream));
        HIP_TRY(hipMemcpyAsync(sums_out + q0 * L, d_sums, (size_t)nb * L * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(counts_out + q0 * L, d_cnts, (size_t)nb * L * 4, hipMemcpyDeviceToHost, h->stream));
        unsigned long long counted_b = 0;
        HIP_TRY(hipMemcpyAsync(&counted_b, d_counted, 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        counted += (double)counted_b;
        MORNA_TRY(ev.elapsed(0, 1, &scan_ms));
        MORNA_TRY(ev.elapsed(1, 2, &sums_ms));
        eps_half = std::max(eps_half, (double)eps / 2.0);
        batches++;
    }
    h->label_stats[0] = scan_ms;
    h->label_stats[1] = sums_ms;
    h->label_stats[2] = (double)nq;
    h->label_stats[3] = (double)batches;
    h->label_stats[4] = counted;
    h->label_stats[5] = eps_half;
    return MORNA_OK;
}

// =============================================================== radius search (morna_hip.h, "radius search")
// Every row within the fp64 distance r of a query: the scan of the family's front (exact_front_batch), then
//   radius_count_kernel    per (query, chunk of rows): the rows inside the window (exact_radius_window), counted
//   radius_offsets_kernel  per query: exclusive scan of its chunk counts; the total is the query's candidate count
//   (the host sizes the candidate storage from the totals and places the queries one after the other)
//   radius_write_kernel    the same walk: the candidates written by block scan, ascending by id whatever the grid
//   radius_dist_kernel     per 64 candidates of a query: the reference's fp64 chain (exact_ref_distance), d <= r decided
//   radius_sort_kernel     per query of at most RAD_SORT_MAX candidates: the list ordered in LDS
// No atomic decides a position: the two atomics of radius_dist_kernel count the kept entries and raise the NaN flag.

#define RAD_THREADS 256
#define RAD_WAVES (RAD_THREADS / WAVE)
// Lists of up to this many candidates are ordered on the device: key, id key and origin of every entry are 14 bytes, 56 KiB
// of LDS for a workgroup, so two workgroups fit a CU's 160 KiB.  Longer lists are ordered by the host (exact_radius).
#define RAD_SORT_MAX 4096
#define RAD_KEY_PAD (~0ull)
#define RAD_KEY_DROPPED (~0ull - 1)   // a candidate farther than r: behind everything that is kept
#define RAD_KEY_NAN (~0ull - 2)       // NaN distances last, by ascending id

struct RadiusArgs {
    const float *approx;       // [nb][n_items] the scan values, NaN for the rows of `outs`
    int64_t n_items, chunk_rows;
    int32_t chunks;            // chunks of rows per query; slot `chunks` of a query is its share of `outs`
    double thr;                // the window
    const float *qn2;          // [nb] 0: the query lies outside the scan's domain and is compared with every row
    const int32_t *after;      // [nb] only rows with id > after[q], or null
    const int32_t *outs;       // rows outside the scan's domain
    int32_t n_outs;
};

__device__ inline int wave_sum_i32(int v)
{
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// entry e of the (query, chunk) of a workgroup: its row, and whether the row is a candidate.  Eligibility and the id
// bound come first: a row that fails them is not evaluated, whatever its scan value.
template <bool RST>
__device__ __forceinline__ bool radius_candidate(const RadiusArgs &A, const RestrictArgs &R, int64_t qi, int32_t gq, int32_t aft,
                                                 bool all, bool in_outs, int64_t e, int32_t &row)
{
    row = in_outs ? A.outs[e] : (int32_t)e;
    if (row <= aft) return false;
    if constexpr (RST) {
        if (!restrict_eligible(R, gq, row)) return false;
    }
    if (in_outs) return true;
    const float v = A.approx[qi * A.n_items + row];
    return all ? v == v : (double)v <= A.thr;
}

// the entries of chunk c: rows [e0, e1) of the matrix, or positions [0, n_outs) of `outs` for c == chunks
__device__ inline void radius_chunk(const RadiusArgs &A, int c, int64_t &e0, int64_t &e1)
{
    if (c == A.chunks) {
        e0 = 0;
        e1 = A.n_outs;
    } else {
        e0 = (int64_t)c * A.chunk_rows;
        e1 = e0 + A.chunk_rows < A.n_items ? e0 + A.chunk_rows : A.n_items;
    }
}

template <bool RST>
__global__ __launch_bounds__(RAD_THREADS) void radius_count_kernel(RadiusArgs A, RestrictArgs R,
                                                                   int32_t *__restrict__ chunk_cnt /* [nb][chunks + 1] */)
{
    __shared__ int s_w[RAD_WAVES];
    const int tid = threadIdx.x, c = blockIdx.y;
    const int64_t qi = blockIdx.x;
    int32_t gq = -1;
    if constexpr (RST) gq = restrict_query_group(R, qi);
    const int32_t aft = A.after ? A.after[qi] : -1;
    const bool all = A.qn2[qi] == 0.f;
    int64_t e0, e1;
    radius_chunk(A, c, e0, e1);
    int mine = 0;
    for (int64_t e = e0 + tid; e < e1; e += RAD_THREADS) {
        int32_t row;
        mine += radius_candidate<RST>(A, R, qi, gq, aft, all, c == A.chunks, e, row) ? 1 : 0;
    }
    mine = wave_sum_i32(mine);
    if ((tid & (WAVE - 1)) == 0) s_w[tid / WAVE] = mine;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < RAD_WAVES; w++) total += s_w[w];
        chunk_cnt[qi * (A.chunks + 1) + c] = total;
    }
}

// one wave per query: its chunk counts become their exclusive prefix, the total its candidate count
__global__ __launch_bounds__(WAVE) void radius_offsets_kernel(int32_t *__restrict__ chunk_cnt, int32_t per_q,
                                                              int32_t *__restrict__ ncand /* [nb] */)
{
    const int lane = threadIdx.x;
    int32_t *c = chunk_cnt + (int64_t)blockIdx.x * per_q;
    int run = 0;
    for (int b = 0; b < per_q; b += WAVE) {
        const int v = b + lane < per_q ? c[b + lane] : 0;
        int inc = v;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int up = __shfl_up(inc, off, WAVE);
            if (lane >= off) inc += up;
        }
        if (b + lane < per_q) c[b + lane] = run + inc - v;
        run += __shfl(inc, WAVE - 1, WAVE);
    }
    if (lane == 0) ncand[blockIdx.x] = run;
}

template <bool RST>
__global__ __launch_bounds__(RAD_THREADS) void radius_write_kernel(RadiusArgs A, RestrictArgs R,
                                                                   const int32_t *__restrict__ chunk_off /* [nb][chunks + 1] */,
                                                                   const int64_t *__restrict__ qoff /* [nb] */,
                                                                   int32_t *__restrict__ cand)
{
    __shared__ int s_w[RAD_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE, c = blockIdx.y;
    const int64_t qi = blockIdx.x;
    int32_t gq = -1;
    if constexpr (RST) gq = restrict_query_group(R, qi);
    const int32_t aft = A.after ? A.after[qi] : -1;
    const bool all = A.qn2[qi] == 0.f;
    int64_t e0, e1;
    radius_chunk(A, c, e0, e1);
    int32_t *dst = cand + qoff[qi] + chunk_off[qi * (A.chunks + 1) + c];
    int base = 0;
    for (int64_t t0 = e0; t0 < e1; t0 += RAD_THREADS) {   // (uniform: every thread takes every step)
        const int64_t e = t0 + tid;
        int32_t row = -1;
        const bool is = e < e1 && radius_candidate<RST>(A, R, qi, gq, aft, all, c == A.chunks, e, row);
        const unsigned long long m = __ballot(is);
        if (lane == 0) s_w[w] = __popcll(m);
        __syncthreads();
        int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int u = 0; u < RAD_WAVES; u++) {
            before += u < w ? s_w[u] : 0;
            total += s_w[u];
        }
        if (is) dst[base + before] = row;
        base += total;
        __syncthreads();
    }
}

// workgroup b of the grid is 64 candidates of one query: blkoff[q] <= b < blkoff[q + 1] (blkoff: the prefix of
// ceil(ncand / 64) over the batch's queries, made by the host beside qoff)
__global__ __launch_bounds__(WAVE) void radius_dist_kernel(const float *__restrict__ X, int32_t dim, int32_t dpad,
                                                           const double *__restrict__ Qd /* [nb][dim] */, int64_t nb,
                                                           const int32_t *__restrict__ cand, const int64_t *__restrict__ qoff,
                                                           const int64_t *__restrict__ blkoff /* [nb + 1] */, double radius,
                                                           double *__restrict__ cdist, int32_t *__restrict__ nkeep,
                                                           int32_t *__restrict__ nan_flag)
{
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    int64_t lo = 0, hi = nb - 1;   // the last q with blkoff[q] <= b
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (blkoff[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    const int64_t qi = lo;
    const int64_t n = qoff[qi + 1] - qoff[qi];
    const int64_t t = (b - blkoff[qi]) * WAVE + lane;
    bool keep = false, isnan = false;
    if (t < n) {
        const int64_t at = qoff[qi] + t;
        const double d = exact_ref_distance((const float4 *)(X + (int64_t)cand[at] * dpad), Qd + qi * dim, dim);
        isnan = d != d;
        keep = isnan || d <= radius;   // fp64, inclusive; a NaN stays, and fails the query
        cdist[at] = keep ? d : INFINITY;
    }
    const unsigned long long mk = __ballot(keep), mn = __ballot(isnan);
    if (lane == 0) {
        if (mk) atomicAdd(&nkeep[qi], __popcll(mk));
        if (mn) atomicOr(&nan_flag[qi], 1);
    }
}

// (distance ascending, id descending), NaN last by ascending id, the dropped candidates (distance +inf) behind them: the
// order of exact_rerank_kernel.  Non-negative doubles order as their bits.
__device__ inline void radius_key(double d, int32_t id, uint64_t &key, uint32_t &idkey)
{
    if (d != d) {
        key = RAD_KEY_NAN;
        idkey = (uint32_t)id;
    } else {
        key = d == INFINITY ? RAD_KEY_DROPPED : (uint64_t)__double_as_longlong(d);
        idkey = ~(uint32_t)id;
    }
}

__global__ __launch_bounds__(RAD_THREADS) void radius_sort_kernel(int32_t *__restrict__ cand, double *__restrict__ cdist,
                                                                  const int64_t *__restrict__ qoff /* [nb + 1] */)
{
    __shared__ uint64_t s_key[RAD_SORT_MAX];
    __shared__ uint32_t s_id[RAD_SORT_MAX];
    __shared__ uint16_t s_org[RAD_SORT_MAX];
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const int64_t n64 = qoff[qi + 1] - qoff[qi];
    if (n64 < 2 || n64 > RAD_SORT_MAX) return;
    const int n = (int)n64;
    int32_t *c = cand + qoff[qi];
    double *cd = cdist + qoff[qi];
    int P = 2;
    while (P < n) P <<= 1;
    for (int t = tid; t < P; t += RAD_THREADS) {
        uint64_t key = RAD_KEY_PAD;
        uint32_t idkey = ~0u;
        if (t < n) radius_key(cd[t], c[t], key, idkey);
        s_key[t] = key;
        s_id[t] = idkey;
        s_org[t] = (uint16_t)(t < n ? t : 0);
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += RAD_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint64_t ka = s_key[i], kb = s_key[l];
                const uint32_t ia = s_id[i], ib = s_id[l];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                if (gt == ((i & k) == 0)) {
                    s_key[i] = kb, s_key[l] = ka;
                    s_id[i] = ib, s_id[l] = ia;
                    const uint16_t o = s_org[i];
                    s_org[i] = s_org[l], s_org[l] = o;
                }
            }
            __syncthreads();
        }
    // every key below the padding's is one of the n entries, so positions [0, n) hold a permutation of them.  In place: all
    // reads of the old order come before the barrier, all writes after it.
    constexpr int PER = RAD_SORT_MAX / RAD_THREADS;
    int32_t rid[PER];
    double rd[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int t = tid + u * RAD_THREADS;
        if (t < n) {
            rid[u] = c[s_org[t]];
            rd[u] = cd[s_org[t]];
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; u++) {
        const int t = tid + u * RAD_THREADS;
        if (t < n) {
            c[t] = rid[u];
            cd[t] = rd[u];
        }
    }
}

// the order of radius_sort_kernel on the host, for the lists that do not fit it
static bool radius_before(double da, int32_t ia, double db, int32_t ib)
{
    const bool an = da != da, bn = db != db;
    if (an) return bn && ia < ib;
    return bn || da < db || (da == db && ia > ib);
}

int exact_radius(morna_index *h, const morna_restriction *rst, const ExactQueries &Q, int64_t nq, const int32_t *q_group_host,
                 const int32_t *after_host, double radius, morna_radius *out)
{
    int64_t batch_cap = 0;
    if (const char *e = getenv("MORNA_RADIUS_BATCH")) batch_cap = atoll(e);   // (read per call: a test puts a batch edge inside a small call)
    ExactFront F;
    MORNA_TRY(exact_front(h, "exact_radius", "exact_radius", rst, Q, nq, q_group_host, batch_cap, [&]() -> int {
        if (nq < 0) {
            set_error("exact_radius: a negative number of queries");
            return MORNA_E_INVALID;
        }
        if (!(radius >= 0.0) || radius > DBL_MAX) {
            set_error("exact_radius: the radius %g is not a finite number >= 0", radius);
            return MORNA_E_INVALID;
        }
        out->nq = nq;
        out->off.assign((size_t)nq + 1, 0);
        out->count.assign((size_t)nq, 0);
        return MORNA_OK;
    }, [](Carver &, int64_t) {}, F));
    if (nq == 0) return MORNA_OK;
    const int64_t N = F.N, batch = F.batch;
    const size_t s_b4 = align_up((size_t)batch * 4, 256), s_b8 = align_up(((size_t)batch + 1) * 8, 256);
    std::vector<int32_t> h_ncand((size_t)batch), h_flags(2 * (s_b4 / 4)), h_ids;
    std::vector<int64_t> h_off(2 * (s_b8 / 8));
    std::vector<double> h_dist;
    std::vector<std::pair<double, int32_t>> longlist;
    HipEvents ev;
    MORNA_TRY(ev.create(6));
    double scan_ms = 0.0, sel_ms = 0.0, dist_ms = 0.0, candidates = 0.0, window = 0.0;
    int64_t batches = 0, results = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += batch) {
        const int64_t nb = std::min(batch, nq - q0);
        // (the chunks of a full batch are the fewest, so a short last batch is sized on its own)
        int64_t chunk_rows = 0;
        const int32_t chunks = exact_row_chunks(N, nb, RAD_THREADS, &chunk_rows), per_q = chunks + 1;
        const size_t s_cc = align_up((size_t)nb * per_q * 4, 256);
        MORNA_TRY(h->rd_ws.alloc(s_cc + 4 * s_b4 + 2 * s_b8));
        uint8_t *w = h->rd_ws.p;
        int32_t *chunk_cnt = (int32_t *)w; w += s_cc;
        int32_t *ncand = (int32_t *)w; w += s_b4;
        int32_t *nkeep = (int32_t *)w; w += s_b4;      // nkeep | nan_flag: one memset, one copy
        int32_t *nan_flag = (int32_t *)w; w += s_b4;
        int32_t *d_after = (int32_t *)w; w += s_b4;
        int64_t *qoff = (int64_t *)w; w += s_b8;       // qoff | blkoff: one copy
        int64_t *blkoff = (int64_t *)w; w += s_b8;
        if (after_host) HIP_TRY(hipMemcpyAsync(d_after, after_host + q0, (size_t)nb * 4, hipMemcpyHostToDevice, h->stream));
        float eps = 0.f;
        MORNA_TRY(exact_front_batch(h, F, q0, nb, true, &ev, &eps));
        RadiusArgs A;
        A.approx = F.approx;
        A.n_items = N;
        A.chunk_rows = chunk_rows;
        A.chunks = chunks;
        A.thr = exact_radius_window(radius, eps);
        A.qn2 = F.qn2;
        A.after = after_host ? d_after : nullptr;
        A.outs = F.outs;
        A.n_outs = F.n_outs;
        window = std::max(window, A.thr);
        const dim3 grid((unsigned)nb, (unsigned)per_q);
        MORNA_TRY(with_flag(rst != nullptr, [&](auto restricted) {
            hipLaunchKernelGGL(radius_count_kernel<decltype(restricted)::value>, grid, dim3(RAD_THREADS), 0, h->stream, A, F.R, chunk_cnt);
            return MORNA_OK;
        }));
        hipLaunchKernelGGL(radius_offsets_kernel, dim3((unsigned)nb), dim3(WAVE), 0, h->stream, chunk_cnt, per_q, ncand);
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(2, h->stream));
        HIP_TRY(hipMemcpyAsync(h_ncand.data(), ncand, (size_t)nb * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        int64_t *h_qoff = h_off.data(), *h_blkoff = h_off.data() + s_b8 / 8;   // (the device's layout)
        h_qoff[0] = h_blkoff[0] = 0;
        for (int64_t i = 0; i < nb; i++) {
            h_qoff[i + 1] = h_qoff[i] + h_ncand[(size_t)i];
            h_blkoff[i + 1] = h_blkoff[i] + (h_ncand[(size_t)i] + WAVE - 1) / WAVE;
        }
        const int64_t total = h_qoff[nb], blocks = h_blkoff[nb];
        candidates += (double)total;
        MORNA_TRY(h->ex_cand.alloc((size_t)total));
        MORNA_TRY(h->ex_cdist.alloc((size_t)total));
        HIP_TRY(hipMemcpyAsync(qoff, h_qoff, s_b8 + ((size_t)nb + 1) * 8, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemsetAsync(nkeep, 0, 2 * s_b4, h->stream));
        MORNA_TRY(ev.record(3, h->stream));
        MORNA_TRY(with_flag(rst != nullptr, [&](auto restricted) {
            hipLaunchKernelGGL(radius_write_kernel<decltype(restricted)::value>, grid, dim3(RAD_THREADS), 0, h->stream, A, F.R, chunk_cnt,
                               qoff, h->ex_cand.p);
            return MORNA_OK;
        }));
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(4, h->stream));
        if (blocks > 0) {
            hipLaunchKernelGGL(radius_dist_kernel, dim3((unsigned)blocks), dim3(WAVE), 0, h->stream, h->X.p, F.D, F.dpad, F.Qd, nb,
                               h->ex_cand.p, qoff, blkoff, radius, h->ex_cdist.p, nkeep, nan_flag);
            hipLaunchKernelGGL(radius_sort_kernel, dim3((unsigned)nb), dim3(RAD_THREADS), 0, h->stream, h->ex_cand.p,
                               h->ex_cdist.p, qoff);
            HIP_TRY(hipGetLastError());
        }
        MORNA_TRY(ev.record(5, h->stream));
        h_ids.resize((size_t)total);
        h_dist.resize((size_t)total);
        HIP_TRY(hipMemcpyAsync(h_flags.data(), nkeep, s_b4 + (size_t)nb * 4, hipMemcpyDeviceToHost, h->stream));
        if (total > 0) {
            HIP_TRY(hipMemcpyAsync(h_ids.data(), h->ex_cand.p, (size_t)total * 4, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(h_dist.data(), h->ex_cdist.p, (size_t)total * 8, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        const int32_t *h_nkeep = h_flags.data(), *h_nan = h_flags.data() + s_b4 / 4;
        for (int64_t i = 0; i < nb; i++) {
            const int64_t n = h_ncand[(size_t)i], keep = h_nkeep[i], at = h_qoff[i];
            if (n <= RAD_SORT_MAX) {   // ordered by radius_sort_kernel: the kept entries lead
                out->ids.insert(out->ids.end(), h_ids.begin() + at, h_ids.begin() + at + keep);
                out->dist.insert(out->dist.end(), h_dist.begin() + at, h_dist.begin() + at + keep);
            } else {
                longlist.clear();
                for (int64_t t = at; t < at + n; t++)
                    if (h_dist[(size_t)t] != INFINITY) longlist.emplace_back(h_dist[(size_t)t], h_ids[(size_t)t]);
                std::sort(longlist.begin(), longlist.end(), [](const std::pair<double, int32_t> &a, const std::pair<double, int32_t> &b) {
                    return radius_before(a.first, a.second, b.first, b.second);
                });
                for (const auto &e : longlist) {
                    out->ids.push_back(e.second);
                    out->dist.push_back(e.first);
                }
            }
            results += keep;
            out->off[(size_t)(q0 + i) + 1] = results;
            out->count[(size_t)(q0 + i)] = h_nan[i] ? -1 : keep;
            if (results > (int64_t)INT32_MAX) {
                set_error("exact_radius: %lld result entries by query %lld, more than the 2^31 - 1 one call returns",
                          (long long)results, (long long)(q0 + i));
                return MORNA_E_INVALID;
            }
        }
        MORNA_TRY(ev.elapsed(0, 1, &scan_ms));
        MORNA_TRY(ev.elapsed(1, 2, &sel_ms));
        MORNA_TRY(ev.elapsed(3, 4, &sel_ms));
        MORNA_TRY(ev.elapsed(4, 5, &dist_ms));
        batches++;
    }
    h->radius_stats[0] = scan_ms;
    h->radius_stats[1] = sel_ms;
    h->radius_stats[2] = dist_ms;
    h->radius_stats[3] = (double)nq;
    h->radius_stats[4] = (double)batches;
    h->radius_stats[5] = candidates;
    h->radius_stats[6] = (double)results;
    h->radius_stats[7] = window;
    return MORNA_OK;
}

// =============================================================== spherical k-means (morna_hip.h, "spherical k-means")
// The transposed selection: for every ROW the nearest of k fp64 centroids, from the scan of the family's front with the
// centroids as its queries (exact_front_batch), then
//   kmeans_pick_kernel     per row: the smallest scan value over the centroids and the centroids inside its window
//                          (kmeans_window), counted; one survivor decides the row, more make it an open row
//   radius_offsets_kernel  the exclusive prefix of the workgroups' counts
//   kmeans_list_kernel     the same walk: one entry per (row, centroid inside the window), placed by block scan
//   kmeans_resolve_kernel  per entry the reference's fp64 chain (exact_ref_distance)
//   kmeans_min_kernel      per row the minimum of its entries by (distance, centroid), NaN behind every number
// and for the loop around it
//   kmeans_norms_kernel    once per call: 1 / sqrt(pp) of every row, pp the sequential fp64 sum of squares
//   kmeans_hist_kernel     per chunk of rows the members of every cluster, counted; the rows that changed cluster, counted
//   kmeans_starts_kernel   per cluster the prefix of its chunk counts and its size; the prefix of the sizes
//   kmeans_scatter_kernel  the same chunks: cluster-major member lists in ascending id (a row's place is a count of the rows
//                          in front of it, never the arrival order of an atomic)
//   kmeans_update_kernel   per (cluster, 256 columns): the members' scaled rows added in list order, one rounding per
//                          multiply and per add
// Integer atomics count (open rows, changed rows, a chunk's histogram in LDS); none decides a position or a value.

#define KM_THREADS 256
#define KM_WAVES (KM_THREADS / WAVE)
#define KM_CHUNK 1024                   // rows of a member-list chunk (KM_THREADS rows a step)
#define KM_AHEAD 8                      // member rows in flight per thread of kmeans_update_kernel
#define KM_MAX_VALUES ((int64_t)1 << 29)   // scan values of one batch (2 GiB): all centroids share one batch

// The window of the assignment: centroid j is evaluated for row i iff its scan value
//     v_j <= min_j' v_j' + eps + 2 dpad 2^-50 + 2^-48,     eps = exact_scan_eps(dpad, which scan ran), compared in fp64.
// Derivation.  Let t_j be the true 2 - 2cos of (i, j), D_j the reference's fp64 radicand and d_j = sqrt(D_j) correctly
// rounded, the distance exact_ref_distance returns.  The scan keeps |v_j - t_j| <= eps / 2 (eps is that bound taken twice,
// for the two values the top-k threshold of exact_select_body compares: here too two scan values are compared, the
// minimum's and the candidate's, so all of eps is used).  The fp64 chain keeps |D_j - t_j| <= dpad 2^-50.  Let m be the
// centroid of the smallest scan value and w the winner, d_w <= d_m.  The rounded sqrt is monotone but not injective:
// d_w <= d_m gives only D_w <= D_m (1 + 2^-52)^2, distinct radicands can round to one distance and the tie then goes to the
// lower index, which may be the one of the larger radicand; with D <= 4 that slack is below 2^-48.  So
//     t_w <= D_w + dpad 2^-50 <= D_m + 2^-48 + dpad 2^-50 <= t_m + 2 dpad 2^-50 + 2^-48,   v_w <= v_m + eps + 2 dpad 2^-50 + 2^-48.
// The two extra terms are at most 2^-34 + 2^-48 for dpad <= 32768 beside an eps of at least 2^-19; they are added all the same.
// NaN distances.  A radicand is negative only when the fp64 cosine rounds above 1: then t_j <= dpad 2^-50 and v_j <= eps / 2 +
// dpad 2^-50, below the window itself.  A NaN orders BEHIND every number, so the nearest centroid by the scan may lose to any
// other: a row whose smallest scan value is inside [.., window] is open against every centroid.  (Such a row is all but
// parallel to a centroid: the seeds in the first iteration, the only member of a cluster later.)
// Outside the scan's domain the bound does not hold: a row on the list of exact_outside_kernel (scan values NaN) is open
// against every centroid, and a centroid with a zero image (exact_prep_kernel: the zero vector, or a sum of squares outside
// [EX_QQ_LO, EX_QQ_HI]) is evaluated for every row and takes no part in the minimum.
static double kmeans_window(int32_t dpad, float eps) { return (double)eps + 2.0 * (double)dpad * 0x1p-50 + 0x1p-48; }

struct KmeansArgs {
    const float *approx;       // [k][n_items] the scan values, NaN for the rows outside the scan's domain
    const float *qn2;          // [k] 0: the centroid has a zero image
    const uint32_t *deny;      // the restriction's bitmap, or null: every row is eligible
    int64_t n_items;
    int32_t k;
    double window;
};

__device__ __forceinline__ bool kmeans_eligible(const uint32_t *__restrict__ deny, int64_t i)
{
    return !deny || !((deny[i >> 5] >> (i & 31)) & 1u);
}

// row i: lim = its smallest scan value + the window; all: it is open against every centroid.  The reads of a wave are 64
// consecutive rows of one centroid.
__device__ __forceinline__ void kmeans_row_view(const KmeansArgs &A, int64_t i, double &lim, bool &all)
{
    float vmin = INFINITY;
    all = false;
    for (int j = 0; j < A.k; j++) {
        const float v = A.approx[(int64_t)j * A.n_items + i];
        if (A.qn2[j] == 0.f) continue;
        if (v != v) all = true;
        else vmin = fminf(vmin, v);
    }
    if ((double)vmin <= A.window) all = true;
    lim = (double)vmin + A.window;
}

__device__ __forceinline__ bool kmeans_candidate(const KmeansArgs &A, int64_t i, int j, double lim, bool all)
{
    if (all || A.qn2[j] == 0.f) return true;
    return (double)A.approx[(int64_t)j * A.n_items + i] <= lim;
}

__device__ inline int km_block_sum(int v, int *s_w, int tid)
{
    v = wave_sum_i32(v);
    __syncthreads();
    if ((tid & (WAVE - 1)) == 0) s_w[tid / WAVE] = v;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int u = 0; u < KM_WAVES; u++) total += s_w[u];
    return total;
}

// exclusive prefix of v over the workgroup's threads
__device__ inline int km_block_excl(int v, int *s_w, int tid)
{
    const int lane = tid & (WAVE - 1), w = tid / WAVE;
    int inc = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int up = __shfl_up(inc, off, WAVE);
        if (lane >= off) inc += up;
    }
    __syncthreads();
    if (lane == WAVE - 1) s_w[w] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int u = 0; u < KM_WAVES; u++) base += u < w ? s_w[u] : 0;
    return base + inc - v;
}

// cnt[i]: the centroids to evaluate for row i (0: not eligible, and its answer -1 / -1.0 is written here); blk[b]: their sum
// over workgroup b; totals[1] += the open rows
__global__ __launch_bounds__(KM_THREADS) void kmeans_pick_kernel(KmeansArgs A, int32_t *__restrict__ cnt, int32_t *__restrict__ blk,
                                                                 int32_t *__restrict__ totals, int32_t *__restrict__ assign,
                                                                 double *__restrict__ dist)
{
    __shared__ int s_w[KM_WAVES];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * KM_THREADS + tid;
    int c = 0;
    if (i < A.n_items) {
        if (!kmeans_eligible(A.deny, i)) {
            assign[i] = -1;
            dist[i] = -1.0;
        } else {
            double lim;
            bool all;
            kmeans_row_view(A, i, lim, all);
            for (int j = 0; j < A.k; j++) c += kmeans_candidate(A, i, j, lim, all) ? 1 : 0;
        }
        cnt[i] = c;
    }
    const int total = km_block_sum(c, s_w, tid);
    const int open = km_block_sum(c > 1 ? 1 : 0, s_w, tid);
    if (tid == 0) {
        blk[blockIdx.x] = total;
        if (open) atomicAdd(&totals[1], open);
    }
}

// the entries of row i at rowoff[i] .. + cnt[i], ascending by centroid; blkoff: the exclusive prefix of blk
__global__ __launch_bounds__(KM_THREADS) void kmeans_list_kernel(KmeansArgs A, const int32_t *__restrict__ cnt,
                                                                 const int32_t *__restrict__ blkoff, int32_t *__restrict__ rowoff,
                                                                 int32_t *__restrict__ item_row, int32_t *__restrict__ item_j)
{
    __shared__ int s_w[KM_WAVES];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * KM_THREADS + tid;
    const int c = i < A.n_items ? cnt[i] : 0;
    const int off = blkoff[blockIdx.x] + km_block_excl(c, s_w, tid);
    if (i < A.n_items) rowoff[i] = off;
    if (c > 0) {
        double lim;
        bool all;
        kmeans_row_view(A, i, lim, all);
        int at = 0;
        for (int j = 0; j < A.k; j++)
            if (kmeans_candidate(A, i, j, lim, all) && at < c) {
                item_row[off + at] = (int32_t)i;
                item_j[off + at] = j;
                at++;
            }
    }
}

// one thread per (row, centroid) entry: d(i, c_j), the reference's chain
__global__ __launch_bounds__(WAVE) void kmeans_resolve_kernel(const float *__restrict__ X, int32_t dim, int32_t dpad,
                                                              const double *__restrict__ Qd /* [k][dim] */,
                                                              const int32_t *__restrict__ item_row, const int32_t *__restrict__ item_j,
                                                              int64_t total, double *__restrict__ item_d)
{
    const int64_t t = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    if (t >= total) return;
    item_d[t] = exact_ref_distance((const float4 *)(X + (int64_t)item_row[t] * dpad), Qd + (int64_t)item_j[t] * dim, dim);
}

// a_i: the entry of the smallest distance, the first of equal ones (the entries ascend by centroid), a NaN behind every number;
// a NaN is returned as the canonical quiet NaN
__global__ __launch_bounds__(KM_THREADS) void kmeans_min_kernel(const int32_t *__restrict__ cnt, const int32_t *__restrict__ rowoff,
                                                                const int32_t *__restrict__ item_j, const double *__restrict__ item_d,
                                                                int64_t n_items, int32_t *__restrict__ assign, double *__restrict__ dist)
{
    const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    if (i >= n_items) return;
    const int c = cnt[i];
    if (c <= 0) return;
    const int off = rowoff[i];
    double bd = item_d[off];
    int32_t bj = item_j[off];
    for (int w = 1; w < c; w++) {
        const double d = item_d[off + w];
        if (d < bd || (bd != bd && d == d)) {
            bd = d;
            bj = item_j[off + w];
        }
    }
    assign[i] = bj;
    dist[i] = bd == bd ? bd : __longlong_as_double(0x7ff8000000000000ll);
}

// scale[i] = s_i = 1 / sqrt(pp_i), pp_i the sum of squares of row i in cosine_distance's order; -1: the member is skipped
// (not (0 < pp_i < inf))
__global__ __launch_bounds__(KM_THREADS) void kmeans_norms_kernel(const float *__restrict__ X, int64_t n_items, int32_t dim, int32_t dpad,
                                                                  double *__restrict__ scale)
{
    const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    if (i >= n_items) return;
    const float4 *row = (const float4 *)(X + i * dpad);
    double pp = 0.0;
    for (int z0 = 0; z0 < dim; z0 += 4) {
        const float4 x = row[z0 / 4];
        const float e4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int v = 0; v < 4; v++)
            if (z0 + v < dim) {
                const double e = (double)e4[v];
                pp = __dadd_rn(pp, __dmul_rn(e, e));
            }
    }
    scale[i] = pp > 0.0 && pp < INFINITY ? __ddiv_rn(1.0, __dsqrt_rn(pp)) : -1.0;
}

// chunk_cnt[c][j]: the rows of chunk c assigned to cluster j; totals[2] += the rows whose cluster changed
__global__ __launch_bounds__(KM_THREADS) void kmeans_hist_kernel(const int32_t *__restrict__ assign, const int32_t *__restrict__ prev,
                                                                 int64_t n_items, int32_t k, int32_t *__restrict__ chunk_cnt,
                                                                 int32_t *__restrict__ totals)
{
    __shared__ int s_w[KM_WAVES];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *hist = (int *)smem;   // [k]
    const int tid = threadIdx.x;
    for (int j = tid; j < k; j += KM_THREADS) hist[j] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * KM_CHUNK;
    int changed = 0;
    for (int s = 0; s < KM_CHUNK; s += KM_THREADS) {
        const int64_t i = r0 + s + tid;
        if (i < n_items) {
            const int32_t a = assign[i];
            changed += a != prev[i] ? 1 : 0;
            if (a >= 0 && a < k) atomicAdd(&hist[a], 1);
        }
    }
    changed = km_block_sum(changed, s_w, tid);
    for (int j = tid; j < k; j += KM_THREADS) chunk_cnt[(int64_t)blockIdx.x * k + j] = hist[j];
    if (tid == 0 && changed) atomicAdd(&totals[2], changed);
}

// one workgroup: chunk_cnt[c][j] becomes the members of cluster j in the chunks before c, sizes[j] their total, start[j] the
// exclusive prefix of the sizes (k <= 4096)
__global__ __launch_bounds__(KM_THREADS) void kmeans_starts_kernel(int32_t *__restrict__ chunk_cnt, int32_t chunks, int32_t k,
                                                                   int32_t *__restrict__ sizes, int32_t *__restrict__ start)
{
    __shared__ int s_w[KM_WAVES];
    __shared__ int s_sz[MORNA_LABELS_MAX];
    const int tid = threadIdx.x;
    for (int j = tid; j < k; j += KM_THREADS) {
        int run = 0;
        for (int c = 0; c < chunks; c++) {
            const int v = chunk_cnt[(int64_t)c * k + j];
            chunk_cnt[(int64_t)c * k + j] = run;
            run += v;
        }
        s_sz[j] = run;
        sizes[j] = run;
    }
    __syncthreads();
    const int per = (k + KM_THREADS - 1) / KM_THREADS, lo = tid * per, hi = lo + per < k ? lo + per : k;
    int mine = 0;
    for (int j = lo; j < hi; j++) mine += s_sz[j];
    int at = km_block_excl(mine, s_w, tid);
    for (int j = lo; j < hi; j++) {
        start[j] = at;
        at += s_sz[j];
    }
}

// member[start[j] + ...]: the rows of cluster j in ascending id.  A chunk takes its rows KM_THREADS at a time; a row's place
// is the cluster's running count plus the rows of the step in front of it with the same cluster.
__global__ __launch_bounds__(KM_THREADS) void kmeans_scatter_kernel(const int32_t *__restrict__ assign, int64_t n_items, int32_t k,
                                                                    const int32_t *__restrict__ chunk_off, const int32_t *__restrict__ start,
                                                                    int32_t *__restrict__ member)
{
    __shared__ int s_lab[KM_THREADS];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *run = (int *)smem;   // [k]
    const int tid = threadIdx.x;
    for (int j = tid; j < k; j += KM_THREADS) run[j] = start[j] + chunk_off[(int64_t)blockIdx.x * k + j];
    const int64_t r0 = (int64_t)blockIdx.x * KM_CHUNK;
    for (int s = 0; s < KM_CHUNK; s += KM_THREADS) {
        const int64_t i = r0 + s + tid;
        int32_t a = i < n_items ? assign[i] : -1;
        if (a >= k) a = -1;
        s_lab[tid] = a;
        __syncthreads();
        int before = 0;
        bool last = true;
        if (a >= 0) {
            for (int u = 0; u < KM_THREADS; u++) {
                const bool same = s_lab[u] == a;
                before += same && u < tid ? 1 : 0;
                last = last && !(same && u > tid);
            }
            member[run[a] + before] = (int32_t)i;
        }
        __syncthreads();
        if (a >= 0 && last) run[a] += before + 1;
        __syncthreads();
    }
}

// c_j[z] = sum of (double)x_i[z] * s_i over the unskipped members of cluster j in list order, from 0.0, every product and
// every sum rounded once (no fma); a cluster without an unskipped member keeps its centroid.  KM_AHEAD member rows are
// requested before the first of them is consumed; the sum itself is one dependent chain as long as the cluster.
__global__ __launch_bounds__(KM_THREADS) void kmeans_update_kernel(const float *__restrict__ X, int32_t dim, int32_t dpad,
                                                                   const int32_t *__restrict__ member, const int32_t *__restrict__ start,
                                                                   const int32_t *__restrict__ sizes, const double *__restrict__ scale,
                                                                   double *__restrict__ cent /* [k][dim] */)
{
    const int j = blockIdx.x, z = blockIdx.y * KM_THREADS + threadIdx.x;
    const bool live = z < dim;
    const int32_t *mem = member + start[j];
    const int n = sizes[j];
    double acc = 0.0;
    bool any = false;
    for (int m0 = 0; m0 < n; m0 += KM_AHEAD) {
        float x[KM_AHEAD];
        double s[KM_AHEAD];
#pragma unroll
        for (int u = 0; u < KM_AHEAD; u++) {
            const int32_t id = m0 + u < n ? mem[m0 + u] : -1;
            s[u] = id >= 0 ? scale[id] : -1.0;
            x[u] = id >= 0 && live ? X[(int64_t)id * dpad + z] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < KM_AHEAD; u++)
            if (s[u] > 0.0) {
                acc = __dadd_rn(acc, __dmul_rn((double)x[u], s[u]));
                any = true;
            }
    }
    if (any && live) cent[(int64_t)j * dim + z] = acc;
}

// morna_kmeans (seeds: the loop) and morna_kmeans_assign (cent_host: one assignment) behind their null checks.
int kmeans(morna_index *h, const morna_restriction *rst, const int32_t *seeds, const double *cent_host, int32_t k, int32_t max_iter,
           int32_t *assign_out, double *dist_out, double *cent_out, int32_t *sizes_out, int32_t *info_out)
{
    const bool loop = seeds != nullptr;
    const char *who = loop ? "kmeans" : "kmeans_assign";
    ExactFront F;
    double *cent = nullptr, *scale = nullptr, *d_dist = nullptr;
    int32_t *d_assign = nullptr, *d_prev = nullptr, *cnt = nullptr, *rowoff = nullptr, *blk = nullptr, *totals = nullptr;
    int32_t *member = nullptr, *sizes = nullptr, *start = nullptr, *chunk_cnt = nullptr;
    int64_t nblk = 0, chunks = 0;
    MORNA_TRY(exact_front(h, who, who, rst, loop ? ExactQueries::stored(seeds) : ExactQueries::host(cent_host), (int64_t)k, nullptr, 0,
                          [&]() -> int {
        const int64_t N = h->n_items;
        if (rst && rst->has_group) {
            set_error("%s: a restriction that holds groups is not taken, only an allow-list", who);
            return MORNA_E_INVALID;
        }
        const int64_t n_elig = rst ? rst->n_allowed : N;
        // (given centroids are not drawn from E: only the loop, whose seeds are k distinct eligible rows, is bounded by |E|)
        if (k < 1 || k > MORNA_LABELS_MAX || (loop && k > n_elig)) {
            set_error("%s: k = %d, 1 to min(%d, the %lld eligible rows) are taken", who, k, MORNA_LABELS_MAX, (long long)n_elig);
            return MORNA_E_INVALID;
        }
        if ((int64_t)k * N > KM_MAX_VALUES) {
            set_error("%s: k * n_items = %lld, above the 2^29 = %lld scan values of one batch", who, (long long)((int64_t)k * N),
                      (long long)KM_MAX_VALUES);
            return MORNA_E_INVALID;
        }
        if (!loop) return MORNA_OK;
        if (max_iter < 1) {
            set_error("kmeans: max_iter = %d, at least 1 is taken", max_iter);
            return MORNA_E_INVALID;
        }
        for (int32_t j = 0; j < k; j++)
            if (seeds[j] < 0 || seeds[j] >= N) {
                set_error("Item index %d out of range [0, %lld)", seeds[j], (long long)N);
                return MORNA_E_RANGE;
            }
        std::vector<int32_t> sorted(seeds, seeds + k);
        std::sort(sorted.begin(), sorted.end());
        for (int32_t j = 1; j < k; j++)
            if (sorted[(size_t)j] == sorted[(size_t)j - 1]) {
                set_error("kmeans: the seed item %d is given twice", sorted[(size_t)j]);
                return MORNA_E_INVALID;
            }
        if (rst) {
            std::vector<uint32_t> deny((size_t)(N + 31) / 32);
            HIP_TRY(hipMemcpyAsync(deny.data(), rst->deny.p, deny.size() * 4, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            for (int32_t j = 0; j < k; j++)
                if ((deny[(size_t)seeds[j] >> 5] >> (seeds[j] & 31)) & 1u) {
                    set_error("kmeans: the seed item %d is not eligible under the restriction", seeds[j]);
                    return MORNA_E_INVALID;
                }
        }
        return MORNA_OK;
    }, [&](Carver &c, int64_t) {
        const size_t N = (size_t)h->n_items;
        nblk = (int64_t)((N + KM_THREADS - 1) / KM_THREADS);
        chunks = (int64_t)((N + KM_CHUNK - 1) / KM_CHUNK);
        cent = c.take<double>((size_t)k * h->dim);
        scale = c.take<double>(loop ? N : 0);
        d_dist = c.take<double>(N);
        d_assign = c.take<int32_t>(N);
        d_prev = c.take<int32_t>(loop ? N : 0);
        cnt = c.take<int32_t>(N);
        rowoff = c.take<int32_t>(N);
        blk = c.take<int32_t>((size_t)nblk);
        totals = c.take<int32_t>(4);   // entries | open rows | rows that changed cluster
        member = c.take<int32_t>(loop ? N : 0);
        sizes = c.take<int32_t>(loop ? (size_t)k : 0);
        start = c.take<int32_t>(loop ? (size_t)k : 0);
        chunk_cnt = c.take<int32_t>(loop ? (size_t)chunks * k : 0);
    }, F));
    const int64_t N = F.N;
    const int32_t D = F.D, dpad = F.dpad;
    if (F.batch != k) {   // (k * N <= KM_MAX_VALUES was checked: the front's cap is the same number)
        set_error("%s: the centroids do not share one batch", who);
        return MORNA_E_INVALID;
    }
    const uint32_t *deny = rst ? rst->deny.p : nullptr;
    HipEvents ev;
    MORNA_TRY(ev.create(9));
    if (loop) {
        HIP_TRY(hipMemcpyAsync(F.d_items, seeds, (size_t)k * 4, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(exact_widen_kernel, dim3((unsigned)k), dim3(256), 0, h->stream, h->X.p, (int64_t)dpad, F.d_items, D, cent);
        hipLaunchKernelGGL(kmeans_norms_kernel, dim3((unsigned)nblk), dim3(KM_THREADS), 0, h->stream, h->X.p, N, D, dpad, scale);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemsetAsync(d_prev, 0xff, (size_t)N * 4, h->stream));
        F.Q = ExactQueries::device64(cent);   // every iteration scans the centroids where the update left them
    }
    int32_t h_tot[4] = {0, 0, 0, 0};
    double ms[4] = {0.0, 0.0, 0.0, 0.0}, open_rows = 0.0, chains = 0.0;
    int32_t iterations = 0, converged = 0;
    bool update_pending = false;
    for (int32_t t = 1;; t++) {
        HIP_TRY(hipMemsetAsync(totals, 0, 16, h->stream));
        float eps = 0.f;
        MORNA_TRY(exact_front_batch(h, F, 0, k, true, &ev, &eps));   // events 0, 1
        KmeansArgs A;
        A.approx = F.approx;
        A.qn2 = F.qn2;
        A.deny = deny;
        A.n_items = N;
        A.k = k;
        A.window = kmeans_window(dpad, eps);
        hipLaunchKernelGGL(kmeans_pick_kernel, dim3((unsigned)nblk), dim3(KM_THREADS), 0, h->stream, A, cnt, blk, totals, d_assign, d_dist);
        hipLaunchKernelGGL(radius_offsets_kernel, dim3(1), dim3(WAVE), 0, h->stream, blk, (int32_t)nblk, totals);
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(2, h->stream));
        HIP_TRY(hipMemcpyAsync(h_tot, totals, 16, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // the entries size their storage
        if (update_pending) MORNA_TRY(ev.elapsed(7, 8, &ms[3]));
        update_pending = false;
        const int64_t total = h_tot[0];
        MORNA_TRY(h->ex_cand.alloc((size_t)std::max<int64_t>(2 * total, 1)));
        MORNA_TRY(h->ex_cdist.alloc((size_t)std::max<int64_t>(total, 1)));
        int32_t *item_row = h->ex_cand.p, *item_j = h->ex_cand.p + total;
        MORNA_TRY(ev.record(3, h->stream));
        hipLaunchKernelGGL(kmeans_list_kernel, dim3((unsigned)nblk), dim3(KM_THREADS), 0, h->stream, A, cnt, blk, rowoff, item_row, item_j);
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(4, h->stream));
        if (total > 0)
            hipLaunchKernelGGL(kmeans_resolve_kernel, dim3((unsigned)((total + WAVE - 1) / WAVE)), dim3(WAVE), 0, h->stream, h->X.p, D, dpad,
                               F.Qd, item_row, item_j, total, h->ex_cdist.p);
        hipLaunchKernelGGL(kmeans_min_kernel, dim3((unsigned)nblk), dim3(KM_THREADS), 0, h->stream, cnt, rowoff, item_j, h->ex_cdist.p, N,
                           d_assign, d_dist);
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(5, h->stream));
        if (loop) {
            hipLaunchKernelGGL(kmeans_hist_kernel, dim3((unsigned)chunks), dim3(KM_THREADS), (size_t)k * 4, h->stream, d_assign, d_prev, N, k,
                               chunk_cnt, totals);
            hipLaunchKernelGGL(kmeans_starts_kernel, dim3(1), dim3(KM_THREADS), 0, h->stream, chunk_cnt, (int32_t)chunks, k, sizes, start);
            hipLaunchKernelGGL(kmeans_scatter_kernel, dim3((unsigned)chunks), dim3(KM_THREADS), (size_t)k * 4, h->stream, d_assign, N, k,
                               chunk_cnt, start, member);
            HIP_TRY(hipGetLastError());
        }
        MORNA_TRY(ev.record(6, h->stream));
        HIP_TRY(hipMemcpyAsync(h_tot, totals, 16, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));   // the rows that changed cluster
        MORNA_TRY(ev.elapsed(0, 1, &ms[0]));
        MORNA_TRY(ev.elapsed(1, 2, &ms[1]));
        MORNA_TRY(ev.elapsed(3, 4, &ms[1]));
        MORNA_TRY(ev.elapsed(4, 5, &ms[2]));
        MORNA_TRY(ev.elapsed(5, 6, &ms[3]));
        open_rows += (double)h_tot[1];
        chains += (double)total;
        iterations = t;
        if (!loop) break;
        if (t > 1 && h_tot[2] == 0) {
            converged = 1;
            break;
        }
        if (t == max_iter) break;   // (the update after the last assignment would not be seen)
        MORNA_TRY(ev.record(7, h->stream));
        hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)k, (unsigned)((D + KM_THREADS - 1) / KM_THREADS)), dim3(KM_THREADS), 0,
                           h->stream, h->X.p, D, dpad, member, start, sizes, scale, cent);
        HIP_TRY(hipGetLastError());
        MORNA_TRY(ev.record(8, h->stream));
        update_pending = true;
        std::swap(d_assign, d_prev);   // the next assignment is written beside this one
    }
    // the last assignment, its distances and the centroids it was made against (F.Qd: the front's copy of them)
    std::vector<int32_t> h_sizes(loop ? (size_t)k : 0);
    HIP_TRY(hipMemcpyAsync(assign_out, d_assign, (size_t)N * 4, hipMemcpyDeviceToHost, h->stream));
    if (dist_out) HIP_TRY(hipMemcpyAsync(dist_out, d_dist, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    if (cent_out) HIP_TRY(hipMemcpyAsync(cent_out, F.Qd, (size_t)k * D * 8, hipMemcpyDeviceToHost, h->stream));
    if (loop) HIP_TRY(hipMemcpyAsync(h_sizes.data(), sizes, (size_t)k * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (sizes_out) memcpy(sizes_out, h_sizes.data(), (size_t)k * 4);
    if (info_out) {
        info_out[0] = iterations;
        info_out[1] = converged;
    }
    for (int i = 0; i < 4; i++) h->kmeans_stats[i] = ms[i];
    h->kmeans_stats[4] = open_rows;
    h->kmeans_stats[5] = chains;
    h->kmeans_stats[6] = (double)iterations;
    h->kmeans_stats[7] = loop ? (double)*std::max_element(h_sizes.begin(), h_sizes.end()) : 0.0;
    return MORNA_OK;
}

// The update alone, for a labelling that is given (mixture.hip): the scales of every row, the label-major member lists of
// assign[n_items] (in [-1, k): -1 belongs to no list) and the sums, enqueued on the handle's stream.  W: the caller's arrays,
// sized by kmeans_lists_chunks; sums[k][dim] keeps what it held for a label without an unskipped member.
int64_t kmeans_lists_chunks(int64_t n_items) { return (n_items + KM_CHUNK - 1) / KM_CHUNK; }

int kmeans_label_sums(morna_index *h, const int32_t *assign, int32_t k, const KmeansLists &W, double *sums)
{
    const int64_t N = h->n_items, nblk = (N + KM_THREADS - 1) / KM_THREADS, chunks = kmeans_lists_chunks(N);
    const int32_t D = h->dim, dpad = h->dpad;
    hipLaunchKernelGGL(kmeans_norms_kernel, dim3((unsigned)nblk), dim3(KM_THREADS), 0, h->stream, h->X.p, N, D, dpad, W.scale);
    // (prev = assign: no row counts as changed)
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3((unsigned)chunks), dim3(KM_THREADS), (size_t)k * 4, h->stream, assign, assign, N, k,
                       W.chunk_cnt, W.totals);
    hipLaunchKernelGGL(kmeans_starts_kernel, dim3(1), dim3(KM_THREADS), 0, h->stream, W.chunk_cnt, (int32_t)chunks, k, W.sizes, W.start);
    hipLaunchKernelGGL(kmeans_scatter_kernel, dim3((unsigned)chunks), dim3(KM_THREADS), (size_t)k * 4, h->stream, assign, N, k,
                       W.chunk_cnt, W.start, W.member);
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)k, (unsigned)((D + KM_THREADS - 1) / KM_THREADS)), dim3(KM_THREADS), 0,
                       h->stream, h->X.p, D, dpad, W.member, W.start, W.sizes, W.scale, sums);
    HIP_TRY(hipGetLastError());
    return MORNA_OK;
}

// The scales alone (pca.hip), enqueued on the handle's stream.
int kmeans_row_scales(morna_index *h, double *scale)
{
    const int64_t N = h->n_items, nblk = (N + KM_THREADS - 1) / KM_THREADS;
    hipLaunchKernelGGL(kmeans_norms_kernel, dim3((unsigned)nblk), dim3(KM_THREADS), 0, h->stream, h->X.p, N, h->dim, h->dpad, scale);
    HIP_TRY(hipGetLastError());
    return MORNA_OK;
}

}  // namespace morna
