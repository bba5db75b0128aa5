// forest.hip -- level-synchronous random-projection forest build on gfx950.
//
// Replaces AnnoyIndex.build(n_trees) (reference call site morna.py:425; the
// algorithm is spotify/annoy's _make_tree / two_means / Angular::create_split,
// restated in oracle/annoy_oracle.c mode 1 and SURVEY.md section 2.1).
//
// All n_trees trees advance one level per round.  A tree is a permutation of the
// item ids (perm[tree][N]); a node is a contiguous segment of it.  During a build the
// permutations live in a work buffer of two images per tree, [tree][2][N]: a node of depth
// L has its items in image L & 1 (TASK_ITEMS_AT), a partition writes its children into the
// other image, and the finished leaves are gathered into perm at the end.  Per level:
//   two_means_wave_kernel  one WAVE per split node, centroids / current row / next
//                     row in registers: 200 sequential centroid updates, the row of
//                     step l+1 in flight during step l (the Kiss32 stream does not
//                     depend on data; it arrives by LDS-DMA).  two_means_strip_kernel:
//                     four waves per node, each owning 16 of the 64 canonical lanes of every
//                     dot product and that strip of the centroids, for levels whose nodes
//                     fit the chip at once.  two_means_kernel: the LDS form (one workgroup
//                     per node) for rows too long for the register file.  two_means_wide_kernel:
//                     rows past 8192 floats (up to 32768), p in registers, q in LDS, rows streamed.
//   (splitmm.hip)     the sides of the whole level as one fp16 MFMA product that filters,
//                     exact fp32 dots for the pairs it cannot decide -- the form that runs
//                     while a tree has at most 32 split nodes, and, once the rows of the
//                     contraction are ordered and a row tile is multiplied with its own list
//                     of tasks, up to 256 per tree and for retries.  Otherwise:
//   split_kernel      every row of every split node is dotted (wavefront dot product,
//                     hyperplane resident in LDS) against its node's hyperplane, one
//                     workgroup per 64 positions of a node; launch order sorted by row
//                     id, one run per XCD, so the trees' re-reads hit L2.
//   post_counts_kernel  the level's right-side counts into a page-locked mailbox the host polls
//   (host)            annoy's 3-attempt / 0.95 imbalance rule on the counts
//   fallback_kernel   random sides for nodes still above 0.99
//   partition_stream_kernel  stable partition of each segment by side, from one image of the tree into the other: wide
//                     aligned loads, the chunk compacted through LDS, 16-byte stores; one workgroup per 4096-position
//                     chunk behind partition_count_kernel (which posts the counts too) where nodes span several chunks
//   partition_kernel  the earlier form (MORNA_PARTITION_FORM=0, and the one that keeps `inv`: MORNA_PARTITION_INV=1)
//   (splitmm.hip)     split_inv_kernel: inv[tree][row], the position in the tree of the item a row of the contraction stands
//                     for (what the matrix-core split finds a row's node with), rewritten for what the level's partitions
//                     moved -- on the side stream, under the NEXT level's two_means
//   pull_tasks_kernel / gather_leaves_kernel  task lists and node tables out of page-locked host memory; the leaves
//                     into perm when the build ends
// Node ids are handed out breadth-first, children of the i-th split node of a
// level get consecutive ids, exactly as oracle mode 1 does.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "devutil.hpp"

namespace morna {

#define TM_THREADS 256
#define TM_ITERS 200
#ifndef TM_STRIP_DEPTH
#define TM_STRIP_DEPTH 4   // rows in flight per node in two_means_strip_kernel
#endif

// ------------------------------------------------------------------ two_means

// normalise an LDS vector in place: v /= sqrt(dot(v, v)) when the norm is > 0
__device__ inline void lds_normalize(float *v, int dpad, int tid, int lane, int w, float *s_tmp)
{
    if (w == 0) {
        float n2 = wave_dot((const float4 *)v, (const float4 *)v, dpad / 4, lane);
        if (lane == 0) s_tmp[0] = sqrtf(n2);
    }
    __syncthreads();
    const float norm = s_tmp[0];
    if (norm > 0.f)
        for (int z = tid; z < dpad; z += TM_THREADS) v[z] = v[z] / norm;
    __syncthreads();
}

__global__ __launch_bounds__(TM_THREADS) void two_means_kernel(const float *__restrict__ X,
                                                               const float *__restrict__ norm2, int64_t n_items,
                                                               int32_t dpad, const int32_t *__restrict__ perm,
                                                               const SplitTask *__restrict__ tasks, uint32_t seed,
                                                               float *__restrict__ hp, int32_t *__restrict__ ones)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (threadIdx.x == 0) ones[blockIdx.x] = 0;   // the split kernels that follow count this task's right side here
    float *p = (float *)smem;        // centroid p   [dpad]
    float *q = p + dpad;             // centroid q   [dpad]
    float *xs = q + dpad;            // current row  [dpad]
    __shared__ float s_tmp[4];       // 0: scratch norm, 1: pp, 2: qq
    __shared__ float s_pq[2];

    const SplitTask t = tasks[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int nvec = dpad / 4;
    const int32_t *items = perm + TASK_ITEMS_AT(t, n_items);
    Kiss32 rng(node_seed(seed, (uint32_t)t.tree, (uint32_t)t.level, (uint32_t)t.start, (uint32_t)t.attempt));

    // two distinct random items seed the centroids
    uint32_t i = rng.index((uint32_t)t.count);
    uint32_t j = rng.index((uint32_t)t.count - 1u);
    j += (j >= i);
    {
        const float4 *xi = (const float4 *)(X + (int64_t)items[i] * dpad);
        const float4 *xj = (const float4 *)(X + (int64_t)items[j] * dpad);
        for (int v = tid; v < nvec; v += TM_THREADS) {
            ((float4 *)p)[v] = xi[v];
            ((float4 *)q)[v] = xj[v];
        }
    }
    __syncthreads();
    lds_normalize(p, dpad, tid, lane, w, s_tmp);
    lds_normalize(q, dpad, tid, lane, w, s_tmp);
    if (w == 0) {
        float v = wave_dot((const float4 *)p, (const float4 *)p, nvec, lane);
        if (lane == 0) s_tmp[1] = v;
    } else if (w == 1) {
        float v = wave_dot((const float4 *)q, (const float4 *)q, nvec, lane);
        if (lane == 0) s_tmp[2] = v;
    }
    // first row of the loop
    uint32_t k = rng.index((uint32_t)t.count);
    int32_t it = items[k];
    {
        const float4 *xk = (const float4 *)(X + (int64_t)it * dpad);
        for (int v = tid; v < nvec; v += TM_THREADS) ((float4 *)xs)[v] = xk[v];
    }
    __syncthreads();

    int ic = 1, jc = 1;
    // registers for the prefetched next row: nvec / 256 float4 per thread (<= 8 for D <= 8192)
    constexpr int PF = 8;
    for (int l = 0; l < TM_ITERS; l++) {
        // prefetch row l+1 while row l is being used
        uint32_t k_next = 0;
        int32_t it_next = 0;
        float4 pf[PF];
#pragma unroll
        for (int u = 0; u < PF; u++) pf[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool more = l + 1 < TM_ITERS;
        if (more) {
            k_next = rng.index((uint32_t)t.count);
            it_next = items[k_next];
            const float4 *xn = (const float4 *)(X + (int64_t)it_next * dpad);
#pragma unroll
            for (int u = 0; u < PF; u++) {
                const int v = tid + u * TM_THREADS;
                if (v < nvec) pf[u] = xn[v];
            }
        }
        const float nk2 = norm2[it];
        if (w == 0) {
            float v = wave_dot((const float4 *)p, (const float4 *)xs, nvec, lane);
            if (lane == 0) s_pq[0] = v;
        } else if (w == 1) {
            float v = wave_dot((const float4 *)q, (const float4 *)xs, nvec, lane);
            if (lane == 0) s_pq[1] = v;
        }
        __syncthreads();
        const float di = (float)ic * ang_dist(s_tmp[1], nk2, s_pq[0]);
        const float dj = (float)jc * ang_dist(s_tmp[2], nk2, s_pq[1]);
        const float norm = sqrtf(nk2);
        if (norm > 0.f) {
            if (di < dj) {
                const float fic = (float)ic, fic1 = (float)(ic + 1);
                for (int z = tid; z < dpad; z += TM_THREADS) p[z] = (p[z] * fic + xs[z] / norm) / fic1;
                __syncthreads();
                if (w == 0) {
                    float v = wave_dot((const float4 *)p, (const float4 *)p, nvec, lane);
                    if (lane == 0) s_tmp[1] = v;
                }
                ic++;
            } else if (dj < di) {
                const float fjc = (float)jc, fjc1 = (float)(jc + 1);
                for (int z = tid; z < dpad; z += TM_THREADS) q[z] = (q[z] * fjc + xs[z] / norm) / fjc1;
                __syncthreads();
                if (w == 0) {
                    float v = wave_dot((const float4 *)q, (const float4 *)q, nvec, lane);
                    if (lane == 0) s_tmp[2] = v;
                }
                jc++;
            }
        }
        __syncthreads();   // everyone is done with xs (and sees the new pp / qq)
        if (more) {
#pragma unroll
            for (int u = 0; u < PF; u++) {
                int v = tid + u * TM_THREADS;
                if (v < nvec) ((float4 *)xs)[v] = pf[u];
            }
            it = it_next;
        }
        __syncthreads();
    }
    // create_split: n = normalize(p - q)
    for (int z = tid; z < dpad; z += TM_THREADS) p[z] = p[z] - q[z];
    __syncthreads();
    lds_normalize(p, dpad, tid, lane, w, s_tmp);
    float4 *out = (float4 *)(hp + (int64_t)t.slot * dpad);
    for (int v = tid; v < nvec; v += TM_THREADS) out[v] = ((float4 *)p)[v];
}

// ---- two_means, one WAVE per node, everything in registers ------------------------
// For dpad <= 3072 the two centroids, the current row and the prefetched next row fit the
// register file (4 x NV float4 per lane): no LDS, no workgroup barrier in the 200-step loop.
// Same arithmetic, same order as two_means_kernel (the lane owns the same elements).

#define EW4(dst, expr_x, expr_y, expr_z, expr_w) \
    do { (dst).x = (expr_x); (dst).y = (expr_y); (dst).z = (expr_z); (dst).w = (expr_w); } while (0)

template <int NV>
__device__ inline float reg_dot(const float4 (&a)[NV], const float4 (&b)[NV])
{
    Acc4 s = acc4_zero();
#pragma unroll
    for (int k = 0; k < NV; k++) fma4(s, a[k], b[k]);   // pad elements are 0 in both: fmaf(0, 0, s) == s
    return acc4_finish(s);
}

// rows are padded to NV * 256 floats exactly (dpad is a multiple of 256): no lane is ever idle
template <int NV>
__device__ inline void reg_load_row(const float *row, int nvec, int lane, float4 (&x)[NV])
{
    const float4 *xp = (const float4 *)row;
#pragma unroll
    for (int k = 0; k < NV; k++) x[k] = xp[lane + k * WAVE];
}

template <int NV>
__device__ inline void reg_normalize(float4 (&v)[NV])
{
    const float norm = sqrtf(reg_dot<NV>(v, v));
    if (norm > 0.f) {
#pragma unroll
        for (int k = 0; k < NV; k++) EW4(v[k], v[k].x / norm, v[k].y / norm, v[k].z / norm, v[k].w / norm);
    }
}

// RN32(1 / n) for the counts a centroid can reach in TM_ITERS steps (1 + 200, then + 1): folded by the compiler,
// read through the scalar cache when a count changes.
struct RecipTable {
    float v[TM_ITERS + 8];
    constexpr RecipTable() : v()
    {
        for (int n = 1; n < TM_ITERS + 8; n++) v[n] = 1.0f / (float)n;
    }
};
__constant__ RecipTable k_recip = RecipTable();
__device__ inline float tm_recip(int n) { return k_recip.v[__builtin_amdgcn_readfirstlane(n)]; }   // n is wave-uniform

// One wave per node: both centroids and the current row in registers (3 x NV float4 per lane).  The row of the
// NEXT step is fetched by LDS-DMA (global_load_lds, no destination registers) at the top of a step and read into
// the row registers when the step's update is done: a register double buffer instead (NV = 12: 48 more VGPRs
// and 24 v_mov per step) does not fit two waves per SIMD without spilling, and a spill inside this loop waits
// for the whole prefetch (vmcnt is counted in order).
template <int NV>
__global__ __launch_bounds__(256, 3) void two_means_wave_kernel(const float *__restrict__ X, const RowInfo *__restrict__ rowinfo,
                                                             int64_t n_items, int32_t dpad,
                                                             const int32_t *__restrict__ perm,
                                                             const SplitTask *__restrict__ tasks, int32_t n_tasks,
                                                             uint32_t seed, float *__restrict__ hp, int32_t *__restrict__ ones,
                                                             const HalfImageOut img)
{
    __shared__ float4 xnext[256 / WAVE][NV * WAVE];   // per wave: the row of the coming step
    const int lane = threadIdx.x & (WAVE - 1);
    // the wave number as a scalar: the task, the node's Kiss32 stream and the row base addresses are then
    // wave-uniform to the compiler (scalar registers)
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int ti = blockIdx.x * (256 / WAVE) + wv;
    if (ti >= n_tasks) return;   // no barrier below: waves are independent
    if (lane == 0) ones[ti] = 0;   // the split kernels that follow count this task's right side here
    if (img.h16 && ti == 0 && lane == 0) *img.zero_me = 0u;   // ... and list the pairs their filter leaves open from here
    const SplitTask t = tasks[ti];
    const int nvec = dpad / 4;
    const int32_t *items = perm + TASK_ITEMS_AT(t, n_items);
    Kiss32 rng(node_seed(seed, (uint32_t)t.tree, (uint32_t)t.level, (uint32_t)t.start, (uint32_t)t.attempt));

    uint32_t i = rng.index((uint32_t)t.count);
    uint32_t j = rng.index((uint32_t)t.count - 1u);
    j += (j >= i);
    float4 p[NV], q[NV], x[NV];
    reg_load_row<NV>(X + (int64_t)items[i] * dpad, nvec, lane, p);
    reg_load_row<NV>(X + (int64_t)items[j] * dpad, nvec, lane, q);
    reg_normalize<NV>(p);
    reg_normalize<NV>(q);
    float pp = reg_dot<NV>(p, p), qq = reg_dot<NV>(q, q);
    uint32_t k = rng.index((uint32_t)t.count);
    const int32_t it = items[k];
    reg_load_row<NV>(X + (int64_t)it * dpad, nvec, lane, x);
    // The Kiss32 stream does not depend on data: the INDEX of row l+2 and the RowInfo of row l+1 are requested a step
    // before row l+1 itself, so that row's load never waits for its index (two dependent HBM round trips per step
    // otherwise bound the deep levels).  Draws past step 199 are never used: the stream is the node's own.
    // These look-ups go through the vector memory path (vgather) and come back to scalar registers when used.
    int32_t it_n1 = vgather(items, rng.index((uint32_t)t.count));
    RowInfo riv = vgather(rowinfo, (uint32_t)it);   // in flight: RowInfo of the row of the coming step
    float4 *xl = xnext[wv];

    int ic = 1, jc = 1;
    float r2p = tm_recip(2), r2q = tm_recip(2);   // RN32 of 1 / (ic + 1), 1 / (jc + 1), fetched when the count changes
    for (int l = 0; l < TM_ITERS; l++) {
        // this step's row: what was requested a step ago, now wave-uniform values in scalar registers
        const float nk2 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(riv.norm2)));
        const int norm_bits = __builtin_amdgcn_readfirstlane(__float_as_int(riv.norm));
        const long long r1_bits = ((long long)__builtin_amdgcn_readfirstlane((int)(__double_as_longlong(riv.rnorm) >> 32)) << 32) |
                                  (unsigned)__builtin_amdgcn_readfirstlane((int)__double_as_longlong(riv.rnorm));
        const int32_t it_next = __builtin_amdgcn_readfirstlane(it_n1);
        {
            // row l+1 -> LDS while row l is used; the reads of the previous row out of this buffer have returned.
            // (After the last step this fetches a row nobody uses: the stream has more draws and every index is valid.)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const float4 *src = (const float4 *)(X + (int64_t)it_next * dpad) + lane;
            // the instruction's immediate offset (< 4 KiB) moves both addresses: one base per four 1-KiB pieces
#define TM_GLDS(KK)                                                                                                       \
    if constexpr ((KK) < NV)                                                                                              \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + ((KK) & ~3) * WAVE),      \
                                         (__attribute__((address_space(3))) void *)(xl + ((KK) & ~3) * WAVE), 16,         \
                                         ((KK) & 3) * 1024, 0)
            TM_GLDS(0); TM_GLDS(1); TM_GLDS(2); TM_GLDS(3); TM_GLDS(4); TM_GLDS(5);
            TM_GLDS(6); TM_GLDS(7); TM_GLDS(8); TM_GLDS(9); TM_GLDS(10); TM_GLDS(11);
#undef TM_GLDS
            static_assert(NV <= 12, "TM_GLDS list");
        }
        it_n1 = vgather(items, rng.index((uint32_t)t.count));   // index of row l+2
        riv = vgather(rowinfo, (uint32_t)it_next);
        const float di = (float)ic * ang_dist(pp, nk2, reg_dot<NV>(p, x));
        const float dj = (float)jc * ang_dist(qq, nk2, reg_dot<NV>(q, x));
        const float norm = __int_as_float(norm_bits & 0x7fffffff);   // sqrtf(nk2)
        const unsigned long long force = norm_bits < 0 ? ~0ull : 0ull;   // x / norm may be subnormal somewhere in this row
        const double r1 = __longlong_as_double(r1_bits);
        if (norm > 0.f) {
            if (di < dj) {
                const float f0 = (float)ic, f1 = (float)(ic + 1);
#pragma unroll
                for (int kk = 0; kk < NV; kk++) p[kk] = centroid_step4(p[kk], x[kk], f0, f1, norm, r1, r2p, force);
                pp = reg_dot<NV>(p, p);
                ic++;
                r2p = tm_recip(ic + 1);
            }
            // not `else if`: as two independent branches each centroid is updated in place; chained, the compiler
            // writes the new p to a second set of registers and copies p there on every step that leaves it alone
            if (dj < di) {
                const float f0 = (float)jc, f1 = (float)(jc + 1);
#pragma unroll
                for (int kk = 0; kk < NV; kk++) q[kk] = centroid_step4(q[kk], x[kk], f0, f1, norm, r1, r2q, force);
                qq = reg_dot<NV>(q, q);
                jc++;
                r2q = tm_recip(jc + 1);
            }
        }
        // the row registers are free: row l+1 has had the whole step to land in LDS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int kk = 0; kk < NV; kk++) x[kk] = xl[kk * WAVE + lane];
    }
    // create_split: n = normalize(p - q)
#pragma unroll
    for (int kk = 0; kk < NV; kk++) EW4(p[kk], p[kk].x - q[kk].x, p[kk].y - q[kk].y, p[kk].z - q[kk].z, p[kk].w - q[kk].w);
    reg_normalize<NV>(p);
    float4 *out = (float4 *)(hp + (int64_t)t.slot * dpad);
#pragma unroll
    for (int kk = 0; kk < NV; kk++) out[lane + kk * WAVE] = p[kk];
    // the fp16 image the matrix-core split filters with: the lane holds what a lane of rows_to_half_kernel would read back
    if (img.h16) half_image_wave<NV>(p, lane, img.h16 + (int64_t)t.slot * dpad, img.norm + t.slot, img.err + t.slot);
}

// ---- two_means, four waves per node, by STRIPS of the canonical lanes ----------------------
// The shallow levels have fewer nodes than the chip has SIMDs and every node is one dependent chain of 200
// steps: what counts is the length of a step.  Here wave w of a node's workgroup owns the canonical lanes
// 16 w .. 16 w + 15 of every dot product: its lane l holds, for each 256-float k-step, element 64 w + l of the
// two centroids and of the row, i.e. chain (l & 3) of canonical lane 16 w + (l >> 2).  A dot is then
//   * the lane's ONE fmaf chain over the k-steps (the same chain wave_dot runs, four to a lane),
//   * the fold (a0 + a1) + (a2 + a3) across four neighbouring lanes (two DPP quad permutes),
//   * 64 folded values through LDS (one barrier), after which every wave runs the canonical butterfly on all of
//     them and holds the same result: same operations on the same values as wave_dot, bit for bit.
// Nothing else is exchanged and nothing is computed twice except the butterfly and the scalar distance
// arithmetic: a wave updates only its strip of the chosen centroid (12 elements per lane at D = 3000) and never
// sees the rest.  The dots of step l+1 (and the self-dot of the centroid just updated) are folded right after
// the update of step l, so a step has ONE barrier.  Rows are fetched DEPTH steps ahead into a register ring
// (a strip of a row is 12 registers), their index and RowInfo likewise: a step is several times shorter than an
// HBM round trip.  The loop is unrolled DEPTH times so that ring slots are compile-time registers.
template <int NV, int DEPTH>
__global__ __launch_bounds__(256) void two_means_strip_kernel(const float *__restrict__ X, const RowInfo *__restrict__ rowinfo,
                                                            int64_t n_items, int32_t dpad,
                                                            const int32_t *__restrict__ perm,
                                                            const SplitTask *__restrict__ tasks, uint32_t seed,
                                                            float *__restrict__ hp, int32_t *__restrict__ ones,
                                                            const HalfImageOut img)
{
    static_assert(NV % 4 == 0, "the update works on groups of four k-steps");
    if (threadIdx.x == 0) ones[blockIdx.x] = 0;   // the split kernels that follow count this task's right side here
    if (img.h16 && blockIdx.x == 0 && threadIdx.x == 0) *img.zero_me = 0u;   // ... and list their open pairs from here
    __shared__ float s_img[12];   // the image's largest element and two sums, per wave (half_block_*)
    static_assert(TM_ITERS % DEPTH == 0, "the step loop is unrolled DEPTH times");
    constexpr int NS = NV / 4;
    __shared__ float ex[2][3][WAVE];   // folded values of up to three dots per canonical lane, by exchange parity

    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int L = 16 * w + (lane >> 2);   // the canonical lane this lane's chain belongs to
    const SplitTask t = tasks[blockIdx.x];
    const int32_t *items = perm + TASK_ITEMS_AT(t, n_items);
    // every wave runs the node's Kiss32 stream itself: no index is exchanged
    Kiss32 rng(node_seed(seed, (uint32_t)t.tree, (uint32_t)t.level, (uint32_t)t.start, (uint32_t)t.attempt));
    const float *Xs = X + 64 * w + lane;   // this lane's element of k-step 0 of row 0

    // this lane's strip of a row: element 64 w + l of each k-step, four k-steps to a float4
    auto load_strip = [&](int32_t it, float4 (&dst)[NS]) {
        const float *r = Xs + (int64_t)it * dpad;
#pragma unroll
        for (int s = 0; s < NS; s++) EW4(dst[s], r[(4 * s) * 256], r[(4 * s + 1) * 256], r[(4 * s + 2) * 256], r[(4 * s + 3) * 256]);
    };
    // the lane's chain of a canonical dot: fmaf over the k-steps in order, from 0
    auto chain = [&](const float4 (&a)[NS], const float4 (&b)[NS]) {
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            acc = fmaf(a[s].x, b[s].x, acc);
            acc = fmaf(a[s].y, b[s].y, acc);
            acc = fmaf(a[s].z, b[s].z, acc);
            acc = fmaf(a[s].w, b[s].w, acc);
        }
        return acc;
    };
    int xpar = 0;
    // up to three dots at once: fold, exchange, butterfly.  Results in lanes 0 / 16 / 32 of the return value.
    auto exchange3 = [&](float a, float b, float c) {
        // (a0 + a1) + (a2 + a3) over the four chains of a canonical lane (quad_perm [1,0,3,2], then [2,3,0,1])
        a = a + dpp_move<0xB1>(a);
        b = b + dpp_move<0xB1>(b);
        c = c + dpp_move<0xB1>(c);
        a = a + dpp_move<0x4E>(a);
        b = b + dpp_move<0x4E>(b);
        c = c + dpp_move<0x4E>(c);
        if ((lane & 3) == 0) {
            ex[xpar][0][L] = a;
            ex[xpar][1][L] = b;
            ex[xpar][2][L] = c;
        }
        __syncthreads();
        const float f[3] = {ex[xpar][0][lane], ex[xpar][1][lane], ex[xpar][2][lane]};
        xpar ^= 1;   // the next exchange writes the other buffer: a wave may still be reading this one
        return wave_sum_multi<3>(f, lane);
    };
    auto lane_value = [](float u, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u), l)); };

    uint32_t i = rng.index((uint32_t)t.count);
    uint32_t j = rng.index((uint32_t)t.count - 1u);
    j += (j >= i);
    float4 p[NS], q[NS];
    load_strip(items[i], p);
    load_strip(items[j], q);
    {   // normalise both (reg_normalize), then their self-dots
        const float u = exchange3(chain(p, p), chain(q, q), 0.f);
        const float np = sqrtf(lane_value(u, 0)), nq = sqrtf(lane_value(u, 16));
        if (np > 0.f) {
#pragma unroll
            for (int s = 0; s < NS; s++) EW4(p[s], p[s].x / np, p[s].y / np, p[s].z / np, p[s].w / np);
        }
        if (nq > 0.f) {
#pragma unroll
            for (int s = 0; s < NS; s++) EW4(q[s], q[s].x / nq, q[s].y / nq, q[s].z / nq, q[s].w / nq);
        }
    }
    float pp, qq;
    {
        const float u = exchange3(chain(p, p), chain(q, q), 0.f);
        pp = lane_value(u, 0);
        qq = lane_value(u, 16);
    }

    // ring slot r holds the row of step l with l % DEPTH == r, its item id and its RowInfo (still vector registers
    // when they arrive; made scalar when used); it_ahead is the item of the step DEPTH ahead of the one running
    float4 x[DEPTH][NS];
    RowInfo ri[DEPTH];
#pragma unroll
    for (int r = 0; r < DEPTH; r++) {
        const int32_t it = items[rng.index((uint32_t)t.count)];
        load_strip(it, x[r]);
        ri[r] = rowinfo[it];
    }
    int32_t it_ahead = vgather(items, rng.index((uint32_t)t.count));

    int ic = 1, jc = 1;
    float r2p = tm_recip(2), r2q = tm_recip(2);   // RN32 of 1 / (ic + 1), 1 / (jc + 1)
    float u = exchange3(chain(p, x[0]), chain(q, x[0]), 0.f);   // the dots of step 0
    int upd_prev = 0;
#ifdef MORNA_TM_PROBE
    long long c_decide = 0, c_update = 0, c_fetch = 0, c_dots = 0, c_t;
#define TMP(acc) do { const long long n_ = clock64(); acc += n_ - c_t; c_t = n_; } while (0)
    c_t = clock64();
#else
#define TMP(acc) do { } while (0)
#endif
    for (int l0 = 0; l0 < TM_ITERS; l0 += DEPTH) {
#pragma unroll
        for (int r = 0; r < DEPTH; r++) {
            // ---- decide (every wave: same values, same decision)
            if (upd_prev == 1) pp = lane_value(u, 32);
            if (upd_prev == 2) qq = lane_value(u, 32);
            const float nk2 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ri[r].norm2)));
            const int norm_bits = __builtin_amdgcn_readfirstlane(__float_as_int(ri[r].norm));
            const long long r1_bits = ((long long)__builtin_amdgcn_readfirstlane((int)(__double_as_longlong(ri[r].rnorm) >> 32)) << 32) |
                                      (unsigned)__builtin_amdgcn_readfirstlane((int)__double_as_longlong(ri[r].rnorm));
            const float di = (float)ic * ang_dist(pp, nk2, lane_value(u, 0));
            const float dj = (float)jc * ang_dist(qq, nk2, lane_value(u, 16));
            const float norm = __int_as_float(norm_bits & 0x7fffffff);   // sqrtf(nk2)
            const unsigned long long force = norm_bits < 0 ? ~0ull : 0ull;
            const double r1 = __longlong_as_double(r1_bits);
            int upd = 0;
            if (norm > 0.f) upd = di < dj ? 1 : (dj < di ? 2 : 0);
            TMP(c_decide);
            // ---- update this wave's strip of the chosen centroid, and its chain of the new self-dot
            float cc = 0.f;
            if (upd == 1) {
                const float f0 = (float)ic, f1 = (float)(ic + 1);
#pragma unroll
                for (int s = 0; s < NS; s++) p[s] = centroid_step4(p[s], x[r][s], f0, f1, norm, r1, r2p, force);
                cc = chain(p, p);
                ic++;
                r2p = tm_recip(ic + 1);
            }
            if (upd == 2) {
                const float f0 = (float)jc, f1 = (float)(jc + 1);
#pragma unroll
                for (int s = 0; s < NS; s++) q[s] = centroid_step4(q[s], x[r][s], f0, f1, norm, r1, r2q, force);
                cc = chain(q, q);
                jc++;
                r2q = tm_recip(jc + 1);
            }
            upd_prev = upd;
            TMP(c_update);
            // ---- slot r is free: the row DEPTH steps ahead goes there.  (Past step 199 these fetch rows nobody
            // uses: the stream has more draws and every index is valid.)
            const int32_t it_new = it_ahead;
            load_strip(it_new, x[r]);
            ri[r] = vgather(rowinfo, (uint32_t)it_new);
            it_ahead = vgather(items, rng.index((uint32_t)t.count));
            TMP(c_fetch);
            // ---- the dots of the next step, with the row in the next slot
            constexpr int DUMMY = 0;
            (void)DUMMY;
            const int rn = (r + 1) % DEPTH;
            u = exchange3(chain(p, x[rn]), chain(q, x[rn]), cc);
            TMP(c_dots);
        }
    }
#ifdef MORNA_TM_PROBE
    if (blockIdx.x == 0 && threadIdx.x == 0)
        printf("[tm_strip probe] cycles per step: decide %lld update %lld fetch %lld dots+exchange %lld (nodes %d)\n",
               c_decide / TM_ITERS, c_update / TM_ITERS, c_fetch / TM_ITERS, c_dots / TM_ITERS, (int)gridDim.x);
#endif
#undef TMP
    // create_split: n = normalize(p - q), each wave its strip
#pragma unroll
    for (int s = 0; s < NS; s++) EW4(p[s], p[s].x - q[s].x, p[s].y - q[s].y, p[s].z - q[s].z, p[s].w - q[s].w);
    {
        const float un = exchange3(chain(p, p), 0.f, 0.f);
        const float nn = sqrtf(lane_value(un, 0));
        if (nn > 0.f) {
#pragma unroll
            for (int s = 0; s < NS; s++) EW4(p[s], p[s].x / nn, p[s].y / nn, p[s].z / nn, p[s].w / nn);
        }
    }
    float *out = hp + (int64_t)t.slot * dpad + 64 * w + lane;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        out[(4 * s) * 256] = p[s].x;
        out[(4 * s + 1) * 256] = p[s].y;
        out[(4 * s + 2) * 256] = p[s].z;
        out[(4 * s + 3) * 256] = p[s].w;
    }
    // the fp16 image the matrix-core split filters with (rows_to_half_kernel's, from the strips in registers): the scale
    // needs the row's largest element and the bounds two sums over all four waves, a barrier each
    if (img.h16) {   // uniform
        float m = 0.f;
        bool bad = false;
#pragma unroll
        for (int s = 0; s < NS; s++) m = fmaxf(m, half_absmax4(p[s], bad));
        const float sc = half_block_scale(m, bad, lane, w, s_img, bad);
        float sum = 0.f, sume = 0.f;
        _Float16 *o16 = img.h16 + (int64_t)t.slot * dpad + 64 * w + lane;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            o16[(4 * s) * 256] = half_convert1(p[s].x, sc, sum, sume);
            o16[(4 * s + 1) * 256] = half_convert1(p[s].y, sc, sum, sume);
            o16[(4 * s + 2) * 256] = half_convert1(p[s].z, sc, sum, sume);
            o16[(4 * s + 3) * 256] = half_convert1(p[s].w, sc, sum, sume);
        }
        half_block_bounds(sum, sume, bad, lane, w, s_img, img.norm + t.slot, img.err + t.slot);
    }
}

// ---- two_means for wide rows, 8192 < dpad <= 32768 ----------------------------------------------
// The strip layout of two_means_strip_kernel (lane l of wave w owns element 64 w + l of every 256-float k-step,
// chain (l & 3) of canonical lane 16 w + (l >> 2)), one workgroup per node, for rows whose strips no longer fit
// the register file three times over.  Of the nk = dpad / 256 k-steps of a lane, the first 4 * nf (nf = nk / 4
// groups of four, at most NG) are held as float4: centroid p in registers (128 floats per lane at 32768),
// centroid q in LDS, the lane's own slots only, so it needs no barrier.  The last nk % 4 k-steps of both
// centroids are LDS slots as well.  Rows are not kept: step l reads row l (the update) and row l+1 (the dots of
// the next step) strip by strip from HBM / L2 in one pass over the k-steps, so every chain still runs in k order.
// Same operations on the same values as two_means_strip_kernel and wave_dot, bit for bit.
// LDS: (4 nf + 2 (nk % 4)) x 1 KiB, 128 KiB at 32768.
#define TMW_MAX_DPAD 32768
template <int NG>
__global__ __launch_bounds__(256) void two_means_wide_kernel(const float *__restrict__ X, const RowInfo *__restrict__ rowinfo,
                                                           int64_t n_items, int32_t dpad,
                                                           const int32_t *__restrict__ perm,
                                                           const SplitTask *__restrict__ tasks, uint32_t seed,
                                                           float *__restrict__ hp, int32_t *__restrict__ ones,
                                                           const HalfImageOut img)
{
    // the launch picks the smallest NG of 12, 16, 24, 32 that holds nf: groups below the next smaller one always exist
    constexpr int NGLO = NG <= 12 ? 8 : NG <= 16 ? 12 : NG <= 24 ? 16 : 24;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float ex[2][3][WAVE];
    __shared__ float s_img[12];   // the image's largest element and two sums, per wave (half_block_*)
    if (threadIdx.x == 0) ones[blockIdx.x] = 0;   // the split kernels that follow count this task's right side here
    if (img.h16 && blockIdx.x == 0 && threadIdx.x == 0) *img.zero_me = 0u;   // ... and list their open pairs from here

    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int L = 16 * w + (lane >> 2);
    const int nk = dpad / 256, nf = nk / 4, nt = nk % 4;   // k-steps, full groups, k-steps of the tail
    // group g of q at QS(g) (an LDS instruction's offset reaches 64 KiB: groups 16 and up from a second base)
    float4 *qs = (float4 *)smem + threadIdx.x, *qs_hi = qs + 256 * 16;
    asm volatile("" : "+v"(qs_hi));
#define QS(g) ((g) < 16 ? qs : qs_hi)[256 * ((g) & 15)]
    float *pt = (float *)((float4 *)smem + 256 * nf) + threadIdx.x;   // tail k-step c of p at pt[256 c]
    float *qt = pt + 256 * nt;                                       // ... and of q
    const SplitTask t = tasks[blockIdx.x];
    const int32_t *items = perm + TASK_ITEMS_AT(t, n_items);
    Kiss32 rng(node_seed(seed, (uint32_t)t.tree, (uint32_t)t.level, (uint32_t)t.start, (uint32_t)t.attempt));
    const float *Xs = X + 64 * w + lane;

    // the next four k-steps of a row's strip, and the cursor moved past them.  The cursor is stepped in the loop
    // (opaque to the compiler): hoisted, the offsets of every group of two rows would crowd the registers.
    auto next4 = [](const float *&r) {
        const float4 v = make_float4(r[0], r[256], r[512], r[768]);
        r += 1024;
        asm volatile("" : "+v"(r));
        return v;
    };
    auto next1 = [](const float *&r) {
        const float v = r[0];
        r += 256;
        return v;
    };
    auto chain4 = [](float acc, const float4 a, const float4 b) {
        acc = fmaf(a.x, b.x, acc);
        acc = fmaf(a.y, b.y, acc);
        acc = fmaf(a.z, b.z, acc);
        acc = fmaf(a.w, b.w, acc);
        return acc;
    };
    int xpar = 0;
    auto exchange3 = [&](float a, float b, float c) {   // as in two_means_strip_kernel
        a = a + dpp_move<0xB1>(a);
        b = b + dpp_move<0xB1>(b);
        c = c + dpp_move<0xB1>(c);
        a = a + dpp_move<0x4E>(a);
        b = b + dpp_move<0x4E>(b);
        c = c + dpp_move<0x4E>(c);
        if ((lane & 3) == 0) {
            ex[xpar][0][L] = a;
            ex[xpar][1][L] = b;
            ex[xpar][2][L] = c;
        }
        __syncthreads();
        const float f[3] = {ex[xpar][0][lane], ex[xpar][1][lane], ex[xpar][2][lane]};
        xpar ^= 1;
        return wave_sum_multi<3>(f, lane);
    };
    auto lane_value = [](float u, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(u), l)); };
    auto step1 = [](float c, float x, float f0, float f1, float norm, double r1, float y, unsigned long long force) {
        return centroid_step4(make_float4(c, 0.f, 0.f, 0.f), make_float4(x, 0.f, 0.f, 0.f), f0, f1, norm, r1, y, force).x;
    };

    uint32_t i = rng.index((uint32_t)t.count);
    uint32_t j = rng.index((uint32_t)t.count - 1u);
    j += (j >= i);
    float4 p[NG];
    float pp, qq;
    {
        const float *ri_ = Xs + (int64_t)items[i] * dpad, *rj_ = Xs + (int64_t)items[j] * dpad;   // cursors
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int g = 0; g < NG; g++) {
            if (g < NGLO || g < nf) {
                p[g] = next4(ri_);
                const float4 qg = next4(rj_);
                QS(g) = qg;
                a = chain4(a, p[g], p[g]);
                b = chain4(b, qg, qg);
            } else {
                p[g] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        for (int c = 0; c < nt; c++) {
            const float pc = next1(ri_), qc = next1(rj_);
            pt[256 * c] = pc;
            qt[256 * c] = qc;
            a = fmaf(pc, pc, a);
            b = fmaf(qc, qc, b);
        }
        const float u = exchange3(a, b, 0.f);
        const float np = sqrtf(lane_value(u, 0)), nq = sqrtf(lane_value(u, 16));
        a = 0.f;
        b = 0.f;
#pragma unroll
        for (int g = 0; g < NG; g++) {
            if (g < NGLO || g < nf) {
                if (np > 0.f) EW4(p[g], p[g].x / np, p[g].y / np, p[g].z / np, p[g].w / np);
                float4 qg = QS(g);
                if (nq > 0.f) EW4(qg, qg.x / nq, qg.y / nq, qg.z / nq, qg.w / nq);
                QS(g) = qg;
                a = chain4(a, p[g], p[g]);
                b = chain4(b, qg, qg);
            }
        }
        for (int c = 0; c < nt; c++) {
            float pc = pt[256 * c], qc = qt[256 * c];
            if (np > 0.f) pc = pc / np;
            if (nq > 0.f) qc = qc / nq;
            pt[256 * c] = pc;
            qt[256 * c] = qc;
            a = fmaf(pc, pc, a);
            b = fmaf(qc, qc, b);
        }
        const float v = exchange3(a, b, 0.f);
        pp = lane_value(v, 0);
        qq = lane_value(v, 16);
    }

    // row 0 and the dots of step 0
    int32_t it_cur = items[rng.index((uint32_t)t.count)];
    RowInfo ri_cur = rowinfo[it_cur];
    float u;
    {
        const float *r = Xs + (int64_t)it_cur * dpad;   // cursor
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int g = 0; g < NG; g++) {
            if (g < NGLO || g < nf) {
                const float4 x = next4(r);
                a = chain4(a, p[g], x);
                b = chain4(b, QS(g), x);
            }
        }
        for (int c = 0; c < nt; c++) {
            const float x = next1(r);
            a = fmaf(pt[256 * c], x, a);
            b = fmaf(qt[256 * c], x, b);
        }
        u = exchange3(a, b, 0.f);
    }
    int ic = 1, jc = 1;
    float r2p = tm_recip(2), r2q = tm_recip(2);   // RN32 of 1 / (ic + 1), 1 / (jc + 1)
    int upd_prev = 0;
    for (int l = 0; l < TM_ITERS; l++) {
        // the row of the next step (past step 199 a row nobody uses: the stream has more draws, every index is valid)
        const int32_t it_nxt = vgather(items, rng.index((uint32_t)t.count));
        const RowInfo ri_nxt = vgather(rowinfo, (uint32_t)it_nxt);
        // ---- decide (every wave: same values, same decision)
        if (upd_prev == 1) pp = lane_value(u, 32);
        if (upd_prev == 2) qq = lane_value(u, 32);
        const float nk2 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ri_cur.norm2)));
        const int norm_bits = __builtin_amdgcn_readfirstlane(__float_as_int(ri_cur.norm));
        const long long r1_bits = ((long long)__builtin_amdgcn_readfirstlane((int)(__double_as_longlong(ri_cur.rnorm) >> 32)) << 32) |
                                  (unsigned)__builtin_amdgcn_readfirstlane((int)__double_as_longlong(ri_cur.rnorm));
        const float di = (float)ic * ang_dist(pp, nk2, lane_value(u, 0));
        const float dj = (float)jc * ang_dist(qq, nk2, lane_value(u, 16));
        const float norm = __int_as_float(norm_bits & 0x7fffffff);   // sqrtf(nk2)
        const unsigned long long force = norm_bits < 0 ? ~0ull : 0ull;
        const double r1 = __longlong_as_double(r1_bits);
        int upd = 0;
        if (norm > 0.f) upd = di < dj ? 1 : (dj < di ? 2 : 0);

        // ---- one pass over the k-steps: the update of step l with row l, then the chains of the new self-dot and of
        // the dots of step l+1 with the updated centroids
        const float *rc = Xs + (int64_t)__builtin_amdgcn_readfirstlane(it_cur) * dpad;   // cursors
        const float *rn = Xs + (int64_t)__builtin_amdgcn_readfirstlane(it_nxt) * dpad;
        float a = 0.f, b = 0.f, cc = 0.f;
        if (upd == 1) {
            const float f0 = (float)ic, f1 = (float)(ic + 1);
#pragma unroll
            for (int g = 0; g < NG; g++) {
                if (g < NGLO || g < nf) {
                    const float4 xc = next4(rc), xn = next4(rn);
                    p[g] = centroid_step4(p[g], xc, f0, f1, norm, r1, r2p, force);
                    cc = chain4(cc, p[g], p[g]);
                    a = chain4(a, p[g], xn);
                    b = chain4(b, QS(g), xn);
                }
            }
            for (int c = 0; c < nt; c++) {
                const float xc = next1(rc), xn = next1(rn);
                const float pc = step1(pt[256 * c], xc, f0, f1, norm, r1, r2p, force);
                pt[256 * c] = pc;
                cc = fmaf(pc, pc, cc);
                a = fmaf(pc, xn, a);
                b = fmaf(qt[256 * c], xn, b);
            }
            ic++;
            r2p = tm_recip(ic + 1);
        } else if (upd == 2) {
            const float f0 = (float)jc, f1 = (float)(jc + 1);
#pragma unroll
            for (int g = 0; g < NG; g++) {
                if (g < NGLO || g < nf) {
                    const float4 xc = next4(rc), xn = next4(rn);
                    const float4 qg = centroid_step4(QS(g), xc, f0, f1, norm, r1, r2q, force);
                    QS(g) = qg;
                    cc = chain4(cc, qg, qg);
                    a = chain4(a, p[g], xn);
                    b = chain4(b, qg, xn);
                }
            }
            for (int c = 0; c < nt; c++) {
                const float xc = next1(rc), xn = next1(rn);
                const float qc = step1(qt[256 * c], xc, f0, f1, norm, r1, r2q, force);
                qt[256 * c] = qc;
                cc = fmaf(qc, qc, cc);
                a = fmaf(pt[256 * c], xn, a);
                b = fmaf(qc, xn, b);
            }
            jc++;
            r2q = tm_recip(jc + 1);
        } else {
#pragma unroll
            for (int g = 0; g < NG; g++) {
                if (g < NGLO || g < nf) {
                    const float4 xn = next4(rn);
                    a = chain4(a, p[g], xn);
                    b = chain4(b, QS(g), xn);
                }
            }
            for (int c = 0; c < nt; c++) {
                const float xn = next1(rn);
                a = fmaf(pt[256 * c], xn, a);
                b = fmaf(qt[256 * c], xn, b);
            }
        }
        upd_prev = upd;
        u = exchange3(a, b, cc);
        it_cur = it_nxt;
        ri_cur = ri_nxt;
    }
    // create_split: n = normalize(p - q)
    float a = 0.f;
#pragma unroll
    for (int g = 0; g < NG; g++) {
        if (g < NGLO || g < nf) {
            const float4 qg = QS(g);
            EW4(p[g], p[g].x - qg.x, p[g].y - qg.y, p[g].z - qg.z, p[g].w - qg.w);
            a = chain4(a, p[g], p[g]);
        }
    }
    for (int c = 0; c < nt; c++) {
        const float d = pt[256 * c] - qt[256 * c];
        pt[256 * c] = d;
        a = fmaf(d, d, a);
    }
    const float nn = sqrtf(lane_value(exchange3(a, 0.f, 0.f), 0));
    float *out = hp + (int64_t)t.slot * dpad + 64 * w + lane;
#pragma unroll
    for (int g = 0; g < NG; g++) {
        if (g < NGLO || g < nf) {
            if (nn > 0.f) EW4(p[g], p[g].x / nn, p[g].y / nn, p[g].z / nn, p[g].w / nn);
            out[(4 * g) * 256] = p[g].x;
            out[(4 * g + 1) * 256] = p[g].y;
            out[(4 * g + 2) * 256] = p[g].z;
            out[(4 * g + 3) * 256] = p[g].w;
        }
    }
    for (int c = 0; c < nt; c++) {
        float d = pt[256 * c];
        if (nn > 0.f) d = d / nn;
        out[(4 * nf + c) * 256] = d;
        pt[256 * c] = d;   // (the lane's own slot: read back below)
    }
    // the fp16 image the matrix-core split filters with, as in two_means_strip_kernel: the hyperplane is p and the tail slots
    if (img.h16) {   // uniform
        float m = 0.f;
        bool bad = false;
#pragma unroll
        for (int g = 0; g < NG; g++)
            if (g < NGLO || g < nf) m = fmaxf(m, half_absmax4(p[g], bad));
        for (int c = 0; c < nt; c++) m = fmaxf(m, half_absmax4(make_float4(pt[256 * c], 0.f, 0.f, 0.f), bad));
        const float sc = half_block_scale(m, bad, lane, w, s_img, bad);
        float sum = 0.f, sume = 0.f;
        _Float16 *o16 = img.h16 + (int64_t)t.slot * dpad + 64 * w + lane;
#pragma unroll
        for (int g = 0; g < NG; g++) {
            if (g < NGLO || g < nf) {
                o16[(4 * g) * 256] = half_convert1(p[g].x, sc, sum, sume);
                o16[(4 * g + 1) * 256] = half_convert1(p[g].y, sc, sum, sume);
                o16[(4 * g + 2) * 256] = half_convert1(p[g].z, sc, sum, sume);
                o16[(4 * g + 3) * 256] = half_convert1(p[g].w, sc, sum, sume);
            }
        }
        for (int c = 0; c < nt; c++) o16[(4 * nf + c) * 256] = half_convert1(pt[256 * c], sc, sum, sume);
        half_block_bounds(sum, sume, bad, lane, w, s_img, img.norm + t.slot, img.err + t.slot);
    }
}
// dynamic LDS of two_means_wide_kernel
#undef QS
static inline size_t tm_wide_lds(int32_t dpad) { return (size_t)((dpad / 256) / 4 * 4 + 2 * ((dpad / 256) % 4)) * 256 * 4; }

// ---------------------------------------------------------------- split kernel

#define SP_THREADS 256
#define SP_WAVES (SP_THREADS / WAVE)
#define SP_ROWS 64      // rows per workgroup

// ---- XCD-aware launch order of the split kernel ---------------------------------
// Every row is read once per TREE at every level, and a node's item list is sorted
// by id (stable partitions of the identity permutation).  Chunks are therefore
// ordered by the id of their first row, and the sorted list is cut into 8
// contiguous runs, one per XCD (workgroup b runs on XCD b % 8): the ~n_trees
// chunks that need the same rows then run back to back on ONE XCD and find them in
// its L2 instead of HBM.  The order only affects speed, never results.

#define SCHED_MAX_BUCKETS 65536

__global__ void sched_bucket_kernel(const SplitTask *__restrict__ tasks, int32_t n_tasks, int32_t n_chunks,
                                    const int32_t *__restrict__ perm, int64_t n_items, int32_t n_buckets,
                                    int32_t *__restrict__ hist, int2 *__restrict__ info /* [n_chunks] task, bucket */)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    int lo = 0, hi = n_tasks - 1;   // the task owning this chunk (tasks sorted by chunk0)
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (tasks[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    const SplitTask t = tasks[lo];
    const int pos0 = (c - t.chunk0) * 64;
    const int64_t first = perm[TASK_ITEMS_AT(t, n_items) + pos0];
    const int b = (int)(first * n_buckets / n_items);
    atomicAdd(&hist[b], 1);
    info[c] = make_int2(lo, b);
}

__global__ __launch_bounds__(1024) void sched_scan_kernel(const int32_t *__restrict__ hist, int32_t n_buckets,
                                                          int32_t *__restrict__ cursor /* [n_buckets] start offsets */)
{
    __shared__ int s_part[1024];
    const int tid = threadIdx.x;
    const int per = (n_buckets + 1023) / 1024;
    const int lo = tid * per, hi = lo + per < n_buckets ? lo + per : n_buckets;
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += hist[i];
    s_part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        int v = tid >= o ? s_part[tid - o] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int run = tid ? s_part[tid - 1] : 0;
    for (int i = lo; i < hi; i++) {
        cursor[i] = run;
        run += hist[i];
    }
}

__global__ void sched_scatter_kernel(const SplitTask *__restrict__ tasks, int32_t n_chunks,
                                     const int2 *__restrict__ info, int32_t *__restrict__ cursor,
                                     int2 *__restrict__ sched /* [n_chunks] task, chunk in task */)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const int2 e = info[c];
    const int pos = atomicAdd(&cursor[e.y], 1);
    sched[pos] = make_int2(e.x, c - tasks[e.x].chunk0);
}

// rows [chunk*SP_ROWS, ...) of one task get their side
__global__ __launch_bounds__(SP_THREADS) void split_kernel(const float *__restrict__ X, int64_t n_items, int32_t dpad,
                                                           const int32_t *__restrict__ perm,
                                                           const SplitTask *__restrict__ tasks,
                                                           const int2 *__restrict__ sched, int32_t n_chunks,
                                                           uint32_t seed, const float *__restrict__ hp,
                                                           uint8_t *__restrict__ side, int32_t *__restrict__ ones)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *hs = (float4 *)smem;   // hyperplane [dpad]
    __shared__ int s_ones;

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int nvec = dpad / 4;
    // workgroup b runs on XCD b % 8: XCD x walks the x-th eighth of the sorted chunk list
    const int per_xcd = (n_chunks + 7) / 8;
    const int si = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per_xcd || si >= n_chunks) return;
    const int2 se = sched[si];
    const int lo = se.x;
    const SplitTask t = tasks[lo];
    const int pos0 = se.y * SP_ROWS;
    const int nrows = (t.count - pos0) < SP_ROWS ? (t.count - pos0) : SP_ROWS;

    const float4 *hsrc = (const float4 *)(hp + (int64_t)t.slot * dpad);
    for (int v = tid; v < nvec; v += SP_THREADS) hs[v] = hsrc[v];
    if (tid == 0) s_ones = 0;
    __syncthreads();

    const int32_t *items = perm + TASK_ITEMS_AT(t, n_items) + pos0;
    uint8_t *sd = side + (int64_t)t.tree * n_items + t.start + pos0;
    const uint32_t nseed = node_seed(seed, (uint32_t)t.tree, (uint32_t)t.level, (uint32_t)t.start, (uint32_t)t.attempt);
    int my_ones = 0;
    // A wave takes FOUR rows at a time: one LDS read of the hyperplane serves four rows, four row
    // streams are in flight, and the four lane-sums are reduced together (wave_sum_multi: row j's dot
    // arrives in lane 16 j, which writes its side).  Same chains per row as wave_dot.
    // Default cache policy on purpose: with non-temporal loads the rows are not kept in L2 for the
    // other trees' chunks that follow on this XCD (measured: 8.7 ms instead of 4.9 ms per level).
    for (int r = 4 * w; r < nrows; r += 4 * SP_WAVES) {
        const float4 *x[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int rj = r + j < nrows ? r + j : r;   // a missing row repeats row r; its result is dropped
            x[j] = (const float4 *)(X + (int64_t)items[rj] * dpad);
        }
        Acc4 c[4] = {acc4_zero(), acc4_zero(), acc4_zero(), acc4_zero()};
#pragma unroll 2
        for (int i = lane; i < nvec; i += WAVE) {   // nvec is a multiple of 64: no lane idles
            const float4 x0 = x[0][i], x1 = x[1][i], x2 = x[2][i], x3 = x[3][i];
            const float4 hv = hs[i];
            fma4(c[0], x0, hv);
            fma4(c[1], x1, hv);
            fma4(c[2], x2, hv);
            fma4(c[3], x3, hv);
        }
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; j++) f[j] = (c[j].lo.x + c[j].lo.y) + (c[j].hi.x + c[j].hi.y);
        const float d = wave_sum_multi<4>(f, lane);
        const int rr = r + (lane >> 4);
        int s = 0;
        if ((lane & 15) == 0 && rr < nrows) {
            // Angular::side: dot != 0 ? dot > 0 : coin flip
            s = d != 0.f ? (d > 0.f) : pos_flip(nseed, (uint32_t)(pos0 + rr));
            sd[rr] = (uint8_t)s;
        }
        my_ones += __builtin_popcountll(__ballot(s));
    }
    if (lane == 0 && my_ones) atomicAdd(&s_ones, my_ones);
    __syncthreads();
    if (tid == 0 && s_ones) atomicAdd(&ones[lo], s_ones);
}

// random sides for nodes whose best split is still > 0.99 imbalanced
__global__ __launch_bounds__(256) void fallback_kernel(const SplitTask *__restrict__ tasks, int64_t n_items,
                                                       int32_t dpad, uint32_t seed, uint8_t *__restrict__ side,
                                                       int32_t *__restrict__ ones, float *__restrict__ hp)
{
    __shared__ int s_cnt;
    const SplitTask t = tasks[blockIdx.x];
    const int tid = threadIdx.x;
    uint8_t *sd = side + (int64_t)t.tree * n_items + t.start;
    for (int z = tid; z < dpad; z += 256) hp[(int64_t)t.slot * dpad + z] = 0.f;   // m->v = 0
    for (int round = 0;; round++) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        int mine = 0;
        if (round >= 32) {   // give up on chance: halve by position
            for (int p = tid; p < t.count; p += 256) {
                int s = p >= t.count / 2;
                sd[p] = (uint8_t)s;
                mine += s;
            }
        } else {
            const uint32_t ns = node_seed(seed, (uint32_t)t.tree, (uint32_t)t.level, (uint32_t)t.start, (uint32_t)(3 + round));
            for (int p = tid; p < t.count; p += 256) {
                int s = pos_flip(ns, (uint32_t)p);
                sd[p] = (uint8_t)s;
                mine += s;
            }
        }
        if (mine) atomicAdd(&s_cnt, mine);
        __syncthreads();
        const int n1 = s_cnt;
        __syncthreads();
        if (round >= 32 || !(split_imbalance(t.count - n1, n1) > 0.99)) {
            if (tid == 0) ones[blockIdx.x] = n1;
            break;
        }
    }
}

// annoy's rule for the sides of one attempt (_make_tree): attempts 0 and 1 stand when the imbalance is below 0.95,
// the last attempt (2) unless it is above 0.99 (then the node gets random sides: tasks of "attempt" 3, which always
// stand).  The host driver applies the same expressions to the same counts.
__host__ __device__ inline bool sides_stand(int attempt, int64_t n0, int64_t n1)
{
    if (attempt >= 3) return true;
    const double imb = split_imbalance(n0, n1);
    return attempt == 2 ? !(imb > 0.99) : imb < 0.95;
}

// stable partition of one segment by side; one workgroup per node (PT threads: 1024 while nodes are large).
// Launched right behind the split of every attempt, before the host has seen the counts: a node whose sides do
// not stand is left alone (its next attempt, or the fallback, partitions it).
// INV (MORNA_PARTITION_INV=1 only): inv[tree][rank ? rank[item] : item] = position of the item in the tree's permutation is
// kept current here, behind a gather of `rank` and with one scattered store per item.  Nothing on a level's chain reads
// `inv` before the next level's contraction, so by default it is rewritten beside that level's two_means instead
// (splitmm.hip, split_inv_kernel) and this kernel -- a chain of memory round trips -- has neither.
// The right-side counts of a level's tasks, posted to page-locked host memory tagged with the call's epoch: a launch of its
// own in front of the partition, so that ALL counts are with the host a few microseconds after the split and its
// bookkeeping for the next attempt or level runs while the partition does (posted by the partition workgroups themselves,
// the last counts arrived when the last workgroups started, near the partition's end: 20-65 us of idle device per level).
__global__ void post_counts_kernel(const int32_t *__restrict__ ones, int32_t n, unsigned long long *__restrict__ host_counts,
                                   uint32_t epoch)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    // relaxed: the word carries everything the host reads (a release here would write back this CU's whole L2 share)
    if (i < n)
        __hip_atomic_store(&host_counts[i], ((unsigned long long)epoch << 32) | (unsigned int)ones[i], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

// the level's task list, pulled out of page-locked host memory by the device itself: a hipMemcpyAsync of more than a few KB
// goes to the SDMA engine, ~20 us of start-up during which the stream has nothing else to run
// (dst2: where the words from n_first on go -- the runs of split_inv_kernel ride behind the level's tasks)
__global__ void pull_tasks_kernel(const int4 *__restrict__ src /* host memory, device-visible */, int4 *__restrict__ dst, int32_t n16,
                                  int4 *__restrict__ dst2 = nullptr, int32_t n_first = 0)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n16) return;
    if (dst2 && i >= n_first) dst2[i - n_first] = src[i];
    else dst[i] = src[i];
}

template <int PT, bool INV>
__global__ __launch_bounds__(PT) void partition_kernel(const SplitTask *__restrict__ tasks, int64_t n_items,
                                                       const uint8_t *__restrict__ side,
                                                       const int32_t *__restrict__ ones, int32_t *__restrict__ perm /* work buffer [tree][2][n_items] */,
                                                       int32_t *__restrict__ inv,
                                                       const int32_t *__restrict__ rank /* inv is indexed by rank[item] (or null: by item) */)
{
    __shared__ int s_w1[PT / WAVE];
    const SplitTask t = tasks[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int n1 = ones[blockIdx.x], n0 = t.count - n1;
    if (!sides_stand(t.attempt, n0, n1)) return;   // uniform over the workgroup
    const int64_t base = (int64_t)t.tree * n_items + t.start;   // of the node's side bytes (and of its positions in `inv`)
    // the node's items are read from the image of its depth and its children are written into the other one: no copy back
    const int32_t *src = perm + TASK_ITEMS_AT(t, n_items);
    int32_t *dst_img = perm + ((int64_t)t.tree * 2 + ((t.level + 1) & 1)) * n_items + t.start;
    // PT_PER consecutive positions per thread and round: a round costs two barriers whatever it moves, and with one
    // position per thread the root level took 49 of them (0.08 ms).  Ranks: right-side and valid counts of a thread
    // packed into one integer (16 bits each: a round has at most 4096 positions), scanned over the wave, wave totals
    // through LDS.
    constexpr int PT_PER = 4;
    int run0 = 0, run1 = 0;   // items already placed on each side
    // a round's sides and items are asked for one round ahead (they depend on nothing the round before computes): the
    // kernel is a chain of memory round trips, three per round when each waits for the one before
    int sd_n[PT_PER], it_n[PT_PER];
    auto fetch = [&](int p0) {
        const int pb = p0 + tid * PT_PER;
#pragma unroll
        for (int u = 0; u < PT_PER; u++) {
            const bool valid = pb + u < t.count;
            sd_n[u] = valid ? (int)side[base + pb + u] : -1;
            it_n[u] = valid ? src[pb + u] : 0;
        }
    };
    fetch(0);
    for (int p0 = 0; p0 < t.count; p0 += PT * PT_PER) {
        int sd[PT_PER], it[PT_PER], pk = 0;
#pragma unroll
        for (int u = 0; u < PT_PER; u++) {
            sd[u] = sd_n[u];
            it[u] = it_n[u];
            pk += sd[u] >= 0 ? (sd[u] ? 0x10001 : 0x10000) : 0;
        }
        if (p0 + PT * PT_PER < t.count) fetch(p0 + PT * PT_PER);   // uniform
        int incl = pk;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int v = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += v;
        }
        if (lane == WAVE - 1) s_w1[w] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < PT / WAVE; i++) {
            if (i < w) before += s_w1[i];
            total += s_w1[i];
        }
        const int excl = incl - pk + before;
        int r1 = excl & 0xffff, rv = excl >> 16;   // right-side / valid positions before this thread's first
        int rk[PT_PER];
        if constexpr (INV) {
#pragma unroll
            for (int u = 0; u < PT_PER; u++) rk[u] = (rank && sd[u] >= 0) ? rank[it[u]] : it[u];   // the four look-ups together
        }
#pragma unroll
        for (int u = 0; u < PT_PER; u++)
            if (sd[u] >= 0) {
                const int dst = sd[u] ? (n0 + run1 + r1) : (run0 + (rv - r1));
                dst_img[dst] = it[u];
                if constexpr (INV) inv[(int64_t)t.tree * n_items + rk[u]] = t.start + dst;
                r1 += sd[u];
                rv += 1;
            }
        run1 += total & 0xffff;
        run0 += (total >> 16) - (total & 0xffff);
        __syncthreads();
    }
}

// ---- the streaming form of the partition (the default; MORNA_PARTITION_FORM=0: partition_kernel above) -------------
// Same result -- a stable partition has one -- by wide, aligned accesses: a thread takes PS_PER = 16 consecutive
// positions (its sides are two aligned 16-byte loads and a byte shift, its items four dwordx4), the chunk's items are
// compacted through LDS in their final order, the left block then the right block, and go out so that consecutive lanes
// store consecutive 16-byte groups, scalar only at a block's unaligned head and tail.  A chunk is PS_CHUNK positions
// (one round of a 256-thread workgroup) and starts where the node's items are 16-byte aligned in their image: chunk k
// of a node holds the positions [k PS_CHUNK - m, (k + 1) PS_CHUNK - m) that exist, m = (element index of the node's
// first item) & 3.  One workgroup per node walks its chunks one after the other (gridDim.y == 1), or, where nodes
// span several chunks, one workgroup per chunk (CHUNKS): the right-side counts of the chunks come from
// partition_count_kernel, and a workgroup sums those in front of its own.
#define PS_THREADS 256
#define PS_WAVES (PS_THREADS / WAVE)
#define PS_PER 16
#define PS_CHUNK (PS_THREADS * PS_PER)

__host__ __device__ inline int part_chunks(int count, int m) { return (count + m + PS_CHUNK - 1) / PS_CHUNK; }

// 16 side bytes at the 16-byte aligned offset o, zeros for what lies outside the array
__device__ inline uint4 side_quad(const uint8_t *__restrict__ side, int64_t o, int64_t total)
{
    if (o >= 0 && o + 16 <= total) return *(const uint4 *)(side + o);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int64_t a = o + j;
        if (a >= 0 && a < total) w[j >> 2] |= (uint32_t)side[a] << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// The sides of the positions [p0, p0 + 16) of the node whose side bytes start at sbase, of which [vlo, vhi) exist: four
// words of 0 / 1 bytes, zero where no position is.  The byte offset of p0 has any alignment, the same (mod 16) for every
// thread of the workgroup: the selects below are uniform.
__device__ inline void part_sides(const uint8_t *__restrict__ side, int64_t side_total, int64_t sbase, int p0, int vlo, int vhi,
                                  uint32_t s[4])
{
    s[0] = s[1] = s[2] = s[3] = 0u;
    if (vlo >= vhi) return;
    const int64_t b = sbase + p0, o = b & ~(int64_t)15;
    const int a = (int)(b - o), q = a >> 2, r = a & 3;
    const uint4 lo = side_quad(side, o, side_total);
    const uint4 hi = a ? side_quad(side, o + 16, side_total) : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t v[5];
#pragma unroll
    for (int j = 0; j < 5; j++) v[j] = q == 0 ? w[j] : q == 1 ? w[j + 1] : q == 2 ? w[j + 2] : w[j + 3];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int l = vlo - 4 * j < 0 ? 0 : vlo - 4 * j, h = vhi - 4 * j > 4 ? 4 : vhi - 4 * j;   // bytes [l, h) of word j exist
        const uint32_t m = h > l ? (0xffffffffu >> (8 * (4 - h))) & (0xffffffffu << (8 * l)) : 0u;
        s[j] = __builtin_amdgcn_alignbyte(v[j + 1], v[j], (uint32_t)r) & m & 0x01010101u;
    }
}

// right-side count of every chunk but a node's last (nobody sums that one), cc[task * stride + chunk]; grid (tasks, stride).
// Its first workgroups post the level's counts to the host, as post_counts_kernel does where this kernel does not run.
__global__ __launch_bounds__(PS_THREADS) void partition_count_kernel(const SplitTask *__restrict__ tasks, int32_t n_tasks, int64_t n_items,
                                                                     const uint8_t *__restrict__ side, int64_t side_total,
                                                                     const int32_t *__restrict__ ones, int32_t *__restrict__ cc,
                                                                     unsigned long long *__restrict__ host_counts, uint32_t epoch)
{
    __shared__ int s_w[PS_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t post = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * PS_THREADS + tid;   // the first workgroups dispatched
    if (post < n_tasks)
        __hip_atomic_store(&host_counts[post], ((unsigned long long)epoch << 32) | (unsigned int)ones[post], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    const SplitTask t = tasks[blockIdx.x];
    const int m = (int)(TASK_ITEMS_AT(t, n_items) & 3), k = blockIdx.y;
    if (k + 1 >= part_chunks(t.count, m)) return;   // uniform
    const int p0 = k * PS_CHUNK - m + tid * PS_PER;
    const int vlo = p0 < 0 ? -p0 : 0, vhi = t.count - p0 < PS_PER ? t.count - p0 : PS_PER;
    uint32_t s[4];
    part_sides(side, side_total, (int64_t)t.tree * n_items + t.start, p0, vlo, vhi, s);
    int c = __builtin_popcount(s[0]) + __builtin_popcount(s[1]) + __builtin_popcount(s[2]) + __builtin_popcount(s[3]);
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, WAVE);
    if (lane == 0) s_w[w] = c;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
#pragma unroll
        for (int i = 0; i < PS_WAVES; i++) sum += s_w[i];
        cc[(int64_t)blockIdx.x * gridDim.y + k] = sum;
    }
}

// one block of a chunk, `len` items in LDS, to perm[d0, d0 + len): 16-byte stores where a whole aligned group is the block's
__device__ inline void part_store_block(int32_t *__restrict__ perm, int64_t d0, int len, const int32_t *ls, int tid)
{
    const int64_t q0 = d0 >> 2, q1 = (d0 + len + 3) >> 2;
    for (int64_t q = q0 + tid; q < q1; q += PS_THREADS) {
        const int64_t e = q * 4;
        const int off = (int)(e - d0);
        if (off >= 0 && off + 4 <= len) {
            *(int4 *)(perm + e) = make_int4(ls[off], ls[off + 1], ls[off + 2], ls[off + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (off + j >= 0 && off + j < len) perm[e + j] = ls[off + j];
        }
    }
}

// grid (tasks, CHUNKS ? most chunks of a node : 1)
template <bool CHUNKS>
__global__ __launch_bounds__(PS_THREADS) void partition_stream_kernel(const SplitTask *__restrict__ tasks, int64_t n_items,
                                                                      const uint8_t *__restrict__ side, int64_t side_total,
                                                                      const int32_t *__restrict__ ones,
                                                                      int32_t *__restrict__ perm /* work buffer [tree][2][n_items] */,
                                                                      int64_t perm_total, const int32_t *__restrict__ cc)
{
    __shared__ int32_t s_items[PS_CHUNK];
    __shared__ int s_w[PS_WAVES], s_c[PS_WAVES];
    const SplitTask t = tasks[blockIdx.x];
    const int n1 = ones[blockIdx.x], n0 = t.count - n1;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t gsrc = TASK_ITEMS_AT(t, n_items);
    const int64_t gdst = ((int64_t)t.tree * 2 + ((t.level + 1) & 1)) * n_items + t.start;
    const int64_t sbase = (int64_t)t.tree * n_items + t.start;
    const int m = (int)(gsrc & 3), nchunks = part_chunks(t.count, m);
    if ((int)blockIdx.y >= nchunks) return;   // uniform
    int run1 = 0;                             // right-side items of the chunks before (one workgroup per node)
    for (int k = blockIdx.y; k < nchunks; k += gridDim.y) {
        // the chunk's sides and items are asked for before the counts are looked at: their addresses need the task alone
        const int p0 = k * PS_CHUNK - m + tid * PS_PER;
        const int vlo = p0 < 0 ? -p0 : 0, vhi = t.count - p0 < PS_PER ? t.count - p0 : PS_PER;
        uint32_t s[4];
        part_sides(side, side_total, sbase, p0, vlo, vhi, s);
        int it[PS_PER];
        const int64_t e0 = gsrc + p0;   // a multiple of 4, never below 0
#pragma unroll
        for (int j = 0; j < PS_PER / 4; j++) {
            int4 v = make_int4(0, 0, 0, 0);
            if (4 * j + 4 > vlo && 4 * j < vhi) {
                const int64_t e = e0 + 4 * j;
                if (e + 4 <= perm_total) v = *(const int4 *)(perm + e);
                else {
                    v.x = perm[e];   // e itself exists: the group holds an item of the node
                    if (e + 1 < perm_total) v.y = perm[e + 1];
                    if (e + 2 < perm_total) v.z = perm[e + 2];
                }
            }
            it[4 * j] = v.x, it[4 * j + 1] = v.y, it[4 * j + 2] = v.z, it[4 * j + 3] = v.w;
        }
        // the right-side counts of the chunks in front of this one (asked for with the rest), beside the scan's wave totals
        int c = 0;
        if constexpr (CHUNKS)
            for (int j = tid; j < k; j += PS_THREADS) c += cc[(int64_t)blockIdx.x * gridDim.y + j];
        if (k == (int)blockIdx.y && !sides_stand(t.attempt, n0, n1)) return;   // uniform; nothing has been stored
        if constexpr (CHUNKS) {
#pragma unroll
            for (int o = WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, WAVE);
        }
        // right-side and existing positions of a thread packed into one integer (16 bits each: a chunk has 4096 positions)
        const int c1 = __builtin_popcount(s[0]) + __builtin_popcount(s[1]) + __builtin_popcount(s[2]) + __builtin_popcount(s[3]);
        const int pk = ((vhi > vlo ? vhi - vlo : 0) << 16) | c1;
        int incl = pk;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int v = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += v;
        }
        if (lane == WAVE - 1) s_w[w] = incl;
        if (CHUNKS && lane == 0) s_c[w] = c;
        __syncthreads();
        int before = 0, total = 0, before1 = run1;
#pragma unroll
        for (int i = 0; i < PS_WAVES; i++) {
            if (i < w) before += s_w[i];
            total += s_w[i];
            if constexpr (CHUNKS) before1 += s_c[i];
        }
        const int excl = incl - pk + before;
        int r1 = excl & 0xffff, rv = excl >> 16;   // right-side / existing positions of the chunk before this thread's first
        const int R = total & 0xffff, L = (total >> 16) - R;
        const int before0 = (k * PS_CHUNK - m > 0 ? k * PS_CHUNK - m : 0) - before1;
#pragma unroll
        for (int u = 0; u < PS_PER; u++)
            if (u >= vlo && u < vhi) {
                const int sd = (int)((s[u >> 2] >> (8 * (u & 3))) & 1u);
                s_items[sd ? L + r1 : rv - r1] = it[u];
                r1 += sd;
                rv += 1;
            }
        __syncthreads();
        part_store_block(perm, gdst + before0, L, s_items, tid);
        part_store_block(perm, gdst + n0 + before1, R, s_items + L, tid);
        run1 += R;
        if (k + (int)gridDim.y < nchunks) __syncthreads();   // the next chunk reuses the LDS
    }
}

// roots: image 0 of every tree = the identity
__global__ void iota_perm_kernel(int32_t *perm /* work buffer [tree][2][n_items] */, int32_t *inv, int64_t n_items, int64_t total)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const int64_t t = i / n_items, r = i - t * n_items;
        perm[t * 2 * n_items + r] = (int32_t)r;
        if (inv) inv[i] = (int32_t)r;
    }
}

// the finished forest's leaves, out of the image of their depth into the permutation the searches read: one workgroup per leaf
__global__ __launch_bounds__(256) void gather_leaves_kernel(const LeafSeg *__restrict__ leaves, const int32_t *__restrict__ work,
                                                            int64_t n_items, int32_t *__restrict__ perm)
{
    const LeafSeg l = leaves[blockIdx.x];
    const int32_t *src = work + ((int64_t)l.tree * 2 + (l.level & 1)) * n_items + l.start;
    int32_t *dst = perm + (int64_t)l.tree * n_items + l.start;
    for (int i = threadIdx.x; i < l.count; i += 256) dst[i] = src[i];
}

// -------------------------------------------------------------- host driver

#include "forest_host.hpp"

}  // namespace morna
