// knn.hip -- batched nearest-neighbour queries on gfx950.
//
// query_*_kernel : annoy's _get_all_nns (get_nns_by_vector / get_nns_by_item,
//                  reference call sites morna.py:651, 659, 762, 769) -- the
//                  best-first forest traversal, the brute-force angular refine
//                  of the candidate rows and the (distance, id) top-k selection.
//                  The host side (query_batch, "the approximate search, host
//                  side" below) runs in stages, and per batch of queries launches
//                    stage     the queries' vectors or item ids (copies only)
//                    traverse  spread form (under 64 queries): query_roots_kernel,
//                              query_descend_kernel; else root margins by query
//                              groups and one-wave descents: query_roots_batch_kernel,
//                              query_descend_kernel; or fused: query_traverse_kernel
//                              (a restricted call: the *_restricted_kernel forms)
//                    filter    beside the traversal, for a dense batch: the fp16
//                              image of the queries (splitmm.hip) and the whole-batch
//                              contraction, query_scores_big_kernel + query_scores_kernel
//                              -- for the first batch after build() already beside
//                              the build's tail (EarlyContraction)
//                    refine    spread form: query_cand_dots_kernel, query_topk_kernel;
//                              else query_refine_kernel<0 none / 1 gather / 2 dense>
//                    deliver   one copy of the result block (pack_topk_kernel for
//                              the row-sharded search)
//                  search_sweep has the same stages for a grid of (tree count,
//                  search_k) cells: query_roots[_batch]_kernel, query_descend_sweep_kernel,
//                  [query_scores_kernel, sweep_bounds_kernel, sweep_threshold_kernel,]
//                  sweep_cand_dots_kernel, sweep_topk_kernel, [sweep_hits_kernel].
// merge_topk_kernel : the row-sharded search's merge of the shards' top-k lists.
// The exact search, the label sums and the radius search are in exact.hip; what both files use, in search_common.hpp.
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "common.hpp"
#include "devutil.hpp"
#include "mm16.hpp"
#include "search_common.hpp"

namespace morna {

#define Q_LDS_MAX (152 * 1024)      // dynamic LDS a query kernel may ask for: 160 KiB less its static arrays

struct QueryParams {
    const float *X;
    const float *norm2;
    int64_t n_items;
    int32_t dpad, n_trees, K;
    const int32_t *node_rec;   // [n_nodes][4] child0, child1, start, count
    const int32_t *node_tree;
    const int32_t *node_hp;
    const float *hp;
    const int32_t *perm;
    int64_t n_nodes;
    const float *Q;            // [nq][dpad] or null
    const int32_t *items;      // [nq] or null
    int32_t n_inline;          // spread form, by item, up to 16 queries: the item numbers travel with the launch (no copy)
    int32_t inline_items[16];
    int32_t k, search_k;
    int32_t cap;               // candidate capacity per query
    int32_t bm_words;
    // workspace, one slice per query
    uint64_t *pq;              // [nq][n_nodes]
    int32_t *cand;             // [nq][cap]
    int64_t *cand_off;         // [nq] one-wave descent: >= 0: the candidates are perm[cand_off .. + ncand) (one leaf, not copied); -1: cand[]
    int32_t zero_copy;         // the consumer reads the candidates through cand_off (query_cand_dots_kernel); 0: always copied to cand[]
    uint64_t *keys;            // [nq][cap]
    float *low;                // [nq][cap] lower bound of a candidate's distance (filter modes)
    int32_t *ncand;            // [nq] unique candidates found by the traversal (may exceed cap)
    float *qpp;                // [nq] canonical dot(q, q)
    uint32_t *bm_global;       // [nq][bm_words] when the bitmap does not fit LDS
    int32_t *ids_out;          // [nq][k]
    float *dist_out;           // [nq][k]
    int32_t *count_out;        // [nq]
    unsigned long long *stat;  // rows read: hyperplane dots + unique candidates + query
    // Candidate filter on the fp16 image of the rows (splitmm.hip); X16 null: every candidate gets the fp32 dot.
    // scores null: the refine kernel takes the filter dots itself, row by row (fp16 row x fp32 query), and every
    // filter distance is within `delta` of the canonical one.  scores set: they were taken for ALL rows at once on
    // the matrix cores (query_scores_kernel) from the fp16 images of rows AND queries; the bound is then per pair,
    // from the measured norms and rounding-error norms of the two images.
    const _Float16 *X16;       // [n_items][dpad], row r scaled by 2^e(r)
    const float *xscale;       // [n_items] 2^-e(r); 0: the row has no fp16 image
    const float *xn16, *xe16;  // [n_items] upper bounds of |y_r| and |2^e x_r - y_r|
    float delta;
    const float *scores;       // [nq][n_items]  sum_i y_r[i] g_q[i]
    const float *qscale, *qn16, *qe16;   // per query image: indexed by the item id (by-item) or the query number
    float eacc;       // bound of the fp32 accumulation of a filter dot: two chains (128 x 128 form) ...
    float eacc_big;   // ... one chain: the rows below big_rows went through the 256 x 256 form
    int64_t big_rows;
    // MORNA_DEBUG_OPEN=1 only (else null): query_refine_kernel<2> adds (candidates << 32) + survivors of every query to it
    unsigned long long *refine_stat;
};

// A sweep over (tree count, search_k) cells from one forest (include/morna_hip.h, "search sweep").  Only the *_sweep_kernel
// forms take it.  A launch's "virtual query" v = i * nq + q is query q of the batch walked over the first trees[i] trees.
#define SWEEP_MAX_LIST 64
struct SweepArgs {
    int32_t n_t, n_s, nq;                  // tree counts, search_k values, queries of the batch
    int32_t trees[SWEEP_MAX_LIST];         // strictly ascending, the last at most the forest's
    int32_t search_ks[SWEEP_MAX_LIST];     // strictly ascending
    const uint64_t *root_pq;               // [nq][n_nodes] the root margins of every query at trees[n_t - 1], read only
    int32_t *cell_ncand, *cell_ndots;      // [n_t][n_s][nq] unique candidates / hyperplane dots when nn first reached search_ks[j]
};

__device__ inline uint64_t pq_key(float d, int32_t node)
{
    return ((uint64_t)f32_orderable(d) << 32) | (uint32_t)node;
}

// the query's row (spread kernels): a stored row -- its number from the launch arguments or from the items array -- or a
// row of the staged query vectors
__device__ inline const float4 *query_row(const QueryParams &P, int64_t qi)
{
    if (P.n_inline) return (const float4 *)(P.X + (int64_t)P.inline_items[qi] * P.dpad);
    return P.items ? (const float4 *)(P.X + (int64_t)P.items[qi] * P.dpad) : (const float4 *)(P.Q + qi * P.dpad);
}

// k-th smallest of n distinct keys (~0 when n < k), the same value in every thread.  While a thread's share of the keys
// fits KTH_HELD registers and k <= KTH_MAX_K: every wave extracts the k smallest of ITS keys in k rounds of register compares
// and a wave minimum -- no barrier -- and the k-th smallest of the waves' k-lists is found by counting, one key per lane.
// Otherwise (and as round 1 did throughout): k rounds of a block-wide minimum over the keys in memory, two barriers each.
#define KTH_HELD 16
#define KTH_MAX_K 32
__device__ inline uint64_t block_kth_smallest(const uint64_t *keys, int n, int k, int tid, uint64_t *s_red, uint64_t *s_top)
{
    const int lane = tid & (WAVE - 1), w = tid / WAVE;
    if (n <= Q_THREADS * KTH_HELD && k <= KTH_MAX_K) {
        uint64_t held[KTH_HELD];
#pragma unroll
        for (int u = 0; u < KTH_HELD; u++) held[u] = tid + Q_THREADS * u < n ? keys[tid + Q_THREADS * u] : ~0ull;
        uint64_t prev = 0;
        for (int r = 0; r < k; r++) {
            uint64_t best = ~0ull;
#pragma unroll
            for (int u = 0; u < KTH_HELD; u++)
                if ((r == 0 || held[u] > prev) && held[u] < best) best = held[u];
            prev = wave_min_u64(best);
            if (lane == 0) s_top[w * KTH_MAX_K + r] = prev;   // ~0: this wave has run out of keys
        }
        __syncthreads();
        // Q_WAVES * k keys, k-th smallest: a key's rank is the number of keys below it (the real ones are distinct)
        uint64_t found = ~0ull;
        for (int i = tid; i < Q_WAVES * k; i += Q_THREADS) {
            const uint64_t v = s_top[(i / k) * KTH_MAX_K + i % k];
            int below = 0;
            for (int j = 0; j < Q_WAVES * k; j++) below += s_top[(j / k) * KTH_MAX_K + j % k] < v ? 1 : 0;
            if (v != ~0ull && below == k - 1) found = v;
        }
        return block_min_u64(found, s_red, tid);
    }
    uint64_t kth = 0;
    for (int r = 0; r < k; r++) {
        uint64_t best = ~0ull;
        for (int c = tid; c < n; c += Q_THREADS) {
            const uint64_t kk = keys[c];
            if ((r == 0 || kk > kth) && kk < best) best = kk;
        }
        kth = block_min_u64(best, s_red, tid);
    }
    return kth;
}

// A canonical dot with the query held in the wave's registers: the whole row is requested at once, all its 1-KiB pieces in
// flight together (through wave_dot(), four loads in flight, a lone wave moves a 12-KB hyperplane in ~2 us).  NV = float4
// per lane of a row (dpad / 256).  The same fmaf chains as wave_dot().
template <int NV>
__device__ inline float wave_dot_held(const float4 *__restrict__ row, const float4 (&qr)[NV > 0 ? NV : 1], int lane)
{
    float4 x[NV > 0 ? NV : 1];
#pragma unroll
    for (int k = 0; k < NV; k++) x[k] = row[lane + WAVE * k];
    Acc4 s = acc4_zero();
#pragma unroll
    for (int k = 0; k < NV; k++) fma4(s, x[k], qr[k]);
    return acc4_finish(s);
}

// ---- traversal: annoy's _get_all_nns up to the candidate set (oracle/annoy_oracle.c:453-504) -------------------
// One workgroup per query: all root margins (every wave takes trees), then the best-first descent by wave 0 (array
// priority queue, bitmap de-duplication of the leaves' ids).  Leaves the unique candidates in cand[].
// RST: the restricted form -- the same pops and the same nn accounting, but the bitmap starts as the complement of the
// allow-list (an item that is not allowed counts as seen already) and a leaf's ids of the query's own group are passed over.
template <bool BM_LDS, bool RST>
__device__ __forceinline__ void query_traverse_body(const QueryParams &P, const RestrictArgs &R)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *qv = (float4 *)smem;
    uint32_t *bm = BM_LDS ? (uint32_t *)(smem + (size_t)P.dpad * sizeof(float))
                          : P.bm_global + (size_t)blockIdx.x * P.bm_words;
    __shared__ int s_ncand;

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t qi = blockIdx.x;
    const int nvec = P.dpad / 4;
    const int T = P.n_trees;

    const float4 *src = P.items ? (const float4 *)(P.X + (int64_t)P.items[qi] * P.dpad)
                                : (const float4 *)(P.Q + qi * P.dpad);
    for (int i = tid; i < nvec; i += Q_THREADS) qv[i] = src[i];
    if constexpr (RST) {
        for (int i = tid; i < P.bm_words; i += Q_THREADS) bm[i] = R.deny[i];
    } else {
        for (int i = tid; i < P.bm_words; i += Q_THREADS) bm[i] = 0u;
    }
    if (tid == 0) s_ncand = 0;
    __syncthreads();
    int32_t gq = -1;
    if constexpr (RST) gq = restrict_query_group(R, qi);

    uint64_t *pq = P.pq + qi * P.n_nodes;
    int32_t *cand = P.cand + qi * P.cap;
    const bool roots_split = P.n_items > P.K;   // every root is a split node (count = N > K)

    // ---- phase 1: the roots all sit at +inf and are expanded before anything else;
    //      their margins are independent, so every wave takes a share.
    if (w == Q_WAVES - 1) {
        float pp = wave_dot(qv, qv, nvec, lane);
        if (lane == 0) P.qpp[qi] = pp;
    }
    if (roots_split) {
        for (int t = w; t < T; t += Q_WAVES) {
            const float m = wave_dot((const float4 *)(P.hp + (int64_t)P.node_hp[t] * P.dpad), qv, nvec, lane);
            // slot s is only ever touched by lane s % 64 of wave 0 later on; written here once
            if (lane == 0) {
                pq[2 * t] = pq_key(m, P.node_rec[4 * t + 1]);       // min(+inf, margin), children[1]
                pq[2 * t + 1] = pq_key(-m, P.node_rec[4 * t + 0]);  // min(+inf, -margin), children[0]
            }
        }
    } else {
        for (int t = tid; t < T; t += Q_THREADS) pq[t] = pq_key(INFINITY, t);
    }
    __syncthreads();

    // ---- phase 2: best-first traversal by wave 0 (max-heap semantics on (bound, node id));
    //      the queue is an unsorted array scanned by the wave, popped slots are zeroed.
    if (w == 0) {
        int ndots = roots_split ? T : 0;
        int hn = roots_split ? 2 * T : T;
        int64_t nn = 0;
        const int64_t search_k = P.search_k;
        while (nn < search_k) {
            uint64_t best = 0;
            int bestpos = -1;
            for (int i = lane; i < hn; i += WAVE) {
                uint64_t kk = pq[i];
                if (kk > best) { best = kk; bestpos = i; }
            }
            const uint64_t top = wave_max_u64(best);
            if (top == 0) break;                       // queue empty
            if (best == top && bestpos >= 0) pq[bestpos] = 0;   // exactly one lane owns it
            const int32_t node = (int32_t)(uint32_t)top;
            const float d = f32_from_orderable((uint32_t)(top >> 32));
            const int32_t c0 = P.node_rec[4 * node + 0], c1 = P.node_rec[4 * node + 1];
            const int32_t start = P.node_rec[4 * node + 2], count = P.node_rec[4 * node + 3];
            if (c0 < 0) {
                // leaf: nns.insert(all ids); duplicates across trees are dropped by the bitmap
                const int32_t *src_ids = P.perm + (int64_t)P.node_tree[node] * P.n_items + start;
                for (int i = lane; i < count; i += WAVE) {
                    const int32_t id = src_ids[i];
                    if constexpr (RST) {
                        if (gq >= 0 && R.group[id] == gq) continue;
                    }
                    const uint32_t bit = 1u << (id & 31);
                    const uint32_t old = atomicOr(&bm[id >> 5], bit);
                    if (!(old & bit)) {
                        const int slot = atomicAdd(&s_ncand, 1);
                        if (slot < P.cap) cand[slot] = id;
                    }
                }
                nn += count;
            } else {
                const float m = wave_dot((const float4 *)(P.hp + (int64_t)P.node_hp[node] * P.dpad), qv, nvec, lane);
                if (lane == (hn & (WAVE - 1))) pq[hn] = pq_key(d < m ? d : m, c1);
                if (lane == ((hn + 1) & (WAVE - 1))) pq[hn + 1] = pq_key(d < -m ? d : -m, c0);
                hn += 2;
                ndots++;
            }
        }
        if (lane == 0) {   // (LDS operations of a wave complete in order: the count includes the last leaf's atomics)
            const int nc = s_ncand;
            P.ncand[qi] = nc;
            atomicAdd(P.stat, (unsigned long long)(ndots + (nc < P.cap ? nc : P.cap) + 1));
        }
    }
}

template <bool BM_LDS>
__global__ __launch_bounds__(Q_THREADS) void query_traverse_kernel(QueryParams P)
{
    query_traverse_body<BM_LDS, false>(P, RestrictArgs());
}

template <bool BM_LDS>
__global__ __launch_bounds__(Q_THREADS) void query_traverse_restricted_kernel(QueryParams P, RestrictArgs R)
{
    query_traverse_body<BM_LDS, true>(P, R);
}

// ---- small batches: ONE query spread over the chip ----------------------------------------------------------------
// The reference answers one query per process (morna.py:1345-1484 -> 651-665 / 762-774).  With one workgroup per query
// (above) a lone query has one CU of 256: its ~200 root margins and the ~2000 candidate rows of its leaf are read by four
// waves, 0.78 ms at C3 against 2 us for the bytes at the HBM rate.  For batches too small to fill the chip the same
// arithmetic is dealt out: (A) a wave per (query, tree) for the root margins, (B) one wave per query for the best-first
// descent -- a chain of dependent pops, each a node record, a hyperplane and one canonical dot --, (C) a wave per two
// candidates for the CANONICAL fp32 dot of every candidate (no fp16 filter: twice the bytes of the filter, but one
// dependent stage less: no k-th smallest bound, no compaction, no second gather), (D) the k smallest (distance, id) of
// the keys by one workgroup.  Same operations on the same values as the batch forms: identical answers.
__global__ __launch_bounds__(Q_THREADS) void query_roots_kernel(QueryParams P)
{
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t qi = blockIdx.y;
    const int nvec = P.dpad / 4;
    const float4 *q = query_row(P, qi);
    if (blockIdx.x == 0 && w == Q_WAVES - 1) {
        const float pp = wave_dot(q, q, nvec, lane);
        if (lane == 0) P.qpp[qi] = pp;
    }
    const int t = blockIdx.x * Q_WAVES + w;
    if (t >= P.n_trees || !(P.n_items > P.K)) return;   // (roots that are leaves: the descent seeds the queue itself)
    uint64_t *pq = P.pq + qi * P.n_nodes;
    const float m = wave_dot((const float4 *)(P.hp + (int64_t)P.node_hp[t] * P.dpad), q, nvec, lane);
    if (lane == 0) {
        pq[2 * t] = pq_key(m, P.node_rec[4 * t + 1]);       // min(+inf, margin), children[1]
        pq[2 * t + 1] = pq_key(-m, P.node_rec[4 * t + 0]);  // min(+inf, -margin), children[0]
    }
}

// Root margins of a BATCH: a workgroup takes QR_Q queries (their rows in LDS) and a share of the trees; a wave fetches a
// root's hyperplane ONCE into registers, all its pieces in flight, and takes its canonical dot with each of the QR_Q queries
// (one workgroup per query fetched every hyperplane once per query: 200 k dots x 12 KB out of L2 for 1000 queries, and a
// wave's 50 dots one after the other, 100 us of a workgroup's life).  The descent then runs as in the spread form, one wave
// per query (query_descend_kernel).  Same fmaf chains as wave_dot(): a product's factors commute.
#ifndef QR_Q
#define QR_Q 4         // (8 queries and / or 512 threads, 2 queries: the same time within 2 % at 50k and at 6250 rows)
#endif
#ifndef QR_THREADS
#define QR_THREADS 256
#endif
#define QR_WAVES (QR_THREADS / WAVE)
#define QR_TREES 48   // trees per workgroup
template <int NV>
__global__ __launch_bounds__(QR_THREADS) void query_roots_batch_kernel(QueryParams P, int32_t nq)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *qs = (float4 *)smem;   // [QR_Q][nvec]
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int nvec = P.dpad / 4;
    const int64_t q0 = (int64_t)blockIdx.x * QR_Q;
    const int nqs = (int)(nq - q0 < QR_Q ? nq - q0 : QR_Q);
    for (int i = tid; i < QR_Q * nvec; i += QR_THREADS) {
        const int qq = i / nvec, v = i - qq * nvec;
        qs[i] = qq < nqs ? query_row(P, q0 + qq)[v] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    if (blockIdx.y == 0)   // the queries' own canonical norms, once
        for (int qq = w; qq < nqs; qq += QR_WAVES) {
            const float pp = wave_dot(qs + qq * nvec, qs + qq * nvec, nvec, lane);
            if (lane == 0) P.qpp[q0 + qq] = pp;
        }
    const int t_end = (int)(blockIdx.y + 1) * QR_TREES < P.n_trees ? (int)(blockIdx.y + 1) * QR_TREES : P.n_trees;
    for (int t = (int)blockIdx.y * QR_TREES + w; t < t_end; t += QR_WAVES) {
        const float4 *hrow = (const float4 *)(P.hp + (int64_t)P.node_hp[t] * P.dpad);
        const int32_t c0 = P.node_rec[4 * t + 0], c1 = P.node_rec[4 * t + 1];
        float4 hr[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) hr[k] = hrow[lane + WAVE * k];
#pragma unroll
        for (int qq = 0; qq < QR_Q; qq++) {
            if (qq < nqs) {   // uniform
                Acc4 s4 = acc4_zero();
#pragma unroll
                for (int k = 0; k < NV; k++) fma4(s4, hr[k], qs[qq * nvec + lane + WAVE * k]);
                const float m = acc4_finish(s4);
                if (lane == 0) {
                    uint64_t *pq = P.pq + (q0 + qq) * P.n_nodes;
                    pq[2 * t] = pq_key(m, c1);        // min(+inf, margin), children[1]
                    pq[2 * t + 1] = pq_key(-m, c0);   // min(+inf, -margin), children[0]
                }
            }
        }
    }
}

#define PQ_LDS 1024   // queue entries kept in LDS by the one-wave descent; entries beyond stay in the global array
// One wave per query.  A pop is a chain -- the entry with the largest bound, its node's record and hyperplane, one dot, two
// pushes -- and the descent is a chain of pops (C3 at morna's defaults: 14 internal nodes and one leaf; annoy's queue hops
// between the trees), so what counts is the length of ONE pop.  A lone wave issues an instruction every ~4.3 cycles and a
// trip to HBM takes ~1000, so:
//   * the queue sits in LDS, bounds and nodes as two 32-bit arrays: the maximum is taken on the 32-bit bounds (8 x v_max +
//     a 6-step cross-lane maximum); only when two entries share the largest bound do the 64-bit keys decide (annoy's
//     (bound, node) order), by the slow scan;
//   * the record and the hyperplane of a popped node are requested together (the hyperplane slot of every entry sits beside
//     it: looked up when the node is PUSHED, under its parent's hyperplane fetch): one round trip per pop; the query stays in
//     registers (NV > 0) and a hyperplane's 1-KiB pieces are all requested at once;
//   * (tried: the margins, records and child slots of the roots' children -- most of the pops -- made ahead by the root-margin
//     kernel, so that those pops touch LDS only: the descent 22 -> 18 us, the root kernel 4.9 -> 7.3 us with three times the
//     dots, the launch no shorter; dropped)
//   * the first leaf, when it ends the search (search_k = 100, leaves of ~K ids), is not copied: its slice of the tree's
//     permutation IS the candidate list (distinct ids: a tree lists an item once).
// NV: float4 per lane of a row (dpad / 256) when the query fits the wave's registers; 0: any row length, through
// wave_dot().  Same fmaf chains either way.
// the wave's maximum of a 32-bit value (0 = nothing), every lane gets it: cross-lane moves only
__device__ inline uint32_t wave_max_u32_fast(uint32_t v)
{
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    u32x2 r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    v = v > r[1] ? v : r[1];
    r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = v > r[1] ? v : r[1];
    uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x108, 0xf, 0xf, true);
    v = v > o ? v : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xf, 0xf, true);
    v = v > o ? v : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x102, 0xf, 0xf, true);
    v = v > o ? v : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true);
    v = v > o ? v : o;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// RST: the restricted form, as in query_traverse_body; the group test sits in the leaf branch only (the pops' chain does
// not see it), and the first leaf is always copied: its slice of the permutation is not filtered.
// SWP: the sweep form.  Block v is a virtual query (SweepArgs): the queue is seeded from the first 2 * trees[i] entries of
// the query's root margins (made once, for the largest tree count: tree t's entries do not depend on the trees behind it),
// the queue overflow, bitmap and candidates are the block's own, the descent runs to the LARGEST search_k, and whenever a
// leaf pop carries nn past search_ks[j] -- the moment the search with that search_k would have stopped -- the candidates
// and hyperplane dots so far are recorded for cell (i, j).  The first leaf is always copied.
template <bool BM_LDS, int NV, bool RST, bool SWP = false>
__device__ __forceinline__ void query_descend_body(const QueryParams &P, const RestrictArgs &R, const SweepArgs *S = nullptr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // a queue entry = (bound as an orderable 32-bit word, node); an empty slot has bound word 0 (no real bound maps to 0:
    // f32_orderable() of a non-NaN float is >= 0x00800000 ... and the words of the negative floats are the complements)
    __shared__ uint32_t s_bound[PQ_LDS];
    __shared__ int32_t s_node[PQ_LDS];
    __shared__ int32_t s_slot[PQ_LDS];    // hyperplane slot of the entry's node, -1: a leaf
    __shared__ int s_ncand;
    const int lane = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const int nvec = P.dpad / 4;
    int T = P.n_trees;
    int64_t qsrc = qi;          // the query whose row this block reads
    int ti = 0, jrec = 0;       // sweep: the tree count's number, the search_k values recorded so far
    if constexpr (SWP) {
        ti = (int)(qi / S->nq);
        qsrc = qi - (int64_t)ti * S->nq;
        T = S->trees[ti];
    }
    uint32_t *bm = BM_LDS ? (uint32_t *)smem : P.bm_global + (size_t)qi * P.bm_words;
    const float4 *q = query_row(P, qsrc);
    uint64_t *gpq = P.pq + qi * P.n_nodes;
    const uint64_t *rpq = gpq;  // where the root margins are
    if constexpr (SWP) rpq = S->root_pq + qsrc * P.n_nodes;
    int32_t *cand = P.cand + qi * P.cap;
    const bool roots_split = P.n_items > P.K;
    int hn = roots_split ? 2 * T : T;
#ifdef MORNA_DESCEND_PROBE
    long long tp[40];
    int ntp = 0;
#define TP() do { if (ntp < 40) tp[ntp++] = clock64(); } while (0)
#else
#define TP() do { } while (0)
#endif
    TP();
    float4 qr[NV > 0 ? NV : 1];
#pragma unroll
    for (int k = 0; k < NV; k++) qr[k] = q[lane + WAVE * k];
    {
        // the queue as the root margins left it, and the hyperplane slot of every entry's node: all the loads of a phase in
        // flight together (written as one loop, every iteration waited for its two dependent round trips)
        auto init = [&](auto NU) {
            constexpr int nu = decltype(NU)::value;
            uint64_t k16[nu];
            int32_t s16[nu];
#pragma unroll
            for (int u = 0; u < nu; u++) {
                const int i = lane + WAVE * u;
                k16[u] = i < hn ? (roots_split ? rpq[i] : pq_key(INFINITY, i)) : 0;
            }
#pragma unroll
            for (int u = 0; u < nu; u++) s16[u] = lane + WAVE * u < hn ? P.node_hp[(int32_t)(uint32_t)k16[u]] : -1;
#pragma unroll
            for (int u = 0; u < nu; u++) {
                s_bound[lane + WAVE * u] = (uint32_t)(k16[u] >> 32);   // (0 beyond hn: an empty slot)
                s_node[lane + WAVE * u] = (int32_t)(uint32_t)k16[u];
                s_slot[lane + WAVE * u] = s16[u];
            }
        };
        if (hn <= 8 * WAVE) {
            init(std::integral_constant<int, 8>());
            for (int i = 8 * WAVE + lane; i < PQ_LDS; i += WAVE) s_bound[i] = 0;   // slots the pushes will fill
        } else {
            init(std::integral_constant<int, PQ_LDS / WAVE>());
        }
    }
    if (!roots_split)
        for (int i = PQ_LDS + lane; i < hn; i += WAVE) gpq[i] = pq_key(INFINITY, i);
    if constexpr (SWP) {
        if (roots_split)   // the root entries past the LDS arrays: into the block's own overflow
            for (int i = PQ_LDS + lane; i < hn; i += WAVE) gpq[i] = rpq[i];
    }
    auto record = [&](int ndots_now) {   // sweep: cell (ti, jrec) stops here
        if constexpr (SWP) {
            if (lane == 0) {   // (lane 0 made the counter updates itself: its read follows them)
                const int64_t cell = ((int64_t)ti * S->n_s + jrec) * S->nq + qsrc;
                S->cell_ncand[cell] = s_ncand;
                S->cell_ndots[cell] = ndots_now;
            }
        }
    };
    int32_t gq = -1;
    if constexpr (RST) {
        for (int i = lane; i < P.bm_words; i += WAVE) bm[i] = R.deny[i];
        gq = restrict_query_group(R, qi);
    } else {
        for (int i = lane; i < P.bm_words; i += WAVE) bm[i] = 0u;
    }
    if (lane == 0) s_ncand = 0;
    __syncthreads();   // (one wave: orders the LDS / global initialisation in front of the loop)
    int ndots = roots_split ? T : 0, n_leaves = 0;
    int64_t nn = 0, cand_off = -1;
    const int64_t search_k = P.search_k;
    TP();
    while (nn < search_k) {
        // ---- the entry with the largest (bound, node)
        int pos = -1;
        uint32_t top_b = 0;
        {
            const int hl = hn < PQ_LDS ? hn : PQ_LDS;
            auto pick = [&](auto NU) {
                constexpr int nu = decltype(NU)::value;
                uint32_t bb[nu], mb = 0;
#pragma unroll
                for (int u = 0; u < nu; u++) bb[u] = s_bound[lane + WAVE * u];   // (slots beyond hn hold 0)
#pragma unroll
                for (int u = 0; u < nu; u++) mb = bb[u] > mb ? bb[u] : mb;
                for (int i = PQ_LDS + lane; i < hn; i += WAVE) {   // (entries beyond the LDS arrays: global)
                    const uint32_t b = (uint32_t)(gpq[i] >> 32);
                    mb = b > mb ? b : mb;
                }
                top_b = wave_max_u32_fast(mb);
                if (top_b == 0) return;               // queue empty
                // who holds it?  One entry as a rule; several (equal bounds, e.g. both children behind a zero margin): annoy's
                // pair order pops the larger node id first
                int cnt = 0, mypos = -1;
#pragma unroll
                for (int u = 0; u < nu; u++)
                    if (bb[u] == top_b) { cnt++; mypos = lane + WAVE * u; }
                const unsigned long long holders = __ballot(cnt > 0);
                if (hn <= PQ_LDS && __popcll(holders) == 1 && __builtin_amdgcn_readlane(cnt, __ffsll((long long)holders) - 1) == 1) {
                    pos = __builtin_amdgcn_readlane(mypos, __ffsll((long long)holders) - 1);
                    return;
                }
                int32_t mynode = -1;                  // the slow way: the largest node among the holders
                mypos = -1;
                for (int i = lane; i < hn; i += WAVE) {
                    const bool il = i < PQ_LDS;
                    const uint32_t b = il ? s_bound[i] : (uint32_t)(gpq[i] >> 32);
                    if (b == top_b) {
                        const int32_t nd = il ? s_node[i] : (int32_t)(uint32_t)gpq[i];
                        if (nd > mynode) { mynode = nd; mypos = i; }
                    }
                }
                const uint32_t best_node = wave_max_u32_fast(mypos >= 0 ? (uint32_t)mynode + 1u : 0u) - 1u;   // node ids are >= 0
                const unsigned long long w2 = __ballot(mypos >= 0 && (uint32_t)mynode == best_node);
                pos = __builtin_amdgcn_readlane(mypos, __ffsll((long long)w2) - 1);
            };
            if (hl <= 8 * WAVE) pick(std::integral_constant<int, 8>());
            else pick(std::integral_constant<int, PQ_LDS / WAVE>());
            if (top_b == 0) break;
        }
        TP();
        const bool in_lds = pos < PQ_LDS;
        const int32_t node = in_lds ? s_node[pos] : (int32_t)(uint32_t)gpq[pos];
        const float d = f32_from_orderable(top_b);
        if (lane == 0) {
            if (in_lds) s_bound[pos] = 0;
            else gpq[pos] = 0;
        }
        const int32_t slot = in_lds ? s_slot[pos] : P.node_hp[node];
        if (slot < 0) {
            // leaf: nns.insert(all ids); duplicates across trees are dropped by the bitmap
            const int4 rec = *(const int4 *)(P.node_rec + 4 * (int64_t)node);
            const int32_t *src_ids = P.perm + (int64_t)P.node_tree[node] * P.n_items + rec.z;
            const int count = rec.w;
            bool whole_leaf = false;
            if constexpr (!RST && !SWP) whole_leaf = P.zero_copy && n_leaves == 0 && nn + count >= search_k;
            if (whole_leaf) {
                // the first leaf ends the search: its ids ARE the candidates -- not copied
                if (lane == 0) {
                    s_ncand = count;
                    cand_off = (int64_t)P.node_tree[node] * P.n_items + rec.z;
                }
            } else {
                for (int base = 0; base < count; base += 8 * WAVE) {
                    int32_t idv[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const int i = base + u * WAVE + lane;
                        idv[u] = i < count ? src_ids[i] : -1;
                    }
                    if constexpr (RST) {
                        if (gq >= 0) {   // uniform; the eight labels in flight together, the own group's ids dropped
                            int32_t gv[8];
#pragma unroll
                            for (int u = 0; u < 8; u++) gv[u] = idv[u] >= 0 ? R.group[idv[u]] : -1;
#pragma unroll
                            for (int u = 0; u < 8; u++) idv[u] = gv[u] == gq ? -1 : idv[u];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        bool fresh = false;
                        if (idv[u] >= 0) {
                            const uint32_t bit = 1u << (idv[u] & 31);
                            fresh = !(atomicOr(&bm[idv[u] >> 5], bit) & bit);
                        }
                        const unsigned long long mask = __ballot(fresh);
                        if (mask) {   // one counter update per 64 ids: the fresh ones take consecutive slots
                            int first = 0;
                            if (lane == 0) first = atomicAdd(&s_ncand, __popcll(mask));
                            first = __builtin_amdgcn_readfirstlane(first);
                            const int slot_c = first + __popcll(mask & ((1ull << lane) - 1ull));
                            if (fresh && slot_c < P.cap) cand[slot_c] = idv[u];
                        }
                    }
                }
            }
            nn += count;
            n_leaves++;
            if constexpr (SWP) {
                while (jrec < S->n_s && nn >= (int64_t)S->search_ks[jrec]) {
                    record(ndots);
                    jrec++;
                }
            }
        } else {
            const int4 rec = *(const int4 *)(P.node_rec + 4 * (int64_t)node);
            // the children's slots are wanted when they are popped, not now: requested here, under the hyperplane fetch
            const int32_t slot_c = lane < 2 ? P.node_hp[lane == 0 ? rec.y : rec.x] : 0;
            const float4 *hrow = (const float4 *)(P.hp + (int64_t)slot * P.dpad);
            const float m = NV > 0 ? wave_dot_held<NV>(hrow, qr, lane) : wave_dot(hrow, q, nvec, lane);
            if (lane < 2) {
                const uint64_t key = lane == 0 ? pq_key(d < m ? d : m, rec.y) : pq_key(d < -m ? d : -m, rec.x);
                if (hn + lane < PQ_LDS) {
                    s_bound[hn + lane] = (uint32_t)(key >> 32);
                    s_node[hn + lane] = (int32_t)(uint32_t)key;
                    s_slot[hn + lane] = slot_c;
                } else {
                    gpq[hn + lane] = key;
                }
            }
            hn += 2;
            ndots++;
        }
        __syncthreads();   // one wave: the queue writes above are seen by the next scan
        TP();
    }
    if constexpr (SWP) {
        for (; jrec < S->n_s; jrec++) record(ndots);   // the queue ran empty: the searches that wanted more stop here too
    }
    if (lane == 0) {
        const int nc = s_ncand;
        P.ncand[qi] = nc;
        P.cand_off[qi] = cand_off;
        atomicAdd(P.stat, (unsigned long long)(ndots + (nc < P.cap ? nc : P.cap) + 1));
    }
#ifdef MORNA_DESCEND_PROBE
    TP();
    if (lane == 0 && qi == 0) {
        float *o = P.low + 2 * gridDim.x + 16;
        o[0] = (float)ntp;
        for (int i = 1; i < ntp; i++) o[i] = (float)(tp[i] - tp[i - 1]);
    }
#endif
#undef TP
}

template <bool BM_LDS, int NV>
__global__ __launch_bounds__(WAVE) void query_descend_kernel(QueryParams P)
{
    query_descend_body<BM_LDS, NV, false>(P, RestrictArgs());
}

template <bool BM_LDS, int NV>
__global__ __launch_bounds__(WAVE) void query_descend_restricted_kernel(QueryParams P, RestrictArgs R)
{
    query_descend_body<BM_LDS, NV, true>(P, R);
}

template <bool BM_LDS, int NV>
__global__ __launch_bounds__(WAVE) void query_descend_sweep_kernel(QueryParams P, SweepArgs S)
{
    query_descend_body<BM_LDS, NV, false, true>(P, RestrictArgs(), &S);
}

#define QS_CPW 1   // candidates per wave of query_cand_dots_kernel
__global__ __launch_bounds__(Q_THREADS) void query_cand_dots_kernel(QueryParams P)
{
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t qi = blockIdx.y;
    const int nvec = P.dpad / 4;
    const int ncand = P.ncand[qi] < P.cap ? P.ncand[qi] : P.cap;
    const int c0 = (blockIdx.x * Q_WAVES + w) * QS_CPW;
    if (c0 >= ncand) return;
    const float4 *q = query_row(P, qi);
    const int64_t off = P.cand_off[qi];
    const int32_t *cand = off >= 0 ? P.perm + off : P.cand + qi * P.cap;
    uint64_t *keys = P.keys + qi * P.cap;
    const float pp = P.qpp[qi];
#pragma unroll
    for (int j = 0; j < QS_CPW; j++) {
        const int c = c0 + j;
        if (c < ncand) {
            const int32_t id = cand[c];
            const float pqv = wave_dot((const float4 *)(P.X + (int64_t)id * P.dpad), q, nvec, lane);
            if (lane == 0) keys[c] = ((uint64_t)f32_orderable(ang_dist(pp, P.norm2[id], pqv)) << 32) | (uint32_t)id;
        }
    }
}

// Sweep: the canonical dot of every candidate of every virtual query's deepest list -- a cell's candidates are a prefix of
// it, and a candidate's key does not depend on the prefix it is judged in, so no dot is taken twice.  A wave per candidate,
// the blocks of one virtual query side by side (bpv of them), in a 1-D grid.
// FLT: only the candidates that pass the threshold of the shortest prefix holding them (below, "sweep with the fp16 filter").
template <bool FLT>
__global__ __launch_bounds__(Q_THREADS) void sweep_cand_dots_kernel(QueryParams P, int32_t nq, int32_t bpv, int32_t n_s,
                                                                   const int32_t *__restrict__ cell_ncand, const float *__restrict__ thr)
{
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t vq = blockIdx.x / (unsigned)bpv;
    const int c = (int)(blockIdx.x - vq * bpv) * Q_WAVES + w;
    const int ncand = P.ncand[vq] < P.cap ? P.ncand[vq] : P.cap;
    if (c >= ncand) return;
    const int64_t qsrc = vq % nq;
    if constexpr (FLT) {
        const int64_t ti = vq / nq;
        int j = 0;   // the first cell whose prefix holds candidate c (the deepest one's does)
        while (j < n_s - 1 && cell_ncand[(ti * n_s + j) * nq + qsrc] <= c) j++;
        if (P.low[vq * P.cap + c] > thr[(ti * n_s + j) * nq + qsrc]) {   // (a NaN on either side: kept)
            if (lane == 0) P.keys[vq * P.cap + c] = ~0ull;
            return;
        }
        if (lane == 0) atomicAdd(P.stat + 3, 1ull);
    }
    const float4 *q = query_row(P, qsrc);
    const int32_t id = P.cand[vq * P.cap + c];
    const float pqv = wave_dot((const float4 *)(P.X + (int64_t)id * P.dpad), q, P.dpad / 4, lane);
    if (lane == 0)
        P.keys[vq * P.cap + c] = ((uint64_t)f32_orderable(ang_dist(P.qpp[qsrc], P.norm2[id], pqv)) << 32) | (uint32_t)id;
}

// The k smallest (distance, id) keys of a query's candidates, in order.  Two looks at the keys instead of k rounds of a
// block-wide minimum: every thread's own minimum -- the k-th smallest of those 256 bounds the k-th smallest key from above --,
// then the few keys at or below that bound are collected and ranked by counting (the keys are distinct: the id is in them).
#define QT_HELD 16
#define QT_LIST 1024
// keys[0 .. nsel): the keys to rank; qi: the slot of the answer in ids_out / dist_out / count_out
__device__ __forceinline__ void query_topk_body(const QueryParams &P, const uint64_t *keys, const int nsel, const int64_t qi)
{
    __shared__ uint64_t s_red[Q_WAVES];
    __shared__ uint64_t s_min[Q_THREADS];
    __shared__ uint64_t s_list[QT_LIST];
    __shared__ uint64_t s_bound;
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int kout = P.k < nsel ? P.k : nsel;
    auto emit = [&](int r, uint64_t key) {
        P.ids_out[qi * P.k + r] = (int32_t)(uint32_t)key;
        const float d = f32_from_orderable((uint32_t)(key >> 32));
        P.dist_out[qi * P.k + r] = sqrtf(d > 0.f ? d : 0.f);   // normalized_distance
    };
    bool done = false;
    if (nsel <= Q_THREADS * QT_HELD && kout > 0 && kout <= Q_THREADS) {
        uint64_t held[QT_HELD], mine = ~0ull;
#pragma unroll
        for (int u = 0; u < QT_HELD; u++) {
            held[u] = tid + Q_THREADS * u < nsel ? keys[tid + Q_THREADS * u] : ~0ull;
            mine = held[u] < mine ? held[u] : mine;
        }
        s_min[tid] = mine;
        if (tid == 0) { s_n = 0; s_bound = ~0ull; }
        __syncthreads();
        if (nsel <= Q_THREADS) {
            if (tid == 0) s_bound = ~0ull - 1;   // a key per thread at most: all of them are collected
        } else {
            int below = 0;
            for (int j = 0; j < Q_THREADS; j++) below += s_min[j] < mine ? 1 : 0;
            if (mine != ~0ull && below == kout - 1) s_bound = mine;   // kout threads hold a key at or below it
        }
        __syncthreads();
        const uint64_t bound = s_bound;
#pragma unroll
        for (int u = 0; u < QT_HELD; u++)
            if (held[u] <= bound && held[u] != ~0ull) {
                const int slot = atomicAdd(&s_n, 1);
                if (slot < QT_LIST) s_list[slot] = held[u];
            }
        __syncthreads();
        const int m = s_n;
        if (m <= QT_LIST) {
            for (int i = tid; i < m; i += Q_THREADS) {
                const uint64_t v = s_list[i];
                int below = 0;
                for (int j = 0; j < m; j++) below += s_list[j] < v ? 1 : 0;
                if (below < kout) emit(below, v);
            }
            done = true;
        }
    }
    if (!done) {   // more keys than the registers hold, or a tie of thousands at the bound: k rounds of a block-wide minimum
        uint64_t prev = 0;
        for (int r = 0; r < kout; r++) {
            uint64_t best = ~0ull;
            for (int c = tid; c < nsel; c += Q_THREADS) {
                const uint64_t kk = keys[c];
                if ((r == 0 || kk > prev) && kk < best) best = kk;
            }
            best = block_min_u64(best, s_red, tid);
            if (tid == 0) emit(r, best);
            prev = best;
        }
    }
    for (int r = kout + tid; r < P.k; r += Q_THREADS) {
        P.ids_out[qi * P.k + r] = -1;
        P.dist_out[qi * P.k + r] = INFINITY;
    }
    if (tid == 0) P.count_out[qi] = kout;
}

__global__ __launch_bounds__(Q_THREADS) void query_topk_kernel(QueryParams P)
{
    const int64_t qi = blockIdx.x;
    query_topk_body(P, P.keys + qi * P.cap, P.ncand[qi] < P.cap ? P.ncand[qi] : P.cap, qi);
}

// Sweep: block c = (i * n_s + j) * nq + q ranks the first cell_ncand[c] keys of virtual query i * nq + q -- the candidates
// the search with trees[i] and search_ks[j] had when it stopped -- into answer slot c.
__global__ __launch_bounds__(Q_THREADS) void sweep_topk_kernel(QueryParams P, int32_t n_s, int32_t nq, const int32_t *cell_ncand)
{
    const int64_t cell = blockIdx.x;
    const int64_t q = cell % nq, ti = cell / ((int64_t)n_s * nq);
    const int nc = cell_ncand[cell];
    query_topk_body(P, P.keys + (ti * nq + q) * P.cap, nc < P.cap ? nc : P.cap, cell);
}

// Recall of a sweep: hits[c] = |ids of cell c  n  exact ids of its query|, a wave per (cell, query); -1 where the exact
// search failed (count -1: a row parallel to the query).  Lists of at most a few hundred ids: compared pair by pair.
__global__ __launch_bounds__(WAVE) void sweep_hits_kernel(const int32_t *__restrict__ ids, const int32_t *__restrict__ count,
                                                          const int32_t *__restrict__ ex_ids, const int32_t *__restrict__ ex_count,
                                                          int32_t nq, int32_t k, int32_t *__restrict__ hits)
{
    const int lane = threadIdx.x;
    const int64_t cell = blockIdx.x, q = cell % nq;
    const int ec = ex_count[q], ac = count[cell];
    if (ec < 0) {
        if (lane == 0) hits[cell] = -1;
        return;
    }
    int mine = 0;
    for (int a = lane; a < ac; a += WAVE) {
        const int32_t id = ids[cell * k + a];
        for (int e = 0; e < ec; e++) mine += ex_ids[q * k + e] == id ? 1 : 0;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, WAVE);
    if (lane == 0) hits[cell] = mine;
}

// Sweep with the fp16 filter (the batch's scores[] are there): the bounds of a candidate's distance do not depend on the
// prefix it is judged in, so they are made once per virtual query (sweep_bounds_kernel: the arithmetic of
// query_refine_kernel<2>); per cell the k-th smallest UPPER bound of its prefix is the cell's threshold
// (sweep_threshold_kernel).  That threshold only falls as the prefix grows, so a candidate is wanted by some cell iff it
// passes the threshold of the SHORTEST prefix that holds it: sweep_cand_dots_kernel<true> takes the canonical dot of those
// alone -- once -- and leaves ~0 in the key of every other candidate, which no cell's k smallest keys can be.
__global__ __launch_bounds__(Q_THREADS) void sweep_bounds_kernel(QueryParams P, int32_t nq, uint64_t *__restrict__ ub)
{
    const int64_t vq = blockIdx.x, q = vq % nq;
    const int ncand = P.ncand[vq] < P.cap ? P.ncand[vq] : P.cap;
    const int32_t qsrc = P.items ? P.items[q] : (int32_t)q;
    const float qs = P.qscale[qsrc], qn = P.qn16[qsrc], qe = P.qe16[qsrc];
    const float rq = qe / (qn * 0.996f);
    const float *sc_row = P.scores + q * P.n_items;
    const float pp = P.qpp[q];
    const float nan = __int_as_float(0x7fc00000);
    for (int c = threadIdx.x; c < ncand; c += Q_THREADS) {
        const int32_t id = P.cand[vq * P.cap + c];
        const float sc = P.xscale[id] * qs;
        const float rx = P.xe16[id] / (P.xn16[id] * 0.996f);
        float df = nan, dl = 0.f;
        if (sc != 0.f && rx < 0.125f && rq < 0.125f) {   // (the bound of query_refine_kernel<2>; every row went through the two-chain form)
            const float cerr = ((P.eacc + rx) + (1.f + rx) * rq) / ((1.f - rx) * (1.f - rq));
            df = ang_dist(pp, P.norm2[id], sc_row[id] * sc);
            dl = 2.02f * cerr + 1e-5f;
        }
        ub[vq * P.cap + c] = ((uint64_t)f32_orderable(df + dl) << 32) | (uint32_t)c;
        P.low[vq * P.cap + c] = df - dl;
    }
}

__global__ __launch_bounds__(Q_THREADS) void sweep_threshold_kernel(QueryParams P, int32_t n_s, int32_t nq, const int32_t *__restrict__ cell_ncand,
                                                                   const uint64_t *__restrict__ ub, float *__restrict__ thr)
{
    __shared__ uint64_t s_red[Q_WAVES];
    __shared__ uint64_t s_top[Q_WAVES * KTH_MAX_K];
    const int64_t cell = blockIdx.x;
    const int64_t q = cell % nq, ti = cell / ((int64_t)n_s * nq);
    const int nc = cell_ncand[cell] < P.cap ? cell_ncand[cell] : P.cap;
    if (nc <= P.k) {   // every candidate is an answer (uniform)
        if (threadIdx.x == 0) thr[cell] = INFINITY;
        return;
    }
    const uint64_t kth = block_kth_smallest(ub + (ti * nq + q) * P.cap, nc, P.k, threadIdx.x, s_red, s_top);
    if (threadIdx.x == 0) thr[cell] = f32_from_orderable((uint32_t)(kth >> 32));   // (NaN when fewer than k have a bound: all pass)
}

// ---- filter dots of a whole batch on the matrix cores ----------------------------------------------------------
// scores[q][r] = sum_i g_q[i] y_r[i] for ALL rows r and all queries q of the batch, from the fp16 images: a
// nq x N x dpad contraction that reads the fp16 matrix once (0.3 GB at 50k x 3000) where the per-query form gathers
// every query's ~K candidate rows separately (12 GB for 1000 queries).  It does ~N / K times the arithmetic the
// candidates need, which the matrix cores deliver in less time than the gathers take while
// nq * K >> N.  Queries are the A side (m), rows the B side (n): 32 lanes hold 32 consecutive rows of one query, so
// the result goes out in 128-byte runs.  qrow: row of Q16 that holds query q (by-item queries point into the
// matrix's own image), or null for the identity.
template <int BR, int BK, int NS>   // rows of the matrix per workgroup tile, halfs per K-step, stages in flight (mm16.hpp)
__global__ __launch_bounds__(MM16_THREADS) void query_scores_kernel(const _Float16 *__restrict__ X16, int64_t n_items, int32_t dpad,
                                                                    const _Float16 *__restrict__ Q16,
                                                                    const int32_t *__restrict__ qrow, int32_t nq,
                                                                    float *__restrict__ scores, int64_t r_begin /* rows [r_begin, n_items) */)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int32_t s_qrow[MM16_TILE];
    constexpr int NB = BR / 128;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int wm = w >> 1, wn = w & 1;
    // workgroup b runs on XCD b % 8: an XCD takes every 8th row tile and walks that tile's query tiles back to back,
    // so the row tile comes from HBM once and then from that XCD's L2
    const int n_ct = (nq + MM16_TILE - 1) / MM16_TILE;
    const int64_t row_tile = (int64_t)((blockIdx.x >> 3) / n_ct) * 8 + (blockIdx.x & 7);
    const int64_t r0 = r_begin + row_tile * BR;
    const int c0 = (int)((blockIdx.x >> 3) % n_ct) * MM16_TILE;
    if (r0 >= n_items) return;
    if (tid < MM16_TILE) {
        const int q = c0 + tid < nq ? c0 + tid : nq - 1;
        s_qrow[tid] = qrow ? qrow[q] : q;
    }
    __syncthreads();
    mm16_f32x16 acc[NB][2];
    mm16_tile<BR, BK, NS>(X16, Q16, dpad, smem, [&](int rt) { return r0 + rt < n_items ? r0 + rt : n_items - 1; },
                          [&](int rt) { return (int64_t)s_qrow[rt]; }, acc);
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int tb = 0; tb < NB; tb++) {
        const int64_t r = r0 + wm * 32 * NB + tb * 32 + lr;
        if (r < n_items) {
#pragma unroll
            for (int tn = 0; tn < 2; tn++)
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int q = c0 + wn * 64 + tn * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                    if (q < nq) scores[(int64_t)q * n_items + r] = acc[tb][tn][e];
                }
        }
    }
}

// The same product in 256 x 256 tiles, 16 waves, ONE accumulation chain (mm16.hpp): half the operand bytes delivered to LDS
// per product, which is what bounds the loop.  Its workgroups take the whole CU, so it covers only as many 256-row tiles as
// fill the chip in whole rounds (the host picks n_row_tiles); the 128 x 128 form above takes the rows behind them.  The
// bound on its accumulation is the one-chain EACC (QueryParams::eacc_big).
template <int BK, int NS>
__global__ __launch_bounds__(1024) void query_scores_big_kernel(const _Float16 *__restrict__ X16, int64_t n_items, int32_t dpad,
                                                                const _Float16 *__restrict__ Q16, const int32_t *__restrict__ qrow,
                                                                int32_t nq, float *__restrict__ scores, int32_t n_row_tiles)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int32_t s_qrow[256];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int wm = w >> 2, wn = w & 3;   // the wave's part of the tile: rows wm * 64 .., queries wn * 64 ..
    const int n_ct = (nq + 255) / 256;
    const int64_t row_tile = (int64_t)((blockIdx.x >> 3) / n_ct) * 8 + (blockIdx.x & 7);   // XCD b % 8 keeps its row tiles
    if (row_tile >= n_row_tiles) return;
    const int64_t r0 = row_tile * 256;   // (+ 255 < n_items: the host covers whole tiles only)
    const int c0 = (int)((blockIdx.x >> 3) % n_ct) * 256;
    if (tid < 256) {
        const int q = c0 + tid < nq ? c0 + tid : nq - 1;
        s_qrow[tid] = qrow ? qrow[q] : q;
    }
    __syncthreads();
    mm16_f32x16 acc[2][2];
    mm16_tile_256x256<BK, NS>(X16, Q16, dpad, smem, [&](int rt) { return r0 + rt; }, [&](int rt) { return (int64_t)s_qrow[rt]; }, acc);
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int tb = 0; tb < 2; tb++) {
        const int64_t r = r0 + wm * 64 + tb * 32 + lr;
#pragma unroll
        for (int tn = 0; tn < 2; tn++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int q = c0 + wn * 64 + tn * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (q < nq) scores[(int64_t)q * n_items + r] = acc[tb][tn][e];
            }
    }
}

// ---- refine: angular distance to the candidates, k smallest (distance, id) --------------------------------------
// FILTER (modes 1 and 2): a distance taken from fp16 data is within delta of the canonical fp32 one, so the k
// smallest canonical distances are among the candidates whose lower bound does not exceed the k-th smallest upper
// bound; only those get the canonical wave_dot, and the ranking is done on canonical values alone.  Candidates
// without a usable fp16 value (inf, NaN, unscalable rows or queries) are never filtered out.
template <int MODE>   // 0: no filter; 1: fp16 row x fp32 query per candidate (gather); 2: scores[] of the whole batch
__global__ __launch_bounds__(Q_THREADS) void query_refine_kernel(QueryParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *qv = (float4 *)smem;
    __shared__ uint64_t s_red[Q_WAVES];
    __shared__ uint64_t s_top[Q_WAVES * KTH_MAX_K];
    __shared__ int s_nsurv;

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int64_t qi = blockIdx.x;
    const int nvec = P.dpad / 4;
    const float4 *src = P.items ? (const float4 *)(P.X + (int64_t)P.items[qi] * P.dpad)
                                : (const float4 *)(P.Q + qi * P.dpad);
    for (int i = tid; i < nvec; i += Q_THREADS) qv[i] = src[i];
    if (tid == 0) s_nsurv = 0;
    __syncthreads();

    int32_t *cand = P.cand + qi * P.cap;
    uint64_t *keys = P.keys + qi * P.cap;
    const int ncand = P.ncand[qi] < P.cap ? P.ncand[qi] : P.cap;
    const float pp = P.qpp[qi];
    int nsel = ncand;          // candidates that get the canonical dot; their ids in cand[0 .. nsel)

    if (MODE != 0 && ncand > P.k) {
        float *low = P.low + qi * P.cap;
        const float nan = __int_as_float(0x7fc00000);
        if (MODE == 1) {
            typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
            const int nv8 = P.dpad / 8;
            for (int c = w; c < ncand; c += Q_WAVES) {
                const int32_t id = cand[c];
                const f16x8 *y = (const f16x8 *)(P.X16 + (int64_t)id * P.dpad);
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                auto mac8 = [&](const f16x8 hv, int i) {
                    const float4 qa = qv[2 * i], qb = qv[2 * i + 1];
                    s0 = fmaf((float)hv[0], qa.x, s0);
                    s1 = fmaf((float)hv[1], qa.y, s1);
                    s2 = fmaf((float)hv[2], qa.z, s2);
                    s3 = fmaf((float)hv[3], qa.w, s3);
                    s0 = fmaf((float)hv[4], qb.x, s0);
                    s1 = fmaf((float)hv[5], qb.y, s1);
                    s2 = fmaf((float)hv[6], qb.z, s2);
                    s3 = fmaf((float)hv[7], qb.w, s3);
                };
                int i = lane;
                for (; i + 5 * WAVE < nv8; i += 6 * WAVE) {   // six 1-KiB loads in flight before the first use
                    const f16x8 h0 = y[i], h1 = y[i + WAVE], h2 = y[i + 2 * WAVE], h3 = y[i + 3 * WAVE];
                    const f16x8 h4 = y[i + 4 * WAVE], h5 = y[i + 5 * WAVE];
                    mac8(h0, i);
                    mac8(h1, i + WAVE);
                    mac8(h2, i + 2 * WAVE);
                    mac8(h3, i + 3 * WAVE);
                    mac8(h4, i + 4 * WAVE);
                    mac8(h5, i + 5 * WAVE);
                }
                for (; i < nv8; i += WAVE) mac8(y[i], i);
                const float sc = P.xscale[id];   // 0: the row has no fp16 image (inf, NaN or below the scalable range)
                const float dotf = wave_sum_xor((s0 + s1) + (s2 + s3)) * sc;
                const float df = sc != 0.f ? ang_dist(pp, P.norm2[id], dotf) : nan;
                if (lane == 0) {
                    // a NaN sorts after every number: it takes none of the k places that set the threshold
                    keys[c] = ((uint64_t)f32_orderable(df + P.delta) << 32) | (uint32_t)c;
                    low[c] = df - P.delta;
                }
            }
        } else {
            const int32_t qsrc = P.items ? P.items[qi] : (int32_t)qi;
            const float qs = P.qscale[qsrc], qn = P.qn16[qsrc], qe = P.qe16[qsrc];
            const float rq = qe / (qn * 0.996f);          // |f| / |g|, |g| from its upper bound less the slack put on it
            const float *sc_row = P.scores + qi * P.n_items;
            for (int c = tid; c < ncand; c += Q_THREADS) {
                const int32_t id = cand[c];
                const float sc = P.xscale[id] * qs;
                const float rx = P.xe16[id] / (P.xn16[id] * 0.996f);
                float df = nan, dl = 0.f;
                if (sc != 0.f && rx < 0.125f && rq < 0.125f) {
                    // |sum y g - s t x.q| <= (EACC |y| + |d|) |g| + (|y| + |d|) |f|, and s |x| >= |y| - |d|, t |q| >= |g| - |f|:
                    // the cosine taken from the images is within this of the exact one
                    const float cerr = (((id < P.big_rows ? P.eacc_big : P.eacc) + rx) + (1.f + rx) * rq) / ((1.f - rx) * (1.f - rq));
                    df = ang_dist(pp, P.norm2[id], sc_row[id] * sc);
                    dl = 2.02f * cerr + 1e-5f;           // distance = 2 - 2 cos; the canonical norms and ang_dist's own rounding
                }
                keys[c] = ((uint64_t)f32_orderable(df + dl) << 32) | (uint32_t)c;
                low[c] = df - dl;
            }
        }
        __syncthreads();
        // the k-th smallest upper bound (keys are distinct: the candidate index is in them)
        const uint64_t kth = block_kth_smallest(keys, ncand, P.k, tid, s_red, s_top);
        const float thr = f32_from_orderable((uint32_t)(kth >> 32));
        // survivors, compacted to the front of keys[] as ids (order is irrelevant: the ranking below is by value)
        __syncthreads();
        for (int c0 = 0; c0 < ncand; c0 += Q_THREADS) {
            const int c = c0 + tid;
            const bool in = c < ncand && !(low[c] > thr);   // NaN stays in
            const int32_t id = c < ncand ? cand[c] : 0;
            __syncthreads();                                // every cand[c] of this round is read before a slot is written
            if (in) cand[atomicAdd(&s_nsurv, 1)] = id;      // slots < c0 + Q_THREADS: none beyond the round just read
            __syncthreads();
        }
        nsel = s_nsurv;
    }
    if (MODE == 2 && P.refine_stat && tid == 0)   // (one batch: at most 2^26 candidates, the 1 GiB workspace rule)
        atomicAdd(P.refine_stat, ((unsigned long long)ncand << 32) + (unsigned long long)nsel);
    __syncthreads();
    for (int c = w; c < nsel; c += Q_WAVES) {
        const int32_t id = cand[c];
        const float pqv = wave_dot((const float4 *)(P.X + (int64_t)id * P.dpad), qv, nvec, lane);
        if (lane == 0) keys[c] = ((uint64_t)f32_orderable(ang_dist(pp, P.norm2[id], pqv)) << 32) | (uint32_t)id;
    }
    __syncthreads();

    // ---- k smallest (distance, id) pairs, in order
    const int kout = P.k < nsel ? P.k : nsel;
    uint64_t prev = 0;
    bool have_prev = false;
    if (nsel <= WAVE * KTH_HELD) {
        // few enough for one wave's registers (the usual case: ~2k survivors): k rounds of register compares and a wave
        // minimum, no barrier
        if (w == 0) {
            uint64_t held[KTH_HELD];
#pragma unroll
            for (int u = 0; u < KTH_HELD; u++) held[u] = lane + WAVE * u < nsel ? keys[lane + WAVE * u] : ~0ull;
            for (int r = 0; r < kout; r++) {
                uint64_t best = ~0ull;
#pragma unroll
                for (int u = 0; u < KTH_HELD; u++)
                    if ((r == 0 || held[u] > prev) && held[u] < best) best = held[u];
                prev = wave_min_u64(best);
                if (lane == 0) {
                    P.ids_out[qi * P.k + r] = (int32_t)(uint32_t)prev;
                    const float d = f32_from_orderable((uint32_t)(prev >> 32));
                    P.dist_out[qi * P.k + r] = sqrtf(d > 0.f ? d : 0.f);   // normalized_distance
                }
            }
        }
    } else
    for (int r = 0; r < kout; r++) {
        uint64_t best = ~0ull;
        for (int c = tid; c < nsel; c += Q_THREADS) {
            const uint64_t kk = keys[c];
            if ((!have_prev || kk > prev) && kk < best) best = kk;
        }
        best = block_min_u64(best, s_red, tid);
        if (tid == 0) {
            P.ids_out[qi * P.k + r] = (int32_t)(uint32_t)best;
            const float d = f32_from_orderable((uint32_t)(best >> 32));
            P.dist_out[qi * P.k + r] = sqrtf(d > 0.f ? d : 0.f);   // normalized_distance
        }
        prev = best;
        have_prev = true;
    }
    for (int r = kout + tid; r < P.k; r += Q_THREADS) {
        P.ids_out[qi * P.k + r] = -1;
        P.dist_out[qi * P.k + r] = INFINITY;
    }
    if (tid == 0) P.count_out[qi] = kout;
}

// [n][k] ids / distances of a batch -> the [n][2k] int32 message of the top-k all-gather: global ids, distance bits
__global__ void pack_topk_kernel(const int32_t *__restrict__ ids, const float *__restrict__ dist, int64_t total, int32_t k,
                                 int32_t id_offset, int32_t *__restrict__ packed)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t q = i / k;
    const int r = (int)(i - q * k);
    const int32_t id = ids[i];
    packed[q * 2 * k + r] = id >= 0 ? id + id_offset : -1;
    packed[q * 2 * k + k + r] = __float_as_int(dist[i]);
}

int fetch_results(morna_index *h, const uint8_t *d_block, size_t bytes, size_t s_ids, size_t s_dist, size_t dist_elt, int64_t nq,
                  int32_t k, int32_t *ids_out, void *dist_out, int32_t *count_out)
{
    MORNA_TRY(h->host_out.reserve(bytes));
    HIP_TRY(hipMemcpyAsync(h->host_out.p, d_block, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->unsettled = false;
    memcpy(ids_out, h->host_out.p, (size_t)nq * k * 4);
    if (dist_out) memcpy(dist_out, h->host_out.p + s_ids, (size_t)nq * k * dist_elt);
    if (count_out) memcpy(count_out, h->host_out.p + s_ids + s_dist, (size_t)nq * 4);
    return MORNA_OK;
}

// ---- the approximate search, host side --------------------------------------------------------------------------------
// query_batch and search_sweep read from top to bottom: check, plan, [start the early contraction,] then per batch: bind
// the workspace, stage the queries, traverse, refine, deliver.  What the two share comes first: the dispatch over the row
// width, the launchers, the set-up of QueryParams and the staging of the queries (launch_lds, with_flag and the workspace
// carver are in search_common.hpp: the exact family uses them too).

// float4 per lane of a row, where the kernels have a register form of that width and it is at most max_nv; else 0
static inline int row_nv(int32_t dpad, int max_nv)
{
    const int nv = dpad / 256;
    const bool built = nv == 1 || nv == 2 || nv == 3 || nv == 4 || nv == 6 || nv == 8 || nv == 12 || nv == 16 || nv == 24 || nv == 32;
    return dpad % 256 == 0 && built && nv <= max_nv ? nv : 0;
}

// The one switch over the row width: f(std::integral_constant<int, NV>) with NV = row_nv(dpad, MAX_NV).  MAX_NV bounds what
// a call site instantiates: 32 for the plain and restricted descents, 12 for the sweep descent and the root margins.
template <int NV, int MAX_NV>
using nv_upto = std::integral_constant<int, (NV <= MAX_NV ? NV : 0)>;

template <int MAX_NV, class F>
static inline int with_row_nv(int32_t dpad, F &&f)
{
    switch (row_nv(dpad, MAX_NV)) {
    case 1: return f(nv_upto<1, MAX_NV>{});
    case 2: return f(nv_upto<2, MAX_NV>{});
    case 3: return f(nv_upto<3, MAX_NV>{});
    case 4: return f(nv_upto<4, MAX_NV>{});
    case 6: return f(nv_upto<6, MAX_NV>{});
    case 8: return f(nv_upto<8, MAX_NV>{});
    case 12: return f(nv_upto<12, MAX_NV>{});
    case 16: return f(nv_upto<16, MAX_NV>{});
    case 24: return f(nv_upto<24, MAX_NV>{});
    case 32: return f(nv_upto<32, MAX_NV>{});
    default: return f(nv_upto<0, MAX_NV>{});
    }
}

// What a search call works out once, before its first batch.  search_sweep fills the same plan for its deepest cell.
struct QueryPlan {
    int32_t T_used;        // the trees the search walks: all of them, or a prefix (morna_hip.h, "tree-prefix search")
    int32_t search_k;
    int32_t cap;           // candidates per query: |nns| < search_k before the last pop, which adds at most K ids
    int32_t bm_words;
    bool bm_lds;           // the sample bitmap lives in LDS (else in the workspace)
    size_t lds_q, lds_bm;  // dynamic LDS of the query image and of the bitmap (0: not in LDS)
    bool spread;           // fewer queries than would give every CU a workgroup: each query's work is dealt out
    bool use_filter;       // candidate filter on the fp16 rows; pays when a query has many more candidates than results
    bool may_dense;        // ... through the whole-batch contraction, for the batches dense_pays() says so of
    int64_t batch;         // queries per batch (the 1 GiB workspace rule)
};

// once per process: MORNA_QUERY_FILTER=0: every candidate gets the fp32 dot; MORNA_QUERY_DENSE=0 keeps the per-candidate
// gather form of the filter
static bool query_filter_on() { static const bool on = env_on("MORNA_QUERY_FILTER"); return on; }
static bool query_dense_on() { static const bool on = env_on("MORNA_QUERY_DENSE"); return on; }

// the whole-batch contraction reads every fp16 row once; the gather form reads min(cap, ~K) rows per query
// (C3, 48 / 63 queries: 207 us through the contraction, 231 / 282 us through the spread form; 32: the spread form's 174 us)
static bool dense_pays(const morna_index *h, int32_t cap, int64_t nb)
{
    return nb >= 40 && nb * std::min<int64_t>(cap, h->K) >= 2 * h->n_items;
}

static int require_built(const morna_index *h)
{
    if (h->built) return MORNA_OK;
    set_error("index has not been built: call build() before searching");
    return MORNA_E_STATE;
}

// the checks of both searches; what: "get_nns" / "search_sweep"
static int check_search_call(const morna_index *h, const char *what, int32_t k, int64_t nq)
{
    if (k <= 0 || nq < 0) {
        set_error("%s: n must be positive", what);
        return MORNA_E_INVALID;
    }
    if (h->dpad > Q_MAX_DPAD) {   // the query image and the traversal's LDS (an index built elsewhere, loaded here)
        set_error("%s: dimension %d is above the supported %d", what, h->dim, Q_MAX_DPAD);
        return MORNA_E_INVALID;
    }
    return MORNA_OK;
}

static int check_tree_count(const morna_index *h, const char *what, int32_t t)
{
    if (t >= 1 && t <= h->n_trees) return MORNA_OK;
    set_error("%s: %d trees asked for, the forest has %d", what, t, h->n_trees);
    return MORNA_E_RANGE;
}

static int check_items(const morna_index *h, const int32_t *items_host, int64_t nq)
{
    for (int64_t i = 0; i < nq; i++)
        if (items_host[i] < 0 || items_host[i] >= h->n_items) {
            set_error("item id %d out of range [0, %lld)", items_host[i], (long long)h->n_items);
            return MORNA_E_RANGE;
        }
    return MORNA_OK;
}

// the handle's rows and forest, and the plan's numbers; everything of the workspace, the queries and the filter is null
static QueryParams base_params(const morna_index *h, const QueryPlan &pl, int32_t k)
{
    QueryParams P = {};
    P.X = h->X.p; P.norm2 = h->norm2.p; P.n_items = h->n_items; P.dpad = h->dpad; P.n_trees = pl.T_used; P.K = h->K;
    P.node_rec = h->node_rec.p; P.node_tree = h->node_tree.p; P.node_hp = h->node_hp.p; P.hp = h->hp.p;
    P.perm = h->perm.p; P.n_nodes = h->n_nodes;
    P.k = k; P.search_k = pl.search_k; P.cap = pl.cap; P.bm_words = pl.bm_words;
    P.stat = h->d_stat.p;
    return P;
}

// the fp16 image of the rows and its bounds (split_mm_prepare_rows has made them)
static void set_filter_rows(const morna_index *h, QueryParams &P)
{
    const float *xn = h->half.xn.p;
    P.X16 = h->half.x16.p;
    P.xn16 = xn; P.xscale = xn + h->n_items; P.xe16 = xn + 2 * h->n_items;
    // gather form: |cos from the fp16 row - cos from the fp32 row| <= 2^-11 (one rounding to 11 bits, the query
    // is not rounded) + the fp32 accumulations of both dots (any order: < dpad * 2^-24 each); the distance is
    // 2 - 2 cos; 1e-5 covers the evaluation of ang_dist itself
    P.delta = 2.f * (1.02f * 0.00048828125f + 2.f * (float)h->dpad * 5.9604645e-8f) + 1e-5f;
    P.eacc = mm16_eacc(h->dpad);
}

// The queries of a batch on the device, and what the whole-batch contraction makes of them.  Part of h->ws; for a batch that
// starts beside a pending build, of h->q_early (EarlyContraction).
struct QueryInputs {
    int32_t *items;                // [n] by item (part of the workspace: a hipMalloc / hipFree per call costs tens of microseconds)
    float *Q;                      // [n][dpad] by vector
    _Float16 *Q16;                 // [n][dpad] by vector, when the contraction may run: the fp16 image of Q ...
    float *qn16, *qe16, *qscale;   // [n] ... and its norms, rounding-error norms and scales
    float *scores;                 // [n][n_items] the contraction's output
    void carve(Carver &c, const morna_index *h, int64_t n, bool by_vector, bool half_image, bool with_scores)
    {
        items = c.take<int32_t>((size_t)n);
        Q = c.take<float>(by_vector ? (size_t)n * h->dpad : 0);
        Q16 = c.take<_Float16>(by_vector && half_image ? (size_t)n * h->dpad : 0);
        qn16 = c.take<float>((size_t)n);
        qe16 = c.take<float>((size_t)n);
        qscale = c.take<float>((size_t)n);
        scores = c.take<float>(with_scores ? (size_t)n * h->n_items : 0);
    }
};

// Queries q0 .. q0 + nb of the call onto stream st: the vectors padded to the row stride (q_host: host OR device memory,
// q_stride floats apart), or the item ids.
static int stage_queries(morna_index *h, const QueryInputs &in, const float *q_host, int64_t q_stride, const int32_t *items_host,
                         int64_t q0, int64_t nb, hipStream_t st)
{
    if (q_host) {
        HIP_TRY(hipMemsetAsync(in.Q, 0, (size_t)nb * h->dpad * 4, st));
        HIP_TRY(hipMemcpy2DAsync(in.Q, (size_t)h->dpad * 4, q_host + q0 * q_stride, (size_t)q_stride * 4, (size_t)h->dim * 4, (size_t)nb,
                                 hipMemcpyDefault, st));
    } else {
        HIP_TRY(hipMemcpyAsync(in.items, items_host + q0, (size_t)nb * 4, hipMemcpyHostToDevice, st));
    }
    return MORNA_OK;
}

// The queries' fp16 image, for the contraction (q16, qrow) and for the bound of every pair (qn16, qe16, qscale, indexed by
// the item id or by the query number).  By item it is the image of the stored rows.  By vector it is made from the staged
// rows on stream st (convert), unless the early contraction has made it.
struct HalfImage {
    const _Float16 *q16;
    const int32_t *qrow;
    const float *qn16, *qe16, *qscale;
};

static int half_image(morna_index *h, const QueryInputs &in, bool by_vector, int64_t nb, bool convert, hipStream_t st, HalfImage &im)
{
    if (by_vector) {
        if (convert) MORNA_TRY(split_mm_convert_rows(h, in.Q, nb, in.Q16, in.qn16, in.qe16, in.qscale, st));
        im = {in.Q16, nullptr, in.qn16, in.qe16, in.qscale};
    } else {
        const float *xn = h->half.xn.p;
        im = {h->half.x16.p, in.items, xn, xn + 2 * h->n_items, xn + h->n_items};
    }
    return MORNA_OK;
}

// MORNA_DEBUG_OPEN=1 (read once per process): one line per contraction and per dense batch on stderr
static bool query_debug_open()
{
    static const bool on = getenv("MORNA_DEBUG_OPEN") && atoi(getenv("MORNA_DEBUG_OPEN")) != 0;
    return on;
}

// The whole-batch contraction: 256 x 256 tiles for as many 256-row tiles as make whole rounds of the chip (one workgroup
// per CU), the 128 x 128 form for the rows behind them (MORNA_QUERY_BIG=0, read once per process, or !allow_big: for all
// rows).  st_big / st_rem: the streams of the two launches; *big_rows_out: the rows the large form took.
// site: the caller, for the MORNA_DEBUG_OPEN line (host values only).
static int launch_contraction(morna_index *h, int64_t nb, const HalfImage &im, float *scores, hipStream_t st_big, hipStream_t st_rem,
                              bool allow_big, int64_t *big_rows_out, const char *site)
{
    static const bool big_on = env_on("MORNA_QUERY_BIG");
    const _Float16 *X16 = h->half.x16.p;
    const int64_t N = h->n_items;
    int64_t big_tiles = 0, big_rows = 0;
    if (allow_big && big_on && nb >= 512) {
        const int64_t n_ct_big = (nb + 255) / 256;
        int64_t a = h->n_cus, b = n_ct_big;   // tiles per round of the chip: n_cus / gcd(n_cus, n_ct_big)
        while (b) { const int64_t t = a % b; a = b; b = t; }
        const int64_t per_round = h->n_cus / a;
        big_tiles = (N / 256) / per_round * per_round;
    }
    if (big_tiles > 0) {
        const unsigned n_ct_big = (unsigned)((nb + 255) / 256);
        MORNA_TRY(launch_lds(query_scores_big_kernel<64, 2>, dim3(8u * (unsigned)((big_tiles + 7) / 8) * n_ct_big), dim3(1024),
                             128 * 256 * 4, LDS_ALWAYS, st_big, X16, N, h->dpad, im.q16, im.qrow, (int32_t)nb, scores, (int32_t)big_tiles));
        big_rows = big_tiles * 256;
    }
    if (big_rows < N) {
        const unsigned n_ct = (unsigned)((nb + MM16_TILE - 1) / MM16_TILE), n_rt = (unsigned)((N - big_rows + 127) / 128);
        // (the rows behind the whole rounds of the 256 x 256 form: on the side stream, in front of the traversal,
        // when the large form runs -- behind it on the main stream they were 0.05 ms of the batch's critical path)
        MORNA_TRY(launch_lds(query_scores_kernel<128, 64, 2>, dim3(8u * ((n_rt + 7) / 8) * n_ct), dim3(MM16_THREADS), MM16_LDS, LDS_ALWAYS,
                             big_tiles > 0 ? st_rem : st_big, X16, N, h->dpad, im.q16, im.qrow, (int32_t)nb, scores, big_rows));
    }
    HIP_TRY(hipGetLastError());
    if (query_debug_open())   // which form took which rows: a test can see what it exercised
        fprintf(stderr, "[morna] query contraction: site=%s queries=%lld rows=%lld big_tiles=%lld rem_rows=%lld query_tiles=%lld %s\n", site,
                (long long)nb, (long long)N, (long long)big_tiles, (long long)(N - big_rows),
                (long long)(big_tiles > 0 ? (nb + 255) / 256 : (nb + MM16_TILE - 1) / MM16_TILE), im.qrow ? "by_item" : "by_vector");
    *big_rows_out = big_rows;
    return MORNA_OK;
}

// ---- traversal launches --------------------------------------------------------------------------------------------

// Root margins by query groups (query_roots_batch_kernel: a hyperplane fetched once per QR_Q queries) exist while the rows
// have a length its register forms are built for, its query images fit LDS and the roots do split.
static bool roots_by_groups_ok(const morna_index *h)
{
    return row_nv(h->dpad, 12) != 0 && h->n_items > h->K && (size_t)QR_Q * h->dpad * 4 <= 128 * 1024;
}

// ... of nb queries into P.pq; the caller has asked roots_by_groups_ok
static int launch_roots_by_groups(const QueryParams &P, int64_t nb, hipStream_t st)
{
    const dim3 grid((unsigned)((nb + QR_Q - 1) / QR_Q), (unsigned)((P.n_trees + QR_TREES - 1) / QR_TREES));
    const size_t ql = (size_t)QR_Q * P.dpad * 4;
    return with_row_nv<12>(P.dpad, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        if constexpr (NV != 0)   // (the kernel has no form without registers; roots_by_groups_ok keeps such rows away)
            MORNA_TRY(launch_lds(query_roots_batch_kernel<NV>, grid, dim3(QR_THREADS), ql, LDS_DEFAULT, st, P, (int32_t)nb));
        return MORNA_OK;
    });
}

// the best-first descent, one wave per query (query_descend_kernel; R: its restricted form), behind the root margins on st
static int launch_descents(const QueryPlan &pl, const QueryParams &P, const RestrictArgs *R, int64_t nb, hipStream_t st)
{
    return with_row_nv<32>(P.dpad, [&](auto nv) {
        return with_flag(pl.bm_lds, [&](auto bm) {
            constexpr int NV = decltype(nv)::value;
            constexpr bool BM = decltype(bm)::value;
            if (R) return launch_lds(query_descend_restricted_kernel<BM, NV>, dim3((unsigned)nb), dim3(WAVE), pl.lds_bm, LDS_1WAVE, st, P, *R);
            return launch_lds(query_descend_kernel<BM, NV>, dim3((unsigned)nb), dim3(WAVE), pl.lds_bm, LDS_1WAVE, st, P);
        });
    });
}

// ... of the sweep: one per virtual query
static int launch_sweep_descents(const QueryPlan &pl, const QueryParams &P, const SweepArgs &S, int64_t nv_queries, hipStream_t st)
{
    return with_row_nv<12>(P.dpad, [&](auto nv) {
        return with_flag(pl.bm_lds, [&](auto bm) {
            return launch_lds(query_descend_sweep_kernel<decltype(bm)::value, decltype(nv)::value>, dim3((unsigned)nv_queries), dim3(WAVE),
                              pl.lds_bm, LDS_1WAVE, st, P, S);
        });
    });
}

// the split traversal: root margins by query groups, then the one-wave descents
static int launch_split_traversal(const QueryPlan &pl, const QueryParams &P, const RestrictArgs *R, int64_t nb, hipStream_t st)
{
    MORNA_TRY(launch_roots_by_groups(P, nb, st));
    return launch_descents(pl, P, R, nb, st);
}

// the fused traversal, one workgroup per query: the query image in LDS, and the sample bitmap beside it when it fits
static int launch_fused_traversal(const QueryPlan &pl, const QueryParams &P, const RestrictArgs *R, int64_t nb, hipStream_t st)
{
    const size_t lds = pl.lds_q + pl.lds_bm;   // (can pass the default dynamic-LDS limit; the query image alone: up to 128 KiB past dpad 12288)
    return with_flag(pl.bm_lds, [&](auto bm) {
        constexpr bool BM = decltype(bm)::value;
        if (R) return launch_lds(query_traverse_restricted_kernel<BM>, dim3((unsigned)nb), dim3(Q_THREADS), lds, LDS_DEFAULT, st, P, *R);
        return launch_lds(query_traverse_kernel<BM>, dim3((unsigned)nb), dim3(Q_THREADS), lds, LDS_DEFAULT, st, P);
    });
}

// the refine step: no filter; the filter dots taken row by row (gather); the scores of the whole batch (dense)
static int launch_refine(const QueryPlan &pl, const QueryParams &P, bool dense, int64_t nb, hipStream_t st)
{
    auto go = [&](auto mode) {
        return launch_lds(query_refine_kernel<decltype(mode)::value>, dim3((unsigned)nb), dim3(Q_THREADS), pl.lds_q, LDS_DEFAULT, st, P);
    };
    if (!pl.use_filter) return go(std::integral_constant<int, 0>{});
    if (!dense) return go(std::integral_constant<int, 1>{});
    return go(std::integral_constant<int, 2>{});
}

// ---- query_batch ---------------------------------------------------------------------------------------------------

static QueryPlan plan_query(const morna_index *h, int64_t nq, int32_t k, int32_t search_k, int32_t T_used)
{
    QueryPlan pl = {};
    const int64_t N = h->n_items;
    pl.T_used = T_used;
    pl.search_k = search_k == -1 ? (int32_t)std::min<int64_t>((int64_t)k * T_used, INT32_MAX) : search_k;
    pl.cap = (int32_t)std::max<int64_t>(std::min<int64_t>(N, (int64_t)std::max(pl.search_k, 0) + h->K), 1);
    pl.bm_words = (int32_t)((N + 31) / 32);
    pl.lds_q = (size_t)h->dpad * sizeof(float);
    // the sample bitmap goes to LDS when it is at most 64 KiB and fits beside the query image (always, up to dpad 8192;
    // past it the 160 KiB of LDS decide, and the global bitmap takes over)
    pl.bm_lds = (size_t)pl.bm_words * 4 <= 64 * 1024 && pl.lds_q + (size_t)pl.bm_words * 4 <= Q_LDS_MAX;
    pl.lds_bm = pl.bm_lds ? (size_t)pl.bm_words * 4 : 0;
    const bool filter_pays = query_filter_on() && pl.cap > 4 * (int64_t)k;
    const bool batch_dense = filter_pays && query_dense_on() && dense_pays(h, pl.cap, nq);
    // (MORNA_QUERY_SPREAD=0, read per call: one workgroup per query)
    pl.spread = env_on("MORNA_QUERY_SPREAD") && nq < 64 && !batch_dense;
    pl.use_filter = !pl.spread && filter_pays;
    pl.may_dense = pl.use_filter && batch_dense;
    return pl;
}

// workspace bytes of one query, for the 1 GiB rule; n_nodes 0: without the per-node term
static size_t query_bytes(const morna_index *h, const QueryPlan &pl, int32_t k, bool by_vector, int64_t n_nodes)
{
    return (size_t)n_nodes * 8 + (size_t)pl.cap * 16 + (by_vector ? (size_t)h->dpad * 6 + 16 : 0) +
           (pl.bm_lds ? 0 : (size_t)pl.bm_words * 4) + (size_t)k * 8 + 16 + (pl.may_dense ? (size_t)h->n_items * 4 : 0);
}

// ---- The first batch beside a pending build (a build that returned with its last narrow levels pending, forest.hip).  What
// does not depend on the forest -- the item ids or query vectors, their fp16 image, both contraction launches -- goes onto
// stream3, behind ev_tail (recorded in front of the deferred attempt: the wide levels and the fp16 rows are done, the tail's
// own kernels are not waited for).  Not stream2: a tail attempt in the matrix-core form puts its side work there and would
// queue behind the contraction.  Everything these kernels read or write lies in h->q_early, sized and placed now: h->ws is
// sized from n_nodes, which only the finished tail knows, and may move when it grows.  Nothing of the build uses q_early.
// Then the tail is finished; root margins and descents follow it on h->stream; the refine step joins both.
struct EarlyContraction {
    bool live = false;      // the batch reads its queries and scores from `in`
    QueryInputs in = {};    // in h->q_early
    int64_t big_rows = 0;

    // Decided here and nowhere else: the build is pending, the call is a plain one with its answers wanted on the host and no
    // timer on it, and its plan is the dense one with all queries in one batch whatever n_nodes turns out to be.  (Only
    // abandon() below takes it back, when the finished forest says otherwise.)
    static bool wanted(const morna_index *h, bool by_vector, int64_t nq, int32_t k, int32_t search_k, const int32_t *ids_out,
                       const int32_t *packed_dev, const morna_restriction *rst, int32_t n_trees_used)
    {
        const bool timed = h->timing && (h->timing_mask & ((1u << MORNA_T_QUERY) | (1u << MORNA_T_QUERY_FILTER)));
        if (!(h->fb.pending && !rst && !packed_dev && n_trees_used == 0 && ids_out && !timed && h->half.valid && k > 0 && nq > 0 &&
              h->dpad <= Q_MAX_DPAD))
            return false;
        const QueryPlan pl = plan_query(h, nq, k, search_k, h->n_trees);
        return pl.may_dense && nq <= (int64_t)(((size_t)1 << 30) / query_bytes(h, pl, k, by_vector, 0));
    }

    int start(morna_index *h, const float *q_host, int64_t q_stride, const int32_t *items_host, int64_t nq)
    {
        MORNA_TRY(carve_workspace(h->q_early, [&](Carver &c) { in.carve(c, h, nq, q_host != nullptr, true, true); }));
        hipStream_t s3 = h->stream3;
        HIP_TRY(hipStreamWaitEvent(s3, h->ev_tail, 0));
        MORNA_TRY(stage_queries(h, in, q_host, q_stride, items_host, 0, nq, s3));
        HalfImage im;
        MORNA_TRY(half_image(h, in, q_host != nullptr, nq, true, s3, im));
        HIP_TRY(hipEventRecord(h->ev_early_in, s3));   // the traversal reads the ids / vectors too
        MORNA_TRY(launch_contraction(h, nq, im, in.scores, s3, s3, true, &big_rows, "early"));
        HIP_TRY(hipEventRecord(h->ev_early_out, s3));
        const int rc = finish_build(h, "query_batch, beside its contraction");
        if (rc != MORNA_OK) {
            (void)hipStreamSynchronize(s3);
            return rc;
        }
        live = true;
        return MORNA_OK;
    }

    // the finished forest has so many nodes that the queries go in several batches: the scores are not used (the same
    // kernels make them again, batch by batch)
    int abandon(morna_index *h)
    {
        HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_early_out, 0));
        live = false;
        return MORNA_OK;
    }
};

// A few query vectors from host memory (spread form): padded on the host into page-locked memory and sent as ONE copy (a
// memset + a 2-D copy out of pageable memory are two stream operations of ~10 us each).  *staged: q_host was host memory.
static int stage_queries_pinned(morna_index *h, float *Qd, const float *q_host, int64_t q_stride, int64_t nb, bool *staged)
{
    hipPointerAttribute_t at;
    const bool on_host = hipPointerGetAttributes(&at, q_host) != hipSuccess || at.type == hipMemoryTypeHost ||
                         at.type == hipMemoryTypeUnregistered;
    (void)hipGetLastError();   // (an unregistered host pointer reports an error on some runtimes)
    *staged = on_host;
    if (!on_host) return MORNA_OK;
    const size_t need = (size_t)nb * h->dpad * 4;
    MORNA_TRY(h->host_q.reserve(need));
    float *hq = (float *)h->host_q.p;
    for (int64_t i = 0; i < nb; i++) {
        memcpy(hq + i * h->dpad, q_host + i * q_stride, (size_t)h->dim * 4);
        memset(hq + i * h->dpad + h->dim, 0, (size_t)(h->dpad - h->dim) * 4);
    }
    HIP_TRY(hipMemcpyAsync(Qd, hq, need, hipMemcpyHostToDevice, h->stream));
    return MORNA_OK;
}

// q_host: query vectors in host OR device memory (unified addressing), q_stride floats apart (0 = dim)
// rst (or null): the restriction of the call, q_group_host [nq] (or null) the queries' own groups (morna_hip.h, "restricted
// search"); only the traversal kernels differ, every kernel behind them reads candidate lists.
int query_batch(morna_index *h, const float *q_host, int64_t q_stride, const int32_t *items_host, int64_t nq, int32_t k,
                int32_t search_k, int32_t *ids_out, float *dist_out, int32_t *count_out, int32_t *packed_dev, int64_t id_offset,
                const morna_restriction *rst, const int32_t *q_group_host, int32_t n_trees_used)
{
    if (q_stride <= 0) q_stride = h->dim;
    const bool by_vector = q_host != nullptr;
    // ---- check.  A pending build is finished first thing, unless the first batch's contraction is to start beside it.
    const bool beside_build = EarlyContraction::wanted(h, by_vector, nq, k, search_k, ids_out, packed_dev, rst, n_trees_used);
    if (!beside_build) {
        MORNA_TRY(finish_build(h, "query_batch"));
        MORNA_TRY(require_built(h));
    }
    MORNA_TRY(check_search_call(h, "get_nns", k, nq));
    if (rst) MORNA_TRY(restriction_usable(h, rst));
    if (n_trees_used != 0) MORNA_TRY(check_tree_count(h, "get_nns", n_trees_used));
    if (nq == 0) return MORNA_OK;
    if (items_host) MORNA_TRY(check_items(h, items_host, nq));

    // ---- plan, and the early contraction (it finishes the build)
    QueryPlan pl = plan_query(h, nq, k, search_k, n_trees_used ? n_trees_used : h->n_trees);
    EarlyContraction early;
    if (beside_build) MORNA_TRY(early.start(h, q_host, q_stride, items_host, nq));
    pl.batch = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(((size_t)1 << 30) / query_bytes(h, pl, k, by_vector, h->n_nodes))));
    if (early.live && pl.batch != nq) MORNA_TRY(early.abandon(h));

    // ---- the workspace, one slice per query of a batch: bound once, every batch uses the same slices
    const int64_t N = h->n_items;
    const bool q_groups = rst && rst->has_group && q_group_host;
    MORNA_TRY(h->d_stat.alloc(4));
    QueryParams W = base_params(h, pl, k);
    QueryInputs ws_in;
    int32_t *d_qg = nullptr;
    size_t out0 = 0, s_ids = 0, out_bytes = 0;
    MORNA_TRY(carve_workspace(h->ws, [&](Carver &c) {
        const size_t b = (size_t)pl.batch;
        W.pq = c.take<uint64_t>(b * h->n_nodes);
        W.keys = c.take<uint64_t>(b * pl.cap);
        W.qpp = c.take<float>(b);
        W.ncand = c.take<int32_t>(b);
        W.cand_off = c.take<int64_t>(b);
        W.cand = c.take<int32_t>(b * pl.cap);
        W.low = c.take<float>(b * pl.cap);
        W.bm_global = c.take<uint32_t>(pl.bm_lds ? 0 : b * pl.bm_words);
        ws_in.carve(c, h, pl.batch, by_vector, pl.may_dense, pl.may_dense && !early.live);
        d_qg = c.take<int32_t>(q_groups ? b : 0);
        out0 = c.used;   // ids, distances, counts: one block, one copy to the host
        W.ids_out = c.take<int32_t>(b * k);
        s_ids = c.used - out0;
        W.dist_out = c.take<float>(b * k);
        W.count_out = c.take<int32_t>(b);
        out_bytes = c.used - out0;
    }));
    const uint8_t *const out_block = (const uint8_t *)W.ids_out;
    W.zero_copy = pl.spread && !rst ? 1 : 0;   // (a restricted call never takes a leaf's slice of perm as its candidates)
    if (pl.use_filter) {
        MORNA_TRY(split_mm_prepare_rows(h, h->stream));
        set_filter_rows(h, W);
    }
    const QueryInputs &in = early.live ? early.in : ws_in;   // (early: one batch, q0 == 0 and nb == nq)
    const RestrictArgs R = restrict_args(rst, q_groups ? d_qg : nullptr);
    const RestrictArgs *const Rp = rst ? &R : nullptr;
    // spread form, answers wanted on the host: the last kernel writes them straight into page-locked memory of the handle
    // (a copy out of HBM is another ~8 us operation on the stream for 160 bytes per query), and the batch ends with a host wait
    const bool direct = pl.spread && ids_out && !packed_dev;
    if (direct) {
        MORNA_TRY(h->host_small.reserve(out_bytes));
        uint8_t *dp = (uint8_t *)h->host_small.dev();
        if (!dp) {
            set_error("query: the answer staging is not visible to the device");
            return MORNA_E_HIP;
        }
        W.ids_out = (int32_t *)dp;
        W.dist_out = (float *)(dp + s_ids);
        W.count_out = (int32_t *)(dp + 2 * s_ids);
    }

    for (int64_t q0 = 0; q0 < nq; q0 += pl.batch) {
        const int64_t nb = std::min(pl.batch, nq - q0);
        const bool dense = pl.may_dense && dense_pays(h, pl.cap, nb);
        QueryParams P = W;
        // ---- stage the queries
        if (q_groups) HIP_TRY(hipMemcpyAsync(d_qg, q_group_host + q0, (size_t)nb * 4, hipMemcpyHostToDevice, h->stream));
        if (pl.spread && !by_vector && nb <= 16) {   // the item numbers travel with the launch
            P.n_inline = (int32_t)nb;
            for (int64_t i = 0; i < nb; i++) P.inline_items[i] = items_host[q0 + i];
        } else {
            if (early.live) {   // in place since stream3's copies; whatever reads them on h->stream comes behind those
                HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_early_in, 0));
            } else {
                bool staged = false;
                if (by_vector && direct) MORNA_TRY(stage_queries_pinned(h, in.Q, q_host + q0 * q_stride, q_stride, nb, &staged));
                if (!staged) MORNA_TRY(stage_queries(h, in, q_host, q_stride, items_host, q0, nb, h->stream));
            }
            if (by_vector) P.Q = in.Q;
            else P.items = in.items;
        }
        // ---- traverse and refine
        if (pl.spread) {
            // a batch too small to fill the chip with one workgroup per query: each query's work is dealt out (kernels above)
            ScopedTimer tm(h, MORNA_T_QUERY, 0);
            hipLaunchKernelGGL(query_roots_kernel, dim3((unsigned)((pl.T_used + Q_WAVES - 1) / Q_WAVES), (unsigned)nb), dim3(Q_THREADS), 0,
                               h->stream, P);
            MORNA_TRY(launch_descents(pl, P, Rp, nb, h->stream));
#ifdef MORNA_DESCEND_PROBE
            {
                float probe[40];
                HIP_TRY(hipStreamSynchronize(h->stream));
                HIP_TRY(hipMemcpy(probe, P.low + 2 * nb + 16, sizeof(probe), hipMemcpyDeviceToHost));
                fprintf(stderr, "[descend probe] cycles:");
                for (int i = 1; i < (int)probe[0] && i < 40; i++) fprintf(stderr, " %.0f", probe[i]);
                fprintf(stderr, "\n");
            }
#endif
            hipLaunchKernelGGL(query_cand_dots_kernel, dim3((unsigned)((pl.cap + Q_WAVES * QS_CPW - 1) / (Q_WAVES * QS_CPW)), (unsigned)nb),
                               dim3(Q_THREADS), 0, h->stream, P);
            hipLaunchKernelGGL(query_topk_kernel, dim3((unsigned)nb), dim3(Q_THREADS), 0, h->stream, P);
        } else {
            // algorithmic bytes = 4*D*(hyperplane dots + unique candidates + 1) per
            // query; the kernel counts them into d_stat[0], resolve_timers() prices them
            ScopedTimer tm(h, MORNA_T_QUERY, 0);
            if (dense) {
                HalfImage im;
                MORNA_TRY(half_image(h, in, by_vector, nb, !early.live, h->stream, im));
                P.qn16 = im.qn16; P.qe16 = im.qe16; P.qscale = im.qscale;
                if (early.live) {   // enqueued on stream3 before the tail was finished
                    P.big_rows = early.big_rows;
                } else {
                    HIP_TRY(hipEventRecord(h->ev_fork, h->stream));   // the query vectors (and their fp16 image) / item ids are in place
                    HIP_TRY(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
                    ScopedTimer tf(h, MORNA_T_QUERY_FILTER, 2 * (int64_t)nb * N * h->dpad);   // "bytes" = executed flops
                    MORNA_TRY(launch_contraction(h, nb, im, in.scores, h->stream, h->stream2, true, &P.big_rows, "query_batch"));
                }
                if (P.big_rows > 0) P.eacc_big = (4.f * (float)h->dpad + 2.f) * 5.9604645e-8f + 4.1e-6f;   // EACC for ONE chain of dpad products
                P.scores = in.scores;
            }
            // beside the contraction (matrix cores, LDS) the traversal is a latency chain on one wave per query: it
            // runs on the side stream and the refine step waits for both
            // (forked above, before the contraction was enqueued; a batch that started beside a pending build: the
            // contraction is on stream3 and the traversal follows the tail on the main stream)
            const bool forked = dense && !early.live;
            hipStream_t ts = forked ? h->stream2 : h->stream;
            // the split traversal where it exists; otherwise (and with MORNA_QUERY_SPLIT_TRAVERSE=0, read per call) the fused kernel
            if (roots_by_groups_ok(h) && env_on("MORNA_QUERY_SPLIT_TRAVERSE")) MORNA_TRY(launch_split_traversal(pl, P, Rp, nb, ts));
            else MORNA_TRY(launch_fused_traversal(pl, P, Rp, nb, ts));
            if (early.live) {
                HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_early_out, 0));
            } else if (forked) {
                HIP_TRY(hipEventRecord(h->ev_join, h->stream2));
                HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
            }
            const bool count_refine = dense && query_debug_open();
            if (count_refine) {
                P.refine_stat = h->d_stat.p + 2;
                HIP_TRY(hipMemsetAsync(P.refine_stat, 0, sizeof(unsigned long long), h->stream));
            }
            MORNA_TRY(launch_refine(pl, P, dense, nb, h->stream));
            if (count_refine) {   // costs a synchronisation, measurement only
                unsigned long long packed = 0;
                HIP_TRY(hipStreamSynchronize(h->stream));
                HIP_TRY(hipMemcpy(&packed, P.refine_stat, sizeof(packed), hipMemcpyDeviceToHost));
                fprintf(stderr, "[morna] query refine: queries=%lld candidates=%llu survivors=%llu\n", (long long)nb, packed >> 32,
                        packed & 0xffffffffull);
            }
        }
        HIP_TRY(hipGetLastError());
        // ---- deliver
        if (packed_dev) {
            // row-sharded search: the answers stay in HBM, packed as the message of the top-k all-gather
            hipLaunchKernelGGL(pack_topk_kernel, dim3((unsigned)((nb * k + 255) / 256)), dim3(256), 0, h->stream, P.ids_out,
                               P.dist_out, nb * k, k, (int32_t)id_offset, packed_dev + q0 * 2 * k);
            HIP_TRY(hipGetLastError());
        }
        if (direct) {
            HIP_TRY(hipStreamSynchronize(h->stream));
            memcpy(ids_out + q0 * k, h->host_small.p, (size_t)nb * k * 4);
            if (dist_out) memcpy(dist_out + q0 * k, h->host_small.p + s_ids, (size_t)nb * k * 4);
            if (count_out) memcpy(count_out + q0, h->host_small.p + 2 * s_ids, (size_t)nb * 4);
        } else if (ids_out) {
            // one copy of the whole result block into page-locked memory of the handle (three copies into the caller's
            // pageable arrays cost ~25 us of idle device each), then plain memcpys
            MORNA_TRY(fetch_results(h, out_block, out_bytes, s_ids, s_ids, 4, nb, k, ids_out + q0 * k,
                                    dist_out ? dist_out + q0 * k : nullptr, count_out ? count_out + q0 : nullptr));
        }
        // (packed answers only: nothing to wait for -- the next batch, and whatever the caller orders on the handle's
        // stream, run behind this one)
    }
    return MORNA_OK;
}

// ---- sweep: every (tree count, search_k) cell of a grid from one forest (morna_hip.h, "search sweep") ----------------
// Per batch: the queries staged once, the root margins once at the largest tree count; per virtual query (query, tree
// count) one one-wave descent to the largest search_k that records where every smaller search_k stops; the canonical dot
// of every candidate of the deepest lists once -- for a batch that query_batch's dense_pays rule sends through the
// whole-batch contraction, only of the candidates the fp16 filter of some cell lets through --; per cell the k smallest
// keys of its prefix.

static int check_sweep_lists(const int32_t *trees, int32_t n_t, const int32_t *search_ks, int32_t n_s)
{
    if (!trees || !search_ks || n_t < 1 || n_s < 1 || n_t > SWEEP_MAX_LIST || n_s > SWEEP_MAX_LIST) {
        set_error("search_sweep: %d tree counts and %d search_k values given, each list holds 1 to %d", n_t, n_s, SWEEP_MAX_LIST);
        return MORNA_E_INVALID;
    }
    for (int i = 0; i < n_t; i++)
        if (trees[i] < 1 || (i > 0 && trees[i] <= trees[i - 1])) {
            set_error("search_sweep: tree counts must be positive and strictly ascending (entry %d is %d)", i, trees[i]);
            return MORNA_E_INVALID;
        }
    for (int j = 0; j < n_s; j++)
        if (search_ks[j] < 1 || (j > 0 && search_ks[j] <= search_ks[j - 1])) {
            set_error("search_sweep: search_k values must be positive and strictly ascending (entry %d is %d)", j, search_ks[j]);
            return MORNA_E_INVALID;
        }
    return MORNA_OK;
}

// the plan of the deepest cell: every cell's own candidate bound is below its
static QueryPlan plan_sweep(const morna_index *h, bool by_vector, int64_t nq, int32_t k, int32_t T_max, int32_t s_max, int32_t n_t,
                            int32_t n_s)
{
    QueryPlan pl = {};
    const int64_t N = h->n_items, n_cells = (int64_t)n_t * n_s;
    pl.T_used = T_max;
    pl.search_k = s_max;
    pl.cap = (int32_t)std::max<int64_t>(std::min<int64_t>(N, (int64_t)s_max + h->K), 1);
    pl.bm_words = (int32_t)((N + 31) / 32);
    pl.lds_q = (size_t)h->dpad * sizeof(float);
    pl.bm_lds = (size_t)pl.bm_words * 4 <= 64 * 1024;   // (nothing else of the descents is in dynamic LDS)
    pl.lds_bm = pl.bm_lds ? (size_t)pl.bm_words * 4 : 0;
    // the fp16 filter through ONE whole-batch contraction, by query_batch's rule for a batch (MORNA_SWEEP_FILTER=0, read per
    // call: canonical dots for every candidate of the deepest lists, as the small batches take them)
    const bool sweep_filter_on = env_on("MORNA_SWEEP_FILTER");
    pl.may_dense = query_filter_on() && query_dense_on() && sweep_filter_on && pl.cap > 4 * (int64_t)k && dense_pays(h, pl.cap, nq);
    pl.use_filter = pl.may_dense;
    // the 1 GiB workspace rule of query_batch; the unit is a query with its n_t virtual queries and n_t * n_s cells
    const size_t per_v = (size_t)h->n_nodes * 8 + (size_t)pl.cap * (pl.may_dense ? 24 : 12) + 16 + (pl.bm_lds ? 0 : (size_t)pl.bm_words * 4);
    const size_t per_c = (size_t)k * 8 + 20;
    const size_t per_q = (size_t)h->n_nodes * 8 + (by_vector ? (size_t)h->dpad * 6 + 16 : 0) + 16 + (size_t)k * 4 + per_v * n_t +
                         per_c * n_cells + (pl.may_dense ? (size_t)N * 4 : 0);
    pl.batch = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nq, 32768), (int64_t)(((size_t)1 << 30) / per_q)));
    return pl;
}

// ex_ids_host [nq][k] / ex_count_host [nq] with hits_out: the exact answers of the same queries, for the recall count.
// q_host: query vectors in host OR device memory, q_stride floats apart (0 = dim), as query_batch takes them.
int search_sweep(morna_index *h, const float *q_host, int64_t q_stride, const int32_t *items_host, int64_t nq, int32_t k,
                 const int32_t *trees, int32_t n_t, const int32_t *search_ks, int32_t n_s, int32_t *ids_out, float *dist_out,
                 int32_t *count_out, int32_t *ncand_out, int32_t *ndots_out, const int32_t *ex_ids_host,
                 const int32_t *ex_count_host, int32_t *hits_out)
{
    // ---- check
    MORNA_TRY(finish_build(h, "search_sweep"));   // (reads the node tables the tail of a pending build writes)
    if (q_stride <= 0) q_stride = h->dim;
    const bool by_vector = q_host != nullptr;
    h->sweep_stats[0] = h->sweep_stats[1] = h->sweep_stats[2] = h->sweep_stats[3] = 0.0;
    MORNA_TRY(require_built(h));
    MORNA_TRY(check_search_call(h, "search_sweep", k, nq));
    MORNA_TRY(check_sweep_lists(trees, n_t, search_ks, n_s));
    MORNA_TRY(check_tree_count(h, "search_sweep", trees[n_t - 1]));
    if (nq == 0) return MORNA_OK;
    if (items_host) MORNA_TRY(check_items(h, items_host, nq));

    // ---- plan
    const int64_t N = h->n_items, n_cells = (int64_t)n_t * n_s;
    const bool want_hits = hits_out && ex_ids_host && ex_count_host;
    const QueryPlan pl = plan_sweep(h, by_vector, nq, k, trees[n_t - 1], search_ks[n_s - 1], n_t, n_s);
    SweepArgs S;
    S.n_t = n_t; S.n_s = n_s;
    for (int i = 0; i < SWEEP_MAX_LIST; i++) {
        S.trees[i] = i < n_t ? trees[i] : 0;
        S.search_ks[i] = i < n_s ? search_ks[i] : 0;
    }
    // ---- the workspace, bound once: slices per query (b), per virtual query (bv) and per cell (bc) of a batch
    MORNA_TRY(h->d_stat.alloc(4));
    QueryParams W = base_params(h, pl, k);
    QueryInputs in;
    uint64_t *root_pq = nullptr, *d_ub = nullptr;
    int32_t *d_exc = nullptr, *d_exi = nullptr, *d_hits = nullptr;
    float *d_thr = nullptr;
    size_t out0 = 0, s_ids = 0, s_cf = 0, out_bytes = 0;
    MORNA_TRY(carve_workspace(h->ws, [&](Carver &c) {
        const size_t b = (size_t)pl.batch, bv = b * n_t, bc = bv * n_s;
        root_pq = c.take<uint64_t>(b * h->n_nodes);   // the root margins at the largest tree count
        W.qpp = c.take<float>(b);
        in.carve(c, h, pl.batch, by_vector, pl.may_dense, pl.may_dense);
        d_exc = c.take<int32_t>(b);
        d_exi = c.take<int32_t>(want_hits ? b * k : 0);
        W.pq = c.take<uint64_t>(bv * h->n_nodes);
        W.keys = c.take<uint64_t>(bv * pl.cap);
        W.cand = c.take<int32_t>(bv * pl.cap);
        W.ncand = c.take<int32_t>(bv);
        W.cand_off = c.take<int64_t>(bv);
        W.bm_global = c.take<uint32_t>(pl.bm_lds ? 0 : bv * pl.bm_words);
        d_ub = c.take<uint64_t>(pl.may_dense ? bv * pl.cap : 0);
        W.low = pl.may_dense ? c.take<float>(bv * pl.cap) : nullptr;
        out0 = c.used;   // ids, distances, counts, ncand, ndots, hits of the batch's cells: one block, one copy to the host
        W.ids_out = c.take<int32_t>(bc * k);
        s_ids = c.used - out0;
        W.dist_out = c.take<float>(bc * k);
        W.count_out = c.take<int32_t>(bc);
        s_cf = c.used - out0 - 2 * s_ids;
        S.cell_ncand = c.take<int32_t>(bc);
        S.cell_ndots = c.take<int32_t>(bc);
        d_hits = c.take<int32_t>(bc);
        out_bytes = c.used - out0;
        d_thr = c.take<float>(bc);   // (behind the block that goes to the host)
    }));
    S.root_pq = root_pq;
    if (pl.may_dense) MORNA_TRY(split_mm_prepare_rows(h, h->stream));
    MORNA_TRY(h->host_out.reserve(out_bytes));

    bool contraction_ran = false;
    double descents = 0, rows_dots = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += pl.batch) {
        const int64_t nb = std::min(pl.batch, nq - q0);
        const int64_t nv = nb * n_t, nc = nb * n_cells;
        const bool dense = pl.may_dense && dense_pays(h, pl.cap, nb);
        QueryParams P = W;
        S.nq = (int32_t)nb;
        // ---- stage the queries, and the exact answers
        MORNA_TRY(stage_queries(h, in, q_host, q_stride, items_host, q0, nb, h->stream));
        if (by_vector) P.Q = in.Q;
        else P.items = in.items;
        if (want_hits) {
            HIP_TRY(hipMemcpyAsync(d_exi, ex_ids_host + q0 * k, (size_t)nb * k * 4, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(d_exc, ex_count_host + q0, (size_t)nb * 4, hipMemcpyHostToDevice, h->stream));
        }
        {
            ScopedTimer tm(h, MORNA_T_QUERY, 0);
            // ---- traverse: root margins and the queries' norms, once, for the largest tree count; one descent per virtual query
            QueryParams PR = P;
            PR.pq = root_pq;
            if (nb >= 64 && roots_by_groups_ok(h))
                MORNA_TRY(launch_roots_by_groups(PR, nb, h->stream));
            else
                hipLaunchKernelGGL(query_roots_kernel, dim3((unsigned)((pl.T_used + Q_WAVES - 1) / Q_WAVES), (unsigned)nb), dim3(Q_THREADS), 0,
                                   h->stream, PR);
            MORNA_TRY(launch_sweep_descents(pl, P, S, nv, h->stream));
            // ---- refine
            const int32_t bpv = (pl.cap + Q_WAVES - 1) / Q_WAVES;
            if (dense) {
                // the contraction of the batch's queries against all rows, once (the 128 x 128 form for every row), and from
                // it the bounds of every virtual query's candidates and every cell's threshold
                set_filter_rows(h, P);
                HalfImage im;
                MORNA_TRY(half_image(h, in, by_vector, nb, true, h->stream, im));
                P.qn16 = im.qn16; P.qe16 = im.qe16; P.qscale = im.qscale;
                {
                    ScopedTimer tf(h, MORNA_T_QUERY_FILTER, 2 * (int64_t)nb * N * h->dpad);   // "bytes" = executed flops
                    MORNA_TRY(launch_contraction(h, nb, im, in.scores, h->stream, h->stream, false, &P.big_rows, "sweep"));
                }
                P.scores = in.scores;
                contraction_ran = true;
                hipLaunchKernelGGL(sweep_bounds_kernel, dim3((unsigned)nv), dim3(Q_THREADS), 0, h->stream, P, (int32_t)nb, d_ub);
                hipLaunchKernelGGL(sweep_threshold_kernel, dim3((unsigned)nc), dim3(Q_THREADS), 0, h->stream, P, n_s, (int32_t)nb,
                                   S.cell_ncand, d_ub, d_thr);
                HIP_TRY(hipMemsetAsync(h->d_stat.p + 3, 0, sizeof(unsigned long long), h->stream));
                hipLaunchKernelGGL(sweep_cand_dots_kernel<true>, dim3((unsigned)(nv * bpv)), dim3(Q_THREADS), 0, h->stream, P, (int32_t)nb,
                                   bpv, n_s, S.cell_ncand, d_thr);
            } else {
                hipLaunchKernelGGL(sweep_cand_dots_kernel<false>, dim3((unsigned)(nv * bpv)), dim3(Q_THREADS), 0, h->stream, P, (int32_t)nb,
                                   bpv, n_s, S.cell_ncand, d_thr);
            }
            hipLaunchKernelGGL(sweep_topk_kernel, dim3((unsigned)nc), dim3(Q_THREADS), 0, h->stream, P, n_s, (int32_t)nb, S.cell_ncand);
            if (want_hits)
                hipLaunchKernelGGL(sweep_hits_kernel, dim3((unsigned)nc), dim3(WAVE), 0, h->stream, P.ids_out, P.count_out, d_exi,
                                   d_exc, (int32_t)nb, k, d_hits);
        }
        HIP_TRY(hipGetLastError());
        // ---- deliver: the batch's block is [cell][nb]; the caller's arrays are [cell][nq]
        HIP_TRY(hipMemcpyAsync(h->host_out.p, W.ids_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->unsettled = false;
        const uint8_t *hb = h->host_out.p, *hc = hb + 2 * s_ids;
        const int32_t *b_ids = (const int32_t *)hb, *b_cnt = (const int32_t *)hc, *b_nc = (const int32_t *)(hc + s_cf),
                      *b_nd = (const int32_t *)(hc + 2 * s_cf), *b_hit = (const int32_t *)(hc + 3 * s_cf);
        const float *b_dist = (const float *)(hb + s_ids);
        for (int64_t c = 0; c < n_cells; c++) {
            const size_t row = (size_t)nb * 4;
            if (ids_out) memcpy(ids_out + (c * nq + q0) * k, b_ids + c * nb * k, row * k);
            if (dist_out) memcpy(dist_out + (c * nq + q0) * k, b_dist + c * nb * k, row * k);
            if (count_out) memcpy(count_out + c * nq + q0, b_cnt + c * nb, row);
            if (ncand_out) memcpy(ncand_out + c * nq + q0, b_nc + c * nb, row);
            if (ndots_out) memcpy(ndots_out + c * nq + q0, b_nd + c * nb, row);
            if (want_hits) memcpy(hits_out + c * nq + q0, b_hit + c * nb, row);
        }
        descents += (double)nv;
        if (dense) {   // the candidates that passed their filter
            unsigned long long kept = 0;
            HIP_TRY(hipMemcpy(&kept, h->d_stat.p + 3, sizeof(kept), hipMemcpyDeviceToHost));
            rows_dots += (double)kept;
        } else
        for (int64_t v = 0; v < nv; v++) {   // the deepest cell of every virtual query: the candidates that got a canonical dot
            const int64_t ti = v / nb, q = v - ti * nb;
            rows_dots += (double)std::min<int32_t>(b_nc[((ti * n_s) + (n_s - 1)) * nb + q], pl.cap);
        }
    }
    h->sweep_stats[0] = descents;
    h->sweep_stats[1] = (double)n_cells * (double)nq;
    h->sweep_stats[2] = rows_dots;
    h->sweep_stats[3] = contraction_ran ? 1.0 : 0.0;
    return MORNA_OK;
}

// ---- row-sharded search: merge of the all-gathered per-shard answers on the device ----------------------------
// gathered[world][nq][2 kk] int32: kk global ids (-1 = empty slot, always last) then the kk fp32 distances' bits, each
// list ascending by (distance, id) as the refine kernel leaves it.  One thread per query walks the `world` list heads.
__global__ __launch_bounds__(256) void merge_topk_kernel(const int32_t *__restrict__ gathered, int32_t world, int64_t nq,
                                                         int32_t kk, int32_t k, int32_t *__restrict__ ids_out,
                                                         float *__restrict__ dist_out, int32_t *__restrict__ count_out)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    constexpr int MAXW = 64;
    uint8_t head[MAXW];   // kk <= 255 checked by the host
    for (int w = 0; w < world; w++) head[w] = 0;
    int n = 0;
    for (; n < k; n++) {
        int best = -1;
        uint32_t bk = 0;
        int32_t bi = 0;
        for (int w = 0; w < world; w++) {
            if (head[w] >= kk) continue;
            const int32_t *lst = gathered + ((int64_t)w * nq + q) * 2 * kk;
            const int32_t id = lst[head[w]];
            if (id < 0) continue;   // the rest of this shard's list is empty
            const uint32_t dk = f32_orderable(__int_as_float(lst[kk + head[w]]));
            if (best < 0 || dk < bk || (dk == bk && id < bi)) {
                best = w;
                bk = dk;
                bi = id;
            }
        }
        if (best < 0) break;
        const int32_t *lst = gathered + ((int64_t)best * nq + q) * 2 * kk;
        ids_out[q * k + n] = lst[head[best]];
        dist_out[q * k + n] = __int_as_float(lst[kk + head[best]]);
        head[best]++;
    }
    count_out[q] = n;
    for (; n < k; n++) {
        ids_out[q * k + n] = -1;
        dist_out[q * k + n] = INFINITY;
    }
}

int merge_topk_dev(morna_index *h, const int32_t *gathered_dev, int32_t world, int64_t nq, int32_t kk, int32_t k,
                   int32_t *ids_out, float *dist_out, int32_t *count_out)
{
    MORNA_TRY(finish_build(h, "merge_topk_dev"));
    if (world <= 0 || world > 64 || nq < 0 || kk <= 0 || kk > 255 || k <= 0 || !gathered_dev || !ids_out) {
        set_error("merge_topk_dev: invalid argument (world <= 64, kk <= 255)");
        return MORNA_E_INVALID;
    }
    if (nq == 0) return MORNA_OK;
    const size_t s_ids = align_up((size_t)nq * k * 4, 256), s_cnt = align_up((size_t)nq * 4, 256);
    MORNA_TRY(h->ws.alloc(2 * s_ids + s_cnt));
    int32_t *d_ids = (int32_t *)h->ws.p;
    float *d_dist = (float *)(h->ws.p + s_ids);
    int32_t *d_cnt = (int32_t *)(h->ws.p + 2 * s_ids);
    hipLaunchKernelGGL(merge_topk_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, h->stream, gathered_dev, world, nq, kk,
                       k, d_ids, d_dist, d_cnt);
    HIP_TRY(hipGetLastError());
    // one copy of the result block into the handle's page-locked staging, then plain memcpys (as query_batch)
    return fetch_results(h, h->ws.p, 2 * s_ids + s_cnt, s_ids, s_ids, 4, nq, k, ids_out, dist_out, count_out);
}

}  // namespace morna
