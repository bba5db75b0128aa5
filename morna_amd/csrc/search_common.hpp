// search_common.hpp -- what the approximate searches (knn.hip) and the exact family (exact.hip) both use: the widest row,
// the restriction as the kernels take it, the workgroup-wide minimum, the workspace carver, the launch helpers and the HIP
// events behind a call's statistics (mixture.hip takes the last three too).
#pragma once
#include <cstdint>
#include <type_traits>

#include "common.hpp"
#include "devutil.hpp"

namespace morna {

#define Q_THREADS 256
#define Q_WAVES (Q_THREADS / WAVE)
#define Q_MAX_DPAD 32768            // widest row the searches take (the build's limit too)

// A restriction of one search call (include/morna_hip.h, "restricted search"): item i is eligible for query q iff its
// deny bit is clear and (g_q < 0 or group[i] != g_q).  Only the *_restricted_kernel forms take it.
struct RestrictArgs {
    const uint32_t *deny;      // [(n_items + 31) / 32] complement of the allow bitmap; the bits past n_items are SET
    const int32_t *group;      // [n_items] label of every item (negative: none), or null
    const int32_t *q_group;    // [nq] g_q of every query of the launch, or null: every g_q is -1
};

__device__ inline int32_t restrict_query_group(const RestrictArgs &R, int64_t qi)
{
    return R.group && R.q_group ? R.q_group[qi] : -1;
}

__device__ inline bool restrict_eligible(const RestrictArgs &R, int32_t gq, int64_t i)
{
    if ((R.deny[i >> 5] >> (i & 31)) & 1u) return false;
    return gq < 0 || R.group[i] != gq;
}

// block-wide min of a uint64 (all threads get the result)
__device__ inline uint64_t block_min_u64(uint64_t v, uint64_t *s_red, int tid)
{
    v = wave_min_u64(v);
    __syncthreads();
    if ((tid & (WAVE - 1)) == 0) s_red[tid / WAVE] = v;
    __syncthreads();
    uint64_t r = s_red[0];
#pragma unroll
    for (int i = 1; i < Q_WAVES; i++) r = s_red[i] < r ? s_red[i] : r;
    return r;
}

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// A restriction a search is about to use: made for this handle and for the rows it holds now.
static inline int restriction_usable(const morna_index *h, const morna_restriction *rst)
{
    if (rst->h != h) {
        set_error("the restriction was made for another index handle");
        return MORNA_E_INVALID;
    }
    if (rst->n_items != h->n_items) {
        set_error("the restriction was made for %lld items, the index now holds %lld: make it again", (long long)rst->n_items,
                  (long long)h->n_items);
        return MORNA_E_STATE;
    }
    return MORNA_OK;
}

// the restriction of a call as the *_restricted_kernel forms take it; q_group_dev [nq] or null: the queries' own groups
static inline RestrictArgs restrict_args(const morna_restriction *rst, const int32_t *q_group_dev)
{
    RestrictArgs R = {nullptr, nullptr, nullptr};
    if (rst) {
        R.deny = rst->deny.p;
        R.group = rst->has_group ? rst->group.p : nullptr;
        R.q_group = R.group ? q_group_dev : nullptr;
    }
    return R;
}

// f(std::true_type) or f(std::false_type): a run-time flag as a template argument
template <class F>
static inline int with_flag(bool b, F &&f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// A launch with `bytes` of dynamic LDS.  Above `limit` bytes the kernel's dynamic-LDS limit is raised first: LDS_1WAVE for
// the one-wave descents, LDS_DEFAULT elsewhere, LDS_ALWAYS for the contraction kernels, whose need is above either, LDS_64K
// for the vector-ALU scan of the exact family.  (Not raised more often than that: hipFuncSetAttribute is host time of the
// single-query path.)
#define LDS_1WAVE ((size_t)32 * 1024)
#define LDS_DEFAULT ((size_t)48 * 1024)
#define LDS_64K ((size_t)64 * 1024)
#define LDS_ALWAYS ((size_t)0)
template <class K, class... A>
static inline int launch_lds(K kernel, dim3 grid, dim3 block, size_t bytes, size_t limit, hipStream_t st, const A &...args)
{
    if (bytes > limit) HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(kernel, grid, block, bytes, st, args...);
    return MORNA_OK;
}

// A workspace described once: the same layout code runs over a null base, for the size, and over the allocation, for the
// pointers, so the two cannot disagree.  Every piece starts on a 256-byte boundary; a piece of no elements takes no room.
struct Carver {
    uint8_t *base;   // null: only the size is wanted
    size_t used = 0;
    template <class T>
    T *take(size_t count)
    {
        T *p = base ? (T *)(base + used) : nullptr;
        used += align_up(count * sizeof(T), 256);
        return p;
    }
};

// layout(Carver &) twice: sizes buf, then binds the pointers
template <class F>
static int carve_workspace(DevBuf<uint8_t> &buf, F &&layout)
{
    Carver size{nullptr};
    layout(size);
    MORNA_TRY(buf.alloc(size.used));
    Carver c{buf.p};
    layout(c);
    return MORNA_OK;
}

// The HIP events behind a call's own statistics (label_stats, radius_stats, mixture_stats), destroyed with the holder on every path.
struct HipEvents {
    std::vector<hipEvent_t> ev;
    ~HipEvents()
    {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    int create(int n)
    {
        for (int i = 0; i < n; i++) {
            hipEvent_t e = nullptr;
            HIP_TRY(hipEventCreate(&e));
            ev.push_back(e);
        }
        return MORNA_OK;
    }
    int record(int i, hipStream_t st)
    {
        HIP_TRY(hipEventRecord(ev[(size_t)i], st));
        return MORNA_OK;
    }
    // *ms += the time from event i to event j
    int elapsed(int i, int j, double *ms)
    {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ev[(size_t)i], ev[(size_t)j]));
        *ms += t;
        return MORNA_OK;
    }
};

}  // namespace morna
