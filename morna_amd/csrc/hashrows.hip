// hashrows.hip -- hashed rows of any width straight from the junction store.
//
// The store holds every sample's (line, coverage) list in ascending line order, which is file order, so a sample's hashed
// row at a width D is a function of its store row, the weights of morna_jstore_set_weights and one int32 hash per line
// (morna.py:370-388 and add_item's fp64 -> fp32): cell c = the terms sgn_j * RN(double(cov) * w[j]) of the entries with
// floormod(hash[j], D) == c and w[j] != 0, added in line order from +0.0, one rounding per operation, rounded once to fp32.
//   hash_cols_kernel   per line and call: its column at this width (-1: the line weighs nothing) and its signed weight
//                      (sgn * RN(cov * w) == RN(cov * (sgn * w)): a sign change is exact)
//   hash_rows_kernel   a workgroup per named row.  The row's fp64 cells sit in LDS (at most 16384 of them, 128 KiB: wider
//                      rows take a second pass over the row for the upper columns).  The row is streamed in chunks staged
//                      in LDS as (cell, term); every wave owns a share of the cells and adds the staged entries of its
//                      cells 64 at a time, the lanes that meet in one cell lowest lane first, so the terms of a cell are
//                      added in line order whatever the chunking (see the kernel).  The cells are rounded and written as
//                      float4.
// No floating-point atomics and nothing that depends on which workgroup or wave runs first: the bytes depend on
// (row, w, hash, D) alone.
#include <algorithm>
#include <cstring>
#include <vector>

#include "jstore.hpp"

using morna::DevBuf;
using morna::EventPair;
using morna::guarded;
using morna::set_error;

namespace {

#define HR_CHUNK 256          // the walk form: threads of a workgroup, and entries staged at once
#define HR_MAX_SPAN 16384     // fp64 cells of a row in LDS: 128 KiB of the 160
#define HR_MAX_DPAD 32768     // the widest row the build and the searches take
#define HR_TAGS 256           // the wave form: tag slots per wave
#define HR_WIDE_SPAN 8960     // the wave form: past this many cells one workgroup fits a CU, and it has 512 threads, not 256

__global__ __launch_bounds__(256) void hash_cols_kernel(const int32_t *__restrict__ hash, const double *__restrict__ w, int64_t n_lines,
                                                        int32_t D, int32_t *__restrict__ col, double *__restrict__ sw)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_lines) return;
    const int32_t h = hash[j];
    const double wj = w[j];
    int32_t m = h % D;   // (D >= 1: no overflow even for INT32_MIN)
    if (m < 0) m += D;   // Python's floored modulo
    col[j] = wj != 0.0 ? m : -1;
    sw[j] = h < 0 ? -wj : wj;   // the sign is the hash's, taken before the modulo
}

// entry e of the row as (cell of this column range | -1, term); the entries past the row's end are (-1, +0.0)
__device__ inline void hr_stage(const int32_t *__restrict__ line, const int32_t *__restrict__ cov, const int32_t *__restrict__ col,
                                const double *__restrict__ sw, int64_t e, int64_t b, int32_t lo, uint32_t span, int32_t *off_out,
                                double *term_out)
{
    int32_t off = -1;
    double term = 0.0;
    if (e < b) {
        const int32_t l = line[e];
        const int32_t c = col[l];
        const uint32_t o = (uint32_t)(c - lo);
        if (c >= 0 && o < span) {
            off = (int32_t)o;
            term = __dmul_rn((double)cov[e], sw[l]);
        }
    }
    *off_out = off;
    *term_out = term;
}

// the cells of a finished column range, rounded once, as whole float4 (the pad columns were never added to: +0.0)
__device__ inline void hr_write_out(const double *acc, uint32_t span, float *out, int tid, int threads)
{
    for (uint32_t c = (uint32_t)tid * 4; c < span; c += (uint32_t)threads * 4) {
        float4 v;
        v.x = __double2float_rn(acc[c]);
        v.y = __double2float_rn(acc[c + 1]);
        v.z = __double2float_rn(acc[c + 2]);
        v.w = __double2float_rn(acc[c + 3]);
        *(float4 *)(out + c) = v;
    }
}

// ---- the wave form (the default) ---------------------------------------------------------------------------------------------
// A workgroup per named row, THREADS / 64 waves.  Wave v owns the cells c with (c / 64) % WAVES == v, so two waves never touch
// one cell and a wave's LDS operations on its cells execute in program order.  A chunk of THREADS entries is staged in LDS as
// (cell, term), one barrier per chunk (two staging buffers); every wave then takes the chunk 64 entries at a time, a lane an
// entry, keeps the entries of its own cells and adds them IN LANE ORDER: each pending lane puts its lane number into the
// tag slot of its cell with an LDS minimum, the lane that finds its own number there adds its term and clears the slot, the
// others go round again.  Lanes of one cell share a slot, so they add lowest lane first, which is line order; lanes of
// different cells that share a slot only wait for each other.  A round retires at least the lowest pending lane of every
// slot: at most 64 rounds, one when no two entries meet.  Which lane wins depends on the lane numbers alone.
// LDS: acc[span_cap] doubles, term[2][THREADS] doubles, off[2][THREADS] int32, tag[WAVES][HR_TAGS] uint32.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void hash_rows_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                            const int32_t *__restrict__ cov, const int32_t *__restrict__ rows,
                                                            const int32_t *__restrict__ col, const double *__restrict__ sw,
                                                            int32_t dpad, int32_t span_cap, float *__restrict__ X)
{
    constexpr int WAVES = THREADS / WAVE;
    constexpr int WAVES_SHIFT = WAVES == 4 ? 2 : 3;
    static_assert(WAVES == 4 || WAVES == 8, "256 or 512 threads");
    extern __shared__ double4 hr_lds[];
    double *acc = (double *)hr_lds;
    double *s_term = acc + span_cap;
    int32_t *s_off = (int32_t *)(s_term + 2 * THREADS);
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    unsigned int *tag = (unsigned int *)(s_off + 2 * THREADS) + wave * HR_TAGS;
    for (int i = lane; i < HR_TAGS; i += WAVE) tag[i] = ~0u;   // (this wave's own: no barrier)
    const int32_t row = rows[blockIdx.x];
    const int64_t a = ptr[row], b = ptr[row + 1];
    float *out = X + (int64_t)blockIdx.x * dpad;
    int buf = 0;
    for (int32_t lo = 0; lo < dpad; lo += span_cap) {   // uniform over the workgroup
        const uint32_t span = (uint32_t)(dpad - lo < span_cap ? dpad - lo : span_cap);
        for (uint32_t c = tid; c < span; c += THREADS) acc[c] = 0.0;   // cells of this thread's wave
        for (int64_t e0 = a; e0 < b; e0 += THREADS, buf ^= 1) {
            hr_stage(line, cov, col, sw, e0 + tid, b, lo, span, &s_off[buf * THREADS + tid], &s_term[buf * THREADS + tid]);
            // One barrier per chunk: the staging buffer written next was last read before this barrier.
            __syncthreads();
            const int cnt = (int)(b - e0 < THREADS ? b - e0 : THREADS);
            for (int s = 0; s < cnt; s += WAVE) {
                const int32_t off = s_off[buf * THREADS + s + lane];
                const double term = s_term[buf * THREADS + s + lane];
                bool pending = off >= 0 && ((off >> 6) & (WAVES - 1)) == wave;
                unsigned int *slot = tag + ((off & 63) | (((off >> (6 + WAVES_SHIFT)) & (HR_TAGS / 64 - 1)) << 6));
                for (int round = 0; round < WAVE && __ballot(pending) != 0; round++) {
                    if (pending) atomicMin(slot, (unsigned int)lane);
                    if (pending && __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == (unsigned int)lane) {
                        acc[off] = __dadd_rn(acc[off], term);
                        __hip_atomic_store(slot, ~0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        pending = false;
                    }
                }
            }
        }
        __syncthreads();   // the write-out reads the cells of every wave
        hr_write_out(acc, span, out + lo, tid, THREADS);
        __syncthreads();   // before the next column range zeroes the cells
    }
}

// ---- the walk form (MORNA_HASHROWS_WALK=1) -----------------------------------------------------------------------------------
// Every thread walks the staged chunk in order and adds the entries of the cells it owns (cell mod 256 == thread): 256
// compares per thread and chunk.  The rows are the wave form's, byte for byte; kept as the form to measure it against.
__device__ inline void hr_add(double *acc, int32_t off, double term, int tid)
{
    if (off >= 0 && (off & (HR_CHUNK - 1)) == tid) acc[off] = __dadd_rn(acc[off], term);
}

// LDS: acc[span_cap] doubles, term[2][HR_CHUNK] doubles, off[2][HR_CHUNK] int32; span_cap = min(dpad, HR_MAX_SPAN), a multiple of 256
__global__ __launch_bounds__(HR_CHUNK) void hash_rows_walk_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                                  const int32_t *__restrict__ cov, const int32_t *__restrict__ rows,
                                                                  const int32_t *__restrict__ col, const double *__restrict__ sw,
                                                                  int32_t dpad, int32_t span_cap, float *__restrict__ X)
{
    extern __shared__ double4 hr_lds[];
    double *acc = (double *)hr_lds;
    double *s_term = acc + span_cap;
    int32_t *s_off = (int32_t *)(s_term + 2 * HR_CHUNK);
    const int tid = threadIdx.x;
    const int32_t row = rows[blockIdx.x];
    const int64_t a = ptr[row], b = ptr[row + 1];
    float *out = X + (int64_t)blockIdx.x * dpad;
    int buf = 0;
    for (int32_t lo = 0; lo < dpad; lo += span_cap) {   // uniform over the workgroup
        const uint32_t span = (uint32_t)(dpad - lo < span_cap ? dpad - lo : span_cap);
        for (uint32_t c = tid; c < span; c += HR_CHUNK) acc[c] = 0.0;   // the cells this thread owns
        for (int64_t e0 = a; e0 < b; e0 += HR_CHUNK, buf ^= 1) {
            hr_stage(line, cov, col, sw, e0 + tid, b, lo, span, &s_off[buf * HR_CHUNK + tid], &s_term[buf * HR_CHUNK + tid]);
            __syncthreads();   // (one per chunk, as above)
            const int cnt = (int)(b - e0 < HR_CHUNK ? b - e0 : HR_CHUNK);
            const int4 *o4 = (const int4 *)(s_off + buf * HR_CHUNK);
            const double *t = s_term + buf * HR_CHUNK;
            for (int j = 0; j < cnt; j += 4) {   // (the entries past cnt carry off = -1)
                const int4 o = o4[j >> 2];
                hr_add(acc, o.x, t[j], tid);
                hr_add(acc, o.y, t[j + 1], tid);
                hr_add(acc, o.z, t[j + 2], tid);
                hr_add(acc, o.w, t[j + 3], tid);
            }
        }
        __syncthreads();   // the write-out reads the cells of four owners
        hr_write_out(acc, span, out + lo, tid, HR_CHUNK);
        __syncthreads();   // before the next column range zeroes the cells
    }
}

int hash_rows_impl(morna_index *h, morna_jstore *s, const int64_t *ext, int64_t n, const int32_t *line_hash)
{
    const int64_t n_lines = s->n_lines;
    std::vector<int32_t> rows((size_t)n);
    int64_t entries = 0;
    for (int64_t i = 0; i < n; i++) {
        auto it = s->row_of.find(ext[i]);
        if (it == s->row_of.end()) {
            set_error("add_items_from_store: sample id %lld (entry %lld) is not in the junction store", (long long)ext[i], (long long)i);
            return MORNA_E_RANGE;
        }
        rows[(size_t)i] = it->second;
        entries += s->ptr[(size_t)it->second + 1] - s->ptr[(size_t)it->second];
    }
    if (n <= 0) {
        set_error("no internal ids were assigned: no sample passes the sample threshold");
        return MORNA_E_EMPTY;
    }
    if (h->dpad > HR_MAX_DPAD) {
        set_error("build: dimension %d is above the supported %d", h->dim, HR_MAX_DPAD);
        return MORNA_E_INVALID;
    }
    // ---- the checks are done: GPU work from here
    HIP_TRY(hipSetDevice(h->device));
    MORNA_TRY(morna::settle(h));
    MORNA_TRY(morna::jstore_make_resident(s));
    const double *d_w = nullptr;
    MORNA_TRY(morna::jstore_device_weights(s, &d_w));
    const bool same_hash = s->hr_hash_resident && (int64_t)s->hr_hash.size() == n_lines &&
                           (n_lines == 0 || memcmp(s->hr_hash.data(), line_hash, (size_t)n_lines * sizeof(int32_t)) == 0);
    if (!same_hash) {
        s->hr_hash_resident = false;
        MORNA_TRY(s->d_hr_hash.alloc((size_t)n_lines));
        if (n_lines > 0) HIP_TRY(hipMemcpy(s->d_hr_hash.p, line_hash, (size_t)n_lines * sizeof(int32_t), hipMemcpyHostToDevice));
        s->hr_hash.assign(line_hash, line_hash + n_lines);
        s->hr_hash_resident = true;
    }
    MORNA_TRY(s->d_hr_col.alloc((size_t)n_lines));
    MORNA_TRY(s->d_hr_sw.alloc((size_t)n_lines));
    MORNA_TRY(s->d_hr_rows.alloc((size_t)n));
    HIP_TRY(hipMemcpy(s->d_hr_rows.p, rows.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    MORNA_TRY(h->X.alloc((size_t)n * h->dpad));
    const int32_t span_cap = std::min<int32_t>(h->dpad, HR_MAX_SPAN);
    // the form: the wave form unless MORNA_HASHROWS_WALK is set to something other than 0; its workgroup has 512 threads where
    // the cells leave room for one workgroup per CU only
    static const bool walk = getenv("MORNA_HASHROWS_WALK") && atoi(getenv("MORNA_HASHROWS_WALK")) != 0;
    const int threads = walk ? HR_CHUNK : span_cap > HR_WIDE_SPAN ? 512 : 256;
    const size_t lds = (size_t)span_cap * sizeof(double) + 2 * (size_t)threads * (sizeof(double) + sizeof(int32_t)) +
                       (walk ? 0 : (size_t)(threads / WAVE) * HR_TAGS * sizeof(unsigned int));
    const void *kernel = walk ? (const void *)hash_rows_walk_kernel
                              : threads == 512 ? (const void *)hash_rows_kernel<512> : (const void *)hash_rows_kernel<256>;
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    EventPair ev;
    MORNA_TRY(ev.create());
    // on the handle's stream, behind whatever it still has queued for these rows; the store's scratch is free again when
    // this call returns (it waits below)
    HIP_TRY(hipEventRecord(ev.a, h->stream));
    if (n_lines > 0)
        hipLaunchKernelGGL(hash_cols_kernel, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, h->stream, s->d_hr_hash.p, d_w, n_lines,
                           h->dim, s->d_hr_col.p, s->d_hr_sw.p);
    if (walk)
        hipLaunchKernelGGL(hash_rows_walk_kernel, dim3((unsigned)n), dim3(HR_CHUNK), lds, h->stream, s->d_ptr.p, s->d_line.p, s->d_cov.p,
                           s->d_hr_rows.p, s->d_hr_col.p, s->d_hr_sw.p, h->dpad, span_cap, h->X.p);
    else if (threads == 512)
        hipLaunchKernelGGL(hash_rows_kernel<512>, dim3((unsigned)n), dim3(512), lds, h->stream, s->d_ptr.p, s->d_line.p, s->d_cov.p,
                           s->d_hr_rows.p, s->d_hr_col.p, s->d_hr_sw.p, h->dpad, span_cap, h->X.p);
    else
        hipLaunchKernelGGL(hash_rows_kernel<256>, dim3((unsigned)n), dim3(256), lds, h->stream, s->d_ptr.p, s->d_line.p, s->d_cov.p,
                           s->d_hr_rows.p, s->d_hr_col.p, s->d_hr_sw.p, h->dpad, span_cap, h->X.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, h->stream));
    // everything that hangs on the rows, as build_features leaves it
    if (h->n_items != n) h->comm_sizes_valid = false;
    h->n_items = n;
    h->host_n = 0;
    h->host_rows.clear();
    h->host_dirty = false;
    h->built = false;
    MORNA_TRY(morna::compute_norms(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->unsettled = false;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    s->hr_stats[0] = ms;
    s->hr_stats[1] = 8.0 * (double)entries + 12.0 * (double)n_lines;
    s->hr_stats[2] = 4.0 * (double)n * (double)h->dpad;
    s->hr_stats[3] = (double)n;
    return MORNA_OK;
}

}  // namespace

extern "C" {

int morna_add_items_from_store(morna_index *h, morna_jstore *s, const int64_t *ext, int64_t n, const int32_t *line_hash, int64_t n_lines)
{
    if (s)   // a refused call leaves no statistics of an earlier one
        for (int i = 0; i < 4; i++) s->hr_stats[i] = 0;
    if (!h || !s || n < 0 || (n > 0 && !ext) || !line_hash) {
        set_error("add_items_from_store: null argument");
        return MORNA_E_INVALID;
    }
    if (n_lines != s->n_lines) {
        set_error("add_items_from_store: %lld line hashes for a store of %lld lines", (long long)n_lines, (long long)s->n_lines);
        return MORNA_E_INVALID;
    }
    if (h->device != s->device) {
        set_error("add_items_from_store: the index is on device %d and the junction store on device %d", h->device, s->device);
        return MORNA_E_INVALID;
    }
    if (n >= INT32_MAX) {
        set_error("add_items_from_store: %lld samples exceed the 2^31 limit", (long long)n);
        return MORNA_E_INVALID;
    }
    if (!s->nearest) {
        set_error("add_items_from_store: the store has no weights: call morna_jstore_set_weights first");
        return MORNA_E_STATE;
    }
    MORNA_TRY(morna::finish_build(h, __func__));   // a build whose last narrow levels are pending is a built index
    if (h->built) {
        set_error("You can't add an item to a built index");
        return MORNA_E_STATE;
    }
    return guarded("add_items_from_store", MORNA_E_INVALID, [&] { return hash_rows_impl(h, s, ext, n, line_hash); });
}

int morna_jstore_hash_rows_stats(const morna_jstore *s, double *stats)
{
    if (!s || !stats) {
        set_error("jstore_hash_rows_stats: null argument");
        return MORNA_E_INVALID;
    }
    for (int i = 0; i < 4; i++) stats[i] = s->hr_stats[i];
    return MORNA_OK;
}

}  // extern "C"
