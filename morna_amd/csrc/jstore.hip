// jstore.hip -- the junctions-by-sample store of `morna junctions` and its filter, on the GPU.
//
// Counterpart of the reference's junction databases and of the retention step of its `junctions` subcommand
// (commanderson/morna morna.py:221-341 update_junction_dbs, 1486-1638), stripped of their storage format (100 sqlite
// shards of run-length strings): the computation is
//   * the STORE: the transpose of the junction x sample CSR the intropolis parse yields -- per sample, the ascending
//     list of (line number, coverage) over ALL lines of the file (update_junction_dbs runs before the threshold test,
//     morna.py:359 vs 361-363);
//   * the FILTER: a set operation over the k rows of one result list -- keep every line at least min_count of the
//     results hold, or that one of them covers at least coverage_filter times (morna.py:1539-1569).
//
// Store build (deterministic, no atomics on global memory): a stable counting sort of the entries by sample.
//   jstore_count_kernel  one workgroup per block of consecutive lines walks ITS lines in file order and counts the
//                        entries of every sample (cnt[block][sample]); a sample occurs at most once in a line, so the
//                        entries of one line never meet -- which the kernel checks with an LDS bitmap (a repeat is
//                        reported, smallest (line, sample) first, and the build fails before anything is placed)
//   jstore_scan_kernel   per sample: exclusive prefix of its counts over the blocks, in place, and its total
//   jstore_ptr_kernel    exclusive prefix of the totals over the samples: ptr[S + 1]
//   jstore_place_kernel  the same walk: entry -> ptr[sample] + cnt[block][sample]++
// Lines are visited in ascending order by exactly one workgroup per sample and block, so a sample's list ascends by
// line number whatever order a line lists its samples in, and two builds give the same bytes.
//
// The tile walk, which the filter and recovery share: grid over (tile of JT_LINES line numbers) x (query).
//   tile_of_block  the workgroup's tile and query, and how many results the query's list holds
//   tile_ranges    one thread per result binary-searches the tile's first line in that sample's list, another its last
//   walk_tile      a wave per result walks that run and hands every entry (rank, index, line in the tile) to a body
//
// Filter: the tile's 64-bit found_in words and its coverage flags sit in LDS; the walk ORs bit `rank` into the line's
// word (LDS atomics: the OR is order-independent).  A first pass counts the retained lines and their found_in bits per
// tile; a scan over the tiles of a query gives each tile its place; the second pass writes the lines ascending and
// their words, and walks the tile again to write the coverages in rank order.
//
// Recovery: the same walk, with the largest coverage kept beside the word, but what leaves the tile is
// a histogram, not lines.  Whether a line is retained under ANY (frequency, coverage) pair follows from two small integers,
// the number of results that hold it and the largest coverage among them; with a truth bit per line that is one of
// 2 x 65 x (B + 1) classes for a grid of B coverage thresholds.  The tile counts its lines per class in LDS and adds its
// non-zero classes to hist[q] with integer atomics: every cell of a filter grid is then a sum over classes on the host,
// and nothing of the size of the line count comes back.
//
// Recovery sweep: the recovery tile for several lengths of every list at once.  The walk takes the ranks
// in the buckets the lengths cut; at every boundary the tile's words and maxima are those of the shorter list, so it is
// classified and added to that length's histogram before the walk goes on.  One read of the rows, one launch.
//
// Pool: the same walk with sums in place of bits.  A group of samples of any size is taken in rounds of 64
// rows; every entry adds its coverage to the line's 64-bit sum and 1 to its holder count (LDS integer atomics: the sums do
// not depend on the order).  Two passes as the filter's: count the held lines per tile, scan, write (line, sum, holders)
// ascending.
//
// Thin: a store row at a fraction of its depth.  Every read of every entry is kept when an integer hash
// of (seed, sample id, line, read number) falls below the job's threshold, so the answer is a function of those alone.  A
// job's row is one contiguous run, so this does not use the tile walk: the host cuts the named rows into chunks of
// JH_CHUNK entries, one workgroup each.  Pass 1 counts the kept reads of every entry into a scratch array (a lane makes
// the draws of a light entry, the wave those of a heavy one) and the survivors of the chunk; jstore_ptr_kernel scans the
// chunk counts; pass 2 writes (line, kept reads) of the survivors, ascending.  No atomics, no floating point.
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "jstore.hpp"

using morna::DevBuf;
using morna::EventPair;
using morna::guarded;
using morna::set_error;

struct morna_jretained {
    int64_t nq = 0;
    std::vector<int64_t> off{0};       // [nq + 1] first retained line of every query in the flat arrays
    std::vector<int32_t> lines;        // retained line numbers, ascending inside a query
    std::vector<uint64_t> masks;       // found_in: bit r set = result r holds the line
    std::vector<int64_t> cov_ptr{0};   // [total + 1] extent of every retained line's coverages in `cov`
    std::vector<int32_t> cov;          // coverages, rank order inside a line
};

struct morna_jpooled {
    int64_t ng = 0;
    std::vector<int64_t> off{0};       // [ng + 1] first held line of every group in the flat arrays
    std::vector<int32_t> lines;        // held line numbers, ascending inside a group
    std::vector<int64_t> sums;         // the members' summed coverage of the line
    std::vector<int32_t> holders;      // the members that hold it
};

struct morna_jthinned {
    int64_t nq = 0;
    std::vector<int64_t> off{0};       // [nq + 1] first surviving line of every job in the flat arrays
    std::vector<int32_t> lines;        // surviving line numbers, ascending inside a job
    std::vector<int32_t> cov;          // their thinned coverages, 1 at the least
};

namespace {

#define JS_THREADS 512
#define JS_BITMAP_WORDS 8192            // per bitmap; two of them: 64 KiB of LDS, up to 262144 samples
#define JT_LINES 4096                   // lines of a filter tile: 32 KiB of found_in words
#define JT_THREADS 256
#define JT_PER (JT_LINES / JT_THREADS)  // consecutive lines per thread when a tile is compacted

// err[0]: smallest (line << 32 | sample) of a repeated sample, err[1]: entries whose sample is out of range
__global__ __launch_bounds__(JS_THREADS) void jstore_count_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ ids,
                                                                  int64_t J, int32_t lines_per_block, int32_t S, int32_t check_dup,
                                                                  int32_t *cnt, unsigned long long *__restrict__ err)
{
    extern __shared__ uint32_t s_bits[];   // two bitmaps of JS_BITMAP_WORDS words, used by alternate lines
    const int tid = threadIdx.x;
    if (check_dup)
        for (int i = tid; i < 2 * JS_BITMAP_WORDS; i += JS_THREADS) s_bits[i] = 0;
    __syncthreads();
    int32_t *my = cnt + (int64_t)blockIdx.x * S;
    const int64_t l0 = (int64_t)blockIdx.x * lines_per_block;
    const int64_t l1 = l0 + lines_per_block < J ? l0 + lines_per_block : J;
    for (int64_t l = l0; l < l1; l++) {
        const int64_t a = row_ptr[l], b = row_ptr[l + 1];
        uint32_t *bits = s_bits + (l & 1) * JS_BITMAP_WORDS;
        for (int64_t e = a + tid; e < b; e += JS_THREADS) {
            const int32_t s = ids[e];
            if (s < 0 || s >= S) {
                atomicAdd(&err[1], 1ull);
                continue;
            }
            if (check_dup) {
                const uint32_t bit = 1u << (s & 31);
                if (atomicOr(&bits[s >> 5], bit) & bit) atomicMin(&err[0], ((unsigned long long)l << 32) | (uint32_t)s);
            }
            my[s] += 1;   // no other entry of this line has sample s
        }
        __syncthreads();   // the next line's entries see this line's counts
        if (check_dup)     // (the line after next is the first to use this bitmap again, a barrier away)
            for (int64_t e = a + tid; e < b; e += JS_THREADS) {
                const int32_t s = ids[e];
                if (s >= 0 && s < S) atomicAnd(&bits[s >> 5], ~(1u << (s & 31)));
            }
    }
}

// one thread per sample: cnt[0 .. n_blocks)[s] -> its exclusive prefix over the blocks; total[s]
__global__ __launch_bounds__(256) void jstore_scan_kernel(int32_t *__restrict__ cnt, int32_t n_blocks, int32_t S, int64_t *__restrict__ total)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    int64_t run = 0;
    for (int32_t b = 0; b < n_blocks; b++) {
        int32_t *c = cnt + (int64_t)b * S + s;
        const int32_t t = *c;
        *c = (int32_t)run;   // a sample holds at most one entry per line: fewer than 2^31 in all
        run += t;
    }
    total[s] = run;
}

// exclusive scan of total[S] into ptr[S + 1] (one workgroup)
__global__ __launch_bounds__(1024) void jstore_ptr_kernel(const int64_t *__restrict__ total, int32_t S, int64_t *__restrict__ ptr)
{
    __shared__ int64_t s_part[1024];
    const int tid = threadIdx.x;
    const int64_t per = ((int64_t)S + 1023) / 1024;
    const int64_t lo = tid * per < S ? tid * per : S, hi = lo + per < S ? lo + per : S;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; i++) sum += total[i];
    s_part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = tid >= o ? s_part[tid - o] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int64_t run = tid ? s_part[tid - 1] : 0;
    for (int64_t i = lo; i < hi; i++) {
        ptr[i] = run;
        run += total[i];
    }
    if (tid == 1023) ptr[S] = s_part[1023];
}

__global__ __launch_bounds__(JS_THREADS) void jstore_place_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ ids,
                                                                  const int32_t *__restrict__ cov, int64_t J, int32_t lines_per_block,
                                                                  int32_t S, int64_t nnz, const int64_t *__restrict__ ptr,
                                                                  int32_t *cnt, int32_t *__restrict__ line_out,
                                                                  int32_t *__restrict__ cov_out)
{
    const int tid = threadIdx.x;
    int32_t *my = cnt + (int64_t)blockIdx.x * S;
    const int64_t l0 = (int64_t)blockIdx.x * lines_per_block;
    const int64_t l1 = l0 + lines_per_block < J ? l0 + lines_per_block : J;
    for (int64_t l = l0; l < l1; l++) {
        const int64_t a = row_ptr[l], b = row_ptr[l + 1];
        for (int64_t e = a + tid; e < b; e += JS_THREADS) {
            const int32_t s = ids[e];   // in range and once per line: the count pass has checked both
            const int32_t at = my[s];
            my[s] = at + 1;
            const int64_t p = ptr[s] + at;
            if (p >= 0 && p < nnz) {
                line_out[p] = (int32_t)l;
                cov_out[p] = cov[e];
            }
        }
        __syncthreads();
    }
}

// ---- the filter ------------------------------------------------------------------------------------------------

// first index in [lo, hi) whose line is >= key
__device__ inline int64_t lower_bound_line(const int32_t *__restrict__ line, int64_t lo, int64_t hi, int64_t key)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)line[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the (tile, query) of a workgroup: lines [t0, t1) of the file against the first m results of list q
struct JTile {
    int64_t q, t0, t1;
    int32_t tile, m;
};

// the tile alone, of no list yet (m = 0)
__device__ __forceinline__ JTile tile_of_block(int64_t n_lines, int32_t n_tiles)
{
    JTile T;
    T.q = blockIdx.x / n_tiles;
    T.tile = (int32_t)(blockIdx.x % n_tiles);
    T.t0 = (int64_t)T.tile * JT_LINES;
    T.t1 = T.t0 + JT_LINES < n_lines ? T.t0 + JT_LINES : n_lines;
    T.m = 0;
    return T;
}

__device__ __forceinline__ JTile tile_of_block(int64_t n_lines, int32_t n_tiles, const int32_t *__restrict__ n_results, int32_t k)
{
    JTile T = tile_of_block(n_lines, n_tiles);
    const int32_t m = n_results[T.q];
    T.m = m < 0 ? 0 : (m > k ? k : m);
    return T;
}

// threads 0-63: s_lo[r], where the tile begins in the list of row rows[T.q * k + r_first + r]; threads 64-127: s_hi[r], where
// it ends; for r < n, at most 64 (a round of a longer list: the pool's)
__device__ __forceinline__ void tile_ranges(const JTile &T, const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                            const int32_t *__restrict__ rows, int32_t k, int64_t *s_lo, int64_t *s_hi, int64_t r_first,
                                            int32_t n)
{
    const int tid = threadIdx.x, r = tid & 63;
    if (tid < 128 && r < n) {
        const int32_t row = rows[T.q * k + r_first + r];
        const int64_t a = ptr[row], b = ptr[row + 1];
        const int64_t at = lower_bound_line(line, a, b, tid < 64 ? T.t0 : T.t1);
        if (tid < 64) s_lo[r] = at;
        else s_hi[r] = at;
    }
}

// every result of the list
__device__ __forceinline__ void tile_ranges(const JTile &T, const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                            const int32_t *__restrict__ rows, int32_t k, int64_t *s_lo, int64_t *s_hi)
{
    tile_ranges(T, ptr, line, rows, k, s_lo, s_hi, 0, T.m);
}

// the walk: one wave per result r of the ranks [r_first, r_end), a workgroup-uniform range inside [0, T.m):
// f(r, i, l) for every entry i of its list on line t0 + l of the tile
template <typename F>
__device__ __forceinline__ void walk_tile(const JTile &T, const int32_t *__restrict__ line, const int64_t *s_lo, const int64_t *s_hi,
                                          int r_first, int r_end, F f)
{
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    for (int r = r_first + wave; r < r_end; r += JT_THREADS / WAVE) {
        const int64_t hi = s_hi[r];
        for (int64_t i = s_lo[r] + lane; i < hi; i += WAVE) {
            const int64_t l = (int64_t)line[i] - T.t0;
            if (l < 0 || l >= JT_LINES) continue;   // (cannot happen in an ascending list)
            f(r, i, l);
        }
    }
}

// every result of the list
template <typename F>
__device__ __forceinline__ void walk_tile(const JTile &T, const int32_t *__restrict__ line, const int64_t *s_lo, const int64_t *s_hi, F f)
{
    walk_tile(T, line, s_lo, s_hi, 0, T.m, f);
}

// One workgroup per (tile, query).  write == 0: tile_n[q][tile] = {retained lines, their found_in bits}.
// write != 0: tile_n holds the exclusive prefix of those pairs over the query's tiles, q_off[q] / q_cov_off[q] the
// query's place in the flat outputs.
__global__ __launch_bounds__(JT_THREADS) void jstore_retain_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                                   const int32_t *__restrict__ cov, int64_t n_lines, int32_t n_tiles,
                                                                   const int32_t *__restrict__ rows, const int32_t *__restrict__ n_results,
                                                                   const int32_t *__restrict__ min_count, int32_t k, int64_t coverage_filter,
                                                                   int32_t write, int64_t *__restrict__ tile_n,
                                                                   const int64_t *__restrict__ q_off, const int64_t *__restrict__ q_cov_off,
                                                                   int32_t *__restrict__ lines_out, unsigned long long *__restrict__ masks_out,
                                                                   int64_t *__restrict__ cov_ptr_out, int32_t *__restrict__ cov_out)
{
    __shared__ unsigned long long s_mask[JT_LINES];
    __shared__ uint32_t s_flag[JT_LINES / 32];
    __shared__ int64_t s_lo[64], s_hi[64];
    __shared__ int32_t s_keep[JT_THREADS], s_bitsum[JT_THREADS];
    __shared__ int32_t s_covoff[JT_LINES];   // write pass: a retained line's first coverage, relative to the tile; -1: not retained
    const int tid = threadIdx.x;
    const JTile T = tile_of_block(n_lines, n_tiles, n_results, k);
    const int64_t q = T.q, t0 = T.t0, t1 = T.t1;
    const int32_t tile = T.tile;
    for (int i = tid; i < JT_LINES; i += JT_THREADS) s_mask[i] = 0;
    for (int i = tid; i < JT_LINES / 32; i += JT_THREADS) s_flag[i] = 0;
    tile_ranges(T, ptr, line, rows, k, s_lo, s_hi);
    __syncthreads();
    walk_tile(T, line, s_lo, s_hi, [&](int r, int64_t i, int64_t l) {
        atomicOr(&s_mask[l], 1ull << r);
        if ((int64_t)cov[i] >= coverage_filter) atomicOr(&s_flag[l >> 5], 1u << (l & 31));
    });
    __syncthreads();
    // compaction: thread t owns lines [t * JT_PER, (t + 1) * JT_PER) of the tile
    const int32_t mc = min_count[q];
    int32_t keep = 0, bitsum = 0;
    uint32_t kept_bits = 0;
    for (int j = 0; j < JT_PER; j++) {
        const int l = tid * JT_PER + j;
        const unsigned long long w = s_mask[l];
        const int c = __popcll(w);
        const bool on = t0 + l < t1 && c >= 1 && (c >= mc || ((s_flag[l >> 5] >> (l & 31)) & 1u));
        if (on) {
            kept_bits |= 1u << j;
            keep++;
            bitsum += c;
        }
    }
    s_keep[tid] = keep;
    s_bitsum[tid] = bitsum;
    __syncthreads();
    for (int o = 1; o < JT_THREADS; o <<= 1) {   // inclusive scans over the threads
        const int32_t a = tid >= o ? s_keep[tid - o] : 0, b = tid >= o ? s_bitsum[tid - o] : 0;
        __syncthreads();
        s_keep[tid] += a;
        s_bitsum[tid] += b;
        __syncthreads();
    }
    int64_t *mine = tile_n + 2 * ((int64_t)q * n_tiles + tile);
    if (!write) {
        if (tid == JT_THREADS - 1) {
            mine[0] = s_keep[tid];
            mine[1] = s_bitsum[tid];
        }
        return;
    }
    const int64_t line_base = q_off[q] + mine[0], cov_base = q_cov_off[q] + mine[1];
    int64_t at = line_base + s_keep[tid] - keep;
    int32_t cat = s_bitsum[tid] - bitsum;
    for (int j = 0; j < JT_PER; j++) {
        const int l = tid * JT_PER + j;
        if ((kept_bits >> j) & 1u) {
            const unsigned long long w = s_mask[l];
            lines_out[at] = (int32_t)(t0 + l);
            masks_out[at] = w;
            cov_ptr_out[at] = cov_base + cat;
            s_covoff[l] = cat;
            cat += __popcll(w);
            at++;
        } else {
            s_covoff[l] = -1;
        }
    }
    __syncthreads();
    walk_tile(T, line, s_lo, s_hi, [&](int r, int64_t i, int64_t l) {
        const int32_t o = s_covoff[l];
        if (o >= 0) cov_out[cov_base + o + __popcll(s_mask[l] & ((1ull << r) - 1ull))] = cov[i];
    });
}

// one wave per query: the (lines, bits) pairs of its tiles -> their exclusive prefix, in place; totals[q] = the sums
__global__ __launch_bounds__(256) void jstore_tile_scan_kernel(int64_t *__restrict__ tile_n, int32_t n_tiles, int64_t nq,
                                                               int64_t *__restrict__ totals)
{
    const int lane = threadIdx.x % WAVE;
    const int64_t q = (int64_t)blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
    if (q >= nq) return;
    int64_t *t = tile_n + 2 * q * n_tiles;
    int64_t run0 = 0, run1 = 0;
    for (int32_t b0 = 0; b0 < n_tiles; b0 += WAVE) {
        const int32_t b = b0 + lane;
        const int64_t v0 = b < n_tiles ? t[2 * b] : 0, v1 = b < n_tiles ? t[2 * b + 1] : 0;
        int64_t i0 = v0, i1 = v1;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int64_t o0 = __shfl_up(i0, off, WAVE), o1 = __shfl_up(i1, off, WAVE);
            if (lane >= off) {
                i0 += o0;
                i1 += o1;
            }
        }
        if (b < n_tiles) {
            t[2 * b] = run0 + i0 - v0;
            t[2 * b + 1] = run1 + i1 - v1;
        }
        run0 += __shfl(i0, WAVE - 1, WAVE);
        run1 += __shfl(i1, WAVE - 1, WAVE);
    }
    if (lane == 0) {
        totals[2 * q] = run0;
        totals[2 * q + 1] = run1;
    }
}

// ---- pool: the summed coverages of a group of samples -----------------------------------------------------------------

// One workgroup per (tile, group).  Group g holds the store rows rows[g_ptr[g] .. g_ptr[g + 1]), distinct, any number of them.
// write == 0: tile_n[g][tile] = {lines at least one member holds, entries of the members in the tile}.  write != 0: tile_n
// holds the exclusive prefix of those pairs over the group's tiles, g_off[g] the group's place in the flat outputs of n_out
// lines.  The number of rounds follows from g_ptr alone, so every barrier is reached by every thread of a workgroup.
// LDS: 32 KiB of sums, 16 KiB of holder counts, 1 KiB of extents, 2 KiB of scan arrays: 51 KiB.
__global__ __launch_bounds__(JT_THREADS) void jstore_pool_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                                 const int32_t *__restrict__ cov, int64_t n_lines, int32_t n_tiles,
                                                                 const int32_t *__restrict__ rows, const int64_t *__restrict__ g_ptr,
                                                                 int32_t write, int64_t *__restrict__ tile_n,
                                                                 const int64_t *__restrict__ g_off, int64_t n_out,
                                                                 int32_t *__restrict__ lines_out, int64_t *__restrict__ sums_out,
                                                                 int32_t *__restrict__ holders_out)
{
    __shared__ unsigned long long s_sum[JT_LINES];   // two's complement: a negative coverage adds its 64-bit pattern
    __shared__ int32_t s_cnt[JT_LINES];
    __shared__ int64_t s_lo[64], s_hi[64];
    __shared__ int32_t s_keep[JT_THREADS], s_ent[JT_THREADS];
    const int tid = threadIdx.x;
    const JTile T = tile_of_block(n_lines, n_tiles);
    const int64_t g = T.q, t0 = T.t0, t1 = T.t1;
    for (int i = tid; i < JT_LINES; i += JT_THREADS) {
        s_sum[i] = 0;
        s_cnt[i] = 0;
    }
    __syncthreads();
    const int64_t m_first = g_ptr[g], m = g_ptr[g + 1] - m_first;
    for (int64_t done = 0; done < m; done += 64) {   // rounds of 64 members
        const int32_t n = (int32_t)(m - done < 64 ? m - done : 64);
        tile_ranges(T, ptr, line, rows + m_first, 0, s_lo, s_hi, done, n);
        __syncthreads();
        walk_tile(T, line, s_lo, s_hi, 0, n, [&](int, int64_t i, int64_t l) {
            atomicAdd(&s_sum[l], (unsigned long long)(long long)cov[i]);
            atomicAdd(&s_cnt[l], 1);
        });
        __syncthreads();   // before the next round overwrites the extents; after the last, before the sums are read
    }
    // compaction: thread t owns lines [t * JT_PER, (t + 1) * JT_PER) of the tile
    int32_t keep = 0, ent = 0;
    uint32_t kept_bits = 0;
    for (int j = 0; j < JT_PER; j++) {
        const int l = tid * JT_PER + j;
        const int32_t c = s_cnt[l];
        if (t0 + l < t1 && c >= 1) {   // held: whatever its sum is
            kept_bits |= 1u << j;
            keep++;
            ent += c;
        }
    }
    s_keep[tid] = keep;
    s_ent[tid] = ent;
    __syncthreads();
    for (int o = 1; o < JT_THREADS; o <<= 1) {   // inclusive scans over the threads
        const int32_t a = tid >= o ? s_keep[tid - o] : 0, b = tid >= o ? s_ent[tid - o] : 0;
        __syncthreads();
        s_keep[tid] += a;
        s_ent[tid] += b;
        __syncthreads();
    }
    int64_t *mine = tile_n + 2 * ((int64_t)g * n_tiles + T.tile);
    if (!write) {
        if (tid == JT_THREADS - 1) {
            mine[0] = s_keep[tid];
            mine[1] = s_ent[tid];
        }
        return;
    }
    int64_t at = g_off[g] + mine[0] + s_keep[tid] - keep;
    for (int j = 0; j < JT_PER; j++) {
        const int l = tid * JT_PER + j;
        if (!((kept_bits >> j) & 1u)) continue;
        if (at >= 0 && at < n_out) {
            lines_out[at] = (int32_t)(t0 + l);
            sums_out[at] = (int64_t)s_sum[l];
            holders_out[at] = s_cnt[l];
        }
        at++;
    }
}

// ---- thin: the rows of a batch of jobs with every read kept with probability keep / 2^32 ----------------------------------

#define JH_THREADS 256
#define JH_PER 8                         // entries per thread
#define JH_CHUNK (JH_THREADS * JH_PER)   // entries of a chunk: one workgroup's
#define JH_WAVES (JH_THREADS / WAVE)
#define JH_LANE_MAX 32                   // a lane makes the draws of an entry covered at most this often; the wave those of the others
#define JH_MAX_COV (1 << 24)             // the domain: one entry is at most 2^18 iterations of the wave's loop
#define JH_GOLDEN 0x9e3779b9u

// entries [first, first + n) of the store belong to job `job`; their thinned coverages sit at scratch[scratch ...]
struct JHChunk {
    int64_t first, scratch;
    int32_t job, n;
};

// MurmurHash3's finalizer
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// what a job's hashing needs: u of (seed, sample id), and the threshold as 32 bits and "keeps everything" (keep = 2^32)
struct JHJob {
    uint32_t u, a;
    bool all;
};

__device__ __forceinline__ JHJob thin_job(const JHChunk &ch, const int64_t *__restrict__ j_ext, const unsigned long long *__restrict__ j_keep,
                                          uint32_t s)
{
    const unsigned long long ext = (unsigned long long)j_ext[ch.job], keep = j_keep[ch.job];
    JHJob J;
    J.u = fmix32((uint32_t)ext ^ fmix32((uint32_t)(ext >> 32) ^ s));
    J.a = (uint32_t)keep;
    J.all = (keep >> 32) != 0;
    return J;
}

// the draw whose hash input is x = v + JH_GOLDEN * (i + 1): kept?
__device__ __forceinline__ uint32_t thin_kept(const JHJob &J, uint32_t x)
{
    return (J.all || fmix32(x) < J.a) ? 1u : 0u;
}

// Pass 1.  One workgroup per chunk; thread t takes entries t, t + JH_THREADS, ... of it (coalesced).  scratch[ch.scratch + e] =
// the kept reads of entry e; chunk_n[chunk] = the entries that keep at least one.  s = fmix32(seed).  Every loop bound that
// a cross-lane operation sits in is wave-uniform; the one barrier is reached by all.
__global__ __launch_bounds__(JH_THREADS) void jstore_thin_count_kernel(const int32_t *__restrict__ line, const int32_t *__restrict__ cov,
                                                                       const JHChunk *__restrict__ chunks, const int64_t *__restrict__ j_ext,
                                                                       const unsigned long long *__restrict__ j_keep, uint32_t s,
                                                                       int32_t *__restrict__ scratch, int64_t *__restrict__ chunk_n)
{
    __shared__ int32_t s_wave[JH_WAVES];
    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const JHChunk ch = chunks[blockIdx.x];
    const JHJob J = thin_job(ch, j_ext, j_keep, s);
    int32_t survivors = 0;
    for (int j = 0; j < JH_PER; j++) {
        const int e = j * JH_THREADS + tid;
        const bool in = e < ch.n;
        uint32_t c = 0, v = 0;
        if (in) {
            c = (uint32_t)cov[ch.first + e];
            v = fmix32(J.u ^ (uint32_t)line[ch.first + e]);
            if (c > JH_MAX_COV) c = 0;   // (the host has refused such a row: this only bounds the loops below)
        }
        uint32_t k = 0;
        if (c <= JH_LANE_MAX) {
            uint32_t x = v;
            for (uint32_t i = 0; i < c; i++) {
                x += JH_GOLDEN;
                k += thin_kept(J, x);
            }
        }
        unsigned long long heavy = __ballot(c > JH_LANE_MAX);
        while (heavy) {   // one heavy entry at a time, its draws dealt over the lanes
            const int src = __ffsll((long long)heavy) - 1;
            heavy &= heavy - 1;
            const uint32_t cc = (uint32_t)__shfl((int)c, src, WAVE), cv = (uint32_t)__shfl((int)v, src, WAVE);
            uint32_t part = 0, x = cv + JH_GOLDEN * (uint32_t)(lane + 1);
            for (uint32_t base = 0; base < cc; base += WAVE) {   // draw i = base + lane
                if (base + (uint32_t)lane < cc) part += thin_kept(J, x);
                x += JH_GOLDEN * (uint32_t)WAVE;
            }
#pragma unroll
            for (int off = WAVE / 2; off; off >>= 1) part += (uint32_t)__shfl_xor((int)part, off, WAVE);
            if (lane == src) k = part;
        }
        if (in) {
            scratch[ch.scratch + e] = (int32_t)k;
            survivors += k ? 1 : 0;
        }
    }
#pragma unroll
    for (int off = WAVE / 2; off; off >>= 1) survivors += __shfl_xor(survivors, off, WAVE);
    if (lane == 0) s_wave[wave] = survivors;
    __syncthreads();
    if (tid == 0) {
        int64_t n = 0;
        for (int w = 0; w < JH_WAVES; w++) n += s_wave[w];
        chunk_n[blockIdx.x] = n;
    }
}

// Pass 2.  chunk_off: the exclusive scan of chunk_n, which is the chunk's place in the flat outputs of n_out lines (a job's
// chunks are consecutive and jobs follow each other, so a job's lines are contiguous and ascend).  Entry e = j * JH_THREADS
// + t: the survivors before it are those of the slots (j', wave') before (j, wave) and of the lower lanes of its own ballot.
__global__ __launch_bounds__(JH_THREADS) void jstore_thin_write_kernel(const int32_t *__restrict__ line, const JHChunk *__restrict__ chunks,
                                                                       const int32_t *__restrict__ scratch,
                                                                       const int64_t *__restrict__ chunk_off, int64_t n_out,
                                                                       int32_t *__restrict__ lines_out, int32_t *__restrict__ cov_out)
{
    __shared__ int32_t s_slot[JH_PER * JH_WAVES];
    const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const JHChunk ch = chunks[blockIdx.x];
    int32_t k[JH_PER];
    unsigned long long below[JH_PER];
#pragma unroll
    for (int j = 0; j < JH_PER; j++) {
        const int e = j * JH_THREADS + tid;
        k[j] = e < ch.n ? scratch[ch.scratch + e] : 0;
        const unsigned long long m = __ballot(k[j] >= 1);
        below[j] = m & ((1ull << lane) - 1ull);
        if (lane == 0) s_slot[j * JH_WAVES + wave] = __popcll(m);
    }
    __syncthreads();
    if (tid == 0) {   // 32 counts -> their exclusive prefix
        int32_t run = 0;
        for (int t = 0; t < JH_PER * JH_WAVES; t++) {
            const int32_t c = s_slot[t];
            s_slot[t] = run;
            run += c;
        }
    }
    __syncthreads();
    const int64_t base = chunk_off[blockIdx.x];
#pragma unroll
    for (int j = 0; j < JH_PER; j++) {
        if (k[j] < 1) continue;
        const int64_t at = base + s_slot[j * JH_WAVES + wave] + __popcll(below[j]);
        if (at >= 0 && at < n_out) {
            lines_out[at] = line[ch.first + j * JH_THREADS + tid];
            cov_out[at] = k[j];
        }
    }
}

// ---- recovery: the classes of every line under a result list and a truth set -------------------------------------------

#define JR_MAX_GRID 15                   // coverage thresholds of one call: b takes 0 .. 15
#define JR_COUNTS 65                     // cnt takes 0 .. 64
#define JR_MAX_PREFIXES 8                // list lengths of one sweep

struct JRGrid {
    int64_t c[JR_MAX_GRID];   // strictly ascending
    int32_t n;
};

struct JRPrefixes {
    int32_t p[JR_MAX_PREFIXES];   // strictly ascending, 1 .. 64
    int32_t n;
};

// the LDS of a recovery tile, 58 KiB
struct JRTile {
    unsigned long long *mask;   // [JT_LINES] found_in of every line
    int32_t *max;               // [JT_LINES] its largest coverage among the results that hold it
    uint32_t *truth;            // [JT_LINES / 32] its truth bit
    int64_t *lo, *hi;           // [65] the tile's extent in every result's list; slot 64: in the truth
    uint32_t *hist;             // [2 * JR_COUNTS * (grid.n + 1)] the tile's lines per class
};

// The tile's LDS cleared and its extents found (a barrier must follow).  Truth: the entries of store row truth_rows[q], or,
// with truth_rows NULL, t_line[t_ptr[q] .. t_ptr[q + 1]); t_arr is the array those positions index.
__device__ __forceinline__ void recovery_begin(const JTile &T, const JRTile &L, int n_bins, const int64_t *__restrict__ ptr,
                                               const int32_t *__restrict__ line, const int32_t *__restrict__ rows, int32_t k,
                                               const int32_t *__restrict__ truth_rows, const int64_t *__restrict__ t_ptr,
                                               const int32_t *__restrict__ t_arr)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < JT_LINES; i += JT_THREADS) {
        L.mask[i] = 0;
        L.max[i] = INT32_MIN;   // below every coverage, a negative one included
    }
    for (int i = tid; i < JT_LINES / 32; i += JT_THREADS) L.truth[i] = 0;
    for (int i = tid; i < n_bins; i += JT_THREADS) L.hist[i] = 0;
    tile_ranges(T, ptr, line, rows, k, L.lo, L.hi);
    if (tid >= 128 && tid < 130) {   // threads 128 and 129: the same in the truth
        int64_t a, b;
        if (truth_rows) {
            const int32_t row = truth_rows[T.q];
            a = ptr[row];
            b = ptr[row + 1];
        } else {
            a = t_ptr[T.q];
            b = t_ptr[T.q + 1];
        }
        const int64_t at = lower_bound_line(t_arr, a, b, tid == 128 ? T.t0 : T.t1);
        if (tid == 128) L.lo[64] = at;
        else L.hi[64] = at;
    }
}

// the truth run of the tile into its bitmap, by the whole workgroup; by_sample: only entries covered truth_min_cov times
__device__ __forceinline__ void recovery_mark_truth(const JTile &T, const JRTile &L, const int32_t *__restrict__ t_arr,
                                                    const int32_t *__restrict__ cov, bool by_sample, int64_t truth_min_cov)
{
    const int64_t hi = L.hi[64];
    for (int64_t i = L.lo[64] + threadIdx.x; i < hi; i += JT_THREADS) {
        const int64_t l = (int64_t)t_arr[i] - T.t0;
        if (l < 0 || l >= JT_LINES) continue;
        if (!by_sample || (int64_t)cov[i] >= truth_min_cov) atomicOr(&L.truth[l >> 5], 1u << (l & 31));
    }
}

// thread t classifies lines [t * JT_PER, (t + 1) * JT_PER) of the tile into L.hist; a run of one class is one LDS add
__device__ __forceinline__ void recovery_classify(const JTile &T, const JRTile &L, const JRGrid &grid)
{
    const int nb = grid.n + 1;
    int cur = -1;
    uint32_t run = 0;
    for (int j = 0; j < JT_PER; j++) {
        const int l = threadIdx.x * JT_PER + j;
        if (T.t0 + l >= T.t1) break;
        const int c = __popcll(L.mask[l]);
        const int t = (int)((L.truth[l >> 5] >> (l & 31)) & 1u);
        if (c == 0 && t == 0) continue;
        int b = 0;
        if (c) {
            const int64_t mx = L.max[l];
#pragma unroll
            for (int i = 0; i < JR_MAX_GRID; i++) b += (i < grid.n && grid.c[i] <= mx) ? 1 : 0;
        }
        const int bin = (t * JR_COUNTS + c) * nb + b;
        if (bin != cur) {
            if (run) atomicAdd(&L.hist[cur], run);
            cur = bin;
            run = 0;
        }
        run++;
    }
    if (run) atomicAdd(&L.hist[cur], run);
}

// One workgroup per (tile, query).  hist[q][t][cnt][b] += the lines of the tile with truth bit t that cnt of the results
// hold and whose largest coverage among them reaches b of the thresholds (b = 0 when cnt = 0); plane t = 0 at cnt = 0 is
// not counted.  Truth: the entries of store row truth_rows[q] covered at least truth_min_cov times, or, with truth_rows
// NULL, the lines t_line[t_ptr[q] .. t_ptr[q + 1]).
__global__ __launch_bounds__(JT_THREADS) void jstore_recovery_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                                     const int32_t *__restrict__ cov, int64_t n_lines, int32_t n_tiles,
                                                                     const int32_t *__restrict__ rows, const int32_t *__restrict__ n_results,
                                                                     int32_t k, const int32_t *__restrict__ truth_rows, int64_t truth_min_cov,
                                                                     const int64_t *__restrict__ t_ptr, const int32_t *__restrict__ t_line,
                                                                     JRGrid grid, int32_t *__restrict__ hist)
{
    __shared__ unsigned long long s_mask[JT_LINES];
    __shared__ int32_t s_max[JT_LINES];
    __shared__ uint32_t s_truth[JT_LINES / 32];
    __shared__ int64_t s_lo[65], s_hi[65];   // slot 64: the truth
    __shared__ uint32_t s_hist[2 * JR_COUNTS * (JR_MAX_GRID + 1)];
    const JRTile L = {s_mask, s_max, s_truth, s_lo, s_hi, s_hist};
    const int tid = threadIdx.x;
    const JTile T = tile_of_block(n_lines, n_tiles, n_results, k);
    const int n_bins = 2 * JR_COUNTS * (grid.n + 1);
    const int32_t *t_arr = truth_rows ? line : t_line;
    recovery_begin(T, L, n_bins, ptr, line, rows, k, truth_rows, t_ptr, t_arr);
    __syncthreads();
    walk_tile(T, line, s_lo, s_hi, [&](int r, int64_t i, int64_t l) {
        atomicOr(&s_mask[l], 1ull << r);
        atomicMax(&s_max[l], cov[i]);
    });
    recovery_mark_truth(T, L, t_arr, cov, truth_rows != nullptr, truth_min_cov);
    __syncthreads();
    recovery_classify(T, L, grid);
    __syncthreads();
    int32_t *mine = hist + T.q * n_bins;
    for (int i = tid; i < n_bins; i += JT_THREADS) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&mine[i], (int32_t)v);   // at most n_lines < 2^31 in all
    }
}

// The recovery kernel for several lengths of every list in one walk: hist[q][i] is what
// jstore_recovery_kernel gives for list q cut to its first min(pre.p[i], m) results.  cnt of a prefix is the popcount of
// the low bits of found_in and maxcov a running maximum over ranks, so the walk visits the ranks in the buckets the
// prefixes cut, and at every boundary s_mask / s_max ARE the shorter list's: classify, add to that slice, go on.  The
// phase count and every boundary are the same for all threads of a workgroup (kernel arguments and n_results[q]), so
// every barrier is reached by all.
__global__ __launch_bounds__(JT_THREADS) void jstore_recovery_sweep_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                                           const int32_t *__restrict__ cov, int64_t n_lines, int32_t n_tiles,
                                                                           const int32_t *__restrict__ rows,
                                                                           const int32_t *__restrict__ n_results, int32_t k,
                                                                           const int32_t *__restrict__ truth_rows, int64_t truth_min_cov,
                                                                           const int64_t *__restrict__ t_ptr, const int32_t *__restrict__ t_line,
                                                                           JRGrid grid, JRPrefixes pre, int32_t *__restrict__ hist)
{
    __shared__ unsigned long long s_mask[JT_LINES];
    __shared__ int32_t s_max[JT_LINES];
    __shared__ uint32_t s_truth[JT_LINES / 32];
    __shared__ int64_t s_lo[65], s_hi[65];   // slot 64: the truth
    __shared__ uint32_t s_hist[2 * JR_COUNTS * (JR_MAX_GRID + 1)];   // one, reused by every prefix
    const JRTile L = {s_mask, s_max, s_truth, s_lo, s_hi, s_hist};
    const int tid = threadIdx.x;
    const JTile T = tile_of_block(n_lines, n_tiles, n_results, k);
    const int n_bins = 2 * JR_COUNTS * (grid.n + 1);
    const int32_t *t_arr = truth_rows ? line : t_line;
    recovery_begin(T, L, n_bins, ptr, line, rows, k, truth_rows, t_ptr, t_arr);
    __syncthreads();
    int32_t m_done = 0;
    for (int32_t p = 0; p < pre.n; p++) {
        const int32_t m_p = pre.p[p] < T.m ? pre.p[p] : T.m;   // an empty bucket once the list has ended: the slices repeat
        walk_tile(T, line, s_lo, s_hi, m_done, m_p, [&](int r, int64_t i, int64_t l) {
            atomicOr(&s_mask[l], 1ull << r);
            atomicMax(&s_max[l], cov[i]);
        });
        m_done = m_p;
        if (p == 0) recovery_mark_truth(T, L, t_arr, cov, truth_rows != nullptr, truth_min_cov);
        __syncthreads();
        recovery_classify(T, L, grid);
        __syncthreads();
        int32_t *mine = hist + (T.q * pre.n + p) * n_bins;
        for (int i = tid; i < n_bins; i += JT_THREADS) {
            const uint32_t v = s_hist[i];
            if (v) {
                atomicAdd(&mine[i], (int32_t)v);   // at most n_lines < 2^31 in all
                s_hist[i] = 0;
            }
        }
        __syncthreads();
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------

const char JSTORE_MAGIC[8] = {'M', 'O', 'R', 'N', 'A', 'J', 'S', '1'};

// what load and from_arrays require of a store; `what` names its source in the message
int validate_store(morna_jstore *st, const char *what, int code)
{
    const int64_t S = (int64_t)st->ext_ids.size(), nnz = (int64_t)st->line.size();
    const char *why = nullptr;
    if (S > INT32_MAX || st->n_lines < 0 || st->n_lines > INT32_MAX) why = "more than 2^31 - 1 samples or lines";
    else if ((int64_t)st->ptr.size() != S + 1 || st->ptr[0] != 0 || st->ptr[(size_t)S] != nnz || st->cov.size() != st->line.size())
        why = "the offsets do not describe the arrays";
    for (int64_t s = 0; !why && s < S; s++) {
        const int64_t a = st->ptr[(size_t)s], b = st->ptr[(size_t)s + 1];
        if (a > b || b > nnz) {
            why = "the offsets do not ascend";
            break;
        }
        for (int64_t i = a; i < b; i++)
            if (st->line[(size_t)i] < 0 || st->line[(size_t)i] >= st->n_lines || (i > a && st->line[(size_t)i] <= st->line[(size_t)i - 1])) {
                why = "a sample's line numbers do not ascend below the line count";
                break;
            }
    }
    if (!why) {
        st->row_of.clear();
        st->row_of.reserve((size_t)S);
        for (int64_t s = 0; s < S; s++)
            if (!st->row_of.emplace(st->ext_ids[(size_t)s], (int32_t)s).second) {
                why = "a sample id occurs twice";
                break;
            }
    }
    if (why) {
        set_error("%s is not a consistent junction store: %s", what, why);
        return code;
    }
    return MORNA_OK;
}

int check_device(int32_t device)
{
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (%s): libmorna_hip has no CPU path", hipGetErrorString(e));
        return MORNA_E_HIP;
    }
    if (device < 0 || device >= ndev) {
        set_error("device %d out of range (%d visible)", device, ndev);
        return MORNA_E_INVALID;
    }
    HIP_TRY(hipSetDevice(device));
    return MORNA_OK;
}

int ensure_stream(morna_jstore *st)
{
    MORNA_TRY(check_device(st->device));
    if (!st->stream) HIP_TRY(hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
    return MORNA_OK;
}

// the host image into HBM (a loaded store, at its first retain)
int make_resident(morna_jstore *st)
{
    MORNA_TRY(ensure_stream(st));
    if (st->resident) return MORNA_OK;
    const size_t S = st->ext_ids.size(), nnz = st->line.size();
    MORNA_TRY(st->d_ptr.alloc(S + 1));
    MORNA_TRY(st->d_line.alloc(nnz));
    MORNA_TRY(st->d_cov.alloc(nnz));
    HIP_TRY(hipMemcpy(st->d_ptr.p, st->ptr.data(), (S + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (nnz) {
        HIP_TRY(hipMemcpy(st->d_line.p, st->line.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(st->d_cov.p, st->cov.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    st->resident = true;
    return MORNA_OK;
}

int build_impl(morna_jstore *st, const morna_lines *L)
{
    int64_t counts[8], info[4];
    MORNA_TRY(morna_lines_counts(L, counts));
    MORNA_TRY(morna_lines_shard_info(L, info));
    const int64_t J = counts[0], nnz = counts[1], S = counts[2];
    if (counts[0] != counts[7] || info[1] != 1) {
        set_error("jstore_build: the lines are not a whole parse with threshold 0 (%lld lines kept of %lld read, shard %lld of %lld): "
                  "kept line j would not be line j of the file", (long long)counts[0], (long long)counts[7], (long long)info[0],
                  (long long)info[1]);
        return MORNA_E_INVALID;
    }
    if (J > INT32_MAX || S > INT32_MAX) {
        set_error("jstore_build: %lld lines and %lld samples: the store holds at most 2^31 - 1 of each", (long long)J, (long long)S);
        return MORNA_E_INVALID;
    }
    const int64_t *row_ptr = nullptr, *ext = nullptr;
    const int32_t *ids = nullptr, *cov = nullptr;
    MORNA_TRY(morna_lines_arrays(L, nullptr, nullptr, &row_ptr, &ids, &cov, nullptr, &ext));
    st->n_lines = J;
    st->ext_ids.assign(ext, ext + S);
    st->ptr.assign((size_t)S + 1, 0);
    st->line.assign((size_t)nnz, 0);
    st->cov.assign((size_t)nnz, 0);
    MORNA_TRY(ensure_stream(st));
    MORNA_TRY(st->d_ptr.alloc((size_t)S + 1));
    MORNA_TRY(st->d_line.alloc((size_t)nnz));
    MORNA_TRY(st->d_cov.alloc((size_t)nnz));
    if (J == 0 || S == 0 || nnz == 0) {
        HIP_TRY(hipMemset(st->d_ptr.p, 0, ((size_t)S + 1) * sizeof(int64_t)));
        st->resident = true;
        return validate_store(st, "the built store", MORNA_E_INVALID);
    }
    // blocks of lines: about 1024 of them, fewer while their count table would pass 1 GiB
    int64_t per = std::max<int64_t>(16, (J + 1023) / 1024);
    while (((J + per - 1) / per) * S * (int64_t)sizeof(int32_t) > ((int64_t)1 << 30) && per < J) per *= 2;
    if (per > INT32_MAX) per = INT32_MAX;
    const int64_t n_blocks = (J + per - 1) / per;
    const bool dup_on_device = (S + 31) / 32 <= JS_BITMAP_WORDS;
    if (!dup_on_device) {   // more samples than the LDS bitmap holds: the same check on the host, with the kernel's answer --
        std::vector<int32_t> last((size_t)S, -1);   // of the first line that repeats a sample, the smallest sample it repeats
        for (int64_t l = 0; l < J; l++) {
            int32_t repeated = -1;
            for (int64_t e = row_ptr[l]; e < row_ptr[l + 1]; e++) {
                const int32_t s = ids[e];
                if (s < 0 || s >= S) continue;   // (reported by the count kernel)
                if (last[(size_t)s] == (int32_t)l && (repeated < 0 || s < repeated)) repeated = s;
                last[(size_t)s] = (int32_t)l;
            }
            if (repeated >= 0) {
                set_error("jstore_build: line %lld lists sample %lld twice", (long long)l, (long long)ext[repeated]);
                return MORNA_E_INVALID;
            }
        }
    }
    DevBuf<int64_t> d_row_ptr, d_total;
    DevBuf<int32_t> d_ids, d_covin, d_cnt;
    DevBuf<unsigned long long> d_err;
    MORNA_TRY(d_row_ptr.alloc((size_t)J + 1));
    MORNA_TRY(d_ids.alloc((size_t)nnz));
    MORNA_TRY(d_covin.alloc((size_t)nnz));
    MORNA_TRY(d_cnt.alloc((size_t)(n_blocks * S)));
    MORNA_TRY(d_total.alloc((size_t)S));
    MORNA_TRY(d_err.alloc(2));
    HIP_TRY(hipMemcpy(d_row_ptr.p, row_ptr, ((size_t)J + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ids.p, ids, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_covin.p, cov, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    const unsigned long long err0[2] = {~0ull, 0ull};
    HIP_TRY(hipMemcpy(d_err.p, err0, sizeof(err0), hipMemcpyHostToDevice));
    EventPair ev;
    MORNA_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.a, st->stream));
    HIP_TRY(hipMemsetAsync(d_cnt.p, 0, (size_t)(n_blocks * S) * sizeof(int32_t), st->stream));
    hipLaunchKernelGGL(jstore_count_kernel, dim3((unsigned)n_blocks), dim3(JS_THREADS), dup_on_device ? 2 * JS_BITMAP_WORDS * sizeof(uint32_t) : 0,
                       st->stream, d_row_ptr.p, d_ids.p, J, (int32_t)per, (int32_t)S, dup_on_device ? 1 : 0, d_cnt.p, d_err.p);
    HIP_TRY(hipGetLastError());
    unsigned long long err[2];
    HIP_TRY(hipMemcpyAsync(err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    if (err[1]) {
        set_error("jstore_build: %llu entries name a sample outside [0, %lld)", err[1], (long long)S);
        return MORNA_E_INVALID;
    }
    if (err[0] != ~0ull) {
        set_error("jstore_build: line %lld lists sample %lld twice", (long long)(err[0] >> 32), (long long)ext[(size_t)(err[0] & 0xffffffffu)]);
        return MORNA_E_INVALID;
    }
    hipLaunchKernelGGL(jstore_scan_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st->stream, d_cnt.p, (int32_t)n_blocks, (int32_t)S,
                       d_total.p);
    hipLaunchKernelGGL(jstore_ptr_kernel, dim3(1), dim3(1024), 0, st->stream, d_total.p, (int32_t)S, st->d_ptr.p);
    hipLaunchKernelGGL(jstore_place_kernel, dim3((unsigned)n_blocks), dim3(JS_THREADS), 0, st->stream, d_row_ptr.p, d_ids.p, d_covin.p, J,
                       (int32_t)per, (int32_t)S, nnz, st->d_ptr.p, d_cnt.p, st->d_line.p, st->d_cov.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    st->ms[0] = ms;
    st->bytes[0] = 2 * 8 * nnz;   // every (sample, coverage) pair read once, every (line, coverage) pair written once
    HIP_TRY(hipMemcpy(st->ptr.data(), st->d_ptr.p, ((size_t)S + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st->line.data(), st->d_line.p, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st->cov.data(), st->d_cov.p, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    st->resident = true;
    return validate_store(st, "the built store", MORNA_E_INVALID);
}

// the store rows of nq result lists of up to k external sample ids each (rows[q * k + r]) and the entries those rows
// hold in all; `who` is the entry point the messages name
int resolve_lists(const morna_jstore *st, const char *who, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k,
                  std::vector<int32_t> &rows, int64_t &entries)
{
    rows.assign((size_t)(nq * k), 0);
    entries = 0;
    for (int64_t q = 0; q < nq; q++) {
        if (n_results[q] < 0 || n_results[q] > k) {
            set_error("%s: result list %lld holds %d results, outside [0, %d]", who, (long long)q, n_results[q], k);
            return MORNA_E_INVALID;
        }
        for (int32_t r = 0; r < n_results[q]; r++) {
            const int64_t id = results[q * k + r];
            auto it = st->row_of.find(id);
            if (it == st->row_of.end()) {
                set_error("%s: sample id %lld (result %d of list %lld) is not in the junction store", who, (long long)id, r, (long long)q);
                return MORNA_E_RANGE;
            }
            rows[(size_t)(q * k + r)] = it->second;
            entries += st->ptr[(size_t)it->second + 1] - st->ptr[(size_t)it->second];
        }
    }
    return MORNA_OK;
}

// the tiles of lines one query takes; nq of them must fit one launch (`lists`: what the caller's queries are)
int tile_count(const morna_jstore *st, const char *who, int64_t nq, int64_t *n_tiles, const char *lists = "result lists")
{
    *n_tiles = std::max<int64_t>(1, (st->n_lines + JT_LINES - 1) / JT_LINES);
    if (nq * *n_tiles > INT32_MAX) {
        set_error("%s: %lld %s over %lld tiles of lines are more than one launch holds (2^31 - 1 workgroups): "
                  "pass fewer per call", who, (long long)nq, lists, (long long)*n_tiles);
        return MORNA_E_INVALID;
    }
    return MORNA_OK;
}

int retain_impl(morna_jstore *st, const int64_t *results, const int32_t *n_results, const int32_t *min_count, int64_t nq, int32_t k,
                int64_t coverage_filter, morna_jretained *R)
{
    R->nq = nq;
    R->off.assign((size_t)nq + 1, 0);
    if (nq == 0) return MORNA_OK;
    std::vector<int32_t> rows;
    int64_t list_entries = 0, n_tiles = 0;
    MORNA_TRY(resolve_lists(st, "jstore_retain", results, n_results, nq, k, rows, list_entries));
    MORNA_TRY(make_resident(st));
    MORNA_TRY(tile_count(st, "jstore_retain", nq, &n_tiles));
    DevBuf<int32_t> d_rows, d_nres, d_minc, d_lines, d_cov;
    DevBuf<int64_t> d_tile, d_totals, d_off, d_covptr;
    DevBuf<unsigned long long> d_masks;
    MORNA_TRY(d_rows.alloc((size_t)(nq * k)));
    MORNA_TRY(d_nres.alloc((size_t)nq));
    MORNA_TRY(d_minc.alloc((size_t)nq));
    MORNA_TRY(d_tile.alloc((size_t)(2 * nq * n_tiles)));
    MORNA_TRY(d_totals.alloc((size_t)(2 * nq)));
    MORNA_TRY(d_off.alloc((size_t)(2 * nq)));
    HIP_TRY(hipMemcpy(d_rows.p, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_nres.p, n_results, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_minc.p, min_count, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice));
    EventPair ev1, ev2;
    MORNA_TRY(ev1.create());
    MORNA_TRY(ev2.create());
    const dim3 grid((unsigned)(nq * n_tiles));
    HIP_TRY(hipEventRecord(ev1.a, st->stream));
    hipLaunchKernelGGL(jstore_retain_kernel, grid, dim3(JT_THREADS), 0, st->stream, st->d_ptr.p, st->d_line.p, st->d_cov.p, st->n_lines,
                       (int32_t)n_tiles, d_rows.p, d_nres.p, d_minc.p, k, coverage_filter, 0, d_tile.p, (const int64_t *)nullptr,
                       (const int64_t *)nullptr, (int32_t *)nullptr, (unsigned long long *)nullptr, (int64_t *)nullptr, (int32_t *)nullptr);
    hipLaunchKernelGGL(jstore_tile_scan_kernel, dim3((unsigned)((nq + 256 / WAVE - 1) / (256 / WAVE))), dim3(256), 0, st->stream, d_tile.p,
                       (int32_t)n_tiles, nq, d_totals.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1.b, st->stream));
    std::vector<int64_t> totals((size_t)(2 * nq));
    HIP_TRY(hipMemcpyAsync(totals.data(), d_totals.p, totals.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    std::vector<int64_t> off((size_t)(2 * nq));   // [0, nq): first line of every query, [nq, 2 nq): its first coverage
    int64_t n_kept = 0, n_cov = 0;
    for (int64_t q = 0; q < nq; q++) {
        R->off[(size_t)q] = off[(size_t)q] = n_kept;
        off[(size_t)(nq + q)] = n_cov;
        n_kept += totals[(size_t)(2 * q)];
        n_cov += totals[(size_t)(2 * q + 1)];
    }
    R->off[(size_t)nq] = n_kept;
    R->lines.assign((size_t)n_kept, 0);
    R->masks.assign((size_t)n_kept, 0);
    R->cov_ptr.assign((size_t)n_kept + 1, 0);
    R->cov.assign((size_t)n_cov, 0);
    R->cov_ptr[(size_t)n_kept] = n_cov;
    float ms1 = 0, ms2 = 0;
    HIP_TRY(hipEventElapsedTime(&ms1, ev1.a, ev1.b));
    if (n_kept) {
        MORNA_TRY(d_lines.alloc((size_t)n_kept));
        MORNA_TRY(d_masks.alloc((size_t)n_kept));
        MORNA_TRY(d_covptr.alloc((size_t)n_kept));
        MORNA_TRY(d_cov.alloc((size_t)n_cov));
        HIP_TRY(hipMemcpy(d_off.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipEventRecord(ev2.a, st->stream));
        hipLaunchKernelGGL(jstore_retain_kernel, grid, dim3(JT_THREADS), 0, st->stream, st->d_ptr.p, st->d_line.p, st->d_cov.p, st->n_lines,
                           (int32_t)n_tiles, d_rows.p, d_nres.p, d_minc.p, k, coverage_filter, 1, d_tile.p, (const int64_t *)d_off.p,
                           (const int64_t *)(d_off.p + nq), d_lines.p, d_masks.p, d_covptr.p, d_cov.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev2.b, st->stream));
        HIP_TRY(hipStreamSynchronize(st->stream));
        HIP_TRY(hipEventElapsedTime(&ms2, ev2.a, ev2.b));
        HIP_TRY(hipMemcpy(R->lines.data(), d_lines.p, (size_t)n_kept * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(R->masks.data(), d_masks.p, (size_t)n_kept * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(R->cov_ptr.data(), d_covptr.p, (size_t)n_kept * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(R->cov.data(), d_cov.p, (size_t)n_cov * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    st->ms[1] = (double)ms1 + (double)ms2;
    st->bytes[1] = 8 * list_entries;   // the k lists of every query, read once
    return MORNA_OK;
}

// the groups of a pool as store rows, group-major; every refusal of morna_jstore_pool that needs the store
int resolve_groups(const morna_jstore *st, const int64_t *members, const int64_t *g_ptr, int64_t ng, std::vector<int32_t> &rows,
                   std::vector<int64_t> &entries)
{
    if (g_ptr[0] != 0) {
        set_error("jstore_pool: the group offsets start at %lld, not at 0", (long long)g_ptr[0]);
        return MORNA_E_INVALID;
    }
    for (int64_t g = 0; g < ng; g++)
        if (g_ptr[g + 1] < g_ptr[g]) {
            set_error("jstore_pool: the offsets of group %lld descend (%lld, %lld)", (long long)g, (long long)g_ptr[g],
                      (long long)g_ptr[g + 1]);
            return MORNA_E_INVALID;
        }
    if (g_ptr[ng] > 0 && !members) {
        set_error("jstore_pool: null argument");
        return MORNA_E_INVALID;
    }
    rows.assign((size_t)g_ptr[ng], 0);
    entries.assign((size_t)ng, 0);
    std::vector<int64_t> seen_in(st->ext_ids.size(), -1);   // the last group that named a row
    for (int64_t g = 0; g < ng; g++)
        for (int64_t i = g_ptr[g]; i < g_ptr[g + 1]; i++) {
            auto it = st->row_of.find(members[i]);
            if (it == st->row_of.end()) {
                set_error("jstore_pool: sample id %lld (member %lld of group %lld) is not in the junction store", (long long)members[i],
                          (long long)(i - g_ptr[g]), (long long)g);
                return MORNA_E_RANGE;
            }
            if (seen_in[(size_t)it->second] == g) {
                set_error("jstore_pool: group %lld names sample id %lld twice: the members of a group must be distinct", (long long)g,
                          (long long)members[i]);
                return MORNA_E_INVALID;
            }
            seen_in[(size_t)it->second] = g;
            rows[(size_t)i] = it->second;
            entries[(size_t)g] += st->ptr[(size_t)it->second + 1] - st->ptr[(size_t)it->second];
        }
    return MORNA_OK;
}

int pool_impl(morna_jstore *st, const int64_t *members, const int64_t *g_ptr, int64_t ng, morna_jpooled *R)
{
    st->pool_ms = 0;
    st->pool_read = st->pool_written = st->pool_groups = 0;
    R->ng = ng;
    R->off.assign((size_t)ng + 1, 0);
    if (ng == 0) return MORNA_OK;
    std::vector<int32_t> rows;
    std::vector<int64_t> entries;
    int64_t n_tiles = 0, all_entries = 0;
    MORNA_TRY(resolve_groups(st, members, g_ptr, ng, rows, entries));
    MORNA_TRY(tile_count(st, "jstore_pool", ng, &n_tiles, "groups"));
    MORNA_TRY(make_resident(st));
    DevBuf<int32_t> d_rows, d_lines, d_holders;
    DevBuf<int64_t> d_gptr, d_tile, d_totals, d_off, d_sums;
    MORNA_TRY(d_rows.alloc(std::max<size_t>(rows.size(), 1)));
    MORNA_TRY(d_gptr.alloc((size_t)ng + 1));
    MORNA_TRY(d_tile.alloc((size_t)(2 * ng * n_tiles)));
    MORNA_TRY(d_totals.alloc((size_t)(2 * ng)));
    MORNA_TRY(d_off.alloc((size_t)ng));
    if (!rows.empty()) HIP_TRY(hipMemcpy(d_rows.p, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_gptr.p, g_ptr, ((size_t)ng + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    EventPair ev1, ev2;
    MORNA_TRY(ev1.create());
    MORNA_TRY(ev2.create());
    const dim3 grid((unsigned)(ng * n_tiles));
    HIP_TRY(hipEventRecord(ev1.a, st->stream));
    hipLaunchKernelGGL(jstore_pool_kernel, grid, dim3(JT_THREADS), 0, st->stream, st->d_ptr.p, st->d_line.p, st->d_cov.p, st->n_lines,
                       (int32_t)n_tiles, d_rows.p, d_gptr.p, 0, d_tile.p, (const int64_t *)nullptr, (int64_t)0, (int32_t *)nullptr,
                       (int64_t *)nullptr, (int32_t *)nullptr);
    hipLaunchKernelGGL(jstore_tile_scan_kernel, dim3((unsigned)((ng + 256 / WAVE - 1) / (256 / WAVE))), dim3(256), 0, st->stream, d_tile.p,
                       (int32_t)n_tiles, ng, d_totals.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1.b, st->stream));
    std::vector<int64_t> totals((size_t)(2 * ng));
    HIP_TRY(hipMemcpyAsync(totals.data(), d_totals.p, totals.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    int64_t n_held = 0;
    for (int64_t g = 0; g < ng; g++) {
        if (totals[(size_t)(2 * g + 1)] != entries[(size_t)g] || totals[(size_t)(2 * g)] < 0 || totals[(size_t)(2 * g)] > st->n_lines) {
            set_error("jstore_pool: the tiles of group %lld hold %lld lines and %lld entries, its rows %lld entries over %lld lines: "
                      "the store on the device is not the store on the host", (long long)g, (long long)totals[(size_t)(2 * g)],
                      (long long)totals[(size_t)(2 * g + 1)], (long long)entries[(size_t)g], (long long)st->n_lines);
            return MORNA_E_STATE;
        }
        R->off[(size_t)g] = n_held;
        n_held += totals[(size_t)(2 * g)];
        all_entries += entries[(size_t)g];
    }
    R->off[(size_t)ng] = n_held;
    R->lines.assign((size_t)n_held, 0);
    R->sums.assign((size_t)n_held, 0);
    R->holders.assign((size_t)n_held, 0);
    float ms1 = 0, ms2 = 0;
    HIP_TRY(hipEventElapsedTime(&ms1, ev1.a, ev1.b));
    if (n_held) {
        MORNA_TRY(d_lines.alloc((size_t)n_held));
        MORNA_TRY(d_sums.alloc((size_t)n_held));
        MORNA_TRY(d_holders.alloc((size_t)n_held));
        HIP_TRY(hipMemcpy(d_off.p, R->off.data(), (size_t)ng * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipEventRecord(ev2.a, st->stream));
        hipLaunchKernelGGL(jstore_pool_kernel, grid, dim3(JT_THREADS), 0, st->stream, st->d_ptr.p, st->d_line.p, st->d_cov.p, st->n_lines,
                           (int32_t)n_tiles, d_rows.p, d_gptr.p, 1, d_tile.p, (const int64_t *)d_off.p, n_held, d_lines.p, d_sums.p,
                           d_holders.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev2.b, st->stream));
        HIP_TRY(hipStreamSynchronize(st->stream));
        HIP_TRY(hipEventElapsedTime(&ms2, ev2.a, ev2.b));
        HIP_TRY(hipMemcpy(R->lines.data(), d_lines.p, (size_t)n_held * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(R->sums.data(), d_sums.p, (size_t)n_held * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(R->holders.data(), d_holders.p, (size_t)n_held * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    st->pool_ms = (double)ms1 + (double)ms2;
    st->pool_read = 2 * 8 * all_entries;   // (line, coverage) of every member row, once per pass
    st->pool_written = 16 * n_held;
    st->pool_groups = ng * n_tiles;
    return MORNA_OK;
}

// The rows of the jobs of a thin, every refusal of morna_jstore_thin that needs the store, and the chunks: a job's are
// consecutive, jobs in order.  first_chunk[q]: job q's first chunk (n_chunks for the jobs after the last entry).
int resolve_thin_jobs(const morna_jstore *st, const int64_t *ext, const uint64_t *keep, int64_t nq, std::vector<JHChunk> &chunks,
                      std::vector<int64_t> &first_chunk, int64_t &entries, int64_t &draws)
{
    std::vector<char> checked(st->ext_ids.size(), 0);
    std::vector<int64_t> row_draws(st->ext_ids.size(), 0);
    chunks.clear();
    first_chunk.assign((size_t)nq + 1, 0);
    entries = draws = 0;
    for (int64_t q = 0; q < nq; q++) {
        if (keep[q] > ((uint64_t)1 << 32)) {
            set_error("jstore_thin: job %lld keeps a read when its hash is below %llu: a threshold is at most 2^32", (long long)q,
                      (unsigned long long)keep[q]);
            return MORNA_E_INVALID;
        }
        auto it = st->row_of.find(ext[q]);
        if (it == st->row_of.end()) {
            set_error("jstore_thin: sample id %lld (job %lld) is not in the junction store", (long long)ext[q], (long long)q);
            return MORNA_E_RANGE;
        }
        const size_t row = (size_t)it->second;
        const int64_t a = st->ptr[row], b = st->ptr[row + 1];
        if (!checked[row]) {
            int64_t sum = 0;
            for (int64_t i = a; i < b; i++) {
                const int32_t c = st->cov[(size_t)i];
                if (c < 0 || c > JH_MAX_COV) {
                    set_error("jstore_thin: sample id %lld holds line %d with coverage %d: a thinned row's coverages lie in [0, 2^24]",
                              (long long)ext[q], st->line[(size_t)i], c);
                    return MORNA_E_INVALID;
                }
                sum += c;
            }
            checked[row] = 1;
            row_draws[row] = sum;
        }
        first_chunk[(size_t)q] = (int64_t)chunks.size();
        for (int64_t at = a; at < b; at += JH_CHUNK)
            chunks.push_back(JHChunk{at, entries + (at - a), (int32_t)q, (int32_t)std::min<int64_t>(JH_CHUNK, b - at)});
        entries += b - a;
        draws += row_draws[row];
    }
    first_chunk[(size_t)nq] = (int64_t)chunks.size();
    if ((int64_t)chunks.size() > INT32_MAX || nq > INT32_MAX) {
        set_error("jstore_thin: %lld jobs in %lld chunks of %d entries are more than one launch holds (2^31 - 1 workgroups): "
                  "pass fewer per call", (long long)nq, (long long)chunks.size(), JH_CHUNK);
        return MORNA_E_INVALID;
    }
    return MORNA_OK;
}

int thin_impl(morna_jstore *st, const int64_t *ext, const uint64_t *keep, int64_t nq, uint32_t seed, morna_jthinned *R)
{
    st->thin_ms = 0;
    st->thin_read = st->thin_written = st->thin_draws = st->thin_groups = 0;
    R->nq = nq;
    R->off.assign((size_t)nq + 1, 0);
    if (nq == 0) return MORNA_OK;
    std::vector<JHChunk> chunks;
    std::vector<int64_t> first_chunk;
    int64_t entries = 0, draws = 0;
    MORNA_TRY(resolve_thin_jobs(st, ext, keep, nq, chunks, first_chunk, entries, draws));
    const int64_t n_chunks = (int64_t)chunks.size();
    if (n_chunks == 0) return MORNA_OK;   // every named row is empty
    MORNA_TRY(make_resident(st));
    DevBuf<JHChunk> d_chunks;
    DevBuf<int64_t> d_ext, d_chunk_n, d_chunk_off;
    DevBuf<unsigned long long> d_keep;
    DevBuf<int32_t> d_scratch, d_lines, d_cov;
    MORNA_TRY(d_chunks.alloc((size_t)n_chunks));
    MORNA_TRY(d_ext.alloc((size_t)nq));
    MORNA_TRY(d_keep.alloc((size_t)nq));
    MORNA_TRY(d_chunk_n.alloc((size_t)n_chunks));
    MORNA_TRY(d_chunk_off.alloc((size_t)n_chunks + 1));
    MORNA_TRY(d_scratch.alloc((size_t)entries));
    HIP_TRY(hipMemcpy(d_chunks.p, chunks.data(), (size_t)n_chunks * sizeof(JHChunk), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ext.p, ext, (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_keep.p, keep, (size_t)nq * sizeof(uint64_t), hipMemcpyHostToDevice));
    EventPair ev1, ev2;
    MORNA_TRY(ev1.create());
    MORNA_TRY(ev2.create());
    const dim3 grid((unsigned)n_chunks);
    HIP_TRY(hipEventRecord(ev1.a, st->stream));
    hipLaunchKernelGGL(jstore_thin_count_kernel, grid, dim3(JH_THREADS), 0, st->stream, st->d_line.p, st->d_cov.p, d_chunks.p, d_ext.p,
                       d_keep.p, fmix32(seed), d_scratch.p, d_chunk_n.p);
    hipLaunchKernelGGL(jstore_ptr_kernel, dim3(1), dim3(1024), 0, st->stream, d_chunk_n.p, (int32_t)n_chunks, d_chunk_off.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1.b, st->stream));
    std::vector<int64_t> chunk_off((size_t)n_chunks + 1);
    HIP_TRY(hipMemcpyAsync(chunk_off.data(), d_chunk_off.p, chunk_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    const int64_t n_kept = chunk_off[(size_t)n_chunks];
    if (n_kept < 0 || n_kept > entries) {
        set_error("jstore_thin: the chunks keep %lld lines of %lld entries: the store on the device is not the store on the host",
                  (long long)n_kept, (long long)entries);
        return MORNA_E_STATE;
    }
    for (int64_t q = 0; q <= nq; q++) R->off[(size_t)q] = chunk_off[(size_t)first_chunk[(size_t)q]];
    R->lines.assign((size_t)n_kept, 0);
    R->cov.assign((size_t)n_kept, 0);
    float ms1 = 0, ms2 = 0;
    HIP_TRY(hipEventElapsedTime(&ms1, ev1.a, ev1.b));
    MORNA_TRY(d_lines.alloc((size_t)n_kept));   // (pass 2 runs for no survivor too: the statistics are then one formula)
    MORNA_TRY(d_cov.alloc((size_t)n_kept));
    HIP_TRY(hipEventRecord(ev2.a, st->stream));
    hipLaunchKernelGGL(jstore_thin_write_kernel, grid, dim3(JH_THREADS), 0, st->stream, st->d_line.p, d_chunks.p, d_scratch.p, d_chunk_off.p,
                       n_kept, d_lines.p, d_cov.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev2.b, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    HIP_TRY(hipEventElapsedTime(&ms2, ev2.a, ev2.b));
    if (n_kept) {
        HIP_TRY(hipMemcpy(R->lines.data(), d_lines.p, (size_t)n_kept * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(R->cov.data(), d_cov.p, (size_t)n_kept * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    st->thin_ms = (double)ms1 + (double)ms2;
    st->thin_read = 16 * entries;                               // pass 1: (line, coverage); pass 2: (line, scratch)
    st->thin_written = 4 * entries + 8 * n_kept;                // the scratch; (line, thinned coverage) of every survivor
    st->thin_draws = draws;
    st->thin_groups = n_chunks;
    return MORNA_OK;
}

// truth_ext != NULL: truth by sample; otherwise the CSR (t_ptr, t_line).  pre != NULL: the sweep, one histogram per prefix
// of every list (hist_out[nq][pre->n][...]) from the first pre->p[pre->n - 1] rows of each
int recovery_impl(morna_jstore *st, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k, const int64_t *t_ptr,
                  const int32_t *t_line, const int64_t *truth_ext, int64_t truth_min_cov, const JRGrid &grid, const JRPrefixes *pre,
                  int32_t *hist_out)
{
    st->rec_ms = 0;
    st->rec_bytes = 0;
    st->rec_groups = 0;
    if (nq == 0) return MORNA_OK;
    std::vector<int32_t> rows, truth_rows;
    std::vector<int64_t> tp;
    int64_t entries = 0, t_base = 0, t_n = 0, n_tiles = 0;
    MORNA_TRY(resolve_lists(st, "jstore_recovery", results, n_results, nq, k, rows, entries));
    if (pre) {   // the rows the longest prefix reaches, each counted once
        entries = 0;
        for (int64_t q = 0; q < nq; q++)
            for (int32_t r = 0; r < std::min(n_results[q], pre->p[pre->n - 1]); r++) {
                const size_t row = (size_t)rows[(size_t)(q * k + r)];
                entries += st->ptr[row + 1] - st->ptr[row];
            }
    }
    if (truth_ext) {
        truth_rows.assign((size_t)nq, 0);
        for (int64_t q = 0; q < nq; q++) {
            auto it = st->row_of.find(truth_ext[q]);
            if (it == st->row_of.end()) {
                set_error("jstore_recovery: sample id %lld (truth of list %lld) is not in the junction store", (long long)truth_ext[q],
                          (long long)q);
                return MORNA_E_RANGE;
            }
            truth_rows[(size_t)q] = it->second;
            entries += st->ptr[(size_t)it->second + 1] - st->ptr[(size_t)it->second];
        }
    } else {
        t_base = t_ptr[0];
        tp.assign((size_t)nq + 1, 0);
        for (int64_t q = 0; q < nq; q++) {
            const int64_t a = t_ptr[q], b = t_ptr[q + 1];
            if (a < 0 || b < a) {
                set_error("jstore_recovery: the truth offsets of list %lld do not ascend (%lld, %lld)", (long long)q, (long long)a,
                          (long long)b);
                return MORNA_E_INVALID;
            }
            for (int64_t i = a; i < b; i++)
                if (t_line[i] < 0 || (int64_t)t_line[i] >= st->n_lines || (i > a && t_line[i] <= t_line[i - 1])) {
                    set_error("jstore_recovery: truth line %d at position %lld of list %lld: the true lines of a list must ascend, "
                              "distinct, inside [0, %lld)", t_line[i], (long long)(i - a), (long long)q, (long long)st->n_lines);
                    return MORNA_E_INVALID;
                }
            tp[(size_t)q + 1] = b - t_base;
        }
        t_n = t_ptr[nq] - t_base;
    }
    MORNA_TRY(make_resident(st));
    MORNA_TRY(tile_count(st, "jstore_recovery", nq, &n_tiles));
    const size_t n_hist = (size_t)nq * (size_t)(pre ? pre->n : 1) * 2 * JR_COUNTS * (size_t)(grid.n + 1);
    DevBuf<int32_t> d_rows, d_nres, d_truth_rows, d_tline, d_hist;
    DevBuf<int64_t> d_tptr;
    MORNA_TRY(d_rows.alloc((size_t)(nq * k)));
    MORNA_TRY(d_nres.alloc((size_t)nq));
    MORNA_TRY(d_hist.alloc(n_hist));
    HIP_TRY(hipMemcpy(d_rows.p, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_nres.p, n_results, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice));
    if (truth_ext) {
        MORNA_TRY(d_truth_rows.alloc((size_t)nq));
        HIP_TRY(hipMemcpy(d_truth_rows.p, truth_rows.data(), (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice));
    } else {
        MORNA_TRY(d_tptr.alloc((size_t)nq + 1));
        MORNA_TRY(d_tline.alloc((size_t)std::max<int64_t>(t_n, 1)));
        HIP_TRY(hipMemcpy(d_tptr.p, tp.data(), tp.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        if (t_n) HIP_TRY(hipMemcpy(d_tline.p, t_line + t_base, (size_t)t_n * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    EventPair ev;
    MORNA_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.a, st->stream));
    HIP_TRY(hipMemsetAsync(d_hist.p, 0, n_hist * sizeof(int32_t), st->stream));
    if (pre)
        hipLaunchKernelGGL(jstore_recovery_sweep_kernel, dim3((unsigned)(nq * n_tiles)), dim3(JT_THREADS), 0, st->stream, st->d_ptr.p,
                           st->d_line.p, st->d_cov.p, st->n_lines, (int32_t)n_tiles, d_rows.p, d_nres.p, k, (const int32_t *)d_truth_rows.p,
                           truth_min_cov, (const int64_t *)d_tptr.p, (const int32_t *)d_tline.p, grid, *pre, d_hist.p);
    else
        hipLaunchKernelGGL(jstore_recovery_kernel, dim3((unsigned)(nq * n_tiles)), dim3(JT_THREADS), 0, st->stream, st->d_ptr.p, st->d_line.p,
                           st->d_cov.p, st->n_lines, (int32_t)n_tiles, d_rows.p, d_nres.p, k, (const int32_t *)d_truth_rows.p, truth_min_cov,
                           (const int64_t *)d_tptr.p, (const int32_t *)d_tline.p, grid, d_hist.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, st->stream));
    HIP_TRY(hipMemcpyAsync(hist_out, d_hist.p, n_hist * sizeof(int32_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    st->rec_ms = ms;
    st->rec_bytes = 8 * entries + 4 * t_n;   // (line, coverage) of every row named, read once; a CSR truth has lines only
    st->rec_groups = nq * n_tiles;
    return MORNA_OK;
}

// the checks both entry points share; MORNA_OK with *grid filled
int recovery_arguments(const morna_jstore *s, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k,
                       const int64_t *cov_grid, int32_t n_grid, const int32_t *hist_out, JRGrid *grid)
{
    if (!s || nq < 0 || (nq > 0 && (!results || !n_results || !hist_out))) {
        set_error("jstore_recovery: null argument");
        return MORNA_E_INVALID;
    }
    if (k < 1 || k > 64) {
        set_error("jstore_recovery: %d results per list: the recovery tables take 1 to 64, as the filter does (one bit per rank in "
                  "a 64-bit word per line)", k);
        return MORNA_E_INVALID;
    }
    if (n_grid < 1 || n_grid > JR_MAX_GRID) {
        set_error("jstore_recovery: %d coverage thresholds: a grid holds 1 to %d", n_grid, JR_MAX_GRID);
        return MORNA_E_INVALID;
    }
    if (!cov_grid) {
        set_error("jstore_recovery: null argument");
        return MORNA_E_INVALID;
    }
    for (int32_t i = 0; i < JR_MAX_GRID; i++) grid->c[i] = i < n_grid ? cov_grid[i] : INT64_MAX;
    grid->n = n_grid;
    for (int32_t i = 1; i < n_grid; i++)
        if (cov_grid[i] <= cov_grid[i - 1]) {
            set_error("jstore_recovery: coverage threshold %d (%lld) is not above threshold %d (%lld): the grid must ascend strictly",
                      i, (long long)cov_grid[i], i - 1, (long long)cov_grid[i - 1]);
            return MORNA_E_INVALID;
        }
    return MORNA_OK;
}

// the prefix lengths of a sweep; MORNA_OK with *pre filled
int sweep_arguments(const int32_t *prefixes, int32_t n_prefixes, JRPrefixes *pre)
{
    if (!prefixes) {
        set_error("jstore_recovery_sweep: null argument (prefixes)");
        return MORNA_E_INVALID;
    }
    if (n_prefixes < 1 || n_prefixes > JR_MAX_PREFIXES) {
        set_error("jstore_recovery_sweep: %d prefix lengths: a sweep holds 1 to %d", n_prefixes, JR_MAX_PREFIXES);
        return MORNA_E_INVALID;
    }
    for (int32_t i = 0; i < JR_MAX_PREFIXES; i++) pre->p[i] = i < n_prefixes ? prefixes[i] : 64;
    pre->n = n_prefixes;
    for (int32_t i = 0; i < n_prefixes; i++) {
        if (prefixes[i] < 1 || prefixes[i] > 64) {
            set_error("jstore_recovery_sweep: prefix length %d (%d) is outside 1 to 64, the results a list holds", i, prefixes[i]);
            return MORNA_E_INVALID;
        }
        if (i > 0 && prefixes[i] <= prefixes[i - 1]) {
            set_error("jstore_recovery_sweep: prefix length %d (%d) is not above prefix length %d (%d): the lengths must ascend strictly",
                      i, prefixes[i], i - 1, prefixes[i - 1]);
            return MORNA_E_INVALID;
        }
    }
    return MORNA_OK;
}

}  // namespace

int morna::jstore_make_resident(morna_jstore *st) { return make_resident(st); }

extern "C" {

int morna_jstore_free(morna_jstore *s)
{
    if (s && s->resident) (void)hipSetDevice(s->device);
    delete s;
    return MORNA_OK;
}

int morna_jstore_build(int32_t device, const morna_lines *all_lines, morna_jstore **out)
{
    if (!all_lines || !out) {
        set_error("jstore_build: null argument");
        return MORNA_E_INVALID;
    }
    *out = nullptr;
    return guarded("jstore_build", MORNA_E_INVALID, [&] {
        std::unique_ptr<morna_jstore> st(new morna_jstore());
        st->device = device;
        MORNA_TRY(build_impl(st.get(), all_lines));
        *out = st.release();
        return MORNA_OK;
    });
}

int morna_jstore_from_arrays(int32_t device, const int64_t *ext_ids, int64_t n_samples, const int64_t *ptr, const int32_t *line,
                             const int32_t *cov, int64_t n_lines, morna_jstore **out)
{
    if (!out || n_samples < 0 || !ptr || (n_samples > 0 && !ext_ids)) {
        set_error("jstore_from_arrays: null argument");
        return MORNA_E_INVALID;
    }
    *out = nullptr;
    const int64_t nnz = ptr[n_samples];
    if (nnz < 0 || (nnz > 0 && (!line || !cov))) {
        set_error("jstore_from_arrays: the offsets end at %lld", (long long)nnz);
        return MORNA_E_INVALID;
    }
    return guarded("jstore_from_arrays", MORNA_E_INVALID, [&] {
        std::unique_ptr<morna_jstore> st(new morna_jstore());
        st->device = device;
        st->n_lines = n_lines;
        st->ext_ids.assign(ext_ids, ext_ids + n_samples);
        st->ptr.assign(ptr, ptr + n_samples + 1);
        st->line.assign(line, line + nnz);
        st->cov.assign(cov, cov + nnz);
        MORNA_TRY(validate_store(st.get(), "jstore_from_arrays: the input", MORNA_E_INVALID));
        *out = st.release();
        return MORNA_OK;
    });
}

// "MORNAJS1", S, nnz, n_lines (int64 each), ext_ids[S] int64, ptr[S + 1] int64, line[nnz] int32, cov[nnz] int32
int morna_jstore_save(const morna_jstore *s, const char *path)
{
    if (!s || !path) {
        set_error("jstore_save: null argument");
        return MORNA_E_INVALID;
    }
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long long)getpid());
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) {
        set_error("Unable to open %s for writing", tmp.c_str());
        return MORNA_E_IO;
    }
    const int64_t head[3] = {(int64_t)s->ext_ids.size(), (int64_t)s->line.size(), s->n_lines};
    auto put = [&](const void *p, size_t elt, size_t n) { return n == 0 || fwrite(p, elt, n, f) == n; };
    bool ok = put(JSTORE_MAGIC, 1, 8) && put(head, 8, 3) && put(s->ext_ids.data(), 8, s->ext_ids.size()) &&
              put(s->ptr.data(), 8, s->ptr.size()) && put(s->line.data(), 4, s->line.size()) && put(s->cov.data(), 4, s->cov.size());
    ok = (fclose(f) == 0) && ok;
    ok = ok && rename(tmp.c_str(), path) == 0;
    if (!ok) {
        (void)remove(tmp.c_str());
        set_error("short write to %s", path);
        return MORNA_E_IO;
    }
    return MORNA_OK;
}

int morna_jstore_load(const char *path, int32_t device, morna_jstore **out)
{
    if (!path || !out) {
        set_error("jstore_load: null argument");
        return MORNA_E_INVALID;
    }
    *out = nullptr;
    FILE *f = fopen(path, "rb");
    if (!f) {
        set_error("Unable to open %s", path);
        return MORNA_E_IO;
    }
    const int rc = guarded("jstore_load", MORNA_E_IO, [&] {
        std::unique_ptr<morna_jstore> st(new morna_jstore());
        st->device = device;
        char magic[8];
        int64_t head[3] = {0, 0, 0};
        bool ok = fread(magic, 1, 8, f) == 8 && memcmp(magic, JSTORE_MAGIC, 8) == 0 && fread(head, 8, 3, f) == 3;
        if (ok) {   // the counts must account for the file's size exactly before anything is allocated from them
            for (int i = 0; i < 3; i++) ok = ok && head[i] >= 0 && head[i] < ((int64_t)1 << 56);
            const long here = ftell(f);
            ok = ok && fseek(f, 0, SEEK_END) == 0;
            const long size = ftell(f);
            ok = ok && fseek(f, here, SEEK_SET) == 0;
            ok = ok && (double)size == (double)here + 8.0 * (double)head[0] + 8.0 * ((double)head[0] + 1) + 8.0 * (double)head[1];
        }
        auto get = [&](void *p, size_t elt, size_t n) { return n == 0 || fread(p, elt, n, f) == n; };
        if (ok) {
            st->n_lines = head[2];
            st->ext_ids.resize((size_t)head[0]);
            st->ptr.resize((size_t)head[0] + 1);
            st->line.resize((size_t)head[1]);
            st->cov.resize((size_t)head[1]);
            ok = get(st->ext_ids.data(), 8, st->ext_ids.size()) && get(st->ptr.data(), 8, st->ptr.size()) &&
                 get(st->line.data(), 4, st->line.size()) && get(st->cov.data(), 4, st->cov.size()) && fgetc(f) == EOF;
        }
        if (!ok) {
            set_error("%s is not a junction store (or is truncated)", path);
            return MORNA_E_IO;
        }
        MORNA_TRY(validate_store(st.get(), path, MORNA_E_IO));
        *out = st.release();
        return MORNA_OK;
    });
    fclose(f);   // on every path: nothing above returns or throws past the guard
    return rc;
}

int morna_jstore_counts(const morna_jstore *s, int64_t *counts)
{
    if (!s || !counts) {
        set_error("jstore_counts: null argument");
        return MORNA_E_INVALID;
    }
    counts[0] = (int64_t)s->ext_ids.size();
    counts[1] = (int64_t)s->line.size();
    counts[2] = s->n_lines;
    return MORNA_OK;
}

int morna_jstore_samples(const morna_jstore *s, int64_t *ext_ids_out)
{
    if (!s || !ext_ids_out) {
        set_error("jstore_samples: null argument");
        return MORNA_E_INVALID;
    }
    if (!s->ext_ids.empty()) memcpy(ext_ids_out, s->ext_ids.data(), s->ext_ids.size() * sizeof(int64_t));
    return MORNA_OK;
}

int morna_jstore_sample(const morna_jstore *s, int64_t ext_id, int64_t *n_out, int32_t *line_out, int32_t *cov_out)
{
    if (!s || !n_out) {
        set_error("jstore_sample: null argument");
        return MORNA_E_INVALID;
    }
    auto it = s->row_of.find(ext_id);
    if (it == s->row_of.end()) {
        set_error("sample id %lld is not in the junction store", (long long)ext_id);
        return MORNA_E_RANGE;
    }
    const int64_t a = s->ptr[(size_t)it->second], b = s->ptr[(size_t)it->second + 1];
    *n_out = b - a;
    if (line_out && b > a) memcpy(line_out, s->line.data() + a, (size_t)(b - a) * sizeof(int32_t));
    if (cov_out && b > a) memcpy(cov_out, s->cov.data() + a, (size_t)(b - a) * sizeof(int32_t));
    return MORNA_OK;
}

int morna_jstore_timers(const morna_jstore *s, double *ms, int64_t *bytes)
{
    if (!s || !ms || !bytes) {
        set_error("jstore_timers: null argument");
        return MORNA_E_INVALID;
    }
    for (int i = 0; i < 2; i++) {
        ms[i] = s->ms[i];
        bytes[i] = s->bytes[i];
    }
    return MORNA_OK;
}

int morna_jstore_retain(morna_jstore *s, const int64_t *results, const int32_t *n_results, const int32_t *min_count, int64_t nq, int32_t k,
                        int64_t coverage_filter, morna_jretained **out)
{
    if (!s || !out || nq < 0 || (nq > 0 && (!results || !n_results || !min_count))) {
        set_error("jstore_retain: null argument");
        return MORNA_E_INVALID;
    }
    *out = nullptr;
    if (k < 1 || k > 64) {
        set_error("jstore_retain: %d results per list: the filter takes 1 to 64 (found_in is one 64-bit word per line)", k);
        return MORNA_E_INVALID;
    }
    return guarded("jstore_retain", MORNA_E_INVALID, [&] {
        std::unique_ptr<morna_jretained> R(new morna_jretained());
        MORNA_TRY(retain_impl(s, results, n_results, min_count, nq, k, coverage_filter, R.get()));
        *out = R.release();
        return MORNA_OK;
    });
}

int morna_jstore_recovery(morna_jstore *s, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k, const int64_t *t_ptr,
                          const int32_t *t_line, const int64_t *cov_grid, int32_t n_grid, int32_t *hist_out)
{
    JRGrid grid;
    MORNA_TRY(recovery_arguments(s, results, n_results, nq, k, cov_grid, n_grid, hist_out, &grid));
    if (nq > 0 && (!t_ptr || (t_ptr[nq] > t_ptr[0] && !t_line))) {
        set_error("jstore_recovery: null argument");
        return MORNA_E_INVALID;
    }
    return guarded("jstore_recovery", MORNA_E_INVALID,
                   [&] { return recovery_impl(s, results, n_results, nq, k, t_ptr, t_line, nullptr, 0, grid, nullptr, hist_out); });
}

int morna_jstore_recovery_by_sample(morna_jstore *s, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k,
                                    const int64_t *truth_ext, int64_t truth_min_cov, const int64_t *cov_grid, int32_t n_grid,
                                    int32_t *hist_out)
{
    JRGrid grid;
    MORNA_TRY(recovery_arguments(s, results, n_results, nq, k, cov_grid, n_grid, hist_out, &grid));
    if (nq > 0 && !truth_ext) {
        set_error("jstore_recovery: null argument");
        return MORNA_E_INVALID;
    }
    return guarded("jstore_recovery", MORNA_E_INVALID,
                   [&] { return recovery_impl(s, results, n_results, nq, k, nullptr, nullptr, truth_ext, truth_min_cov, grid, nullptr, hist_out); });
}

int morna_jstore_recovery_sweep(morna_jstore *s, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k,
                                const int64_t *t_ptr, const int32_t *t_line, const int64_t *cov_grid, int32_t n_grid,
                                const int32_t *prefixes, int32_t n_prefixes, int32_t *hist_out)
{
    JRGrid grid;
    JRPrefixes pre;
    MORNA_TRY(recovery_arguments(s, results, n_results, nq, k, cov_grid, n_grid, hist_out, &grid));
    MORNA_TRY(sweep_arguments(prefixes, n_prefixes, &pre));
    if (nq > 0 && (!t_ptr || (t_ptr[nq] > t_ptr[0] && !t_line))) {
        set_error("jstore_recovery: null argument");
        return MORNA_E_INVALID;
    }
    return guarded("jstore_recovery_sweep", MORNA_E_INVALID,
                   [&] { return recovery_impl(s, results, n_results, nq, k, t_ptr, t_line, nullptr, 0, grid, &pre, hist_out); });
}

int morna_jstore_recovery_sweep_by_sample(morna_jstore *s, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k,
                                          const int64_t *truth_ext, int64_t truth_min_cov, const int64_t *cov_grid, int32_t n_grid,
                                          const int32_t *prefixes, int32_t n_prefixes, int32_t *hist_out)
{
    JRGrid grid;
    JRPrefixes pre;
    MORNA_TRY(recovery_arguments(s, results, n_results, nq, k, cov_grid, n_grid, hist_out, &grid));
    MORNA_TRY(sweep_arguments(prefixes, n_prefixes, &pre));
    if (nq > 0 && !truth_ext) {
        set_error("jstore_recovery: null argument");
        return MORNA_E_INVALID;
    }
    return guarded("jstore_recovery_sweep", MORNA_E_INVALID, [&] {
        return recovery_impl(s, results, n_results, nq, k, nullptr, nullptr, truth_ext, truth_min_cov, grid, &pre, hist_out);
    });
}

int morna_jstore_recovery_stats(const morna_jstore *s, double *stats)
{
    if (!s || !stats) {
        set_error("jstore_recovery_stats: null argument");
        return MORNA_E_INVALID;
    }
    stats[0] = s->rec_ms;
    stats[1] = (double)s->rec_bytes;
    stats[2] = (double)s->rec_groups;
    return MORNA_OK;
}

int morna_jstore_pool(morna_jstore *s, const int64_t *members, const int64_t *g_ptr, int64_t n_groups, morna_jpooled **out)
{
    if (!s || !out || n_groups < 0 || (n_groups > 0 && !g_ptr)) {
        set_error("jstore_pool: null argument");
        return MORNA_E_INVALID;
    }
    *out = nullptr;
    return guarded("jstore_pool", MORNA_E_INVALID, [&] {
        std::unique_ptr<morna_jpooled> R(new morna_jpooled());
        MORNA_TRY(pool_impl(s, members, g_ptr, n_groups, R.get()));
        *out = R.release();
        return MORNA_OK;
    });
}

int morna_jpooled_counts(const morna_jpooled *r, int64_t *count_out)
{
    if (!r || (r->ng > 0 && !count_out)) {
        set_error("jpooled_counts: null argument");
        return MORNA_E_INVALID;
    }
    for (int64_t g = 0; g < r->ng; g++) count_out[g] = r->off[(size_t)g + 1] - r->off[(size_t)g];
    return MORNA_OK;
}

int morna_jpooled_group(const morna_jpooled *r, int64_t g, const int32_t **lines, const int64_t **sums, const int32_t **holders)
{
    if (!r) {
        set_error("jpooled_group: null argument");
        return MORNA_E_INVALID;
    }
    if (g < 0 || g >= r->ng) {
        set_error("jpooled_group: group %lld out of range [0, %lld)", (long long)g, (long long)r->ng);
        return MORNA_E_RANGE;
    }
    const size_t at = (size_t)r->off[(size_t)g];
    if (lines) *lines = r->lines.data() + at;
    if (sums) *sums = r->sums.data() + at;
    if (holders) *holders = r->holders.data() + at;
    return MORNA_OK;
}

int morna_jpooled_free(morna_jpooled *r)
{
    delete r;
    return MORNA_OK;
}

int morna_jstore_pool_stats(const morna_jstore *s, double *stats)
{
    if (!s || !stats) {
        set_error("jstore_pool_stats: null argument");
        return MORNA_E_INVALID;
    }
    stats[0] = s->pool_ms;
    stats[1] = (double)s->pool_read;
    stats[2] = (double)s->pool_written;
    stats[3] = (double)s->pool_groups;
    return MORNA_OK;
}

int morna_jstore_thin(morna_jstore *s, const int64_t *ext, const uint64_t *keep, int64_t nq, uint32_t seed, morna_jthinned **out)
{
    if (s) {   // a refused call leaves no statistics of an earlier one
        s->thin_ms = 0;
        s->thin_read = s->thin_written = s->thin_draws = s->thin_groups = 0;
    }
    if (!s || !out || nq < 0 || (nq > 0 && (!ext || !keep))) {
        set_error("jstore_thin: null argument");
        return MORNA_E_INVALID;
    }
    *out = nullptr;
    return guarded("jstore_thin", MORNA_E_INVALID, [&] {
        std::unique_ptr<morna_jthinned> R(new morna_jthinned());
        MORNA_TRY(thin_impl(s, ext, keep, nq, seed, R.get()));
        *out = R.release();
        return MORNA_OK;
    });
}

int morna_jthinned_counts(const morna_jthinned *r, int64_t *count_out)
{
    if (!r || (r->nq > 0 && !count_out)) {
        set_error("jthinned_counts: null argument");
        return MORNA_E_INVALID;
    }
    for (int64_t q = 0; q < r->nq; q++) count_out[q] = r->off[(size_t)q + 1] - r->off[(size_t)q];
    return MORNA_OK;
}

int morna_jthinned_job(const morna_jthinned *r, int64_t q, const int32_t **lines, const int32_t **cov)
{
    if (!r) {
        set_error("jthinned_job: null argument");
        return MORNA_E_INVALID;
    }
    if (q < 0 || q >= r->nq) {
        set_error("jthinned_job: job %lld out of range [0, %lld)", (long long)q, (long long)r->nq);
        return MORNA_E_RANGE;
    }
    const size_t at = (size_t)r->off[(size_t)q];
    if (lines) *lines = r->lines.data() + at;
    if (cov) *cov = r->cov.data() + at;
    return MORNA_OK;
}

int morna_jthinned_free(morna_jthinned *r)
{
    delete r;
    return MORNA_OK;
}

int morna_jstore_thin_stats(const morna_jstore *s, double *stats)
{
    if (!s || !stats) {
        set_error("jstore_thin_stats: null argument");
        return MORNA_E_INVALID;
    }
    stats[0] = s->thin_ms;
    stats[1] = (double)s->thin_read;
    stats[2] = (double)s->thin_written;
    stats[3] = (double)s->thin_draws;
    stats[4] = (double)s->thin_groups;
    return MORNA_OK;
}

int morna_jretained_counts(const morna_jretained *r, int64_t *count_out)
{
    if (!r || (r->nq > 0 && !count_out)) {
        set_error("jretained_counts: null argument");
        return MORNA_E_INVALID;
    }
    for (int64_t q = 0; q < r->nq; q++) count_out[q] = r->off[(size_t)q + 1] - r->off[(size_t)q];
    return MORNA_OK;
}

int morna_jretained_query(const morna_jretained *r, int64_t q, const int32_t **lines, const uint64_t **masks, const int64_t **cov_ptr,
                          const int32_t **cov)
{
    if (!r) {
        set_error("jretained_query: null argument");
        return MORNA_E_INVALID;
    }
    if (q < 0 || q >= r->nq) {
        set_error("jretained_query: query %lld out of range [0, %lld)", (long long)q, (long long)r->nq);
        return MORNA_E_RANGE;
    }
    const size_t at = (size_t)r->off[(size_t)q];
    if (lines) *lines = r->lines.data() + at;
    if (masks) *masks = r->masks.data() + at;
    if (cov_ptr) *cov_ptr = r->cov_ptr.data() + at;
    if (cov) *cov = r->cov.data();
    return MORNA_OK;
}

int morna_jretained_free(morna_jretained *r)
{
    delete r;
    return MORNA_OK;
}

}  // extern "C"
