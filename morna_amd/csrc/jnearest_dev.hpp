// jnearest_dev.hpp -- what the unhashed search (nearest.hip) and the explanation of its results (explain.hip) share:
// the ordered sums of the contract, the radicand, the dense query image and the rule for its width.
// Every name here is local to the file that includes it.
#pragma once
#include <math.h>
#include <stdlib.h>

#include "jstore.hpp"

namespace {

#define JN_THREADS 256
#define JN_WAVES (JN_THREADS / WAVE)

__device__ inline double lane_value(double x, int j)   // j: a constant
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), j);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
    return __hiloint2double(hi, lo);
}

// acc = RN(acc + term of lane 0), then of lane 1, ... lane 63: the same value in every lane (whole waves only)
__device__ inline double wave_add_in_order(double acc, double term)
{
#pragma unroll
    for (int j = 0; j < WAVE; j++) acc = __dadd_rn(acc, lane_value(term, j));
    return acc;
}

// The contract's sum over the list [a, b) by one whole wave: RN(v * v) (SELF) or RN(v * image[line][t]) of every entry,
// added in list order from 0.0.  The lanes past the end add +0.0, which changes no sum of non-negative terms.
// neg (SELF only): smallest (tag << 32 | line) of a negative coverage.
template <bool SELF>
__device__ inline double wave_list_sum(const int32_t *__restrict__ line, const int32_t *__restrict__ cov, int64_t a, int64_t b,
                                       const double *__restrict__ w, const double *__restrict__ tile, int32_t qt, int32_t t, int lane,
                                       unsigned long long *neg, uint32_t tag)
{
    double acc = 0.0;
    for (int64_t i0 = a; i0 < b; i0 += WAVE) {
        const int64_t i = i0 + lane;
        double term = 0.0;
        if (i < b) {
            const int32_t l = line[i], c = cov[i];
            const double v = __dmul_rn((double)c, w[l]);
            term = SELF ? __dmul_rn(v, v) : __dmul_rn(v, tile[(int64_t)l * qt + t]);
            if (SELF && neg && c < 0) atomicMin(neg, ((unsigned long long)tag << 32) | (uint32_t)l);
        }
        acc = wave_add_in_order(acc, term);
    }
    return acc;
}

__device__ inline double jn_radicand(double pp, double qq, double pq)
{
    const double ppqq = __dmul_rn(pp, qq);
    if (!(ppqq > 0.0)) return 2.0;
    return __dsub_rn(2.0, __ddiv_rn(__dmul_rn(2.0, pq), __dsqrt_rn(ppqq)));
}

// a workgroup per query of the tile: its components into column t of the (zeroed) image, its qq
__global__ __launch_bounds__(JN_THREADS) void jnearest_tile_kernel(const int32_t *__restrict__ line, const int32_t *__restrict__ cov,
                                                                   const int64_t *__restrict__ qrange, const double *__restrict__ w,
                                                                   int32_t qt, double *__restrict__ tile, double *__restrict__ qq_out)
{
    const int t = blockIdx.x, tid = threadIdx.x;
    const int64_t a = qrange[2 * t], b = qrange[2 * t + 1];
    for (int64_t i = a + tid; i < b; i += JN_THREADS) {
        const int32_t l = line[i];
        tile[(int64_t)l * qt + t] = __dmul_rn((double)cov[i], w[l]);
    }
    if (tid < WAVE) {
        const double qq = wave_list_sum<true>(line, cov, a, b, w, nullptr, 0, 0, tid, nullptr, 0);
        if (tid == 0) qq_out[t] = qq;
    }
}

// Queries per pass.  One store entry gathers QT adjacent doubles of the image, so a larger QT spends the stream of the
// store on more queries -- as long as the image stays where the gathers are cheap: 16 while [n_lines][16] doubles fit one
// XCD's 4 MiB L2 (n_lines <= 32768), else 8 (64 B per line: 4.5 MB at 70 000 lines, about that L2; with millions of lines
// the image lives in the Infinity Cache and a wider one would only leave it sooner).  MORNA_UNHASHED_QT = 4 | 8 | 16
// overrides (the answers do not depend on it; tests use it to show so).
inline int choose_qt(int64_t n_lines)
{
    const char *v = getenv("MORNA_UNHASHED_QT");
    if (v) {
        const int q = atoi(v);
        if (q == 4 || q == 8 || q == 16) return q;
    }
    return n_lines * 16 * (int64_t)sizeof(double) <= ((int64_t)4 << 20) ? 16 : 8;
}

}  // namespace
