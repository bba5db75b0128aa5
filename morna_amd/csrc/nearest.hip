// nearest.hip -- unhashed TF-IDF nearest neighbours over the junction store.
//
// The yardstick the reference's author began and left unfinished (commanderson/morna tests/construct_tf_idf.py writes the
// per-junction scores; tests/query_tfidf_db.py stops at its cosine top-20): the samples ranked by cosine_distance
// (morna.py:101-114) in the space of the junctions themselves, one dimension per line of the indexed file, instead of
// the `dim` hashed columns every other search ranks in.  The store of jstore.hip is that matrix's sample-major CSR, so
// the search is a sparse-row x dense-query scan over it and a top-k.
//
// The contract fixes every rounding: a component is v = RN(double(cov) * w[line]); pp, qq and pq are x = RN(x + RN(a * b))
// over ascending lines from 0.0 (a line one side lacks adds +0.0, so the sum over a row's own entries IS the dense loop);
// ppqq = RN(pp * qq); radicand = 2.0 - 2.0 * pq / sqrt(ppqq) when ppqq > 0, else 2.0; distance = sqrt(max(radicand, 0.0)).
// A sequential fp64 sum per (row, query) pair would leave the GPU idle, so the pairs are filtered first:
//   jnearest_norms_kernel   pp of every population row in the contract's order (cached per weights and population);
//                           flags negative coverages
//   jnearest_tile_kernel    QT queries scattered into a dense [n_lines][QT] fp64 image -- one store entry then gathers QT
//                           adjacent values -- and their qq in the contract's order
//   jnearest_scan_kernel    a wave per row streams (line, cov) coalesced, gathers the weight and the image's QT values,
//                           sums pq in fp64 lane by lane and reduces by a fixed butterfly: the pass-1 radicand, from the
//                           exact pp and qq and that pq
//   jnearest_select_kernel  the k-th smallest pass-1 radicand T; the candidates are the rows at or below
//                           max(T, 0) + window, the window DERIVED from the fp64 error bound of the two sums
//   jnearest_rerank_kernel  the contract's sequential pq for the candidates only (a wave per candidate multiplies 64
//                           entries at a time, then adds the 64 products in order), the distances, and the final
//                           (distance, higher id first) top-k
// No floating atomics; the answers are the re-rank's and depend neither on the run nor on QT.
// The ordered sums, the radicand, jnearest_tile_kernel and the rule for QT live in jnearest_dev.hpp: explain.hip (N17) makes
// the same quantities pair by pair.
#include <math.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "jnearest_dev.hpp"
#include "jstore.hpp"

using morna::DevBuf;
using morna::EventPair;
using morna::guarded;
using morna::set_error;

struct morna_jnearest {
    std::vector<double> w;          // [n_lines] host copy of the weights
    bool w_resident = false;
    DevBuf<double> d_w;
    // the population of the last search: its store rows, their norms
    bool pop_valid = false;
    std::vector<int64_t> pop_ext;
    int64_t pop_entries = 0, pop_longest = 0;
    DevBuf<int32_t> d_pop_rows;
    DevBuf<double> d_pp;
    // scratch of a search, kept between calls
    DevBuf<double> d_tile, d_qq, d_rad, d_cdist, d_dist;
    DevBuf<int32_t> d_coll, d_cand, d_ncand, d_ids, d_cnt, d_qline, d_qcov;
    DevBuf<int64_t> d_qrange;
    DevBuf<unsigned long long> d_err;
    double stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace {

const double JN_U = 1.1102230246251565e-16;   // 2^-53, the unit roundoff of fp64
const double JN_W_MIN = 6.223015277861142e-61;   // 2^-200
const double JN_W_MAX = 18446744073709551616.0;  // 2^64

// a wave per population row
__global__ __launch_bounds__(JN_THREADS) void jnearest_norms_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                                    const int32_t *__restrict__ cov, const double *__restrict__ w,
                                                                    const int32_t *__restrict__ pop_rows, int64_t n_pop,
                                                                    double *__restrict__ pp_out, unsigned long long *err)
{
    const int lane = threadIdx.x % WAVE;
    const int64_t p = (int64_t)blockIdx.x * JN_WAVES + threadIdx.x / WAVE;
    if (p >= n_pop) return;
    const int32_t row = pop_rows[p];
    const double pp = wave_list_sum<true>(line, cov, ptr[row], ptr[row + 1], w, nullptr, 0, 0, lane, err, (uint32_t)p);
    if (lane == 0) pp_out[p] = pp;
}

// a wave per population row: rad[t][p] for the nt queries of the tile
template <int QT>
__global__ __launch_bounds__(JN_THREADS) void jnearest_scan_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                                   const int32_t *__restrict__ cov, const double *__restrict__ w,
                                                                   const int32_t *__restrict__ pop_rows, int64_t n_pop,
                                                                   const double *__restrict__ tile, const double *__restrict__ pp,
                                                                   const double *__restrict__ qq, int32_t nt, double *__restrict__ rad)
{
    const int lane = threadIdx.x % WAVE;
    const int64_t p = (int64_t)blockIdx.x * JN_WAVES + threadIdx.x / WAVE;
    if (p >= n_pop) return;
    const int32_t row = pop_rows[p];
    const int64_t a = ptr[row], b = ptr[row + 1];
    double acc[QT];
#pragma unroll
    for (int t = 0; t < QT; t++) acc[t] = 0.0;
    for (int64_t i = a + lane; i < b; i += WAVE) {
        const int32_t l = line[i];
        const double v = (double)cov[i] * w[l];
        if (v != 0.0) {   // (lines under the index's threshold weigh nothing: no gather for them)
            const double2 *q2 = (const double2 *)(tile + (int64_t)l * QT);
#pragma unroll
            for (int t = 0; t < QT / 2; t++) {
                const double2 q = q2[t];
                acc[2 * t] += v * q.x;
                acc[2 * t + 1] += v * q.y;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < QT; t++) {
#pragma unroll
        for (int off = WAVE / 2; off >= 1; off >>= 1) acc[t] += __shfl_xor(acc[t], off, WAVE);
    }
    const double my_pp = pp[p];
#pragma unroll
    for (int t = 0; t < QT; t++)
        if (lane == t && t < nt) rad[(int64_t)t * n_pop + p] = jn_radicand(my_pp, qq[t], acc[t]);
}

// A workgroup per query of the tile.  The smallest value of every thread's strided share: the kk-th smallest of those
// 256 bounds the kk-th smallest of all from above.  Everything at or below max(bound, 0) + window is collected; the kk-th
// smallest of the collected IS the kk-th smallest of all (T); the candidates are the collected at or below
// max(T, 0) + window.  The lists are in no particular order: the re-rank ranks.  n_pop >= 1, kk = min(k, n_pop); beyond 256
// (one minimum per thread) the first bound is +inf.
__global__ __launch_bounds__(256) void jnearest_select_kernel(const double *__restrict__ rad, int64_t n_pop, int32_t k, double window,
                                                              int32_t *__restrict__ coll, int32_t *__restrict__ cand,
                                                              int32_t *__restrict__ ncand)
{
    __shared__ double s_min[256];
    __shared__ double s_thr;
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x;
    const double *r = rad + t * n_pop;
    int32_t *cl = coll + t * n_pop, *cd = cand + t * n_pop;
    const int kk = (int)(k < n_pop ? k : n_pop);
    double mine = INFINITY;
    for (int64_t i = tid; i < n_pop; i += 256) {
        const double v = r[i];
        mine = v < mine ? v : mine;
    }
    s_min[tid] = mine;
    if (tid == 0) s_n = 0;
    __syncthreads();
    if (kk <= 256) {
        int below = 0;
        for (int j = 0; j < 256; j++) below += (s_min[j] < mine || (s_min[j] == mine && j < tid)) ? 1 : 0;
        if (below == kk - 1) s_thr = mine;
    } else if (tid == 0) {
        s_thr = INFINITY;   // more neighbours than minima: every row is collected
    }
    __syncthreads();
    const double bound = (s_thr > 0.0 ? s_thr : 0.0) + window;
    for (int64_t i = tid; i < n_pop; i += 256)
        if (r[i] <= bound) cl[atomicAdd(&s_n, 1)] = (int32_t)i;
    __syncthreads();
    const int m = s_n;
    __syncthreads();
    for (int u = tid; u < m; u += 256) {
        const int32_t iu = cl[u];
        const double v = r[iu];
        int below = 0;
        for (int x = 0; x < m; x++) {
            const int32_t ix = cl[x];
            const double vx = r[ix];
            below += (vx < v || (vx == v && ix < iu)) ? 1 : 0;
        }
        if (below == kk - 1) s_thr = v;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const double thr = (s_thr > 0.0 ? s_thr : 0.0) + window;
    for (int u = tid; u < m; u += 256) {
        const int32_t iu = cl[u];
        if (r[iu] <= thr) cd[atomicAdd(&s_n, 1)] = iu;
    }
    __syncthreads();
    if (tid == 0) ncand[t] = s_n;
}

// A workgroup per query of the tile: a wave per candidate makes the contract's pq and the distance; then every candidate's
// rank -- the candidates bisect_left insertion over ids 0..n-1 leaves in front of it: a smaller distance, or the same
// distance and a HIGHER id (morna.py:700-712).
__global__ __launch_bounds__(JN_THREADS) void jnearest_rerank_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                                     const int32_t *__restrict__ cov, const double *__restrict__ w,
                                                                     const int32_t *__restrict__ pop_rows, int64_t n_pop,
                                                                     const double *__restrict__ tile, int32_t qt,
                                                                     const double *__restrict__ pp, const double *__restrict__ qq,
                                                                     const int32_t *__restrict__ cand, const int32_t *__restrict__ ncand,
                                                                     int32_t k, double *__restrict__ cdist, int32_t *__restrict__ ids_out,
                                                                     double *__restrict__ dist_out, int32_t *__restrict__ count_out)
{
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const int64_t t = blockIdx.x;
    const int n = ncand[t];
    const int32_t *c = cand + t * n_pop;
    double *cd = cdist + t * n_pop;
    const double my_qq = qq[t];
    for (int u = wave; u < n; u += JN_WAVES) {
        const int32_t p = c[u];
        const int32_t row = pop_rows[p];
        const double pq = wave_list_sum<false>(line, cov, ptr[row], ptr[row + 1], w, tile, qt, (int32_t)t, lane, nullptr, 0);
        if (lane == 0) {
            const double radicand = jn_radicand(pp[p], my_qq, pq);
            cd[u] = __dsqrt_rn(radicand > 0.0 ? radicand : 0.0);
        }
    }
    __syncthreads();
    for (int u = tid; u < n; u += JN_THREADS) {
        const double d = cd[u];
        const int32_t id = c[u];
        int rank = 0;
        for (int x = 0; x < n; x++) {
            const double dx = cd[x];
            rank += (dx < d || (dx == d && c[x] > id)) ? 1 : 0;
        }
        if (rank < k) {
            ids_out[t * k + rank] = id;
            dist_out[t * k + rank] = d;
        }
    }
    const int kout = k < n ? k : n;
    for (int r = kout + tid; r < k; r += JN_THREADS) {
        ids_out[t * k + r] = -1;
        dist_out[t * k + r] = INFINITY;
    }
    if (tid == 0) count_out[t] = kout;
}

// ---- host ---------------------------------------------------------------------------------------------------------

// |pass-1 radicand - contract's radicand| for a row of at most n entries: (5 (n + 1) + 7) u; the
// candidates lie within twice that of max(T, 0), plus 32 u for the rounding of sqrt and of the threshold itself.
double window_for(int64_t n) { return 2.0 * (5.0 * (double)(n + 1) + 7.0) * JN_U + 32.0 * JN_U; }

int prepare_weights(morna_jstore *st, morna_jnearest *nr)
{
    if (nr->w_resident) return MORNA_OK;
    MORNA_TRY(nr->d_w.alloc(nr->w.size()));
    if (!nr->w.empty()) HIP_TRY(hipMemcpy(nr->d_w.p, nr->w.data(), nr->w.size() * sizeof(double), hipMemcpyHostToDevice));
    nr->w_resident = true;
    nr->pop_valid = false;
    return MORNA_OK;
}

// the population's store rows and their norms, unless they are those of the last call
int prepare_population(morna_jstore *st, morna_jnearest *nr, const int64_t *pop_ext, int64_t n_pop)
{
    nr->stats[6] = 0;
    if (nr->pop_valid && (int64_t)nr->pop_ext.size() == n_pop && memcmp(nr->pop_ext.data(), pop_ext, (size_t)n_pop * sizeof(int64_t)) == 0)
        return MORNA_OK;
    nr->pop_valid = false;
    std::vector<int32_t> rows((size_t)n_pop);
    std::vector<uint8_t> seen(st->ext_ids.size(), 0);
    int64_t entries = 0, longest = 0;
    for (int64_t p = 0; p < n_pop; p++) {
        auto it = st->row_of.find(pop_ext[p]);
        if (it == st->row_of.end()) {
            set_error("jstore_nearest: sample id %lld (population entry %lld) is not in the junction store", (long long)pop_ext[p], (long long)p);
            return MORNA_E_RANGE;
        }
        if (seen[(size_t)it->second]) {
            set_error("jstore_nearest: sample id %lld is named twice in the population (second at entry %lld)", (long long)pop_ext[p],
                      (long long)p);
            return MORNA_E_RANGE;
        }
        seen[(size_t)it->second] = 1;
        rows[(size_t)p] = it->second;
        const int64_t len = st->ptr[(size_t)it->second + 1] - st->ptr[(size_t)it->second];
        entries += len;
        longest = std::max(longest, len);
    }
    MORNA_TRY(nr->d_pop_rows.alloc((size_t)n_pop));
    MORNA_TRY(nr->d_pp.alloc((size_t)n_pop));
    MORNA_TRY(nr->d_err.alloc(1));
    HIP_TRY(hipMemcpy(nr->d_pop_rows.p, rows.data(), (size_t)n_pop * sizeof(int32_t), hipMemcpyHostToDevice));
    const unsigned long long none = ~0ull;
    HIP_TRY(hipMemcpy(nr->d_err.p, &none, sizeof(none), hipMemcpyHostToDevice));
    EventPair ev;
    MORNA_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.a, st->stream));
    hipLaunchKernelGGL(jnearest_norms_kernel, dim3((unsigned)((n_pop + JN_WAVES - 1) / JN_WAVES)), dim3(JN_THREADS), 0, st->stream, st->d_ptr.p,
                       st->d_line.p, st->d_cov.p, nr->d_w.p, nr->d_pop_rows.p, n_pop, nr->d_pp.p, nr->d_err.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.b, st->stream));
    unsigned long long err = 0;
    HIP_TRY(hipMemcpyAsync(&err, nr->d_err.p, sizeof(err), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    if (err != ~0ull) {
        set_error("jstore_nearest: sample id %lld has a negative coverage at line %lld: the unhashed search takes coverages >= 0",
                  (long long)pop_ext[(size_t)(err >> 32)], (long long)(err & 0xffffffffull));
        return MORNA_E_INVALID;
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    nr->stats[6] = ms;
    nr->pop_ext.assign(pop_ext, pop_ext + n_pop);
    nr->pop_entries = entries;
    nr->pop_longest = longest;
    nr->pop_valid = true;
    return MORNA_OK;
}

template <int QT>
void launch_scan(morna_jstore *st, morna_jnearest *nr, int64_t n_pop, int32_t nt)
{
    hipLaunchKernelGGL(jnearest_scan_kernel<QT>, dim3((unsigned)((n_pop + JN_WAVES - 1) / JN_WAVES)), dim3(JN_THREADS), 0, st->stream,
                       st->d_ptr.p, st->d_line.p, st->d_cov.p, nr->d_w.p, nr->d_pop_rows.p, n_pop, nr->d_tile.p, nr->d_pp.p, nr->d_qq.p, nt,
                       nr->d_rad.p);
}

// q_line / q_cov: device arrays the ranges index (the store's own for queries by sample); qrange: [nq][2] on the host
int search_impl(morna_jstore *st, morna_jnearest *nr, const int64_t *pop_ext, int64_t n_pop, const int32_t *q_line, const int32_t *q_cov,
                const std::vector<int64_t> &qrange, int64_t nq, int32_t k, int32_t *ids_out, double *dist_out, int32_t *count_out)
{
    MORNA_TRY(prepare_population(st, nr, pop_ext, n_pop));
    const int qt = choose_qt(st->n_lines);
    const double window = window_for(nr->pop_longest);
    const int64_t n_lines = std::max<int64_t>(st->n_lines, 1);
    const size_t tile_bytes = (size_t)n_lines * qt * sizeof(double);
    MORNA_TRY(nr->d_tile.alloc((size_t)n_lines * qt));
    MORNA_TRY(nr->d_qq.alloc((size_t)qt));
    MORNA_TRY(nr->d_rad.alloc((size_t)(n_pop * qt)));
    MORNA_TRY(nr->d_cdist.alloc((size_t)(n_pop * qt)));
    MORNA_TRY(nr->d_coll.alloc((size_t)(n_pop * qt)));
    MORNA_TRY(nr->d_cand.alloc((size_t)(n_pop * qt)));
    MORNA_TRY(nr->d_ncand.alloc((size_t)nq));
    MORNA_TRY(nr->d_ids.alloc((size_t)(nq * k)));
    MORNA_TRY(nr->d_dist.alloc((size_t)(nq * k)));
    MORNA_TRY(nr->d_cnt.alloc((size_t)nq));
    MORNA_TRY(nr->d_qrange.alloc((size_t)(2 * nq)));
    HIP_TRY(hipMemcpy(nr->d_qrange.p, qrange.data(), (size_t)(2 * nq) * sizeof(int64_t), hipMemcpyHostToDevice));
    EventPair ev;
    MORNA_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.a, st->stream));
    int64_t passes = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += qt, passes++) {
        const int32_t nt = (int32_t)std::min<int64_t>(qt, nq - q0);
        HIP_TRY(hipMemsetAsync(nr->d_tile.p, 0, tile_bytes, st->stream));
        hipLaunchKernelGGL(jnearest_tile_kernel, dim3((unsigned)nt), dim3(JN_THREADS), 0, st->stream, q_line, q_cov, nr->d_qrange.p + 2 * q0,
                           nr->d_w.p, qt, nr->d_tile.p, nr->d_qq.p);
        if (qt == 4) launch_scan<4>(st, nr, n_pop, nt);
        else if (qt == 8) launch_scan<8>(st, nr, n_pop, nt);
        else launch_scan<16>(st, nr, n_pop, nt);
        hipLaunchKernelGGL(jnearest_select_kernel, dim3((unsigned)nt), dim3(256), 0, st->stream, nr->d_rad.p, n_pop, k, window, nr->d_coll.p,
                           nr->d_cand.p, nr->d_ncand.p + q0);
        hipLaunchKernelGGL(jnearest_rerank_kernel, dim3((unsigned)nt), dim3(JN_THREADS), 0, st->stream, st->d_ptr.p, st->d_line.p, st->d_cov.p,
                           nr->d_w.p, nr->d_pop_rows.p, n_pop, nr->d_tile.p, qt, nr->d_pp.p, nr->d_qq.p, nr->d_cand.p, nr->d_ncand.p + q0, k,
                           nr->d_cdist.p, nr->d_ids.p + q0 * k, nr->d_dist.p + q0 * k, nr->d_cnt.p + q0);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev.b, st->stream));
    std::vector<int32_t> ncand((size_t)nq);
    HIP_TRY(hipMemcpyAsync(ncand.data(), nr->d_ncand.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(ids_out, nr->d_ids.p, (size_t)(nq * k) * sizeof(int32_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(dist_out, nr->d_dist.p, (size_t)(nq * k) * sizeof(double), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(count_out, nr->d_cnt.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    int64_t total = 0, most = 0;
    for (int64_t q = 0; q < nq; q++) {
        total += ncand[(size_t)q];
        most = std::max<int64_t>(most, ncand[(size_t)q]);
    }
    nr->stats[0] = (double)total;
    nr->stats[1] = (double)most;
    nr->stats[2] = (double)passes;
    nr->stats[3] = ms;
    nr->stats[4] = 8.0 * (double)nr->pop_entries * (double)passes;
    nr->stats[5] = qt;
    nr->stats[7] = window;
    return MORNA_OK;
}

// what both entry points check first; *done: nothing left to do (no query, or an empty population)
int begin(morna_jstore *s, const int64_t *pop_ext, int64_t n_pop, int64_t nq, int32_t k, int32_t *ids_out, double *dist_out,
          int32_t *count_out, bool *done)
{
    *done = false;
    if (!s || n_pop < 0 || nq < 0 || (n_pop > 0 && !pop_ext) || (nq > 0 && (!ids_out || !dist_out || !count_out))) {
        set_error("jstore_nearest: null argument");
        return MORNA_E_INVALID;
    }
    if (!s->nearest) {
        set_error("jstore_nearest: the store has no weights: call morna_jstore_set_weights first");
        return MORNA_E_STATE;
    }
    if (k < 1 || k > MORNA_JNEAREST_MAX_K) {
        set_error("jstore_nearest: %d neighbours asked for: the unhashed search returns 1 to %d per query", k, MORNA_JNEAREST_MAX_K);
        return MORNA_E_INVALID;
    }
    if (n_pop > INT32_MAX / 16) {
        set_error("jstore_nearest: a population of %lld samples: at most %d", (long long)n_pop, INT32_MAX / 16);
        return MORNA_E_INVALID;
    }
    for (int i = 0; i < 8; i++) s->nearest->stats[i] = 0;
    if (nq == 0) {
        *done = true;
        return MORNA_OK;
    }
    if (n_pop == 0) {
        for (int64_t i = 0; i < nq * k; i++) {
            ids_out[i] = -1;
            dist_out[i] = INFINITY;
        }
        for (int64_t q = 0; q < nq; q++) count_out[q] = 0;
        *done = true;
    }
    return MORNA_OK;
}

}  // namespace

int morna::jstore_device_weights(morna_jstore *st, const double **d_w)
{
    MORNA_TRY(prepare_weights(st, st->nearest.get()));
    *d_w = st->nearest->d_w.p;
    return MORNA_OK;
}

extern "C" {

int morna_jstore_row_norms(morna_jstore *s, const int64_t *ext, int64_t n, double *pp_out)
{
    if (!s || n < 0 || (n > 0 && (!ext || !pp_out))) {
        set_error("jstore_row_norms: null argument");
        return MORNA_E_INVALID;
    }
    if (!s->nearest) {
        set_error("jstore_row_norms: the store has no weights: call morna_jstore_set_weights first");
        return MORNA_E_STATE;
    }
    if (n > INT32_MAX / 16) {
        set_error("jstore_row_norms: %lld samples: at most %d", (long long)n, INT32_MAX / 16);
        return MORNA_E_INVALID;
    }
    return guarded("jstore_row_norms", MORNA_E_INVALID, [&] {
        std::vector<int32_t> rows((size_t)n);
        for (int64_t p = 0; p < n; p++) {
            auto it = s->row_of.find(ext[p]);
            if (it == s->row_of.end()) {
                set_error("jstore_row_norms: sample id %lld (entry %lld) is not in the junction store", (long long)ext[p], (long long)p);
                return MORNA_E_RANGE;
            }
            rows[(size_t)p] = it->second;
        }
        if (n == 0) return MORNA_OK;
        MORNA_TRY(morna::jstore_make_resident(s));
        morna_jnearest *nr = s->nearest.get();
        MORNA_TRY(prepare_weights(s, nr));
        // buffers of the call's own: the cached population and its norms stay what the last search left
        DevBuf<int32_t> d_rows;
        DevBuf<double> d_pp;
        DevBuf<unsigned long long> d_err;
        MORNA_TRY(d_rows.alloc((size_t)n));
        MORNA_TRY(d_pp.alloc((size_t)n));
        MORNA_TRY(d_err.alloc(1));
        HIP_TRY(hipMemcpy(d_rows.p, rows.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
        const unsigned long long none = ~0ull;
        HIP_TRY(hipMemcpy(d_err.p, &none, sizeof(none), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(jnearest_norms_kernel, dim3((unsigned)((n + JN_WAVES - 1) / JN_WAVES)), dim3(JN_THREADS), 0, s->stream, s->d_ptr.p,
                           s->d_line.p, s->d_cov.p, nr->d_w.p, d_rows.p, n, d_pp.p, d_err.p);
        HIP_TRY(hipGetLastError());
        unsigned long long err = 0;
        HIP_TRY(hipMemcpyAsync(&err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(pp_out, d_pp.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (err != ~0ull) {
            set_error("jstore_row_norms: sample id %lld has a negative coverage at line %lld: the unhashed search takes coverages >= 0",
                      (long long)ext[(size_t)(err >> 32)], (long long)(err & 0xffffffffull));
            return MORNA_E_INVALID;
        }
        return MORNA_OK;
    });
}

int morna_jstore_set_weights(morna_jstore *s, const double *w, int64_t n_lines)
{
    if (!s || (n_lines > 0 && !w)) {
        set_error("jstore_set_weights: null argument");
        return MORNA_E_INVALID;
    }
    if (n_lines != s->n_lines) {
        set_error("jstore_set_weights: %lld weights for a store of %lld lines", (long long)n_lines, (long long)s->n_lines);
        return MORNA_E_INVALID;
    }
    for (int64_t j = 0; j < n_lines; j++) {
        const double x = w[j];
        if (!(x == 0.0 || (x >= JN_W_MIN && x <= JN_W_MAX))) {   // (a NaN fails every comparison)
            set_error("jstore_set_weights: the weight of line %lld is %g: a weight is 0 or a finite number in [2^-200, 2^64]", (long long)j, x);
            return MORNA_E_INVALID;
        }
    }
    return guarded("jstore_set_weights", MORNA_E_INVALID, [&] {
        auto nr = std::make_shared<morna_jnearest>();
        nr->w.assign(w, w + n_lines);
        for (auto &x : nr->w)
            if (x == 0.0) x = 0.0;   // -0.0 weighs nothing, as +0.0
        if (s->nearest) (void)hipSetDevice(s->device);   // the buffers of the weights replaced are freed here
        s->nearest = nr;
        return MORNA_OK;
    });
}

int morna_jstore_nearest_by_sample(morna_jstore *s, const int64_t *pop_ext, int64_t n_pop, const int64_t *q_ext, int64_t nq, int32_t k,
                                   int32_t *ids_out, double *dist_out, int32_t *count_out)
{
    bool done;
    MORNA_TRY(begin(s, pop_ext, n_pop, nq, k, ids_out, dist_out, count_out, &done));
    if (nq > 0 && !q_ext) {
        set_error("jstore_nearest: null argument");
        return MORNA_E_INVALID;
    }
    return guarded("jstore_nearest", MORNA_E_INVALID, [&] {
        std::vector<int64_t> qrange((size_t)(2 * nq));
        for (int64_t q = 0; q < nq; q++) {
            auto it = s->row_of.find(q_ext[q]);
            if (it == s->row_of.end()) {
                set_error("jstore_nearest: sample id %lld (query %lld) is not in the junction store", (long long)q_ext[q], (long long)q);
                return MORNA_E_RANGE;
            }
            const int64_t a = s->ptr[(size_t)it->second], b = s->ptr[(size_t)it->second + 1];
            for (int64_t i = a; i < b; i++)
                if (s->cov[(size_t)i] < 0) {
                    set_error("jstore_nearest: sample id %lld has a negative coverage at line %d: the unhashed search takes coverages >= 0",
                              (long long)q_ext[q], s->line[(size_t)i]);
                    return MORNA_E_INVALID;
                }
            qrange[(size_t)(2 * q)] = a;
            qrange[(size_t)(2 * q + 1)] = b;
        }
        if (done) return MORNA_OK;
        MORNA_TRY(morna::jstore_make_resident(s));
        MORNA_TRY(prepare_weights(s, s->nearest.get()));
        return search_impl(s, s->nearest.get(), pop_ext, n_pop, s->d_line.p, s->d_cov.p, qrange, nq, k, ids_out, dist_out, count_out);
    });
}

int morna_jstore_nearest(morna_jstore *s, const int64_t *pop_ext, int64_t n_pop, const int64_t *q_ptr, const int32_t *q_line,
                         const int32_t *q_cov, int64_t nq, int32_t k, int32_t *ids_out, double *dist_out, int32_t *count_out)
{
    bool done;
    MORNA_TRY(begin(s, pop_ext, n_pop, nq, k, ids_out, dist_out, count_out, &done));
    if (nq > 0 && (!q_ptr || q_ptr[0] != 0 || (q_ptr[nq] > 0 && (!q_line || !q_cov)))) {
        set_error("jstore_nearest: null argument, or query offsets that do not begin at 0");
        return MORNA_E_INVALID;
    }
    return guarded("jstore_nearest", MORNA_E_INVALID, [&] {
        std::vector<int64_t> qrange((size_t)(2 * nq));
        for (int64_t q = 0; q < nq; q++) {
            const int64_t a = q_ptr[q], b = q_ptr[q + 1];
            if (b < a) {
                set_error("jstore_nearest: the offsets of query %lld descend", (long long)q);
                return MORNA_E_INVALID;
            }
            for (int64_t i = a; i < b; i++) {
                if (q_line[i] < 0 || q_line[i] >= s->n_lines || (i > a && q_line[i] <= q_line[i - 1])) {
                    set_error("jstore_nearest: query %lld, term %lld: line %d; a query's lines ascend, distinct, below the store's %lld lines",
                              (long long)q, (long long)(i - a), q_line[i], (long long)s->n_lines);
                    return MORNA_E_INVALID;
                }
                if (q_cov[i] < 0) {
                    set_error("jstore_nearest: query %lld has a negative coverage at line %d: the unhashed search takes coverages >= 0",
                              (long long)q, q_line[i]);
                    return MORNA_E_INVALID;
                }
            }
            qrange[(size_t)(2 * q)] = a;
            qrange[(size_t)(2 * q + 1)] = b;
        }
        if (done) return MORNA_OK;
        MORNA_TRY(morna::jstore_make_resident(s));
        morna_jnearest *nr = s->nearest.get();
        MORNA_TRY(prepare_weights(s, nr));
        const size_t n_terms = (size_t)q_ptr[nq];
        MORNA_TRY(nr->d_qline.alloc(n_terms));
        MORNA_TRY(nr->d_qcov.alloc(n_terms));
        if (n_terms) {
            HIP_TRY(hipMemcpy(nr->d_qline.p, q_line, n_terms * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(nr->d_qcov.p, q_cov, n_terms * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        return search_impl(s, nr, pop_ext, n_pop, nr->d_qline.p, nr->d_qcov.p, qrange, nq, k, ids_out, dist_out, count_out);
    });
}

int morna_jstore_nearest_stats(const morna_jstore *s, double *stats)
{
    if (!s || !stats) {
        set_error("jstore_nearest_stats: null argument");
        return MORNA_E_INVALID;
    }
    for (int i = 0; i < 8; i++) stats[i] = s->nearest ? s->nearest->stats[i] : 0.0;
    return MORNA_OK;
}

}  // extern "C"
