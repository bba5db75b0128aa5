// explain.hip -- the junctions behind a query and each of its results.
//
// Every search answers with sample ids and one distance each; this is the decomposition of the unhashed cosine (N5) of a
// (query, result row) pair: pq, pp and qq in the contract's order, how much of pp and of qq lies on lines both hold, how
// many lines that are, and the `top` lines of largest term RN(v_r * v_q), equal terms by ascending line.  There is no
// reference counterpart: morna.py prints ids and distances and leaves the rest to the reader of intropolis files.
//
// All arithmetic is nearest.hip's: a component is v = RN(double(cov) * w[line]); a sum is x = RN(x + term) from 0.0 over the
// RESULT ROW's entries in ascending line order (qq: over the query's, by jnearest_tile_kernel).
//   jexplain_qcount_kernel  a wave per query: its entries with a nonzero component
//   jnearest_tile_kernel    QT queries scattered into the dense [n_lines][QT] image, their qq (jnearest_dev.hpp)
//   jexplain_pairs_kernel   a wave per (query of the tile, rank): streams the row's (line, cov) 64 entries at a time,
//                           gathers weight and image value, adds the chunk's terms in lane order (four running sums, two
//                           counts by ballot) and keeps the top list ONE SLOT PER LANE, sorted: the entries of a chunk
//                           that beat the slot top - 1 are found by ballot and inserted by a wave-wide compare-and-shift
// No LDS, no floating atomics; nothing depends on the grid, on QT or on the run.
#include <math.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "jnearest_dev.hpp"
#include "jstore.hpp"

using morna::DevBuf;
using morna::EventPair;
using morna::guarded;
using morna::set_error;

struct morna_jexplained {
    int64_t nq = 0;
    int32_t k = 0, top = 0;
    std::vector<int32_t> n_res;   // [nq]
    std::vector<double> sums;     // [nq][k][6]: pq pp qq pp_shared qq_shared distance
    std::vector<int64_t> counts;  // [nq][k][3]: shared n_q n_r
    std::vector<int32_t> lines, cov_r;   // [nq][k][top]
    std::vector<double> terms;           // [nq][k][top]
};

namespace {

// the value of lane j (the same j in every lane) in every lane
__device__ inline int lane_int(int x, int j) { return __builtin_amdgcn_readlane(x, __builtin_amdgcn_readfirstlane(j)); }
__device__ inline double lane_double(double x, int j)
{
    const int sj = __builtin_amdgcn_readfirstlane(j);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), sj), __builtin_amdgcn_readlane(__double2loint(x), sj));
}

// wave_add_in_order for four sums at once: four independent chains of 64 dependent additions each
__device__ inline void wave_add4_in_order(double &a0, double t0, double &a1, double t1, double &a2, double t2, double &a3, double t3)
{
#pragma unroll
    for (int j = 0; j < WAVE; j++) {
        a0 = __dadd_rn(a0, lane_value(t0, j));
        a1 = __dadd_rn(a1, lane_value(t1, j));
        a2 = __dadd_rn(a2, lane_value(t2, j));
        a3 = __dadd_rn(a3, lane_value(t3, j));
    }
}

// (term, line) a ranks ahead of (term, line) b: a larger term, or the same term on a smaller line
__device__ inline bool ahead_of(double ta, int32_t la, double tb, int32_t lb) { return ta > tb || (ta == tb && la < lb); }

// a wave per query: n_q, its entries with a nonzero component
__global__ __launch_bounds__(JN_THREADS) void jexplain_qcount_kernel(const int32_t *__restrict__ line, const int32_t *__restrict__ cov,
                                                                     const int64_t *__restrict__ qrange, const double *__restrict__ w,
                                                                     int64_t nq, int64_t *__restrict__ nq_out)
{
    const int lane = threadIdx.x % WAVE;
    const int64_t q = (int64_t)blockIdx.x * JN_WAVES + threadIdx.x / WAVE;
    if (q >= nq) return;
    const int64_t a = qrange[2 * q], b = qrange[2 * q + 1];
    int64_t n = 0;
    for (int64_t i0 = a; i0 < b; i0 += WAVE) {
        const int64_t i = i0 + lane;
        bool nz = false;
        if (i < b) nz = __dmul_rn((double)cov[i], w[line[i]]) != 0.0;
        n += __popcll(__ballot(nz));
    }
    if (lane == 0) nq_out[q] = n;
}

// A wave per (query t of the tile, rank r): pair u = t * k + r of the tile, pair0 + u of the call.  rows[u]: the store row,
// or -1 for a rank past the query's list.  The list slots: lane i holds the entry of rank i among those seen, (-1.0, INT32_MAX)
// while there is none; terms are >= 0.
__global__ __launch_bounds__(JN_THREADS) void jexplain_pairs_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ line,
                                                                    const int32_t *__restrict__ cov, const double *__restrict__ w,
                                                                    const int32_t *__restrict__ rows, int32_t nt, int32_t k, int32_t top,
                                                                    const double *__restrict__ tile, int32_t qt,
                                                                    const double *__restrict__ qq, const int64_t *__restrict__ n_q,
                                                                    int64_t pair0, double *__restrict__ sums, int64_t *__restrict__ counts,
                                                                    int32_t *__restrict__ o_line, double *__restrict__ o_term,
                                                                    int32_t *__restrict__ o_cov, unsigned long long *err)
{
    const int lane = threadIdx.x % WAVE;
    const int64_t u = (int64_t)blockIdx.x * JN_WAVES + threadIdx.x / WAVE;
    if (u >= (int64_t)nt * k) return;
    const int32_t t = (int32_t)(u / k);
    const int32_t row = rows[u];
    if (row < 0) return;
    const int64_t pair = pair0 + u;
    const int64_t a = ptr[row], b = ptr[row + 1];
    double pq = 0.0, pp = 0.0, pps = 0.0, qqs = 0.0;
    int64_t shared = 0, n_r = 0;
    double s_term = -1.0;
    int32_t s_line = INT32_MAX, s_cov = 0;
    for (int64_t i0 = a; i0 < b; i0 += WAVE) {
        const int64_t i = i0 + lane;
        int32_t l = 0, c = 0;
        double vr = 0.0, vq = 0.0;
        if (i < b) {
            l = line[i];
            c = cov[i];
            vr = __dmul_rn((double)c, w[l]);
            vq = tile[(int64_t)l * qt + t];
            if (c < 0) atomicMin(err, ((unsigned long long)pair << 32) | (uint32_t)l);
        }
        const double term = __dmul_rn(vr, vq), tr = __dmul_rn(vr, vr), tq = __dmul_rn(vq, vq);
        const bool is_r = vr != 0.0, sh = is_r && vq != 0.0;
        const unsigned long long m_r = __ballot(is_r), m_sh = __ballot(sh);
        n_r += __popcll(m_r);
        shared += __popcll(m_sh);
        // a chunk without a nonzero term adds +0.0 sixty-four times to a sum that is >= +0.0: nothing
        if (m_sh) wave_add4_in_order(pq, term, pp, tr, pps, sh ? tr : 0.0, qqs, sh ? tq : 0.0);
        else if (m_r) pp = wave_add_in_order(pp, tr);
        // the entries that beat the last slot of the list, in lane order -- ascending lines
        unsigned long long m = __ballot(sh && ahead_of(term, l, lane_double(s_term, top - 1), lane_int(s_line, top - 1)));
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const double ct = lane_double(term, j);
            const int32_t cl = lane_int(l, j), cc = lane_int(c, j);
            if (!ahead_of(ct, cl, lane_double(s_term, top - 1), lane_int(s_line, top - 1))) continue;   // the list has moved on
            // the slots ahead of the entry are a prefix of the lanes: the entry goes to the lane after them, the rest move up one
            const int pos = __popcll(__ballot(ahead_of(s_term, s_line, ct, cl)));
            const double up_t = __shfl_up(s_term, 1, WAVE);
            const int32_t up_l = __shfl_up(s_line, 1, WAVE), up_c = __shfl_up(s_cov, 1, WAVE);
            if (lane == pos) {
                s_term = ct;
                s_line = cl;
                s_cov = cc;
            } else if (lane > pos) {
                s_term = up_t;
                s_line = up_l;
                s_cov = up_c;
            }
        }
    }
    const int64_t n_top = shared < top ? shared : top;
    if (lane < n_top) {
        o_line[pair * top + lane] = s_line;
        o_term[pair * top + lane] = s_term;
        o_cov[pair * top + lane] = s_cov;
    }
    if (lane == 0) {
        const double my_qq = qq[t];
        const double radicand = jn_radicand(pp, my_qq, pq);
        double *s = sums + pair * 6;
        s[0] = pq;
        s[1] = pp;
        s[2] = my_qq;
        s[3] = pps;
        s[4] = qqs;
        s[5] = __dsqrt_rn(radicand > 0.0 ? radicand : 0.0);
        int64_t *n = counts + pair * 3;
        n[0] = shared;
        n[1] = n_q[t];
        n[2] = n_r;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------

const int64_t JX_MAX_CELLS = (int64_t)1 << 28;   // nq * k * top

// what both entry points check first
int begin(morna_jstore *s, int64_t nq, const int64_t *results, const int32_t *n_results, int32_t k, int32_t top, morna_jexplained **out)
{
    if (s)
        for (int i = 0; i < 6; i++) s->explain_stats[i] = 0;   // a refused call leaves no statistics of an earlier one
    if (!s || !out || nq < 0 || (nq > 0 && (!results || !n_results))) {
        set_error("jstore_explain: null argument");
        return MORNA_E_INVALID;
    }
    *out = nullptr;
    if (!s->nearest) {
        set_error("jstore_explain: the store has no weights: call morna_jstore_set_weights first");
        return MORNA_E_STATE;
    }
    if (k < 1 || k > MORNA_JNEAREST_MAX_K) {
        set_error("jstore_explain: result lists of %d places: a list holds 1 to %d results", k, MORNA_JNEAREST_MAX_K);
        return MORNA_E_INVALID;
    }
    if (top < 1 || top > MORNA_JEXPLAIN_MAX_TOP) {
        set_error("jstore_explain: %d top lines asked for: a pair lists 1 to %d", top, MORNA_JEXPLAIN_MAX_TOP);
        return MORNA_E_INVALID;
    }
    if (nq > JX_MAX_CELLS / ((int64_t)k * top)) {
        set_error("jstore_explain: %lld queries x %d results x %d top lines: one call takes at most 2^28 list places", (long long)nq, k, top);
        return MORNA_E_INVALID;
    }
    for (int64_t q = 0; q < nq; q++)
        if (n_results[q] < 0 || n_results[q] > k) {
            set_error("jstore_explain: query %lld has %d results, outside [0, k = %d]", (long long)q, n_results[q], k);
            return MORNA_E_INVALID;
        }
    return MORNA_OK;
}

// q_line / q_cov: device arrays the ranges index (the store's own for queries by sample); qrange: [nq][2] on the host
int explain_impl(morna_jstore *st, const int32_t *q_line, const int32_t *q_cov, const std::vector<int64_t> &qrange, int64_t nq,
                 const int64_t *results, const int32_t *n_results, int32_t k, int32_t top, morna_jexplained *E)
{
    const int64_t n_pairs = nq * k;
    std::vector<int32_t> rows((size_t)n_pairs, -1);
    int64_t pairs = 0, entries = 0;
    for (int64_t q = 0; q < nq; q++)
        for (int32_t r = 0; r < n_results[q]; r++) {
            const int64_t ext = results[q * k + r];
            auto it = st->row_of.find(ext);
            if (it == st->row_of.end()) {
                set_error("jstore_explain: sample id %lld (query %lld, rank %d) is not in the junction store", (long long)ext, (long long)q, r);
                return MORNA_E_RANGE;
            }
            rows[(size_t)(q * k + r)] = it->second;
            entries += st->ptr[(size_t)it->second + 1] - st->ptr[(size_t)it->second];
            pairs++;
        }
    E->nq = nq;
    E->k = k;
    E->top = top;
    E->n_res.assign(n_results, n_results + nq);
    E->sums.assign((size_t)(n_pairs * 6), 0.0);
    E->counts.assign((size_t)(n_pairs * 3), 0);
    E->lines.assign((size_t)(n_pairs * top), 0);
    E->cov_r.assign((size_t)(n_pairs * top), 0);
    E->terms.assign((size_t)(n_pairs * top), 0.0);
    if (nq == 0) return MORNA_OK;
    const double *d_w = nullptr;
    MORNA_TRY(morna::jstore_device_weights(st, &d_w));
    const int qt = choose_qt(st->n_lines);
    const int64_t n_lines = std::max<int64_t>(st->n_lines, 1);
    const size_t tile_bytes = (size_t)n_lines * qt * sizeof(double);
    DevBuf<double> d_tile, d_qq, d_sums, d_terms;
    DevBuf<int32_t> d_rows, d_lines, d_cov;
    DevBuf<int64_t> d_qrange, d_nq, d_counts;
    DevBuf<unsigned long long> d_err;
    MORNA_TRY(d_tile.alloc((size_t)n_lines * qt));
    MORNA_TRY(d_qq.alloc((size_t)nq));
    MORNA_TRY(d_nq.alloc((size_t)nq));
    MORNA_TRY(d_qrange.alloc((size_t)(2 * nq)));
    MORNA_TRY(d_rows.alloc((size_t)n_pairs));
    MORNA_TRY(d_sums.alloc((size_t)(n_pairs * 6)));
    MORNA_TRY(d_counts.alloc((size_t)(n_pairs * 3)));
    MORNA_TRY(d_lines.alloc((size_t)(n_pairs * top)));
    MORNA_TRY(d_cov.alloc((size_t)(n_pairs * top)));
    MORNA_TRY(d_terms.alloc((size_t)(n_pairs * top)));
    MORNA_TRY(d_err.alloc(1));
    HIP_TRY(hipMemcpy(d_qrange.p, qrange.data(), (size_t)(2 * nq) * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_rows.p, rows.data(), (size_t)n_pairs * sizeof(int32_t), hipMemcpyHostToDevice));
    const unsigned long long none = ~0ull;
    HIP_TRY(hipMemcpy(d_err.p, &none, sizeof(none), hipMemcpyHostToDevice));
    // (the places of the ranks past a list, and of the slots past a pair's list, are never written: they read 0)
    HIP_TRY(hipMemsetAsync(d_sums.p, 0, (size_t)(n_pairs * 6) * sizeof(double), st->stream));
    HIP_TRY(hipMemsetAsync(d_counts.p, 0, (size_t)(n_pairs * 3) * sizeof(int64_t), st->stream));
    HIP_TRY(hipMemsetAsync(d_lines.p, 0, (size_t)(n_pairs * top) * sizeof(int32_t), st->stream));
    HIP_TRY(hipMemsetAsync(d_cov.p, 0, (size_t)(n_pairs * top) * sizeof(int32_t), st->stream));
    HIP_TRY(hipMemsetAsync(d_terms.p, 0, (size_t)(n_pairs * top) * sizeof(double), st->stream));
    EventPair ev;
    MORNA_TRY(ev.create());
    HIP_TRY(hipEventRecord(ev.a, st->stream));
    hipLaunchKernelGGL(jexplain_qcount_kernel, dim3((unsigned)((nq + JN_WAVES - 1) / JN_WAVES)), dim3(JN_THREADS), 0, st->stream, q_line, q_cov,
                       d_qrange.p, d_w, nq, d_nq.p);
    int64_t passes = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += qt, passes++) {
        const int32_t nt = (int32_t)std::min<int64_t>(qt, nq - q0);
        HIP_TRY(hipMemsetAsync(d_tile.p, 0, tile_bytes, st->stream));
        hipLaunchKernelGGL(jnearest_tile_kernel, dim3((unsigned)nt), dim3(JN_THREADS), 0, st->stream, q_line, q_cov, d_qrange.p + 2 * q0, d_w,
                           qt, d_tile.p, d_qq.p + q0);
        const int64_t waves = (int64_t)nt * k;
        hipLaunchKernelGGL(jexplain_pairs_kernel, dim3((unsigned)((waves + JN_WAVES - 1) / JN_WAVES)), dim3(JN_THREADS), 0, st->stream,
                           st->d_ptr.p, st->d_line.p, st->d_cov.p, d_w, d_rows.p + q0 * k, nt, k, top, d_tile.p, qt, d_qq.p + q0, d_nq.p + q0,
                           q0 * k, d_sums.p, d_counts.p, d_lines.p, d_terms.p, d_cov.p, d_err.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev.b, st->stream));
    unsigned long long err = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(E->sums.data(), d_sums.p, E->sums.size() * sizeof(double), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(E->counts.data(), d_counts.p, E->counts.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(E->lines.data(), d_lines.p, E->lines.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(E->cov_r.data(), d_cov.p, E->cov_r.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipMemcpyAsync(E->terms.data(), d_terms.p, E->terms.size() * sizeof(double), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    if (err != ~0ull) {
        set_error("jstore_explain: sample id %lld has a negative coverage at line %lld: the unhashed search takes coverages >= 0",
                  (long long)results[(size_t)(err >> 32)], (long long)(err & 0xffffffffull));
        return MORNA_E_INVALID;
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
    st->explain_stats[0] = (double)pairs;
    st->explain_stats[1] = (double)entries;
    st->explain_stats[2] = (double)passes;
    st->explain_stats[3] = ms;
    st->explain_stats[4] = 8.0 * (double)entries;
    st->explain_stats[5] = qt;
    return MORNA_OK;
}

}  // namespace

extern "C" {

int morna_jstore_explain(morna_jstore *s, const int64_t *q_ptr, const int32_t *q_line, const int32_t *q_cov, int64_t nq,
                         const int64_t *results, const int32_t *n_results, int32_t k, int32_t top, morna_jexplained **out)
{
    MORNA_TRY(begin(s, nq, results, n_results, k, top, out));
    if (nq > 0 && (!q_ptr || q_ptr[0] != 0 || (q_ptr[nq] > 0 && (!q_line || !q_cov)))) {
        set_error("jstore_explain: null argument, or query offsets that do not begin at 0");
        return MORNA_E_INVALID;
    }
    return guarded("jstore_explain", MORNA_E_INVALID, [&] {
        std::vector<int64_t> qrange((size_t)(2 * nq));
        for (int64_t q = 0; q < nq; q++) {
            const int64_t a = q_ptr[q], b = q_ptr[q + 1];
            if (b < a) {
                set_error("jstore_explain: the offsets of query %lld descend", (long long)q);
                return MORNA_E_INVALID;
            }
            for (int64_t i = a; i < b; i++) {
                if (q_line[i] < 0 || q_line[i] >= s->n_lines || (i > a && q_line[i] <= q_line[i - 1])) {
                    set_error("jstore_explain: query %lld, term %lld: line %d; a query's lines ascend, distinct, below the store's %lld lines",
                              (long long)q, (long long)(i - a), q_line[i], (long long)s->n_lines);
                    return MORNA_E_INVALID;
                }
                if (q_cov[i] < 0) {
                    set_error("jstore_explain: query %lld has a negative coverage at line %d: the unhashed search takes coverages >= 0",
                              (long long)q, q_line[i]);
                    return MORNA_E_INVALID;
                }
            }
            qrange[(size_t)(2 * q)] = a;
            qrange[(size_t)(2 * q + 1)] = b;
        }
        std::unique_ptr<morna_jexplained> E(new morna_jexplained());
        DevBuf<int32_t> d_qline, d_qcov;
        if (nq > 0) {
            MORNA_TRY(morna::jstore_make_resident(s));
            const size_t n_terms = (size_t)q_ptr[nq];
            MORNA_TRY(d_qline.alloc(n_terms));
            MORNA_TRY(d_qcov.alloc(n_terms));
            if (n_terms) {
                HIP_TRY(hipMemcpy(d_qline.p, q_line, n_terms * sizeof(int32_t), hipMemcpyHostToDevice));
                HIP_TRY(hipMemcpy(d_qcov.p, q_cov, n_terms * sizeof(int32_t), hipMemcpyHostToDevice));
            }
        }
        MORNA_TRY(explain_impl(s, d_qline.p, d_qcov.p, qrange, nq, results, n_results, k, top, E.get()));
        *out = E.release();
        return MORNA_OK;
    });
}

int morna_jstore_explain_by_sample(morna_jstore *s, const int64_t *q_ext, int64_t nq, const int64_t *results, const int32_t *n_results,
                                   int32_t k, int32_t top, morna_jexplained **out)
{
    MORNA_TRY(begin(s, nq, results, n_results, k, top, out));
    if (nq > 0 && !q_ext) {
        set_error("jstore_explain: null argument");
        return MORNA_E_INVALID;
    }
    return guarded("jstore_explain", MORNA_E_INVALID, [&] {
        std::vector<int64_t> qrange((size_t)(2 * nq));
        for (int64_t q = 0; q < nq; q++) {
            auto it = s->row_of.find(q_ext[q]);
            if (it == s->row_of.end()) {
                set_error("jstore_explain: sample id %lld (query %lld) is not in the junction store", (long long)q_ext[q], (long long)q);
                return MORNA_E_RANGE;
            }
            const int64_t a = s->ptr[(size_t)it->second], b = s->ptr[(size_t)it->second + 1];
            for (int64_t i = a; i < b; i++)
                if (s->cov[(size_t)i] < 0) {
                    set_error("jstore_explain: sample id %lld has a negative coverage at line %d: the unhashed search takes coverages >= 0",
                              (long long)q_ext[q], s->line[(size_t)i]);
                    return MORNA_E_INVALID;
                }
            qrange[(size_t)(2 * q)] = a;
            qrange[(size_t)(2 * q + 1)] = b;
        }
        std::unique_ptr<morna_jexplained> E(new morna_jexplained());
        if (nq > 0) MORNA_TRY(morna::jstore_make_resident(s));
        MORNA_TRY(explain_impl(s, s->d_line.p, s->d_cov.p, qrange, nq, results, n_results, k, top, E.get()));
        *out = E.release();
        return MORNA_OK;
    });
}

int morna_jexplained_pair(const morna_jexplained *e, int64_t q, int32_t rank, double *sums, int64_t *counts, int32_t *n_top,
                          const int32_t **lines, const double **terms, const int32_t **cov_r)
{
    if (!e) {
        set_error("jexplained_pair: null argument");
        return MORNA_E_INVALID;
    }
    if (q < 0 || q >= e->nq) {
        set_error("jexplained_pair: query %lld out of range [0, %lld)", (long long)q, (long long)e->nq);
        return MORNA_E_RANGE;
    }
    if (rank < 0 || rank >= e->n_res[(size_t)q]) {
        set_error("jexplained_pair: rank %d out of range [0, %d), the results of query %lld", rank, e->n_res[(size_t)q], (long long)q);
        return MORNA_E_RANGE;
    }
    const size_t pair = (size_t)(q * e->k + rank);
    if (sums) memcpy(sums, e->sums.data() + pair * 6, 6 * sizeof(double));
    if (counts) memcpy(counts, e->counts.data() + pair * 3, 3 * sizeof(int64_t));
    if (n_top) *n_top = (int32_t)std::min<int64_t>(e->top, e->counts[pair * 3]);
    if (lines) *lines = e->lines.data() + pair * (size_t)e->top;
    if (terms) *terms = e->terms.data() + pair * (size_t)e->top;
    if (cov_r) *cov_r = e->cov_r.data() + pair * (size_t)e->top;
    return MORNA_OK;
}

int morna_jexplained_free(morna_jexplained *e)
{
    delete e;
    return MORNA_OK;
}

int morna_jstore_explain_stats(const morna_jstore *s, double *stats)
{
    if (!s || !stats) {
        set_error("jstore_explain_stats: null argument");
        return MORNA_E_INVALID;
    }
    for (int i = 0; i < 6; i++) stats[i] = s->explain_stats[i];
    return MORNA_OK;
}

}  // extern "C"
