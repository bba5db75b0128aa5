// jstore.hpp -- the junction store as jstore.hip (build, load, filter), nearest.hip (unhashed search) and explain.hip (the
// junctions behind a result) share it.
#pragma once
#include <exception>
#include <memory>
#include <unordered_map>
#include <vector>

#include "common.hpp"

struct morna_jnearest;   // nearest.hip: weights, cached row norms and statistics of the unhashed search

struct morna_jstore {
    int32_t device = 0;
    int64_t n_lines = 0;
    // host image (what save writes)
    std::vector<int64_t> ext_ids;   // [S] external sample id, the parse's first-seen order
    std::vector<int64_t> ptr{0};    // [S + 1]
    std::vector<int32_t> line, cov; // [nnz]
    std::unordered_map<int64_t, int32_t> row_of;   // external sample id -> row
    // HBM image (made by build, or at the first retain / nearest of a loaded store)
    bool resident = false;
    hipStream_t stream = nullptr;
    morna::DevBuf<int64_t> d_ptr;
    morna::DevBuf<int32_t> d_line, d_cov;
    // kernel time of the build and of the last retain (HIP events), with their algorithmic bytes
    double ms[2] = {0, 0};
    int64_t bytes[2] = {0, 0};
    // of the last recovery: kernel ms, algorithmic bytes, workgroups launched
    double rec_ms = 0;
    int64_t rec_bytes = 0, rec_groups = 0;
    // of the last pool: kernel ms, bytes read and written, workgroups per pass
    double pool_ms = 0;
    int64_t pool_read = 0, pool_written = 0, pool_groups = 0;
    // of the last thin: kernel ms, bytes read and written, draws made, workgroups per pass
    double thin_ms = 0;
    int64_t thin_read = 0, thin_written = 0, thin_draws = 0, thin_groups = 0;
    // hashed rows (hashrows.hip): the line hashes of the last call, here and in HBM; every line's column and signed weight at
    // that call's width; the named rows; of the last call: kernel ms, bytes read and written, workgroups
    std::vector<int32_t> hr_hash;
    bool hr_hash_resident = false;
    morna::DevBuf<int32_t> d_hr_hash, d_hr_col, d_hr_rows;
    morna::DevBuf<double> d_hr_sw;
    double hr_stats[4] = {0, 0, 0, 0};
    // of the last explain (explain.hip): pairs, store entries streamed, passes, kernel ms, algorithmic bytes, queries per pass
    double explain_stats[6] = {0, 0, 0, 0, 0, 0};
    std::shared_ptr<morna_jnearest> nearest;   // made by morna_jstore_set_weights
    ~morna_jstore()
    {
        nearest.reset();   // its buffers go before the stream does
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace morna {

// the store's stream exists and its host image is in HBM (jstore.hip)
int jstore_make_resident(morna_jstore *st);
// the weights of morna_jstore_set_weights in the store's HBM (nearest.hip); the store has weights
int jstore_device_weights(morna_jstore *st, const double **d_w);

// The body of a C entry point: its code, or `code` with the error "<who>: <what>" for an exception that leaves it.
template <typename F>
int guarded(const char *who, int code, F body)
{
    try {
        return body();
    } catch (const std::exception &e) {
        set_error("%s: %s", who, e.what());
        return code;
    }
}

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    int create()
    {
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        return MORNA_OK;
    }
};

}  // namespace morna
