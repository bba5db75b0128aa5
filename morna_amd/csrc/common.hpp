// common.hpp -- shared declarations of libmorna_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../include/morna_hip.h"

#define WAVE 64

namespace morna {

void set_error(const char *fmt, ...);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            morna::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                             __LINE__);                                                       \
            return MORNA_E_HIP;                                                               \
        }                                                                                     \
    } while (0)

#define MORNA_TRY(expr)            \
    do {                           \
        int _r = (expr);           \
        if (_r != MORNA_OK) return _r; \
    } while (0)

// ---- device buffer with explicit lifetime -----------------------------------
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t count)
    {
        if (count <= n && p) return MORNA_OK;
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            set_error("hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
            return MORNA_E_HIP;
        }
        n = count;
        return MORNA_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// page-locked host buffer: grows to twice the need (at least `floor` bytes) and keeps nothing when it does
struct PinnedBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;  // bytes
    const unsigned flags;  // hipHostMalloc flags
    explicit PinnedBuf(unsigned f) : flags(f) {}
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    int reserve(size_t bytes, size_t floor = 0)
    {
        if (bytes <= cap) return MORNA_OK;
        release();
        const size_t want = bytes * 2 > floor ? bytes * 2 : floor;
        hipError_t e = hipHostMalloc((void **)&p, want, flags);
        if (e != hipSuccess) {
            p = nullptr;
            set_error("hipHostMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
            return MORNA_E_HIP;
        }
        cap = want;
        return MORNA_OK;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    // the device's view of a mapped buffer (null when there is none)
    void *dev() const
    {
        void *d = nullptr;
        return p && hipHostGetDevicePointer(&d, p, 0) == hipSuccess ? d : nullptr;
    }
};

// switch read from the environment: on unless set to something atoi reads as 0
inline bool env_on(const char *name)
{
    const char *v = getenv(name);
    return !(v && atoi(v) == 0);
}

// one split attempt of one node, as the forest kernels see it
struct SplitTask {
    int32_t tree, level, start, count;
    int32_t slot;      // hyperplane slot
    int32_t attempt;
    int32_t chunk0;    // first chunk index of this task in the split kernel grid
    int32_t pad;
};

// What two_means needs to know of a row besides its elements, made once per set of rows (row_norms_kernel) and
// fetched with one 16-byte load per step: the operations are the ones the step would otherwise perform itself.
struct alignas(16) RowInfo {
    float norm2;    // canonical dot(x, x)
    float norm;     // sqrtf(norm2); SIGN BIT SET when some x_i / norm may be a non-zero subnormal (centroid_step4)
    double rnorm;   // RN64(1 / (double)norm)
};
static_assert(sizeof(RowInfo) == 16, "RowInfo is one dwordx4");

// Where a two_means kernel that holds its hyperplane in registers leaves the fp16 image the matrix-core split filters with
// (splitmm.hip, rows_to_half_kernel's image of the same row); h16 null: nowhere, the image is made by a conversion launch.
struct HalfImageOut {
    _Float16 *h16;           // [slots of the level][dpad]
    float *norm, *err;       // [slots] upper bounds of the image's norm and of its rounding error's norm
    unsigned int *zero_me;   // the level's open-pair counter, reset by the kernel's first workgroup
};

// A node of the forest as the host driver tracks it (perm segment of one tree).
struct Seg {
    int32_t tree, level, start, count, node;
};

// A run of positions of one tree whose entries of `inv` (the position of every row in the tree) are to be rewritten from the
// image the run's items are in (forest.hip, split_inv_kernel): the children of the nodes a level's partitions moved.
struct InvSeg {
    int32_t image;         // tree * 2 + (level & 1): the image of the work buffer the run is read from
    int32_t start, count;  // positions [start, start + count) of the tree
    int32_t first_chunk;   // chunks of SPLIT_INV_CHUNK positions in the runs before this one
};
static_assert(sizeof(InvSeg) == 16, "the runs go up in 16-byte words, behind the tasks");
#define SPLIT_INV_CHUNK 1024   // positions per workgroup of split_inv_kernel

// Where a node's items are DURING a build: the work buffer holds two images of every tree's permutation, [tree][2][n_items],
// and a node of depth `level` has its items in image (level & 1) -- a partition reads one image and writes the node's two
// children into the other, so nothing is copied back (forest.hip; the leaves are gathered into h->perm at the end).
#define TASK_ITEMS_AT(t, n_items) (((int64_t)(t).tree * 2 + ((t).level & 1)) * (int64_t)(n_items) + (t).start)

// a finished leaf's items in the work images, on their way into the permutation the searches read (gather_leaves_kernel)
struct LeafSeg {
    int32_t tree, level, start, count;
};

// A forest build under way (forest.hip): what the host driver carries from attempt to attempt and from level to level.
// build_forest may return with an attempt of a narrow level enqueued and its counts not yet read (`pending`);
// finish_build collects that attempt and runs every further attempt and level, exactly as the loop would have.
struct ForestBuild {
    enum Phase { IDLE, LEVEL, ENQUEUE, COLLECT, FALLBACK, CHILDREN, DONE };
    int phase = IDLE;
    bool pending = false;        // an attempt is enqueued and the build has returned to its caller
    int32_t n_trees = 0;
    uint32_t seed = 0;
    // the forest so far
    std::vector<Seg> cur, nxt;   // the nodes of this level / of the next
    std::vector<LeafSeg> leaves;
    int32_t level = 0, next_node_id = 0;
    int64_t n_split_total = 0;
    // the node-table entries of the level just finished, written once the next level is under way (or at the end)
    std::vector<Seg> late_parents;
    std::vector<int32_t> late_ones;
    int32_t late_first_id = 0;
    int64_t late_first_hp = 0;
    bool late_pending = false;
    // `inv` (matrix-core split): true as of level inv_level; the leaves made since start at leaves[inv_leaf_mark]
    int32_t *inv_p = nullptr;
    const int32_t *rank_p = nullptr;
    int32_t inv_level = 0;
    size_t inv_leaf_mark = 0;
    const char *inv_from = "iota";
    std::vector<InvSeg> inv_segs, inv_segs_next;
    int32_t inv_chunks_next = 0, inv_next_level = -1;
    // the level
    std::vector<int32_t> split_idx, final_ones, todo, tree_first, h_ones;
    std::vector<SplitTask> tasks;
    size_t leaves_before = 0, leaves_after = 0;
    bool leaves_listed = false;
    int32_t S = 0;
    // the attempt
    int attempt = 0;
    int32_t A = 0;               // tasks whose counts the mailbox is polled for
    int64_t rows = 0;
    uint32_t epoch = 0;
    // MORNA_DEBUG_TURN
    double turn_t0 = 0, turn_counts = 0, turn_pulled = 0, turn_tm = 0, turn_split = 0;
    std::string turn_log;
    // what ran behind a deferral (MORNA_DEBUG_OPEN)
    int32_t defer_level = -1, tail_levels = 0, tail_attempts = 0;
};

struct Timer {
    double ms = 0;
    int64_t launches = 0, bytes = 0;
};

// one timed launch group whose events have been recorded but not yet read
struct PendingEv {
    hipEvent_t a, b;
    int which;
    int64_t bytes;
};

// Build scratch kept in the handle between calls, by owner: a rebuild (or the next level) reuses it without hipMalloc.
// The buffers only grow (DevBuf::alloc); release() gives a group's memory back.
struct FeatScratch {   // features.hip
    DevBuf<int32_t> col, col_count, col_off, col_lines;
    DevBuf<double> sidf;
    DevBuf<float> colacc;
    DevBuf<uint8_t> flags;
    DevBuf<int32_t> bucket_aux;  // [J] rank of a line in its chunk, then [n_chunks][D] chunk counts / bases
    DevBuf<int32_t> tile_off;    // [J][aw_tiles + 1] where each tile's piece of a line begins
    DevBuf<int32_t> pid;         // [nnz] position in the order of every entry's item
    void release()
    {
        col.release(); col_count.release(); col_off.release(); col_lines.release(); sidf.release();
        colacc.release(); flags.release(); bucket_aux.release(); tile_off.release(); pid.release();
    }
};

struct ForestScratch {   // forest.hip
    DevBuf<int32_t> work;        // two images of every tree's permutation (TASK_ITEMS_AT)
    DevBuf<int32_t> ones;        // right-side count per task
    DevBuf<int32_t> part_counts; // right-side count per chunk of a task (partition_count_kernel)
    DevBuf<uint8_t> side;        // [n_trees][n_items] side of every row
    DevBuf<SplitTask> tasks;
    DevBuf<int32_t> hist, cursor;   // launch order of the chunk split: buckets of 32 row ids
    DevBuf<int2> info, sched;
    DevBuf<int32_t> inv;         // matrix-core split: position of every item (or row) in every tree's permutation
    DevBuf<InvSeg> inv_segs;     // the runs split_inv_kernel walks on the side stream (d_tasks is the next attempt's by then)
    DevBuf<uint8_t> leaves;      // the leaf segments on their way to gather_leaves_kernel
    void release()
    {
        work.release(); ones.release(); part_counts.release(); side.release(); tasks.release(); hist.release();
        cursor.release(); info.release(); sched.release(); inv.release(); inv_segs.release(); leaves.release();
    }
};

struct HalfRows {   // splitmm.hip: the fp16 image of X, made once per set of rows; the query filter (knn.hip) reads it too
    DevBuf<_Float16> x16;        // [n_items][dpad]
    DevBuf<float> xn;            // [0, N): norms; [N, 2N): 2^-e per row (the query filter unscales with it); [2N, 3N): |s x - y|
    bool valid = false;          // x16 / xn hold the image of the rows as they are now
    void release()
    {
        x16.release(); xn.release();
        valid = false;
    }
};

struct SplitMmScratch {   // splitmm.hip
    DevBuf<_Float16> h16;        // fp16 hyperplanes of the level
    DevBuf<float> hn;            // their norms, then their rounding errors' norms
    DevBuf<uint8_t> amb;         // the open-pair list (first 16 bytes: its counter)
    DevBuf<uint8_t> active;      // per-tile task lists: which tasks hold a row of each row tile
    DevBuf<int32_t> lists;
    // the order of the contraction's rows (split_mm_order_rows): [rank | item_at], inv by row, the counting sort's table (+ keys)
    DevBuf<int32_t> maps, invr, table;
    bool ord_valid = false;      // the build under way has ordered its rows (maps / invr)
    bool ord_line_due = false;   // the MORNA_DEBUG_OPEN line of this order has not been printed yet
    int ord_bits = 0;            // root sides in a row's code
    void release()
    {
        h16.release(); hn.release(); amb.release(); active.release(); lists.release();
        maps.release(); invr.release(); table.release();
        ord_valid = false;
    }
};

struct QueryRows {   // features.hip: rows of query samples built against the index's vocabulary; the index itself untouched
    DevBuf<uint8_t> keys;
    DevBuf<int64_t> key_off, row_ptr;
    DevBuf<int32_t> ids, cov;
    DevBuf<double> w;            // [J] weight of every line's key
    DevBuf<int32_t> col, col_count, col_off, col_lines, bucket_aux;
    DevBuf<double> sidf;
    DevBuf<double> colacc;       // [D][nq] fp64 cell sums
    DevBuf<double> rows64;       // [nq][dim]
    DevBuf<float> rows32;        // [nq][dpad], pad columns zero
    int64_t nq = 0;
    bool valid = false;          // rows64 / rows32 hold the rows of the last morna_build_query_rows
    void release()
    {
        keys.release(); key_off.release(); row_ptr.release(); ids.release(); cov.release(); w.release();
        col.release(); col_count.release(); col_off.release(); col_lines.release(); bucket_aux.release();
        sidf.release(); colacc.release(); rows64.release(); rows32.release();
        nq = 0;
        valid = false;
    }
};

}  // namespace morna

struct morna_index {
    int32_t dim = 0;     // D (f in annoy)
    int32_t dpad = 0;    // row stride in floats: D rounded up to 256 (one 1-KiB load per wave and k-step)
    int32_t device = 0;
    int32_t n_cus = 256;               // compute units of the device (MI355X: 256)
    int32_t K = 0;       // leaf capacity D + 2
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;                 // side stream of the forest build (work that does not depend on two_means)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_tables = nullptr;    // behind the node-table copies of the last forest build
    bool ev_tables_pending = false;
    // A query batch that starts while a build is pending (knn.hip): its contraction runs on stream3, which waits for
    // ev_tail (recorded on `stream` in front of the deferred attempt); ev_early_in / ev_early_out: its inputs are in place /
    // its scores are
    hipStream_t stream3 = nullptr;
    hipEvent_t ev_tail = nullptr, ev_early_in = nullptr, ev_early_out = nullptr;
    // right-side counts of a level, written by partition_kernel straight into page-locked host memory ((epoch << 32) |
    // count per task): the host polls them instead of an event hand-over + copy + stream wait per level
    morna::PinnedBuf host_counts{hipHostMallocCoherent | hipHostMallocMapped};
    uint32_t count_epoch = 0;
    morna::PinnedBuf host_out{hipHostMallocDefault};    // page-locked staging of query results
    // page-locked, device-visible: the answers of a small query batch, written by the kernel itself
    morna::PinnedBuf host_small{hipHostMallocMapped | hipHostMallocCoherent};
    morna::PinnedBuf host_q{hipHostMallocDefault};      // page-locked staging of a small batch's query vectors, padded to the row stride
    morna::PinnedBuf host_tables{hipHostMallocMapped};  // page-locked staging of the node tables on their way to HBM (forest.hip)

    // host staging of add_item() rows until build()
    std::vector<float> host_rows;  // [host_n][dim]
    int64_t host_n = 0;
    bool host_dirty = false;

    // items in HBM
    int64_t n_items = 0;
    morna::DevBuf<float> X;      // [n_items][dpad], pad columns zero
    morna::DevBuf<float> norm2;  // [n_items] canonical dot(x, x)
    morna::DevBuf<morna::RowInfo> rowinfo;   // [n_items] norm2 again with what two_means derives from it
    bool norms_valid = false;
    bool unsettled = false;      // build_features() returned without waiting for its kernels: blocking copies must settle() first

    // staged junction lines (CSR by line, file order)
    int64_t J = 0, nnz = 0, key_bytes_n = 0;
    morna::DevBuf<uint8_t> s_keys;
    morna::DevBuf<int64_t> s_key_off, s_row_ptr;
    morna::DevBuf<int32_t> s_ids, s_cov;
    morna::DevBuf<double> s_idf;
    bool staged = false;
    int32_t s_id_min = 0, s_id_max = -1;   // smallest and largest staged item id (nnz > 0): build_features checks them against n_items
    // optional order of the items in which the lines' sample lists ascend (morna_stage_item_order): rank of every item
    // and the item at every rank
    morna::DevBuf<int32_t> item_rank, item_at;
    int64_t order_n = 0;

    // forest
    int32_t n_trees = 0;
    uint32_t seed = 0;
    bool built = false;
    int64_t n_nodes = 0, n_split = 0;
    morna::DevBuf<int32_t> perm;        // [n_trees][n_items]
    morna::DevBuf<int32_t> node_rec;    // [n_nodes][4] {child0 | -1, child1 | -1, start, count}
    morna::DevBuf<int32_t> node_tree;   // [n_nodes]
    morna::DevBuf<int32_t> node_hp;     // [n_nodes] hyperplane slot or -1
    morna::DevBuf<float> hp;            // [n_split][dpad]
    morna_forest_stats stats = {};
    std::vector<int32_t> h_node_rec, h_node_tree, h_node_hp;  // host mirrors

    // query workspace (grown on demand)
    morna::DevBuf<uint8_t> ws;
    // what the contraction of a batch that starts beside a pending build reads and writes: item ids, query image and its
    // three floats per query, scores (placed before anything is enqueued: `ws` is sized from n_nodes, unknown until the tail ends)
    morna::DevBuf<uint8_t> q_early;
    // exact search: query images, scan values and results of a batch; the candidates and their fp64 distances (exact.hip)
    morna::DevBuf<uint8_t> ex_ws;
    morna::DevBuf<int32_t> ex_cand;
    morna::DevBuf<double> ex_cdist;
    int32_t ex_cap = 0;                // candidates per query the last exact search needed room for
    // rows outside the domain of the exact scan's window (exact.hip, exact_outside_kernel): re-ranked for every query.
    // Made at the first exact search after the rows or their norms change; usually empty
    morna::DevBuf<int32_t> ex_out;     // [0] count, [1..] rows
    int32_t ex_out_n = 0;
    bool ex_out_valid = false;
    // label sums (exact.hip, label_sums): the items' labels and a batch's outputs on the device; the last call's statistics
    morna::DevBuf<int32_t> lb_label;   // [n_items]
    morna::DevBuf<uint8_t> lb_out;     // sums uint64 [batch][L] | counts int32 [batch][L] | rows counted uint64
    double label_stats[6] = {0, 0, 0, 0, 0, 0};
    // radius search (exact.hip, exact_radius): chunk counts, offsets and per-query flags of a batch; the last call's statistics
    morna::DevBuf<uint8_t> rd_ws;
    double radius_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // spherical k-means (exact.hip, kmeans): the last call's statistics (its arrays are pieces of ex_ws, ex_cand and ex_cdist)
    double kmeans_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // label mixture (mixture.hip): the call's arrays on the device; the last call's statistics
    morna::DevBuf<uint8_t> mx_ws;
    double mixture_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // principal axes (pca.hip): the call's arrays on the device; the last call's statistics
    morna::DevBuf<uint8_t> pca_ws;
    double pca_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // build scratch kept between calls
    morna::FeatScratch feat;
    morna::ForestScratch forest;
    morna::ForestBuild fb;
    morna::HalfRows half;
    morna::SplitMmScratch splitmm;
    morna::QueryRows qrows;      // morna_build_query_rows
    // [0] rows read by query kernels (hyperplane dots + candidates + 1 per query)
    morna::DevBuf<unsigned long long> d_stat;
    // the last search sweep (knn.hip): descents, cells, rows read by canonical dots, whether the fp16 contraction ran
    double sweep_stats[4] = {0, 0, 0, 0};

    // row-sharded search (comm.hip): the RCCL communicator of this shard, every shard's first global id, message buffers
    void *comm = nullptr;              // ncclComm_t
    int32_t comm_rank = 0, comm_world = 1;
    bool comm_sizes_valid = false;     // comm_offsets describe the rows the ranks hold NOW (cleared whenever this handle's rows change)
    std::vector<int64_t> comm_offsets; // [world + 1]
    morna::DevBuf<uint8_t> cm_small, cm_msg, cm_q, cm_out;

    // timing
    bool timing = false;
    uint32_t timing_mask = 0;          // bit `which` set: that kernel group is bracketed by events
    morna::Timer timers[MORNA_T_COUNT];
    std::vector<morna::PendingEv> pending_ev;  // resolved by resolve_timers()
    std::vector<hipEvent_t> free_ev;
};

// A restriction of the searches of one handle (morna_hip.h, "restricted search"): the complement of the allow bitmap and
// the items' group labels, in the handle's device memory.
struct morna_restriction {
    morna_index *h = nullptr;
    int32_t device = 0;
    int64_t n_items = 0;               // the handle's items when it was made: a search checks them
    int64_t n_allowed = 0, n_grouped = 0;
    morna::DevBuf<uint32_t> deny;      // [(n_items + 31) / 32], the bits past n_items set
    morna::DevBuf<int32_t> group;      // [n_items]
    bool has_group = false;
};

// The answer of one morna_exact_radius call (morna_hip.h, "radius search"): host memory, every list ordered.
struct morna_radius {
    int64_t nq = 0;
    std::vector<int64_t> off;      // [nq + 1] list q is ids / dist [off[q], off[q + 1])
    std::vector<int64_t> count;    // [nq] the list's length, or -1 (a NaN distance: the reference raises)
    std::vector<int32_t> ids;
    std::vector<double> dist;
};

namespace morna {

// scope timer: records a HIP event pair on the handle's stream around a launch
// group; no host synchronisation here, the pairs are read by resolve_timers().
hipEvent_t take_event(morna_index *h);
void resolve_timers(morna_index *h);
struct ScopedTimer {
    morna_index *h;
    PendingEv pe;
    ScopedTimer(morna_index *h_, int which, int64_t bytes) : h(h_)
    {
        pe.which = which;
        pe.bytes = bytes;
        pe.a = pe.b = nullptr;
        if (!h->timing || !(h->timing_mask & (1u << which))) return;
        pe.a = take_event(h);
        pe.b = take_event(h);
        (void)hipEventRecord(pe.a, h->stream);
    }
    ~ScopedTimer()
    {
        if (!pe.a) return;
        (void)hipEventRecord(pe.b, h->stream);
        h->pending_ev.push_back(pe);
    }
};

// Before a blocking copy (which is not ordered against the handle's non-blocking stream) reads what the feature
// build wrote: wait for the stream once.
inline int settle(morna_index *h)
{
    if (h->unsettled) {
        hipError_t e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            set_error("hipStreamSynchronize failed: %s", hipGetErrorString(e));
            return MORNA_E_HIP;
        }
        h->unsettled = false;
    }
    return MORNA_OK;
}

// implemented in features.hip / forest.hip / knn.hip / exact.hip
int upload_host_rows(morna_index *h);
int compute_norms(morna_index *h);
int build_features(morna_index *h, int64_t n_items);
// rows of the nq query samples of J deduplicated lines (morna_lines_query_terms) into h->qrows; X, its norms, the forest and
// every cache of the index stay as they are
int build_query_rows(morna_index *h, const uint8_t *key_bytes, const int64_t *key_off, int64_t J, const int64_t *row_ptr,
                     const int32_t *ids, const int32_t *cov, const double *w, int64_t nq);
int hash_keys_device(morna_index *h, const uint8_t *key_bytes, const int64_t *key_off, int64_t J,
                     int32_t *hash_out, int32_t *col_out, int32_t *sign_out);
// May return with the last narrow levels still to run (h->fb.pending; MORNA_BUILD_TAIL=0: never).  EVERY entry point that
// touches the handle calls finish_build first, except the dense first batch of query_batch, which starts its contraction first.
int build_forest(morna_index *h, int32_t n_trees, uint32_t seed);
// who: the entry point, for the MORNA_DEBUG_OPEN line.  A no-op when nothing is pending; a failure leaves the handle unbuilt.
int finish_build(morna_index *h, const char *who);
// splitmm.hip: the split of a whole level on the matrix cores (fp16 filter, exact fp32 for what it cannot decide)
int split_mm_prepare_rows(morna_index *h, hipStream_t stream);   // stream: the handle's main or side stream
int split_mm_convert_rows(morna_index *h, const float *src, int64_t rows, _Float16 *dst, float *norm, float *err,
                          float *inv_scale, hipStream_t stream);
// the order of the contraction's rows: begin (buffers, the handle's state; before the level's two_means is launched), then
// the sort itself on `stream`
int split_mm_order_begin(morna_index *h, int32_t n_trees, const int32_t **rank_out, int32_t **inv_out);
int split_mm_order_rows(morna_index *h, const uint8_t *side, int32_t n_trees, hipStream_t stream);
int split_mm_order_read(morna_index *h, int32_t *item_at);
bool split_mm_order_by_groups();   // MORNA_SPLIT_ORDER_GROUPS (on unless 0)
// inv[tree][rank ? rank[item] : item] = position, for every position of the runs (the side stream, under two_means)
int split_mm_level_inv(morna_index *h, const InvSeg *d_segs, int32_t n_segs, int32_t n_chunks, const int32_t *perm, const int32_t *rank,
                       int32_t *inv, hipStream_t stream);
// a level: begin (buffers; before its two_means is launched), its per-tile task lists (any stream, once the tasks are on the
// device), then the contraction
bool split_mm_level_uses_lists(const morna_index *h, int32_t n_tasks);
int split_mm_level_begin(morna_index *h, int32_t n_tasks, int32_t n_slots, HalfImageOut *img);
int split_mm_level_lists(morna_index *h, const SplitTask *d_tasks, int32_t n_tasks, const int32_t *perm, hipStream_t stream);
int split_mm_level(morna_index *h, const SplitTask *d_tasks, int32_t n_tasks, int32_t n_slots, const float *hp_level,
                   const int32_t *perm, const int32_t *inv, uint32_t seed, uint8_t *side, int32_t *ones, const char *image_from,
                   bool lists_ready, const char *inv_from, int32_t level);
// result block in HBM (ids at 0, distances at s_ids, counts at s_ids + s_dist; `bytes` in all) -> the caller's arrays
// through the handle's page-locked staging (knn.hip); waits for the stream
int fetch_results(morna_index *h, const uint8_t *d_block, size_t bytes, size_t s_ids, size_t s_dist, size_t dist_elt, int64_t nq,
                  int32_t k, int32_t *ids_out, void *dist_out, int32_t *count_out);
// packed_dev (device memory, or null): [nq][2k] int32 message of the row-sharded search -- ids + id_offset, distance bits
int query_batch(morna_index *h, const float *q_host, int64_t q_stride, const int32_t *items_host, int64_t nq, int32_t k,
                int32_t search_k, int32_t *ids_out, float *dist_out, int32_t *count_out, int32_t *packed_dev = nullptr,
                int64_t id_offset = 0, const morna_restriction *rst = nullptr, const int32_t *q_group_host = nullptr,
                int32_t n_trees_used = 0 /* the first n_trees_used trees only; 0: the whole forest */);
// every (tree count, search_k) cell of a grid from one forest (morna_hip.h, "search sweep"); outputs [n_t][n_s][nq] ([k]), any may be null
// (q_host: host or device memory, q_stride floats apart, 0 = dim; ex_*: the exact answers, for hits_out)
int search_sweep(morna_index *h, const float *q_host, int64_t q_stride, const int32_t *items_host, int64_t nq, int32_t k,
                 const int32_t *trees, int32_t n_t, const int32_t *search_ks, int32_t n_s, int32_t *ids_out, float *dist_out,
                 int32_t *count_out, int32_t *ncand_out, int32_t *ndots_out, const int32_t *ex_ids_host = nullptr,
                 const int32_t *ex_count_host = nullptr, int32_t *hits_out = nullptr);
int merge_topk_dev(morna_index *h, const int32_t *gathered_dev, int32_t world, int64_t nq, int32_t kk, int32_t k,
                   int32_t *ids_out, float *dist_out, int32_t *count_out);
int exact_search(morna_index *h, const double *q, int64_t nq, int32_t k, int32_t *ids_out,
                 double *dist_out, int32_t *count_out);
// Where the queries of an exact call are, nq of them: one of four sources.
struct ExactQueries {
    enum Source { HOST_F64, DEV_F32, DEV_F64, ITEMS } source;
    const void *p;
    static ExactQueries host(const double *q) { return {HOST_F64, q}; }       // fp64 vectors [nq][dim], host memory
    static ExactQueries device32(const float *q) { return {DEV_F32, q}; }     // fp32 vectors [nq][dim], this device's memory
    // fp64 rows [nq][dim], this device's memory: the query rows of morna_build_query_rows, finite by construction
    static ExactQueries device64(const double *q) { return {DEV_F64, q}; }
    static ExactQueries stored(const int32_t *items) { return {ITEMS, items}; }   // stored rows, their ids [nq] in host memory
    // the source as its own type, null for the other three
    const double *host64() const { return source == HOST_F64 ? (const double *)p : nullptr; }
    const float *dev32() const { return source == DEV_F32 ? (const float *)p : nullptr; }
    const double *dev64() const { return source == DEV_F64 ? (const double *)p : nullptr; }
    const int32_t *items() const { return source == ITEMS ? (const int32_t *)p : nullptr; }
};
// the same for any source of queries, answers to the host and / or packed for the sharded merge
int exact_search_any(morna_index *h, const ExactQueries &Q, int64_t nq, int32_t k, int32_t *ids_out, double *dist_out,
                     int32_t *count_out, uint8_t *msg_dev, int64_t id_offset, const morna_restriction *rst = nullptr,
                     const int32_t *q_group_host = nullptr);
// morna_label_sums behind its argument checks (morna_hip.h, "label distance sums"): rst and q_group_host may be null
int label_sums(morna_index *h, const morna_restriction *rst, const ExactQueries &Q, int64_t nq, const int32_t *q_group_host,
               const int32_t *item_label_host, int32_t L, uint64_t *sums_out, int32_t *counts_out);
// morna_exact_radius behind its argument checks (morna_hip.h, "radius search"): rst, q_group_host and after_host may be null;
// the lists are appended to *out (empty on entry)
int exact_radius(morna_index *h, const morna_restriction *rst, const ExactQueries &Q, int64_t nq, const int32_t *q_group_host,
                 const int32_t *after_host, double radius, morna_radius *out);
// morna_kmeans (seeds [k], cent_host null) and morna_kmeans_assign (cent_host [k][dim], seeds null) behind their null checks
// (morna_hip.h, "spherical k-means"): rst and every output but assign_out may be null
int kmeans(morna_index *h, const morna_restriction *rst, const int32_t *seeds, const double *cent_host, int32_t k, int32_t max_iter,
           int32_t *assign_out, double *dist_out, double *cent_out, int32_t *sizes_out, int32_t *info_out);
// What mixture.hip takes from the exact family (exact.hip): the checks every caller of the front makes on its queries (qt_out:
// the scan's own figure), their staging as fp64 rows, and the update of k-means for a labelling that is given.
int exact_check_queries(morna_index *h, const char *who, const ExactQueries &Q, int64_t nq, int *qt_out);
int exact_stage_queries(morna_index *h, const ExactQueries &Q, int64_t q0, int64_t nb, int32_t *d_items, double *Qd);
struct KmeansLists {
    double *scale;        // [n_items] 1 / sqrt(pp_i), -1: the member is skipped
    int32_t *chunk_cnt;   // [kmeans_lists_chunks(n_items)][k]
    int32_t *sizes;       // [k] members of every label, skipped ones included
    int32_t *start;       // [k] where a label's list begins in member
    int32_t *member;      // [n_items] label-major, ascending id
    int32_t *totals;      // [4] (the counters of the k-means loop: left as they are here)
};
int64_t kmeans_lists_chunks(int64_t n_items);
int kmeans_label_sums(morna_index *h, const int32_t *assign, int32_t k, const KmeansLists &W, double *sums);
// morna_label_centroids (q, weights_out and info_out null, nq 0) and morna_mixture behind their null checks (morna_hip.h,
// "label mixture"; mixture.hip)
int mixture(morna_index *h, const morna_restriction *rst, const ExactQueries &Q, int64_t nq, const int32_t *item_label_host, int32_t L,
            double tol, int32_t max_sweeps, double *sums_out, int32_t *counts_out, double *gram_out, double *weights_out,
            double *info_out, uint8_t *active_out);
// What pca.hip takes from the exact family besides the two query calls above: scale[n_items] of kmeans_norms_kernel on the
// handle's stream
int kmeans_row_scales(morna_index *h, double *scale);
// morna_pca and morna_pca_project behind their null checks (morna_hip.h, "principal axes"; pca.hip): rst may be null
int pca(morna_index *h, const morna_restriction *rst, int32_t p, int32_t extra, bool center, uint64_t seed, double tol, int32_t max_iter,
        double *axes_out, double *mean_out, double *values_out, double *info_out);
int pca_project(morna_index *h, const double *axes_host, const double *mean_host, int32_t p, const ExactQueries &Q, int64_t nq,
                double *coords_out);
size_t exact_msg_dist_offset(int64_t nq, int32_t k);
size_t exact_msg_bytes(int64_t nq, int32_t k);

}  // namespace morna
