// forest_host.hpp -- the host driver of the forest build: included by forest.hip behind its kernels, inside namespace morna.
//
// The build is a loop over levels and, within a level, over attempts (annoy retries a split that came out lopsided, and
// randomises the sides as a last option).  Its state lives in the handle (ForestBuild, common.hpp) and the loop is cut
// into steps -- begin; per level: open it, enqueue an attempt, collect that attempt, fallback, children; tables at the
// end -- so that build_forest can return between "enqueue" and "collect" of a narrow level: a handful of nodes whose
// 200-step two_means chain leaves the chip idle, and beside which a query batch's contraction can already run (knn.hip).
// finish_build takes the loop up where it stopped.  Same kernels, same tasks, same order: the forest does not depend on
// where the build paused.
#pragma once

static void fb_sync(morna_index *h) { (void)hipStreamSynchronize(h->stream); }   // the last partition may still be running

#define F_TRY(e)                                                    \
    do {                                                            \
        hipError_t _e = (e);                                        \
        if (_e != hipSuccess) {                                     \
            set_error("%s failed: %s", #e, hipGetErrorString(_e));  \
            return MORNA_E_HIP;                                     \
        }                                                           \
    } while (0)

static bool fb_mm_on()
{
    static const bool on = env_on("MORNA_SPLIT_MM");
    return on;
}
static bool fb_part_inv()
{
    static const bool on = fb_mm_on() && getenv("MORNA_PARTITION_INV") && atoi(getenv("MORNA_PARTITION_INV")) != 0;
    return on;
}
// MORNA_PARTITION_FORM: 0 = partition_kernel (the earlier form), 2 = the streaming form with one workgroup per node at every
// level; anything else, or unset: the streaming form, one workgroup per chunk where nodes span several
static int fb_part_form()
{
    static const int form = !env_on("MORNA_PARTITION_FORM") ? 0 : getenv("MORNA_PARTITION_FORM") && atoi(getenv("MORNA_PARTITION_FORM")) == 2 ? 2 : 1;
    return form;
}
static bool fb_debug_turn()
{
    static const bool on = getenv("MORNA_DEBUG_TURN") && atoi(getenv("MORNA_DEBUG_TURN")) != 0;
    return on;
}
static bool fb_debug_open()
{
    static const bool on = getenv("MORNA_DEBUG_OPEN") && atoi(getenv("MORNA_DEBUG_OPEN")) != 0;
    return on;
}
// MORNA_DEBUG_TURN=1: host times (steady clock, us since the build began) of a level's turn-around, one stderr line per attempt
static double fb_now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static void fb_write_late_tables(morna_index *h)
{
    ForestBuild &B = h->fb;
    if (!B.late_pending) return;
    B.late_pending = false;
    std::vector<int32_t> &rec = h->h_node_rec, &ntree = h->h_node_tree, &nhp = h->h_node_hp;
    const size_t S2 = B.late_parents.size();
    rec.reserve(rec.size() + S2 * 8);
    ntree.reserve(ntree.size() + S2 * 2);
    nhp.reserve(nhp.size() + S2 * 2);
    for (size_t i = 0; i < S2; i++) {
        const Seg &s = B.late_parents[i];
        const int32_t n1 = B.late_ones[i], n0 = s.count - n1;
        const int32_t id0 = B.late_first_id + 2 * (int32_t)i, id1 = id0 + 1;
        rec[(size_t)s.node * 4 + 0] = id0;
        rec[(size_t)s.node * 4 + 1] = id1;
        nhp[(size_t)s.node] = (int32_t)(B.late_first_hp + (int64_t)i);
        rec.insert(rec.end(), {-1, -1, s.start, n0});
        rec.insert(rec.end(), {-1, -1, s.start + n0, n1});
        ntree.push_back(s.tree);
        ntree.push_back(s.tree);
        nhp.push_back(-1);
        nhp.push_back(-1);
    }
}

// the level's leaves are listed once its two_means has been launched: nothing of the level's start reads them
static void fb_list_leaves(morna_index *h)
{
    ForestBuild &B = h->fb;
    if (B.leaves_listed) return;
    B.leaves_listed = true;
    for (const Seg &s : B.cur)
        if (s.count <= h->K) B.leaves.push_back(LeafSeg{s.tree, s.level, s.start, s.count});
}

static int32_t fb_make_tasks(ForestBuild &B, const std::vector<int32_t> &which, int attempt, std::vector<SplitTask> &out)
{
    out.resize(which.size());
    int32_t chunk = 0;
    for (size_t a = 0; a < which.size(); a++) {
        const Seg &s = B.cur[(size_t)B.split_idx[(size_t)which[a]]];
        out[a] = SplitTask{s.tree, s.level, s.start, s.count, which[a], attempt, chunk, 0};
        chunk += (s.count + SP_ROWS - 1) / SP_ROWS;
    }
    return chunk;
}

// Partition of the nodes whose sides stand, enqueued right behind the kernels that wrote the sides and their
// counts (d_tasks / d_ones as they are on the device).  The counts reach the host through page-locked memory
// that every partition workgroup writes before anything else, tagged with this call's epoch: the host polls the
// tags (no event hand-over, no copy, no stream wait) and prepares the next attempt or level while the partition runs.
static int fb_partition(morna_index *h, int32_t A, int64_t level_rows)
{
    ForestBuild &B = h->fb;
    const int64_t N = h->n_items;
    if ((size_t)A * 8 > h->host_counts.cap) {
        if (hipStreamSynchronize(h->stream) != hipSuccess) return MORNA_E_HIP;   // nobody writes the old buffer any more
        MORNA_TRY(h->host_counts.reserve((size_t)A * 8, 4096 * 8));
        memset(h->host_counts.p, 0, h->host_counts.cap);   // the epochs below start from a zeroed mailbox
    }
    B.epoch = ++h->count_epoch ? h->count_epoch : ++h->count_epoch;   // never 0: the mailbox starts zeroed
    B.A = A;
    // The streaming form (forest.hip, partition_stream_kernel) unless MORNA_PARTITION_FORM=0 or the partition keeps `inv`.
    // Where a node of the attempt spans more than two chunks, one workgroup per chunk, behind a counting pass that also posts
    // the counts; else one workgroup per node and post_counts_kernel as ever.  (MORNA_PARTITION_FORM=2: one workgroup per
    // node whatever the nodes' sizes, for comparison.)
    const int form = fb_part_form();
    if (form != 0 && !fb_part_inv()) {
        int32_t most = 0;
        for (const SplitTask &t : B.tasks) most = std::max(most, t.count);
        const unsigned mc = (unsigned)part_chunks(most, 3);   // no node of the attempt has more chunks
        const int64_t side_total = (int64_t)B.n_trees * N, perm_total = side_total * 2;
        // one workgroup per chunk from three chunks to a node on: at two (the default run's level 4) both forms take the
        // same time, counting pass included (profiles/partition_forms_vs_parent.txt)
        const bool chunks = form != 2 && mc > 2 && mc <= 65535;   // (a grid's second dimension ends there)
        if (chunks) {
            MORNA_TRY(h->forest.part_counts.alloc((size_t)A * mc));
            hipLaunchKernelGGL(partition_count_kernel, dim3((unsigned)A, mc), dim3(PS_THREADS), 0, h->stream, h->forest.tasks.p, A, N,
                               h->forest.side.p, side_total, h->forest.ones.p, h->forest.part_counts.p,
                               (unsigned long long *)h->host_counts.p, B.epoch);
        } else
            hipLaunchKernelGGL(post_counts_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, h->stream, h->forest.ones.p, A,
                               (unsigned long long *)h->host_counts.p, B.epoch);
        {
            ScopedTimer tm(h, MORNA_T_PARTITION, 0);
            if (chunks)
                hipLaunchKernelGGL(partition_stream_kernel<true>, dim3((unsigned)A, mc), dim3(PS_THREADS), 0, h->stream, h->forest.tasks.p,
                                   N, h->forest.side.p, side_total, h->forest.ones.p, h->forest.work.p, perm_total,
                                   h->forest.part_counts.p);
            else
                hipLaunchKernelGGL(partition_stream_kernel<false>, dim3((unsigned)A), dim3(PS_THREADS), 0, h->stream,
                                   h->forest.tasks.p, N, h->forest.side.p, side_total, h->forest.ones.p, h->forest.work.p, perm_total,
                                   (const int32_t *)nullptr);
        }
        if (hipGetLastError() != hipSuccess) {
            set_error("forest build: partition launch failed");
            return MORNA_E_HIP;
        }
        fb_write_late_tables(h);
        return MORNA_OK;
    }
    hipLaunchKernelGGL(post_counts_kernel, dim3((unsigned)((A + 255) / 256)), dim3(256), 0, h->stream, h->forest.ones.p, A,
                       (unsigned long long *)h->host_counts.p, B.epoch);
    {
        ScopedTimer tm(h, MORNA_T_PARTITION, 0);
#define PART_LAUNCH(PT, INV)                                                                                        \
    hipLaunchKernelGGL((partition_kernel<PT, INV>), dim3((unsigned)A), dim3(PT), 0, h->stream, h->forest.tasks.p, N, \
                       h->forest.side.p, h->forest.ones.p, h->forest.work.p, B.inv_p, B.rank_p)
        const bool big_nodes = level_rows >= (int64_t)A * 2048;
        if (fb_part_inv() && big_nodes) PART_LAUNCH(1024, true);
        else if (fb_part_inv()) PART_LAUNCH(256, true);
        else if (big_nodes) PART_LAUNCH(1024, false);
        else PART_LAUNCH(256, false);
#undef PART_LAUNCH
    }
    if (hipGetLastError() != hipSuccess) {
        set_error("forest build: partition launch failed");
        return MORNA_E_HIP;
    }
    fb_write_late_tables(h);   // the previous level's node-table entries, while this level's kernels run
    return MORNA_OK;
}

// the counts of the B.A tasks fb_partition was last called for, into B.h_ones
static int fb_fetch_counts(morna_index *h)
{
    ForestBuild &B = h->fb;
    const int32_t A = B.A;
    B.h_ones.resize((size_t)A);
    volatile unsigned long long *box = (volatile unsigned long long *)h->host_counts.p;
    int64_t spins = 0;
    for (int32_t a = 0; a < A; a++) {
        unsigned long long v;
        while ((uint32_t)((v = box[a]) >> 32) != B.epoch) {
            if (++spins > (int64_t)1 << 22) {
                // not there after a long while: let the stream say what happened (a failed launch, a fault), or
                // simply wait for a very large level the slow way
                if (hipStreamSynchronize(h->stream) != hipSuccess) {
                    set_error("forest build: the partition kernel failed");
                    return MORNA_E_HIP;
                }
                spins = 0;
            }
            __builtin_ia32_pause();
        }
        B.h_ones[(size_t)a] = (int32_t)(uint32_t)v;
    }
    return MORNA_OK;
}

// the level's task list goes up through page-locked staging (the copy of an earlier attempt has long run: its
// counts have been read back since)
// segs (may be null): the runs of split_inv_kernel, behind the tasks in the same staging and the same pull, into a
// buffer of their own -- d_tasks is the next attempt's while the side stream may still be reading them
static int fb_upload_tasks(morna_index *h, const std::vector<SplitTask> &tk, const std::vector<InvSeg> *segs)
{
    const size_t b_tasks = tk.size() * sizeof(SplitTask), b_segs = segs ? segs->size() * sizeof(InvSeg) : 0;
    const size_t bytes = b_tasks + b_segs;
    if (b_segs) MORNA_TRY(h->forest.inv_segs.alloc(segs->size()));
    if (bytes > h->host_tables.cap) {
        if (hipStreamSynchronize(h->stream) != hipSuccess) return MORNA_E_HIP;
        MORNA_TRY(h->host_tables.reserve(bytes, 1 << 16));
    }
    memcpy(h->host_tables.p, tk.data(), b_tasks);
    if (b_segs) memcpy(h->host_tables.p + b_tasks, segs->data(), b_segs);
    static_assert(sizeof(SplitTask) % 16 == 0, "tasks are moved in 16-byte words");
    void *dev_view = h->host_tables.dev();
    if (!dev_view) {
        set_error("forest build: the task staging is not visible to the device");
        return MORNA_E_HIP;
    }
    const int32_t n16 = (int32_t)(bytes / 16);
    if (n16 > 0)
        hipLaunchKernelGGL(pull_tasks_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, h->stream, (const int4 *)dev_view,
                           (int4 *)h->forest.tasks.p, n16, b_segs ? (int4 *)h->forest.inv_segs.p : (int4 *)nullptr, (int32_t)(b_tasks / 16));
    if (hipGetLastError() != hipSuccess) {
        set_error("forest build: task upload failed");
        return MORNA_E_HIP;
    }
    return MORNA_OK;
}

// ---- begin: checks, buffers, the roots
static int fb_begin(morna_index *h, int32_t n_trees, uint32_t seed)
{
    if (h->ev_tables_pending) {   // a previous build may still be copying the host node tables this one is about to clear
        HIP_TRY(hipEventSynchronize(h->ev_tables));   // (only those copies: what was enqueued since is not waited for)
        h->ev_tables_pending = false;
    }
    MORNA_TRY(upload_host_rows(h));
    if (h->n_items <= 0) {
        set_error("no items were added to the index before build()");
        return MORNA_E_EMPTY;
    }
    if (n_trees <= 0) {
        set_error("build: n_trees must be positive (annoy's q = -1 auto mode is not used by morna)");
        return MORNA_E_INVALID;
    }
    if (!h->norms_valid) MORNA_TRY(compute_norms(h));
    if (seed == 0) seed = 123456789u;   // Kiss32Random's default seed
    const int64_t N = h->n_items;
    const int32_t K = h->K, D = h->dim;
    if (h->dpad > TMW_MAX_DPAD) {   // two_means_wide_kernel keeps one centroid in LDS: 128 KiB at 32768
        set_error("build: dimension %d is above the supported %d", D, TMW_MAX_DPAD);
        return MORNA_E_INVALID;
    }
    h->built = false;
    h->n_trees = n_trees;
    h->seed = seed;
    h->stats = morna_forest_stats();
    h->stats.n_items = N;
    h->stats.dim = D;
    h->stats.leaf_capacity = K;
    h->stats.n_trees = n_trees;

    MORNA_TRY(h->perm.alloc((size_t)n_trees * N));
    // scratch lives in the handle: a rebuild (or the next level) reuses it without hipMalloc
    MORNA_TRY(h->forest.work.alloc((size_t)n_trees * N * 2));
    MORNA_TRY(h->forest.side.alloc((size_t)n_trees * N));
    // per-chunk counts of the chunk-parallel partition: what levels of like-sized nodes need (a level of unlike nodes may grow it)
    if (fb_part_form() == 1 && !fb_part_inv()) MORNA_TRY(h->forest.part_counts.alloc((size_t)n_trees * (size_t)(N / PS_CHUNK + 2) * 2));
    // launch-order scratch of the split kernel: buckets of 32 row ids
    const int32_t n_buckets = (int32_t)std::min<int64_t>(SCHED_MAX_BUCKETS, std::max<int64_t>(1, (N + 31) / 32));
    MORNA_TRY(h->forest.hist.alloc((size_t)n_buckets));
    MORNA_TRY(h->forest.cursor.alloc((size_t)n_buckets));
    // matrix-core split: position of every item in every tree's permutation.  The roots' identity at level 0; from then on
    // rewritten for what a level's partitions moved, on the side stream under the next level's two_means (split_inv_kernel)
    // and only in front of a level that takes the matrix-core form.  MORNA_PARTITION_INV=1: kept current by
    // partition_kernel instead (the earlier form, for comparison).
    if (fb_mm_on()) MORNA_TRY(h->forest.inv.alloc((size_t)n_trees * N));
    ForestBuild &B = h->fb;
    B = ForestBuild();
    B.n_trees = n_trees;
    B.seed = seed;
    B.inv_p = fb_mm_on() ? h->forest.inv.p : nullptr;   // by item; by row once the rows have been ordered (rank_p)
    B.turn_t0 = fb_now_us();
    h->splitmm.ord_valid = false;
    {
        const int64_t total = (int64_t)n_trees * N;
        hipLaunchKernelGGL(iota_perm_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->forest.work.p, B.inv_p, N, total);
        HIP_TRY(hipGetLastError());
    }
    // host-side node table, breadth-first ids; roots are 0..T-1
    std::vector<int32_t> &rec = h->h_node_rec, &ntree = h->h_node_tree, &nhp = h->h_node_hp;
    rec.clear(); ntree.clear(); nhp.clear();
    B.cur.resize((size_t)n_trees);
    for (int t = 0; t < n_trees; t++) {
        B.cur[(size_t)t] = Seg{t, 0, 0, (int32_t)N, t};
        rec.insert(rec.end(), {-1, -1, 0, (int32_t)N});
        ntree.push_back(t);
        nhp.push_back(-1);
    }
    B.next_node_id = (int32_t)ntree.size();
    B.phase = ForestBuild::LEVEL;
    return MORNA_OK;
}

// ---- a level opens: its split nodes, room for their hyperplanes (h->hp grows geometrically and is kept across rebuilds;
// slot = n_split_total + index within the level)
static int fb_level(morna_index *h)
{
    ForestBuild &B = h->fb;
    const int32_t dpad = h->dpad, K = h->K;
    if (B.cur.empty()) {
        B.phase = ForestBuild::DONE;
        return MORNA_OK;
    }
    // split nodes of this level, in cur order
    B.split_idx.clear();
    for (size_t i = 0; i < B.cur.size(); i++)
        if (B.cur[i].count > K) B.split_idx.push_back((int32_t)i);
    B.leaves_before = B.leaves.size();
    B.leaves_after = B.leaves_before + B.cur.size() - B.split_idx.size();
    B.leaves_listed = false;
    h->stats.max_depth = std::max<int64_t>(h->stats.max_depth, B.level);
    if (B.split_idx.empty()) {
        fb_list_leaves(h);
        B.phase = ForestBuild::DONE;
        return MORNA_OK;
    }
    if (fb_part_inv() && B.level > 0) {   // the partitions of the level before wrote it
        B.inv_level = B.level;
        B.inv_from = "partition";
    }
    if (B.inv_level == B.level) B.inv_leaf_mark = B.leaves_after;
    const int32_t S = B.S = (int32_t)B.split_idx.size();
    {
        const size_t need = (size_t)(B.n_split_total + S) * dpad;
        if (need > h->hp.n) {
            F_TRY(hipStreamSynchronize(h->stream));   // the previous level's partition may still be running
            DevBuf<float> bigger;
            MORNA_TRY(bigger.alloc(std::max(need, h->hp.n * 2)));
            if (B.n_split_total > 0)
                F_TRY(hipMemcpy(bigger.p, h->hp.p, (size_t)B.n_split_total * dpad * 4, hipMemcpyDeviceToDevice));
            h->hp.release();
            h->hp.p = bigger.p;
            h->hp.n = bigger.n;
            bigger.p = nullptr;
            bigger.n = 0;
        }
    }
    // final outcome per split node of this level
    B.final_ones.assign((size_t)S, 0);
    B.todo.resize((size_t)S);
    for (int32_t i = 0; i < S; i++) B.todo[(size_t)i] = i;
    MORNA_TRY(h->forest.tasks.alloc((size_t)S));
    MORNA_TRY(h->forest.ones.alloc((size_t)S));
    B.attempt = 0;
    B.phase = ForestBuild::ENQUEUE;
    return MORNA_OK;
}

// ---- an attempt is enqueued: tasks up, side work, two_means, split, post_counts and partition
static int fb_enqueue(morna_index *h)
{
    ForestBuild &B = h->fb;
    const int64_t N = h->n_items;
    const int32_t dpad = h->dpad, D = h->dim, n_trees = B.n_trees, level = B.level, S = B.S;
    const int attempt = B.attempt;
    const uint32_t seed = B.seed;
    const bool mm_on = fb_mm_on(), part_inv = fb_part_inv(), debug_turn = fb_debug_turn();
    static const bool order_on = env_on("MORNA_SPLIT_ORDER");
    DevBuf<int32_t> &work = h->forest.work, &d_ones = h->forest.ones;
    DevBuf<uint8_t> &side = h->forest.side;
    DevBuf<SplitTask> &d_tasks = h->forest.tasks;
    float *hp_level = h->hp.p + (size_t)B.n_split_total * dpad;
    std::vector<SplitTask> &tasks = B.tasks;
    std::vector<int32_t> &tree_first = B.tree_first;
    int rc = MORNA_OK;

    const int32_t n_chunks = fb_make_tasks(B, B.todo, attempt, tasks);
    const int32_t A = (int32_t)tasks.size();
    int64_t rows = 0;
    for (const SplitTask &t : tasks) rows += t.count;
    B.rows = rows;
    // most split nodes of one tree in this attempt (tree_first[t]: the first task of tree t)
    int max_per_tree = 0;
    tree_first.assign((size_t)n_trees + 1, A);
    for (int32_t a = A - 1; a >= 0; a--) tree_first[(size_t)tasks[(size_t)a].tree] = a;
    for (int t = n_trees - 1; t >= 0; t--)
        if (tree_first[(size_t)t] > tree_first[(size_t)t + 1]) tree_first[(size_t)t] = tree_first[(size_t)t + 1];
    for (int t = 0; t < n_trees; t++)
        max_per_tree = std::max(max_per_tree, tree_first[(size_t)t + 1] - tree_first[(size_t)t]);
    // While a tree has few split nodes and most rows still sit in split nodes, the whole level is one
    // contraction on the matrix cores (splitmm.hip): its cost grows with the nodes per tree (every row
    // meets every hyperplane), the chunk form's does not -- they meet near 64 nodes per tree.
    // MORNA_SPLIT_MM=0 turns it off (the chunk form at every level).
    // Once the rows of the contraction are ordered and the level has enough tasks for the per-tile lists
    // (splitmm.hip), a row tile meets only the tasks that hold one of its rows, and the cost follows the (tile,
    // task) pairs that exist: then deeper levels (up to 256 nodes per tree) and the retries of a level go there too,
    // as does any set of tasks whose all-pairs product in 128 x 128 tiles is cheaper than streaming the rows once
    // per tree (measured at D = 3000: 0.13 us per tile pair, 0.47 ns per row of the chunk form, both ~ dpad).
    // On a shard of 200k x 3000 the chunk form took 28 of the split's 34 ms, retries and levels 7+.
    static const bool lists_env = env_on("MORNA_SPLIT_LISTS");
    const bool mm_lists = lists_env && h->splitmm.ord_valid && A >= 512 && max_per_tree <= 256;
    const double mm_dense_us = (double)((N + 127) / 128) * (double)((A + 127) / 128) * 0.13, chunk_us = (double)rows * 0.47e-3;
    const bool use_mm = mm_on && max_per_tree >= 1 &&
                        (mm_lists || (max_per_tree <= 32 && (attempt == 0 ? rows * 2 >= (int64_t)n_trees * N : mm_dense_us < chunk_us)));
    // What of the level does not depend on its hyperplanes runs on the side stream, under two_means: the fp16 image
    // of the rows (once per set of rows), the order of the contraction's rows (second level), `inv`, the per-tile
    // task lists.
    const bool prep_job = use_mm && !h->half.valid;
    // second level: the rows of the contraction are put in an order in which neighbours are alike (the sides of
    // the root splits say which are); from here on `inv` is by row (splitmm.hip, split_mm_order_rows; its
    // counting sort's table is 16 KB per 256 rows: up to 4 M rows).  (Under MORNA_PARTITION_INV=1 only on a first
    // attempt: the partitions of the nodes an earlier attempt accepted have written the other buffer.)
    const bool order_job = use_mm && !prep_job && order_on && level == 1 && (attempt == 0 || !part_inv) && !h->splitmm.ord_valid && N >= 8192 &&
                           N <= ((int64_t)1 << 22) && n_trees >= 2;
    // `inv` is brought up to this level when the contraction is about to read it and it is not there yet: the first
    // attempt of a level >= 1 (a retry's tasks were not moved, and the rows of the nodes accepted meanwhile keep
    // positions inside their own old segment, which is no task of the retry), or a retry that is the level's first
    // attempt in the matrix-core form.  Not in front of chunk-form levels, not after the last level.  The
    // contraction decides membership by position alone, so EVERY row moved since inv_level must be rewritten, the
    // rows that landed in a leaf too (a stale position could lie inside their split sibling): the runs cover all of
    // `cur` and the leaves of the levels in between.  A new order of the rows rewrites everything.
    const bool inv_job = use_mm && (order_job || B.inv_level != level);
    int32_t inv_chunks = 0;
    if (inv_job && B.inv_level == level - 1 && B.inv_next_level == level) {
        // the rule: the level before was the last `inv` was true for.  Its split nodes were all partitioned, and a
        // node's segment now holds its two children side by side: the runs are those segments, listed while that
        // level's kernels ran (the roots' segments are every row: a new order of the rows is covered too)
        B.inv_segs.swap(B.inv_segs_next);
        inv_chunks = B.inv_chunks_next;
    } else if (inv_job) {
        B.inv_segs.clear();
        auto add_run = [&](int32_t tree, int32_t lvl, int32_t start, int32_t count) {
            if (count <= 0) return;
            B.inv_segs.push_back(InvSeg{tree * 2 + (lvl & 1), start, count, inv_chunks});
            inv_chunks += (count + SPLIT_INV_CHUNK - 1) / SPLIT_INV_CHUNK;
        };
        for (size_t l = order_job ? 0 : B.inv_leaf_mark; l < B.leaves_before; l++)
            add_run(B.leaves[l].tree, B.leaves[l].level, B.leaves[l].start, B.leaves[l].count);
        for (const Seg &sg : B.cur) add_run(sg.tree, sg.level, sg.start, sg.count);
    }
    MORNA_TRY(fb_upload_tasks(h, tasks, inv_job ? &B.inv_segs : nullptr));
    B.turn_pulled = debug_turn ? fb_now_us() - B.turn_t0 : 0.0;
    // (d_ones is zeroed by the two_means kernel of the attempt, task by task: a hipMemsetAsync costs ~15 us of
    // idle device around its few microseconds)
    // The matrix-core split's buffers for this attempt, before anything of it is enqueued (and the buffers and the
    // state of a new order of the rows: the lists depend on it).  The per-tile task lists read the tasks, the
    // permutations and the order of the rows -- nothing two_means makes: they are built beside it
    // (MORNA_SPLIT_LISTS_AHEAD=0: in front of the contraction, behind two_means).
    HalfImageOut img = {nullptr, nullptr, nullptr, nullptr};
    bool lists_ahead = false;
    if (order_job) MORNA_TRY(split_mm_order_begin(h, n_trees, &B.rank_p, &B.inv_p));
    if (use_mm) {
        static const bool ahead_on = env_on("MORNA_SPLIT_LISTS_AHEAD");
        MORNA_TRY(split_mm_level_begin(h, A, S, &img));
        lists_ahead = ahead_on && split_mm_level_uses_lists(h, A);
    }
    // ONE fork behind the task list (and so behind the previous level's partition), one join in front of the split.
    // (Enqueued in front of the two_means launch: behind it, which would let two_means start up to ten launches of
    // host time sooner, measured no different -- the host is not what a level's start waits for.)
    // The order by groups is some twenty launches, 0.12 ms of host time that this level's two_means would start later by: there
    // the fork alone goes in front of the two_means launch and the side stream's launches behind it.
    const bool side_work = prep_job || order_job || inv_job || lists_ahead;
    // With the streaming partition the device is through a level's partition before the host has enqueued the next level:
    // whatever is launched first starts first, and a side-stream kernel that starts in front of two_means takes the CUs its
    // workgroups would have started on (level 2 of the default run: split_inv_kernel 3 us ahead, two_means 0.54 instead of
    // 0.39 ms).  So there, too, the side stream's launches go behind the two_means launch.
    const bool side_late = (order_job && split_mm_order_by_groups()) || (fb_part_form() != 0 && !part_inv);
    auto enqueue_side = [&]() -> int {
        if (prep_job) MORNA_TRY(split_mm_prepare_rows(h, h->stream2));
        if (order_job) MORNA_TRY(split_mm_order_rows(h, side.p, n_trees, h->stream2));
        if (inv_job)
            MORNA_TRY(split_mm_level_inv(h, h->forest.inv_segs.p, (int32_t)B.inv_segs.size(), inv_chunks, work.p, B.rank_p, B.inv_p,
                                         h->stream2));
        if (lists_ahead) MORNA_TRY(split_mm_level_lists(h, d_tasks.p, A, work.p, h->stream2));
        F_TRY(hipEventRecord(h->ev_join, h->stream2));
        return MORNA_OK;
    };
    if (side_work) {
        F_TRY(hipEventRecord(h->ev_fork, h->stream));
        F_TRY(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
        if (!side_late) MORNA_TRY(enqueue_side());
    }
    if (inv_job) {
        B.inv_level = level;
        B.inv_leaf_mark = B.leaves_after;
        B.inv_from = "side";
    }
    // the two_means forms that end with the hyperplane in registers also write its fp16 image for the split
    // (MORNA_TM_HALF_EPILOGUE=0: a conversion launch behind two_means, as for the LDS form)
    static const bool tm_half_on = env_on("MORNA_TM_HALF_EPILOGUE");
    if (!tm_half_on) img.h16 = nullptr;
    const char *image_from = nullptr;
    {
        ScopedTimer tm(h, MORNA_T_TWO_MEANS, 4 * (int64_t)D * (TM_ITERS + 2) * A);
        const int nvq = (dpad / 4 + WAVE - 1) / WAVE;   // float4 per lane per row
        const unsigned wg = (unsigned)((A + 3) / 4);
#define TMW_LAUNCH(NVV)                                                                                              \
    hipLaunchKernelGGL(two_means_wave_kernel<NVV>, dim3(wg), dim3(256), 0, h->stream, h->X.p, h->rowinfo.p, N, dpad, \
                       work.p, d_tasks.p, A, seed, hp_level, d_ones.p, img)
        // Four waves per node (strips) while the level's nodes fit the chip at once (2 workgroups per CU): the
        // node's 200-step chain is then 2-3x shorter (C3: 0.32 / 0.28 ms instead of 0.7 ms at the two
        // shallowest levels).  Deeper levels are bound by the HBM gather of the rows (C3, 1600 nodes: 5.9 TB/s)
        // and four waves per node only add work there.  MORNA_TM_STRIP=0: one wave per node everywhere.
        static const bool tm_strip_on = env_on("MORNA_TM_STRIP");
        const bool tm_strip = tm_strip_on && A <= 2 * h->n_cus;
        const bool strip_runs = tm_strip && (nvq == 12 || nvq == 8 || nvq == 4 || (nvq >= 16 && nvq <= 32 && nvq % 4 == 0));
        // per kernel, beside the group; the wide form (dpad > 8192: strips, four waves per node) counts as strips
        ScopedTimer tk(h, strip_runs || dpad > 8192 ? MORNA_T_TM_STRIP : MORNA_T_TM_WAVE, 4 * (int64_t)D * (TM_ITERS + 2) * A);
#define TMS_LAUNCH(NVV)                                                                                                 \
    hipLaunchKernelGGL((two_means_strip_kernel<NVV, TM_STRIP_DEPTH>), dim3((unsigned)A), dim3(256), 0, h->stream, h->X.p, \
                       h->rowinfo.p, N, dpad, work.p, d_tasks.p, seed, hp_level, d_ones.p, img)
#define TMX_LAUNCH(NGV)                                                                                                   \
    do {                                                                                                                  \
        F_TRY(hipFuncSetAttribute((const void *)two_means_wide_kernel<NGV>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                    (int)tm_wide_lds(dpad)));                                                             \
        hipLaunchKernelGGL(two_means_wide_kernel<NGV>, dim3((unsigned)A), dim3(256), tm_wide_lds(dpad), h->stream,       \
                           h->X.p, h->rowinfo.p, N, dpad, work.p, d_tasks.p, seed, hp_level, d_ones.p, img);               \
    } while (0)
        // who leaves the image: every form but the LDS one (row lengths without a register form)
        const bool wave_runs = nvq == 1 || nvq == 2 || nvq == 3 || nvq == 4 || nvq == 6 || nvq == 8 || nvq == 12;
        if (img.h16) image_from = dpad > 8192 ? "wide" : strip_runs ? "strip" : wave_runs ? "wave" : nullptr;
        // rows past 8192 floats: the wide form at every level, whatever the switches (one centroid in LDS)
        if (dpad > 8192) {
            const int ngw = dpad / 256 / 4;   // full groups of four k-steps
            if (ngw <= 12) TMX_LAUNCH(12);
            else if (ngw <= 16) TMX_LAUNCH(16);
            else if (ngw <= 24) TMX_LAUNCH(24);
            else TMX_LAUNCH(32);
        } else if (tm_strip && nvq == 12) TMS_LAUNCH(12);
        else if (tm_strip && nvq == 8) TMS_LAUNCH(8);
        else if (tm_strip && nvq == 4) TMS_LAUNCH(4);
        else if (tm_strip && nvq == 16) TMS_LAUNCH(16);   // rows too long for the one-wave register form: strips
        else if (tm_strip && nvq == 20) TMS_LAUNCH(20);   // (8 float4 per lane and array at D = 8192) instead of the
        else if (tm_strip && nvq == 24) TMS_LAUNCH(24);   // LDS form
        else if (tm_strip && nvq == 28) TMS_LAUNCH(28);
        else if (tm_strip && nvq == 32) TMS_LAUNCH(32);
        else if (nvq == 1) TMW_LAUNCH(1);
        else if (nvq == 2) TMW_LAUNCH(2);
        else if (nvq == 3) TMW_LAUNCH(3);
        else if (nvq == 4) TMW_LAUNCH(4);
        else if (nvq == 6) TMW_LAUNCH(6);
        else if (nvq == 8) TMW_LAUNCH(8);
        else if (nvq == 12) TMW_LAUNCH(12);
        else   // other row lengths (or too long for the register file): centroids in LDS, one workgroup per node
            hipLaunchKernelGGL(two_means_kernel, dim3((unsigned)A), dim3(TM_THREADS), (size_t)dpad * 4 * 3, h->stream,
                               h->X.p, h->norm2.p, N, dpad, work.p, d_tasks.p, seed, hp_level, d_ones.p);
#undef TMW_LAUNCH
#undef TMS_LAUNCH
#undef TMX_LAUNCH
    }
    if (side_late) MORNA_TRY(enqueue_side());
    B.turn_tm = debug_turn ? fb_now_us() - B.turn_t0 : 0.0;
    fb_list_leaves(h);
    if (attempt == 0 && mm_on && !part_inv) {
        // the runs the NEXT level's split_inv_kernel walks, should it take the matrix-core form: this level's split
        // nodes, in the image their children will be in (host time nobody waits for)
        B.inv_segs_next.clear();
        B.inv_chunks_next = 0;
        for (int32_t i : B.split_idx) {
            const Seg &sg = B.cur[(size_t)i];
            B.inv_segs_next.push_back(InvSeg{sg.tree * 2 + ((sg.level + 1) & 1), sg.start, sg.count, B.inv_chunks_next});
            B.inv_chunks_next += (sg.count + SPLIT_INV_CHUNK - 1) / SPLIT_INV_CHUNK;
        }
        B.inv_next_level = level + 1;
    }
    if (!use_mm) {
        // chunk form: launch order = chunks sorted by first row id, one contiguous run per XCD
        DevBuf<int32_t> &d_hist = h->forest.hist, &d_cursor = h->forest.cursor;
        DevBuf<int2> &d_info = h->forest.info, &d_sched = h->forest.sched;
        const int32_t n_buckets = (int32_t)std::min<int64_t>(SCHED_MAX_BUCKETS, std::max<int64_t>(1, (N + 31) / 32));
        if ((rc = d_info.alloc((size_t)n_chunks)) || (rc = d_sched.alloc((size_t)n_chunks))) return rc;
        F_TRY(hipMemsetAsync(d_hist.p, 0, (size_t)n_buckets * 4, h->stream));
        const unsigned cb = (unsigned)((n_chunks + 255) / 256);
        hipLaunchKernelGGL(sched_bucket_kernel, dim3(cb), dim3(256), 0, h->stream, d_tasks.p, A, n_chunks, work.p, N,
                           n_buckets, d_hist.p, d_info.p);
        hipLaunchKernelGGL(sched_scan_kernel, dim3(1), dim3(1024), 0, h->stream, d_hist.p, n_buckets, d_cursor.p);
        hipLaunchKernelGGL(sched_scatter_kernel, dim3(cb), dim3(256), 0, h->stream, d_tasks.p, n_chunks, d_info.p,
                           d_cursor.p, d_sched.p);
    }
    if (side_work) F_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
    if (use_mm) {
        ScopedTimer tm(h, MORNA_T_SPLIT, 4 * (int64_t)D * (rows + A));
        MORNA_TRY(split_mm_level(h, d_tasks.p, A, S, hp_level, work.p, B.inv_p, seed, side.p, d_ones.p, image_from, lists_ahead,
                                 B.inv_from, level));
    } else {
        // algorithmic bytes: 4*D*sum|node| + 4*D*#split nodes
        ScopedTimer tm(h, MORNA_T_SPLIT, 4 * (int64_t)D * (rows + A));
        const unsigned grid = 8u * (unsigned)((n_chunks + 7) / 8);
        if (dpad > 8192)   // the hyperplane in LDS: up to 128 KiB
            F_TRY(hipFuncSetAttribute((const void *)split_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, dpad * 4));
        hipLaunchKernelGGL(split_kernel, dim3(grid), dim3(SP_THREADS), (size_t)dpad * 4, h->stream, h->X.p, N, dpad,
                           work.p, d_tasks.p, h->forest.sched.p, n_chunks, seed, hp_level, side.p, d_ones.p);
    }
    F_TRY(hipGetLastError());
    B.turn_split = debug_turn ? fb_now_us() - B.turn_t0 : 0.0;
    MORNA_TRY(fb_partition(h, A, rows));
    B.phase = ForestBuild::COLLECT;
    return MORNA_OK;
}

// ---- the attempt's counts are read: which nodes stand, which go into the next attempt
static int fb_collect(morna_index *h)
{
    ForestBuild &B = h->fb;
    MORNA_TRY(fb_fetch_counts(h));
    const int32_t A = B.A;
    if (fb_debug_turn()) {
        const double now = fb_now_us() - B.turn_t0;
        char line[256];
        snprintf(line, sizeof line,
                 "[morna] turn: level=%d attempt=%d tasks=%d counts_complete=%.1f tasks_pulled=%.1f two_means_enqueued=%.1f "
                 "split_enqueued=%.1f\n",
                 (int)B.level, B.attempt, (int)A, B.turn_counts, B.turn_pulled, B.turn_tm, B.turn_split);
        B.turn_log += line;
        B.turn_counts = now;
    }
    h->stats.split_attempts += A;
    h->stats.split_rows += B.rows;
    std::vector<int32_t> still;
    for (int32_t a = 0; a < A; a++) {
        const int32_t i = B.todo[(size_t)a];
        B.final_ones[(size_t)i] = B.h_ones[(size_t)a];
        const int64_t n1 = B.h_ones[(size_t)a], n0 = B.tasks[(size_t)a].count - n1;
        if (!(split_imbalance(n0, n1) < 0.95)) still.push_back(i);   // attempts 0, 1: sides_stand(); 2: sorted out below
    }
    B.todo.swap(still);
    B.attempt++;
    B.phase = B.attempt < 3 && !B.todo.empty() ? ForestBuild::ENQUEUE : ForestBuild::FALLBACK;
    return MORNA_OK;
}

// ---- "If we didn't find a hyperplane, just randomize sides as a last option"
static int fb_fallback(morna_index *h)
{
    ForestBuild &B = h->fb;
    B.phase = ForestBuild::CHILDREN;
    std::vector<int32_t> fb;
    for (int32_t i : B.todo) {
        const int64_t n1 = B.final_ones[(size_t)i], n0 = B.cur[(size_t)B.split_idx[(size_t)i]].count - n1;
        if (split_imbalance(n0, n1) > 0.99) fb.push_back(i);
    }
    if (fb.empty()) return MORNA_OK;
    fb_make_tasks(B, fb, 3, B.tasks);
    const int32_t A = (int32_t)B.tasks.size();
    MORNA_TRY(fb_upload_tasks(h, B.tasks, nullptr));
    hipLaunchKernelGGL(fallback_kernel, dim3((unsigned)A), dim3(256), 0, h->stream, h->forest.tasks.p, h->n_items, h->dpad, B.seed,
                       h->forest.side.p, h->forest.ones.p, h->hp.p + (size_t)B.n_split_total * h->dpad);
    F_TRY(hipGetLastError());
    int64_t fb_rows = 0;
    for (const SplitTask &t : B.tasks) fb_rows += t.count;
    MORNA_TRY(fb_partition(h, A, fb_rows));
    MORNA_TRY(fb_fetch_counts(h));
    for (int32_t a = 0; a < A; a++) B.final_ones[(size_t)fb[(size_t)a]] = B.h_ones[(size_t)a];
    h->stats.fallback_nodes += A;
    return MORNA_OK;
}

// ---- children: ids base + 2*i + side for the i-th split node of the level.  Only the segments the NEXT level is cut
// from are made now; the node table's entries (a few thousand vector appends) wait until that level's kernels
// have been enqueued -- the device is idle while the host stands between a level's counts and the next launch
static void fb_children(morna_index *h)
{
    ForestBuild &B = h->fb;
    const int32_t S = B.S;
    B.nxt.clear();
    B.nxt.reserve((size_t)S * 2);
    B.late_parents.resize((size_t)S);
    B.late_ones.assign(B.final_ones.begin(), B.final_ones.end());
    B.late_first_id = B.next_node_id;
    B.late_first_hp = B.n_split_total;
    for (int32_t i = 0; i < S; i++) {
        const Seg &s = B.cur[(size_t)B.split_idx[(size_t)i]];
        const int32_t n1 = B.final_ones[(size_t)i], n0 = s.count - n1;
        const int32_t id0 = B.next_node_id + 2 * i, id1 = id0 + 1;
        B.late_parents[(size_t)i] = s;
        B.nxt.push_back(Seg{s.tree, s.level + 1, s.start, n0, id0});
        B.nxt.push_back(Seg{s.tree, s.level + 1, s.start + n0, n1, id1});
    }
    B.next_node_id += 2 * S;
    B.late_pending = true;
    B.n_split_total += S;
    B.cur.swap(B.nxt);
    B.level++;
    B.phase = ForestBuild::LEVEL;
}

// ---- behind the last level: late tables, leaf gather, node tables to HBM, ev_tables, the stats
static int fb_tables(morna_index *h)
{
    ForestBuild &B = h->fb;
    const int64_t N = h->n_items;
    std::vector<int32_t> &rec = h->h_node_rec, &ntree = h->h_node_tree, &nhp = h->h_node_hp;
    fb_write_late_tables(h);
    if (fb_debug_turn()) fputs(B.turn_log.c_str(), stderr);
    // consolidate hyperplanes and node tables in HBM
    h->n_split = B.n_split_total;
    h->n_nodes = (int64_t)ntree.size();
    MORNA_TRY(h->hp.alloc((size_t)h->dpad));   // never a null hyperplane table (N <= K: no split at all)
    MORNA_TRY(h->node_rec.alloc(rec.size()));
    MORNA_TRY(h->node_tree.alloc(ntree.size()));
    MORNA_TRY(h->node_hp.alloc(nhp.size()));
    {
        // through page-locked staging: a copy from the pageable vectors is staged by the runtime, ~20 us of host time each,
        // and the device has nothing else to do just then
        const std::vector<LeafSeg> &leaves = B.leaves;
        const size_t b_rec = rec.size() * 4, b_tree = ntree.size() * 4, b_hp = nhp.size() * 4, b_leaf = leaves.size() * sizeof(LeafSeg);
        const size_t o_tree = b_rec /* 16 bytes per node */, o_hp = (o_tree + b_tree + 15) / 16 * 16, o_leaf = (o_hp + b_hp + 15) / 16 * 16,
                     need = o_leaf + b_leaf;
        static_assert(sizeof(LeafSeg) == 16, "leaves are moved in 16-byte words");
        if (need > h->host_tables.cap) {
            if (h->host_tables.p) {
                if (h->ev_tables_pending) F_TRY(hipEventSynchronize(h->ev_tables));   // a copy out of the old buffer may be in flight
                F_TRY(hipStreamSynchronize(h->stream));                               // (or a task list being pulled)
            }
            MORNA_TRY(h->host_tables.reserve(need));
        }
        memcpy(h->host_tables.p, rec.data(), b_rec);
        memcpy(h->host_tables.p + o_tree, ntree.data(), b_tree);
        memcpy(h->host_tables.p + o_hp, nhp.data(), b_hp);
        memcpy(h->host_tables.p + o_leaf, leaves.data(), b_leaf);
        // (pulled by the device, as the task lists are; the tables are whole 16-byte words apart from their tails)
        const uint8_t *dv = (const uint8_t *)h->host_tables.dev();
        if (!dv) {
            set_error("forest build: the node-table staging is not visible to the device");
            return MORNA_E_HIP;
        }
        auto pull = [&](void *dst, const uint8_t *src, size_t bytes) -> hipError_t {
            const int32_t n16 = (int32_t)(bytes / 16);
            if (n16 > 0)
                hipLaunchKernelGGL(pull_tasks_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, h->stream, (const int4 *)src,
                                   (int4 *)dst, n16, (int4 *)nullptr, 0);
            if (bytes % 16)   // the tail, if any
                return hipMemcpyAsync((uint8_t *)dst + (size_t)n16 * 16, h->host_tables.p + (src - dv) + (size_t)n16 * 16, bytes % 16,
                                      hipMemcpyHostToDevice, h->stream);
            return hipGetLastError();
        };
        // the leaves first: their items go from the work images into the permutation the searches read
        DevBuf<uint8_t> &d_leaves = h->forest.leaves;
        MORNA_TRY(d_leaves.alloc(std::max<size_t>(b_leaf, 16)));
        F_TRY(pull(d_leaves.p, dv + o_leaf, b_leaf));
        if (!leaves.empty())
            hipLaunchKernelGGL(gather_leaves_kernel, dim3((unsigned)leaves.size()), dim3(256), 0, h->stream, (const LeafSeg *)d_leaves.p,
                               h->forest.work.p, N, h->perm.p);
        F_TRY(hipGetLastError());
        F_TRY(pull(h->node_rec.p, dv, b_rec));
        F_TRY(pull(h->node_tree.p, dv + o_tree, b_tree));
        F_TRY(pull(h->node_hp.p, dv + o_hp, b_hp));
    }
    // No wait here: the last partition and these copies are ordered on the handle's stream in front of whatever the caller
    // does next with the handle (a search starts without the device draining first); the staging they read belongs to the
    // handle and is next written by another build, which waits for ev_tables first.  Blocking copies settle() as well.
    if (!h->ev_tables) F_TRY(hipEventCreateWithFlags(&h->ev_tables, hipEventDisableTiming));
    F_TRY(hipEventRecord(h->ev_tables, h->stream));
    h->ev_tables_pending = true;
    h->unsettled = true;
    h->stats.n_nodes = h->n_nodes;
    h->stats.n_split = h->n_split;
    h->stats.n_leaves = h->n_nodes - h->n_split;
    h->built = true;
    return MORNA_OK;
}

// A level is narrow when its first attempt has so few tasks that its two_means leaves nearly every CU idle: n_cus / 8
// nodes, one workgroup each ("the tail").  MORNA_BUILD_TAIL=0: the build never returns early.
static bool fb_narrow(const morna_index *h)
{
    static const bool tail_on = env_on("MORNA_BUILD_TAIL");
    const ForestBuild &B = h->fb;
    return tail_on && B.level >= 1 && B.attempt == 0 && B.S <= h->n_cus / 8;
}

// The loop.  may_defer: return (B.pending) behind the enqueue of the first attempt of the first narrow level.
static int fb_run(morna_index *h, bool may_defer)
{
    ForestBuild &B = h->fb;
    for (;;) {
        switch (B.phase) {
        case ForestBuild::LEVEL:
            MORNA_TRY(fb_level(h));
            if (B.defer_level >= 0 && B.phase == ForestBuild::ENQUEUE) B.tail_levels++;
            break;
        case ForestBuild::ENQUEUE: {
            const bool defer = may_defer && fb_narrow(h);
            // what starts beside the tail waits for everything in front of it (the wide levels, the fp16 rows)
            if (defer) F_TRY(hipEventRecord(h->ev_tail, h->stream));
            MORNA_TRY(fb_enqueue(h));
            if (B.defer_level >= 0) B.tail_attempts++;
            if (defer) {
                B.defer_level = B.level;
                B.tail_levels = B.tail_attempts = 1;
                B.pending = true;
                if (fb_debug_open()) fprintf(stderr, "[morna] build tail: deferred at level=%d tasks=%d\n", (int)B.level, (int)B.A);
                return MORNA_OK;
            }
            break;
        }
        case ForestBuild::COLLECT: MORNA_TRY(fb_collect(h)); break;
        case ForestBuild::FALLBACK: MORNA_TRY(fb_fallback(h)); break;
        case ForestBuild::CHILDREN: fb_children(h); break;
        case ForestBuild::DONE: return fb_tables(h);
        default: set_error("forest build: no build under way"); return MORNA_E_STATE;
        }
    }
}
#undef F_TRY

// a failed build leaves nothing pending, nothing running and the handle unbuilt
static int fb_end(morna_index *h, int rc)
{
    if (rc != MORNA_OK) {
        fb_sync(h);
        h->fb.pending = false;
        h->built = false;
    }
    if (!h->fb.pending) h->fb.phase = ForestBuild::IDLE;
    return rc;
}

int build_forest(morna_index *h, int32_t n_trees, uint32_t seed)
{
    MORNA_TRY(finish_build(h, "build"));
    MORNA_TRY(fb_begin(h, n_trees, seed));
    return fb_end(h, fb_run(h, true));
}

int finish_build(morna_index *h, const char *who)
{
    ForestBuild &B = h->fb;
    if (!B.pending) return MORNA_OK;
    B.pending = false;
    HIP_TRY(hipSetDevice(h->device));
    const int rc = fb_end(h, fb_run(h, false));
    if (fb_debug_open())
        fprintf(stderr, "[morna] build tail: finished by %s: levels=%d attempts=%d%s\n", who, (int)B.tail_levels, (int)B.tail_attempts,
                rc == MORNA_OK ? "" : " (failed)");
    return rc;
}
