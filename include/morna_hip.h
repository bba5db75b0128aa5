/*
 * morna_hip.h -- C ABI of libmorna_hip.so, the MI355X (gfx950) implementation of
 * morna's index-build + nearest-neighbour search hot path.
 *
 * This is the drop-in boundary: the entry points are what a binding for the
 * reference's two native dependencies on this path would call.  Each one cites
 * the reference interface it replaces (file:line under commanderson/morna).
 *
 *   annoy.AnnoyIndex (C++ extension, used angular)  morna.py:26, 166, 543
 *   mmh3.hash        (C extension)                  morna.py:20, 369, 591, 625
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is caller-owned HOST memory
 *     unless the name says _dev; the library copies during the call and never
 *     retains a host pointer.
 *   - every function returns 0 on success or a negative MORNA_E_* code; the
 *     message for the calling thread is available from morna_last_error().
 *   - one host thread per handle; the handle owns its HIP stream.
 *   - ids are dense internal ids 0..n_items-1 (morna.py:378-382).
 *   - distances are annoy "angular": sqrt(max(2 - 2 cos, 0)).
 */
#ifndef MORNA_HIP_H
#define MORNA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MORNA_OK            0
#define MORNA_E_INVALID    -1   /* bad argument              -> ValueError  */
#define MORNA_E_HIP        -2   /* HIP runtime failure       -> RuntimeError */
#define MORNA_E_STATE      -3   /* call order (not built...) -> RuntimeError */
#define MORNA_E_RANGE      -4   /* id out of range           -> IndexError  */
#define MORNA_E_IO         -5   /* save / load               -> IOError     */
#define MORNA_E_EMPTY      -6   /* no items (morna.py:399-403) -> ValueError */

typedef struct morna_index morna_index;

/* AnnoyIndex(dim, metric='angular')                          morna.py:166, 543, 1171 */
int morna_index_create(int32_t dim, int32_t device, morna_index **out);
int morna_index_destroy(morna_index *h);
/* HIP devices the library can create indexes on (0 and MORNA_E_HIP when there is none: the library has no CPU path) */
int morna_device_count(int32_t *count_out);
const char *morna_last_error(void);

/* mmh3.hash(key) -- host mirror of the device hash            morna.py:369, 591, 625 */
int32_t morna_hash32(const uint8_t *key, int64_t len);

/* ---- items --------------------------------------------------------------- */

/* AnnoyIndex.add_item(i, vector): fp64 -> fp32 happens here    morna.py:406, 423 */
int morna_add_item(morna_index *h, int32_t id, const double *v);
/* bulk form: rows[n][dim] fp32 become items first_id .. first_id+n-1 */
int morna_add_items_f32(morna_index *h, int32_t first_id, const float *rows, int64_t n);

/*
 * Fused replacement for the add_junction loop + add_item hand-off
 * (morna.py:344-388, 405-424): J kept junction lines in FILE ORDER.
 *   key_bytes/key_off[J+1]  the "chrom start end" strings        morna.py:849
 *   row_ptr[J+1]            extent of each line's lists
 *   item_ids[nnz]           INTERNAL id of each sample           morna.py:377-382
 *                           (every id lies in [0, n_items) of the build_features call that follows: stage records the
 *                           smallest and the largest, and build_features answers MORNA_E_RANGE, naming the bound
 *                           that is broken, before it launches anything)
 *   cov[nnz]                coverages                            morna.py:852
 *   idf[J]                  log(sample_count / cumulative freq)  morna.py:372-374
 *                           (host libm, so that it is bit-identical to Python)
 * stage = host -> HBM copy only; build_features = the kernels (hash, signed
 * column, fp64 accumulation in file order, fp64 -> fp32, row norms).
 * build_features returns once its kernels are enqueued on the handle's stream: what follows on the handle is
 * ordered behind them (entry points that copy with the host wait first); morna_synchronize() waits explicitly.
 */
int morna_stage_junctions(morna_index *h, const uint8_t *key_bytes, const int64_t *key_off, int64_t J,
                          const int64_t *row_ptr, const int32_t *item_ids, const int32_t *cov,
                          const double *idf);
int morna_build_features(morna_index *h, int64_t n_items);
/*
 * Optional, before build_features: an ORDER of the items in which the sample lists of the lines ascend --
 * order_key[i] for internal id i, e.g. the external sample id (an intropolis line lists its samples in ascending
 * order, morna.py:848-853, while internal ids are first-seen, morna.py:377-382).  Performance only: each entry of the
 * staged lists is then read once instead of once per sample tile; lines that do not ascend in the order, or no
 * order at all, give the same matrix.  Dropped by morna_unstage_junctions; ignored unless n_items matches build_features'.
 */
int morna_stage_item_order(morna_index *h, const int64_t *order_key, int64_t n_items);
int morna_unstage_junctions(morna_index *h);
/* device hash of staged or given keys, for tests: hash/col/sign per key */
int morna_hash_keys(morna_index *h, const uint8_t *key_bytes, const int64_t *key_off, int64_t J,
                    int32_t *hash_out, int32_t *col_out, int32_t *sign_out);

/*
 * Native host pre-pass of `morna index` (no GPU work): go_index's line loop,
 * count_samples and the host half of add_junction                morna.py:841-861, 789-822, 357-382
 * Reads a gzipped (or plain) intropolis file; sample_count <= 0 counts the distinct
 * sample-id strings first, as go_index does without -s.  The result holds exactly the
 * arrays morna_stage_junctions takes, plus the external sample id of every internal id
 * and the final junction -> frequency table (what .map.mor / .freq.mor store).
 */
typedef struct morna_lines morna_lines;
int morna_parse_intropolis(const char *path, int64_t sample_count, int64_t sample_threshold, morna_lines **out);
/* counts[8] = kept lines, nnz, n_items, skipped, sample_count, key bytes, distinct keys, lines read */
int morna_lines_counts(const morna_lines *L, int64_t *counts);
/* borrowed pointers, valid until morna_lines_free; any may be NULL */
int morna_lines_arrays(const morna_lines *L, const uint8_t **key_bytes, const int64_t **key_off,
                       const int64_t **row_ptr, const int32_t **item_ids, const int32_t **cov, const double **idf,
                       const int64_t **ext_ids);
int morna_lines_freq_entry(const morna_lines *L, int64_t i, const char **key, int64_t *key_len, int64_t *freq);
int morna_stage_lines(morna_index *h, const morna_lines *L);
/*
 * Binary pre-tokenised cache of a parse: what go_index's line loop
 * (morna.py:841-861) would recompute on every run over the same file.  tag[4] is the
 * caller's identity of the source (size, mtime, sample_count argument, threshold); load
 * hands it back so the caller can decide whether the cache is still valid.  MORNA_E_IO when
 * the file is missing, truncated or not such a cache.
 */
int morna_lines_save(const morna_lines *L, const char *path, const int64_t *tag);
int morna_lines_load(const char *path, int64_t *tag_out, morna_lines **out);
int morna_lines_free(morna_lines *L);
/*
 * Row shards of ONE parsed data set (the reference has no such path).  The parse is the global pass of
 * add_junction -- threshold on a line's whole sample list, cumulative frequency, idf = log(sample_count / freq) with the
 * GLOBAL sample count (morna.py:357-374), first-seen internal ids over the whole file (morna.py:377-382).  Shard `rank`
 * of `world` owns the global ids [rank * ceil(N / world), (rank + 1) * ceil(N / world)) and gets the lines restricted to
 * the entries of its items, in file order, ids renumbered from 0 (lines left without an entry are dropped; the frequency
 * table stays whole).  The matrices built from the shards, stacked by rank, are the matrix of the whole index bit for bit:
 * a cell's terms and their order (morna.py:376-388) do not depend on the other rows.
 *   morna_lines_shard_info  info[4] = {rank, world, id_offset (global id of local id 0), n_items of the whole data set}
 *   morna_lines_from_arrays the same object from arrays the caller tokenised itself (what morna_stage_junctions takes,
 *                           plus ext_ids[n_items], the external sample id of every internal id, and the sample count)
 */
int morna_lines_shard(const morna_lines *L, int32_t rank, int32_t world, morna_lines **out);
int morna_lines_shard_info(const morna_lines *L, int64_t *info);
int morna_lines_from_arrays(const uint8_t *key_bytes, const int64_t *key_off, int64_t J, const int64_t *row_ptr,
                            const int32_t *item_ids, const int32_t *cov, const double *idf, const int64_t *ext_ids,
                            int64_t n_items, int64_t sample_count, morna_lines **out);
/* Benchmark / test utility (no counterpart in the reference): J lines written as an intropolis text file, gzipped when
 * the path ends in ".gz": key words, "+", "GT", "AG", the sample list, the coverage list, tab separated. */
int morna_write_intropolis(const char *path, const uint8_t *key_bytes, const int64_t *key_off, int64_t J, const int64_t *row_ptr,
                           const int64_t *samples, const int32_t *cov);

/*
 * ---- many query samples at once (the reference answers one per process: MornaSearch, morna.py:597-629, 632-716) ----
 * morna_lines_query_terms  host pre-pass, no GPU work.  L: a QUERY file parsed by morna_parse_intropolis with threshold 0
 *     and a positive sample_count (its idf is not used).  vocab_bytes / vocab_off[V+1] / vocab_df[V]: the index's
 *     junction -> frequency table (.freq.mor; keys "chrom start end", morna.py:849), sample_count: the index's (.stats.mor
 *     line 1, > 0).  The result: the lines whose key is in the table, in file order, each (key, sample) entry on the FIRST
 *     line holding it with its coverages summed (no sample repeats in a line), idf[j] = the key's weight
 *     log(sample_count / df) from libm (0 when df is 0), ext_ids and the query count as in L -- query q is internal id q,
 *     numbered by first appearance (morna.py:377-382).  Keys are compared as written (no normalisation: the raw-stream
 *     key of a canonical decimal coordinate, what intropolis writes).  A summed coverage outside int32 is MORNA_E_INVALID
 *     naming the sample and the key.
 * morna_build_query_rows  the rows of those query samples on the GPU, in buffers of their own on the handle (a second
 *     call replaces them): row[q][c] = +0.0 plus sign(k) * (C(k,q) * w(k)) in fp64, one rounding per operation, once per
 *     distinct key k of q with mmh3(k) mod dim == c, in the order of the first line holding k and q -- exactly
 *     finalize_query's dict order (morna.py:609-629).  Also their fp32 image (what get_nns_by_vector sees).  X, its norms,
 *     the forest and the index's caches are not touched.  Timed under MORNA_T_FEATURES.  With int32 coverages and finite
 *     weights every row is finite and its sum of squares lies inside the exact search's domain ([2^-900, 2^890], or 0).
 * morna_get_query_rows  rows64[nq][dim] fp64 and / or rows32[nq][dim] fp32 to host memory (either may be NULL).
 * morna_get_nns_by_query_rows  morna_get_nns_by_vector with the resident fp32 rows as the queries, nq = the rows built.
 * morna_exact_search_query_rows  morna_exact_search (morna.py:681-716) with the resident fp64 rows as the queries: no
 *     PCIe round trip; batching, count -1 and the rows outside the scan's window as in morna_exact_search.  A query with no
 *     vocabulary junction has the zero row and is answered as the reference answers a zero query_sample.
 */
int morna_lines_query_terms(const morna_lines *L, const uint8_t *vocab_bytes, const int64_t *vocab_off, const int64_t *vocab_df,
                            int64_t V, int64_t sample_count, morna_lines **out);
int morna_build_query_rows(morna_index *h, const morna_lines *T);
int morna_get_query_rows(morna_index *h, double *rows64, float *rows32);
int morna_get_nns_by_query_rows(morna_index *h, int32_t k, int32_t search_k, int32_t *ids_out, float *dist_out, int32_t *count_out);
int morna_exact_search_query_rows(morna_index *h, int32_t k, int32_t *ids_out, double *dist_out, int32_t *count_out);

/*
 * ---- junctions by sample: the store and the filter of `morna junctions` ---------------------------------------------
 * Stand-ins for update_junction_dbs and the per-sample sqlite tables (morna.py:221-341: 100 shards of run-length strings)
 * and for the retention step of the junctions subcommand (morna.py:1501-1569).  The store is the transpose of the
 * junction x sample CSR of a parse: for every sample id of ANY line of the file (update_junction_dbs runs before the
 * threshold test, morna.py:359 vs 361-363) the ascending list of (0-based line number, coverage) (morna.py:215, 357, 1591).
 * A store is one object on one device; one host thread per store.  Limits: 2^31 - 1 lines and samples.
 *   morna_jstore_build        morna.py:221-341 for a whole file: the transpose on the GPU from a parse with threshold 0
 *                             (MORNA_E_INVALID when the lines kept are not the lines read: kept line j must be file line j).
 *                             Deterministic: a stable counting sort without global atomics, the same bytes on every run, a
 *                             sample's lines ascending whatever order a line lists its samples in.  A line that lists a
 *                             sample twice is MORNA_E_INVALID naming the line and the sample: the first such line of the
 *                             file and, of the samples it repeats, the one first seen in the file, whatever the number
 *                             of samples.  The store is resident in HBM and mirrored on the host (what save writes).
 *   morna_jstore_from_arrays  a store from the caller's arrays: ext_ids[n_samples], ptr[n_samples + 1], line / cov
 *                             [ptr[n_samples]].  Validated as load validates (MORNA_E_INVALID).  No GPU work: the arrays
 *                             go to `device` at the first retain.
 *   morna_jstore_save / load  one little-endian blob, <basename>.junc.mor (stands in for the files of morna.py:221-260,
 *                             read back at 1505-1533).  Load checks that ptr is monotone and ends at the entry count, that
 *                             every sample's lines ascend and lie below n_lines, and that the sample ids are distinct:
 *                             MORNA_E_IO for a missing, truncated or inconsistent file.  No GPU work (as from_arrays).
 *   morna_jstore_counts       counts[3] = samples, entries, lines of the file
 *   morna_jstore_samples      ext_ids_out[samples]: the sample ids, the parse's first-seen order
 *   morna_jstore_sample       one sample's list (the SELECT of morna.py:1516-1532): *n_out entries; line_out / cov_out
 *                             (either may be NULL) must hold that many.  MORNA_E_RANGE for an id the store lacks.
 *   morna_jstore_retain       morna.py:1539-1569 for nq result lists at once, on the GPU.  results[nq][k]: EXTERNAL sample
 *                             ids in rank order (morna.py:1501-1504), the first n_results[q] of a row used; min_count[q]:
 *                             int(ceil(frequency_filter * n_results[q])), computed by the caller (morna.py:1551, so that the
 *                             rounding is Python's).  A line is retained when at least one and at least min_count of the
 *                             results hold it, or when one of them covers it coverage_filter times or more.  1 <= k <= 64:
 *                             found_in is one 64-bit word per line (MORNA_E_INVALID beyond, the message names the limit).
 *                             An id the store lacks: MORNA_E_RANGE naming it.
 *   morna_jretained_counts    count_out[nq]: retained lines of every list (len(retain_junctions), morna.py:1573)
 *   morna_jretained_query     borrowed views of list q, valid until morna_jretained_free: lines[count] ascending
 *                             (sorted(retain_junctions), morna.py:1585), masks[count] (bit r set: result r holds the line --
 *                             found_in_map, morna.py:1555), cov_ptr[count + 1] and cov: the coverages of line i in rank
 *                             order are cov[cov_ptr[i] .. cov_ptr[i + 1]) (new_covs, morna.py:1619-1623).  Any may be NULL.
 *   morna_jstore_timers       ms[2] / bytes[2]: HIP-event time of the kernels of the build and of the last retain, and
 *                             their algorithmic bytes (2 x 8 per entry; 8 per entry of the lists named)
 */
typedef struct morna_jstore morna_jstore;
typedef struct morna_jretained morna_jretained;
int morna_jstore_build(int32_t device, const morna_lines *all_lines, morna_jstore **out);
int morna_jstore_from_arrays(int32_t device, const int64_t *ext_ids, int64_t n_samples, const int64_t *ptr, const int32_t *line,
                             const int32_t *cov, int64_t n_lines, morna_jstore **out);
int morna_jstore_save(const morna_jstore *s, const char *path);
int morna_jstore_load(const char *path, int32_t device, morna_jstore **out);
int morna_jstore_free(morna_jstore *s);
int morna_jstore_counts(const morna_jstore *s, int64_t *counts);
int morna_jstore_samples(const morna_jstore *s, int64_t *ext_ids_out);
int morna_jstore_sample(const morna_jstore *s, int64_t ext_id, int64_t *n_out, int32_t *line_out, int32_t *cov_out);
int morna_jstore_retain(morna_jstore *s, const int64_t *results, const int32_t *n_results, const int32_t *min_count, int64_t nq,
                        int32_t k, int64_t coverage_filter, morna_jretained **out);
int morna_jretained_counts(const morna_jretained *r, int64_t *count_out);
int morna_jretained_query(const morna_jretained *r, int64_t q, const int32_t **lines, const uint64_t **masks,
                          const int64_t **cov_ptr, const int32_t **cov);
int morna_jretained_free(morna_jretained *r);
int morna_jstore_timers(const morna_jstore *s, double *ms, int64_t *bytes);

/*
 * ---- unhashed TF-IDF search over the junction store -------------------------------------------------
 * The store is the sample-major CSR of the UNHASHED matrix: dimension j is file line j, a sample's component there is
 * RN(double(coverage) * w[j]).  The distance is cosine_distance's (morna.py:101-114) with its sums taken in ascending
 * line order, `sqrt(max(radicand, 0.0))` at the end; answers are bit-identical to that loop, on every run.
 *   morna_jstore_set_weights  w[n_lines]: the weight of every line; n_lines must be the store's.  Every weight is 0 or a
 *                             finite number in [2^-200, 2^64] (MORNA_E_INVALID naming the line otherwise).  No GPU work:
 *                             the weights go to the device, and the row norms are made, at the first search after it.
 *   morna_jstore_nearest      nq sparse queries: query q holds lines q_line[q_ptr[q] .. q_ptr[q + 1]), ascending, distinct
 *                             and below n_lines, with coverages q_cov >= 0 (MORNA_E_INVALID otherwise); the library forms
 *                             coverage * w itself.  The population is the store samples pop_ext[n_pop] (external ids,
 *                             distinct); results are POSITIONS in pop_ext.  ids_out / dist_out [nq][k], count_out[nq]:
 *                             ascending distance, equal distances by descending position, min(k, n_pop) results and the
 *                             rest -1 / +inf.  1 <= k <= 1024 (MORNA_E_INVALID names the limit).  A negative coverage in a
 *                             population row is MORNA_E_INVALID naming sample and line; an id the store lacks (or one named
 *                             twice in pop_ext) MORNA_E_RANGE naming it.  Any nq: the queries are tiled inside the call.
 *   morna_jstore_nearest_by_sample   the same with the queries taken from the store rows q_ext[nq] (external ids, need not
 *                             be in the population): nothing but ids crosses to the device.
 *   morna_jstore_nearest_stats       of the last call, stats[8]: candidates re-ranked in all, the most for one query, passes
 *                             over the store, kernel ms (HIP events), algorithmic bytes (8 per store entry of the population
 *                             per pass), queries per pass (QT), kernel ms of the row-norm pass (0 when cached), the window.
 */
#define MORNA_JNEAREST_MAX_K 1024
int morna_jstore_set_weights(morna_jstore *s, const double *w, int64_t n_lines);
int morna_jstore_nearest(morna_jstore *s, const int64_t *pop_ext, int64_t n_pop, const int64_t *q_ptr, const int32_t *q_line,
                         const int32_t *q_cov, int64_t nq, int32_t k, int32_t *ids_out, double *dist_out, int32_t *count_out);
int morna_jstore_nearest_by_sample(morna_jstore *s, const int64_t *pop_ext, int64_t n_pop, const int64_t *q_ext, int64_t nq,
                                   int32_t k, int32_t *ids_out, double *dist_out, int32_t *count_out);
int morna_jstore_nearest_stats(const morna_jstore *s, double *stats);

/*
 * ---- the junctions behind a query and each result -----------------------------------------------------
 * The decomposition of the unhashed cosine above for (query, result row) pairs; no counterpart in the reference.  All
 * arithmetic is that search's: v = RN(double(cov) * w[line]); every sum is x = RN(x + term) from 0.0 over the RESULT ROW's
 * entries in ascending line order (qq: over the query's); a line the query lacks has query component +0.0.  Per pair:
 * pq = sum RN(v_r * v_q), pp = sum RN(v_r * v_r), qq, distance (as morna_jstore_nearest); shared = the row's entries with
 * v_r != 0 and v_q != 0; pp_shared = sum of RN(v_r * v_r) where v_q != 0; qq_shared = sum of RN(v_q * v_q) where v_r != 0;
 * n_q, n_r = the entries of query and row with a nonzero component; the top list = the min(top, shared) shared lines of
 * largest RN(v_r * v_q), equal terms by ascending line.  Bit-identical on every run, whatever the tiling.
 *   morna_jstore_explain      nq sparse queries as morna_jstore_nearest takes and checks them; results[nq][k] (external
 *                             sample ids in rank order; list q holds n_results[q] <= k of them, the layout of
 *                             morna_jstore_retain).  Every (query, result) pair of every query in one call; an id may stand
 *                             at several ranks.  1 <= k <= MORNA_JNEAREST_MAX_K, 1 <= top <= MORNA_JEXPLAIN_MAX_TOP,
 *                             nq * k * top <= 2^28 (MORNA_E_INVALID naming the limit); no weights: MORNA_E_STATE; a result id
 *                             the store lacks: MORNA_E_RANGE naming it; a negative coverage in a result row: MORNA_E_INVALID
 *                             naming sample and line.
 *   morna_jstore_explain_by_sample   the same with the queries taken from the store rows q_ext[nq] (external ids; an id the
 *                             store lacks is MORNA_E_RANGE): nothing but ids crosses to the device.
 *   morna_jexplained_pair     the pair (query q, rank < n_results[q]; MORNA_E_RANGE otherwise): sums[6] = pq, pp, qq,
 *                             pp_shared, qq_shared, distance; counts[3] = shared, n_q, n_r; *n_top = min(top, shared);
 *                             lines / terms / cov_r [*n_top]: the top list's line numbers, terms and the RESULT's coverages
 *                             (library-owned, valid until morna_jexplained_free; the lists of a query's ranks follow one
 *                             another, `top` places each).  Any output may be NULL.
 *   morna_jstore_explain_stats       of the last call, stats[6]: pairs, store entries streamed, passes, kernel ms (HIP
 *                             events), algorithmic bytes (8 per entry streamed), queries per pass (QT).  All 0 after a call
 *                             that failed its checks.
 */
#define MORNA_JEXPLAIN_MAX_TOP 64
typedef struct morna_jexplained morna_jexplained;
int morna_jstore_explain(morna_jstore *s, const int64_t *q_ptr, const int32_t *q_line, const int32_t *q_cov, int64_t nq,
                         const int64_t *results /* [nq][k] external ids, rank order */, const int32_t *n_results /* [nq] */,
                         int32_t k, int32_t top, morna_jexplained **out);
int morna_jstore_explain_by_sample(morna_jstore *s, const int64_t *q_ext /* [nq] */, int64_t nq, const int64_t *results,
                                   const int32_t *n_results, int32_t k, int32_t top, morna_jexplained **out);
int morna_jexplained_pair(const morna_jexplained *e, int64_t q, int32_t rank, double *sums /* [6]: pq pp qq pp_shared qq_shared distance */,
                          int64_t *counts /* [3]: shared n_q n_r */, int32_t *n_top, const int32_t **lines, const double **terms,
                          const int32_t **cov_r);
int morna_jexplained_free(morna_jexplained *e);
int morna_jstore_explain_stats(const morna_jstore *s, double *stats /* [6]: pairs, store entries streamed, passes, kernel ms, algorithmic bytes (8 per entry streamed), QT */);

/*
 * ---- junction recovery tables over the filter grid -------------------------------------------------
 * How much of a truth set of lines the retention step gives back under EVERY (frequency, coverage) pair of a grid, from
 * one pass over the result rows.  (The quantities are those junction_recovery_performance.py of the reference's tests/
 * prints per run of its aligner pipeline; here the truth comes from the store or from the caller.)  For list q and line j:
 * cnt = the ranks r < n_results[q] whose row holds j (an id at two ranks counts twice, as retain's one bit per rank does),
 * maxcov = the largest coverage of j among those rows, b = the number of i with cov_grid[i] <= maxcov (0 when cnt = 0),
 * t = 1 when j is a true line of q.  hist_out[nq][2][65][n_grid + 1], int32: entry [q][t][cnt][b] is the number of lines of
 * that class, except that plane t = 0 is left 0 at cnt = 0 (lines nobody holds and nobody wants).  Integer throughout:
 * the same numbers on every run.  retain(f, cov_grid[i]) keeps exactly the lines with cnt >= 1 and (cnt >= min_count or
 * b > i), so every cell of the grid is a sum over hist on the host.
 *   morna_jstore_recovery            results / n_results / k as morna_jstore_retain takes them (1 <= k <= 64, MORNA_E_INVALID
 *                             beyond, the message names the limit; an id the store lacks: MORNA_E_RANGE naming it).  Truth
 *                             as a CSR: the true lines of list q are t_line[t_ptr[q] .. t_ptr[q + 1]), ascending, distinct
 *                             and below the store's line count (MORNA_E_INVALID naming the list and the position otherwise).
 *                             cov_grid[n_grid]: strictly ascending, 1 <= n_grid <= 15 (MORNA_E_INVALID naming the limit).
 *                             nq = 0 succeeds and does no work.  Only hist leaves the device.
 *   morna_jstore_recovery_by_sample  the same with the truth of list q taken from store row truth_ext[q] (an external id,
 *                             in the list or not): its lines covered at least truth_min_cov times.  An id the store lacks:
 *                             MORNA_E_RANGE naming it.
 *   morna_jstore_recovery_stats      of the last call, stats[3]: kernel ms (HIP events), algorithmic bytes (8 per entry of the
 *                             result and truth rows named, 4 per line of a CSR truth), workgroups launched.  All 0 after a
 *                             call with nq = 0 or one that failed its checks.  After a sweep (below): the sweep's.
 *
 * Several result counts from one pass.  prefixes[n_prefixes]: list lengths p_1 < ... < p_P, each in 1 .. 64,
 * 1 <= P <= 8 (MORNA_E_INVALID naming the offending value otherwise; a null pointer likewise).  hist_out is int32
 * [nq][P][2][65][n_grid + 1]; slice [q][i] is, entry for entry, what morna_jstore_recovery returns for list q cut to its first
 * min(p_i, n_results[q]) results with the same truth and grid -- so two prefixes past the end of a list give equal slices.
 * Ranks at or beyond p_P are not read by the kernel (their ids are still looked up: MORNA_E_RANGE for one the store lacks).
 * The rows are read once and one kernel is launched, whatever P.
 *   morna_jstore_recovery_sweep            the arguments and checks of morna_jstore_recovery, truth as a CSR of lines.
 *   morna_jstore_recovery_sweep_by_sample  those of morna_jstore_recovery_by_sample, truth as a store row and a minimum coverage.
 * morna_jstore_recovery_stats after a sweep: bytes = 8 per entry of the first min(p_P, n_results[q]) result rows of every
 * list, counted once, plus the truth as above; workgroups = nq x tiles.
 */
int morna_jstore_recovery(morna_jstore *s, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k,
                          const int64_t *t_ptr, const int32_t *t_line, const int64_t *cov_grid, int32_t n_grid, int32_t *hist_out);
int morna_jstore_recovery_by_sample(morna_jstore *s, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k,
                                    const int64_t *truth_ext, int64_t truth_min_cov, const int64_t *cov_grid, int32_t n_grid,
                                    int32_t *hist_out);
int morna_jstore_recovery_sweep(morna_jstore *s, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k,
                                const int64_t *t_ptr, const int32_t *t_line, const int64_t *cov_grid, int32_t n_grid,
                                const int32_t *prefixes, int32_t n_prefixes, int32_t *hist_out);
int morna_jstore_recovery_sweep_by_sample(morna_jstore *s, const int64_t *results, const int32_t *n_results, int64_t nq, int32_t k,
                                          const int64_t *truth_ext, int64_t truth_min_cov, const int64_t *cov_grid, int32_t n_grid,
                                          const int32_t *prefixes, int32_t n_prefixes, int32_t *hist_out);
int morna_jstore_recovery_stats(const morna_jstore *s, double *stats);

/*
 * ---- pooled samples: the summed coverages of groups of store rows -----------------------------------
 * Stand-in for create_supersample.py of the reference's tests/ (the "supersample" its README searches with: all samples of a
 * tissue summed junction by junction), on the store's rows in place of the intropolis text.  n_groups groups; group g holds
 * the EXTERNAL sample ids members[g_ptr[g] .. g_ptr[g + 1]), distinct inside the group, any number of them up to the store's
 * sample count (the kernel takes them in rounds of 64); an id may be in several groups.  For group g the result is every
 * line at least one member holds, ascending, with holders (int32: the members whose row holds it) and sum (int64: their
 * summed coverage).  A line is there because it is held, not because its sum is non-zero.  Integer throughout: the same
 * numbers whatever the batch, the order of the members and the order in which workgroups finish.
 *   morna_jstore_pool        checks first, all before any GPU work and with the store left usable: a null pointer, or g_ptr
 *                            that does not start at 0 or descends: MORNA_E_INVALID; an id the store lacks: MORNA_E_RANGE
 *                            naming it; an id twice in one group: MORNA_E_INVALID naming the group and the id.  n_groups = 0
 *                            returns an empty result without GPU work (members and g_ptr may then be NULL).  Two passes
 *                            over the member rows: count per tile of 4096 lines, then write.
 *   morna_jpooled_counts     count_out[n_groups]: the held lines of every group
 *   morna_jpooled_group      borrowed views of group g, valid until morna_jpooled_free: lines / sums / holders [count].
 *                            Any may be NULL.  MORNA_E_RANGE for a g outside [0, n_groups).
 *   morna_jstore_pool_stats  of the last call, stats[4]: kernel ms (HIP events, both passes), bytes read (8 per entry of every
 *                            member row, per pass), bytes written (16 per held line), workgroups per pass (n_groups x tiles).
 *                            All 0 after a call with n_groups = 0 or one that failed its checks.  The timers of retain,
 *                            nearest and recovery stay their own.
 */
typedef struct morna_jpooled morna_jpooled;
int morna_jstore_pool(morna_jstore *s, const int64_t *members, const int64_t *g_ptr, int64_t n_groups, morna_jpooled **out);
int morna_jpooled_counts(const morna_jpooled *r, int64_t *count_out /* [n_groups] */);
int morna_jpooled_group(const morna_jpooled *r, int64_t g, const int32_t **lines, const int64_t **sums, const int32_t **holders);
int morna_jpooled_free(morna_jpooled *r);
int morna_jstore_pool_stats(const morna_jstore *s, double *stats);

/*
 * ---- depth thinning: store rows with every read kept with probability keep / 2^32 -----------------------
 * A shallower sequencing of a sample is, to first order, its store row with every read kept independently with one
 * probability: binomial thinning of the coverages (the reference's tests/downsample_fastqs.py keeps a fixed number of reads of
 * the fastq instead, and needs the aligner after it).  nq jobs; job q is (ext[q], keep[q]): an EXTERNAL sample id of the store,
 * which may be named by many jobs, and a threshold in [0, 2^32].  Integers only, uint32 arithmetic modulo 2^32:
 *   fmix32(h)   h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16   (MurmurHash3's finalizer)
 *   s = fmix32(seed);  u = fmix32(lo32(ext) ^ fmix32(hi32(ext) ^ s)), ext as the two's-complement uint64 of the id
 *   v = fmix32(u ^ uint32(line))                        the key of an entry
 *   h_i = fmix32(v + 0x9e3779b9 * (i + 1)), 0 <= i < c  draw i of an entry of coverage c
 *   c' = #{ i < c : h_i < keep }                        compared in 64 bits: keep = 2^32 keeps every read, 0 none
 * The result of job q is every line of the row with c' >= 1, ascending, with c' (int32).  It depends on (seed, ext, line, c,
 * keep) alone: not on the row's place in the store, the batch, or the order workgroups finish in.  The thresholds nest:
 * keep_a <= keep_b gives c'(a) <= c'(b) entry by entry, as a subsample of a subsample.
 *   morna_jstore_thin        checks first, all before any GPU work and with the store left usable: a null pointer or a
 *                            keep above 2^32: MORNA_E_INVALID; an id the store lacks: MORNA_E_RANGE naming it; a named row
 *                            with a coverage outside [0, 2^24]: MORNA_E_INVALID naming the sample and the line (one entry's
 *                            draws are then at most 2^18 iterations of a wave).  nq = 0 returns an empty result without GPU
 *                            work (ext and keep may then be NULL).  Two passes over chunks of 2048 entries of the named rows
 *                            and a scan of the chunks' survivor counts between them.
 *   morna_jthinned_counts    count_out[nq]: the surviving lines of every job
 *   morna_jthinned_job       borrowed views of job q, valid until morna_jthinned_free: lines / cov [count].  Either may be
 *                            NULL.  MORNA_E_RANGE for a q outside [0, nq).
 *   morna_jstore_thin_stats  of the last call, stats[5]: kernel ms (HIP events: both passes and the scan); bytes read (16 per
 *                            entry of every named row: line and coverage in pass 1, line and scratch in pass 2); bytes written
 *                            (4 per entry, the scratch, and 8 per surviving line); draws made (the summed coverage of the
 *                            named rows); workgroups per pass (the chunks).  All 0 after a call with nq = 0 or one that failed
 *                            its checks.  The timers of retain, nearest, recovery and pool stay their own.
 */
typedef struct morna_jthinned morna_jthinned;
int morna_jstore_thin(morna_jstore *s, const int64_t *ext /* [nq] */, const uint64_t *keep /* [nq] */, int64_t nq, uint32_t seed,
                      morna_jthinned **out);
int morna_jthinned_counts(const morna_jthinned *r, int64_t *count_out /* [nq] */);
int morna_jthinned_job(const morna_jthinned *r, int64_t q, const int32_t **lines, const int32_t **cov);
int morna_jthinned_free(morna_jthinned *r);
int morna_jstore_thin_stats(const morna_jstore *s, double *stats);

/*
 * ---- hashed rows from store rows: an index of any width from the store ---------------------------------
 * The store holds every sample's (line, coverage) list in ascending line order, which is file order, so a sample's hashed row
 * at ANY width is a function of its store row, the weights of morna_jstore_set_weights and one int32 hash per line (the
 * murmur3 of the line's "chrom start end" key, morna_hash32 / morna_hash_keys).  After the call the items of h are exactly
 * 0 .. n - 1; item i is the hashed row, at h's dim D, of store sample ext[i] (an EXTERNAL id; the same id may be named more
 * than once).  Cell c of item i: start from S = +0.0; take every entry (j, cov) of the row in ascending j for which
 * w[j] != 0 and floormod(line_hash[j], D) == c (Python's floored modulo); for each, S = RN(S + sgn_j * RN(double(cov) * w[j])),
 * sgn_j = -1 when line_hash[j] < 0, else +1 (the sign is taken before the modulo, morna.py:370-371); the cell is S rounded
 * once to fp32.  fp64 throughout, one rounding per operation, no FMA: morna.py:376-388 followed by add_item's fp64 -> fp32.
 * cov is any int32; pad columns are 0.  The canonical norms are made as morna_build_features makes them, and everything that
 * hangs on the rows is invalidated as it invalidates it.  Nothing but ext, and line_hash when it differs from the last call's,
 * crosses PCIe.  The result depends on (row, w, line_hash, D) alone: not on the batch, the row's place in ext, or the order in
 * which workgroups finish; two calls give the same bytes.  For a file without repeated junctions, with the weights of its
 * index, the rows are the rows morna_build_features makes at that width, bit for bit.
 *   morna_add_items_from_store    checks first, all before any GPU work and with the store and the handle left usable: a null
 *                                 pointer, n_lines that is not the store's, or a handle and a store on different devices (the
 *                                 message names both): MORNA_E_INVALID; a store without weights: MORNA_E_STATE; a built index:
 *                                 MORNA_E_STATE with morna_add_items_f32's message; an id the store lacks: MORNA_E_RANGE naming
 *                                 it; n = 0: MORNA_E_EMPTY as morna_build_features; a dim past the row-width limit: what
 *                                 morna_build returns.  A workgroup per named row, its fp64 cells in LDS; the call returns when
 *                                 the rows and their norms are made.
 *   morna_jstore_hash_rows_stats  of the last call, stats[4]: kernel ms (HIP events), bytes read (8 per entry of every named
 *                                 row, plus 12 per line for hash and weight, counted once), bytes written (4 n dpad, dpad = dim
 *                                 rounded up to 256), workgroups.  All 0 after a call that failed its checks.  The timers of
 *                                 retain, nearest, recovery, pool and thin stay their own.
 *   morna_jstore_row_norms        pp_out[n]: the unhashed squared norm of store rows ext[n] (ids may repeat) under the weights
 *                                 set, the pp of the unhashed search's contract: x = RN(x + RN(v * v)), v = RN(double(cov) * w),
 *                                 over the row's entries in line order from 0.0.  Computed for the rows named, whatever the
 *                                 last search cached.  Null pointer: MORNA_E_INVALID; no weights: MORNA_E_STATE; an id the
 *                                 store lacks: MORNA_E_RANGE naming it; a negative coverage: MORNA_E_INVALID naming sample and
 *                                 line, as morna_jstore_nearest_by_sample.
 */
int morna_add_items_from_store(morna_index *h, morna_jstore *s, const int64_t *ext /* [n] */, int64_t n,
                               const int32_t *line_hash /* [n_lines] */, int64_t n_lines);
int morna_jstore_hash_rows_stats(const morna_jstore *s, double *stats /* [4] */);
int morna_jstore_row_norms(morna_jstore *s, const int64_t *ext /* [n] */, int64_t n, double *pp_out /* [n] */);

/* AnnoyIndex.get_n_items()                                     morna.py:1174 */
int64_t morna_get_n_items(const morna_index *h);
/* AnnoyIndex.get_item_vector(i)                                morna.py:702 */
int morna_get_item_vector(morna_index *h, int32_t id, float *out);
/* rows of several items at once: out[n][dim], host or device memory (query vectors of a row-sharded search) */
int morna_get_item_vectors(morna_index *h, const int32_t *ids, int64_t n, float *out);
/* whole matrix / squared norms, for tests */
int morna_get_items(morna_index *h, float *rows_out /* [n][dim] */);
int morna_get_norms2(morna_index *h, float *out /* [n] */);

/* ---- forest -------------------------------------------------------------- */

/* AnnoyIndex.build(n_trees); seed 0 selects annoy's default 123456789   morna.py:425
 * Limit that annoy does not have: two_means keeps one centroid on chip (LDS), so the build, the approximate and the
 * exact searches reject dimensions whose padded row (dim rounded up to 256 floats) exceeds 32768 floats
 * (MORNA_E_INVALID, the message names the limit).  Rows past 8192 floats take the wide two_means form.  BASELINE's
 * configurations use 3000 and 8192.
 * build may return with the forest's last narrow levels (at most n_cus / 8 split nodes) enqueued but not yet followed up:
 * whichever call touches the handle next finishes them first, and a dense batch of morna_get_nns_by_item / _by_vector /
 * _by_query_rows starts its contraction beside them.  The forest is the same either way; a failure in that part is
 * reported by the call that ran it and leaves the index unbuilt.  A caller that orders its own work on the handle's
 * stream takes the stream from morna_get_stream (or calls morna_synchronize) AFTER build.  MORNA_BUILD_TAIL=0 in the
 * environment: build returns with everything enqueued, as it always did. */
int morna_build(morna_index *h, int32_t n_trees, uint32_t seed);
int32_t morna_get_n_trees(const morna_index *h);

typedef struct {
    int64_t n_items, dim, leaf_capacity;   /* K = dim + 2 */
    int64_t n_trees, n_nodes, n_split, n_leaves, max_depth;
    int64_t split_attempts;                /* create_split calls (incl. rejected) */
    int64_t split_rows;                    /* sum of |node| over those calls      */
    int64_t fallback_nodes;                /* nodes randomised (imbalance > 0.99) */
} morna_forest_stats;
int morna_get_forest_stats(const morna_index *h, morna_forest_stats *out);
/*
 * Forest dump for structural tests.  node_rec[n_nodes][6] =
 * {kind (0 split, 1 leaf), tree, start, count, child0, child1}; perm[n_trees][n_items];
 * hyperplanes[n_split][dim] in the order given by hp_node[n_split] (node id).
 * Any output pointer may be NULL.
 */
int morna_get_forest(morna_index *h, int32_t *node_rec, int32_t *perm, float *hyperplanes, int32_t *hp_node);
/*
 * For tests and probes: item_at[n_items], the item each row of the split contraction stood for in the last build, from its
 * second level on ("the order of the rows").  MORNA_E_STATE when that build did not order its rows (fewer than
 * 8192 items, MORNA_SPLIT_ORDER=0, no level in the matrix-core form) or the index is not built.  Not part of the search.
 */
int morna_debug_split_order(morna_index *h, int32_t *item_at);

/* ---- search -------------------------------------------------------------- */

/*
 * AnnoyIndex.get_nns_by_vector(v, n, search_k, include_distances)  morna.py:651, 659
 * batched over nq queries; q[nq][dim] fp32.  search_k = -1 -> k * n_trees.
 * ids_out[nq][k] (-1 padded), dist_out[nq][k] (may be NULL), count_out[nq] (may be NULL).
 * q may also point to memory of the handle's device (the row-sharded search hands over the
 * all-gathered query rows without a trip through the host); the outputs are host memory.
 */
int morna_get_nns_by_vector(morna_index *h, const float *q, int64_t nq, int32_t k, int32_t search_k,
                            int32_t *ids_out, float *dist_out, int32_t *count_out);
/* AnnoyIndex.get_nns_by_item(i, n, search_k, include_distances)    morna.py:762, 769, 1191 */
int morna_get_nns_by_item(morna_index *h, const int32_t *items, int64_t nq, int32_t k, int32_t search_k,
                          int32_t *ids_out, float *dist_out, int32_t *count_out);
/*
 * MornaSearch.exact_search_nn + cosine_distance                   morna.py:681-716, 101-114
 * q[nq][dim] fp64 (the un-rounded query_sample); distances fp64, accumulated in
 * the reference's sequential order; ties resolved as bisect_left does.
 * count_out[q] = -1: the reference RAISES for this query -- some indexed row is so nearly parallel to it that
 * cosine_distance's radicand rounds below zero and math.sqrt fails (morna.py:101-114); the reference evaluates every row
 * (morna.py:697-700), so the whole query fails whatever that row's rank would have been.  The lists of such a query are
 * filled in for diagnosis only; a caller must test the count before it slices by it.
 * Domain: the answer is the reference's, bit for bit, for every fp32 stored row (any scale: subnormal, zero, with an
 * fp32 norm that underflows or overflows, or with NaN / inf elements) and every fp64 query whose elements and sequential
 * sum of squares are finite, for every k and on every path (this call, by item, sharded, packed).  A query whose fp64 sum
 * of squares lies outside [2^-900, 2^890] -- where the reference's own pp * qq can leave fp64's normal range -- is compared
 * with every row, as the reference does (slower: every row is re-ranked).  A host query with a NaN / inf element or an
 * infinite sum of squares gets MORNA_E_INVALID (the same on every rank of a sharded search: the queries are the same);
 * fp32 queries in device memory (morna_exact_search_packed) are not checked: one with a non-finite element is compared
 * with every row.
 */
int morna_exact_search(morna_index *h, const double *q, int64_t nq, int32_t k,
                       int32_t *ids_out, double *dist_out, int32_t *count_out);
/*
 * The same with STORED rows as the queries (every item of the index against the index: BASELINE configs[4]): the query
 * is the item's fp32 row widened to fp64 on the device -- what exact_search_nn sees when query_sample came out of
 * get_item_vector (morna.py:697-703) -- so nothing but the item numbers crosses PCIe.  The queries are processed in
 * batches inside the call (scan values of a batch: at most 2 GiB).
 */
int morna_exact_search_by_item(morna_index *h, const int32_t *items, int64_t nq, int32_t k,
                               int32_t *ids_out, double *dist_out, int32_t *count_out);

/*
 * Restricted search (no counterpart in the reference): sample allow-lists and leave-out groups.
 * A restriction on an index of n items has two optional parts: an allow bitmap (bit i of allow_bits[i / 32]; NULL: every
 * item is allowed; the bits past n_items in the last word are ignored) and a group label per item (item_group[i], negative:
 * none; NULL: no item has one).  Every query q of a restricted call carries g_q (q_group[q], negative or q_group NULL:
 * none).  Item i is ELIGIBLE for q iff allow[i] holds and (g_q < 0 or item_group[i] != g_q); call that set E(q).
 *   Exact: the answer for q is what morna_exact_search returns on an index that holds exactly the rows of E(q) in
 *     ascending id order, ids mapped back: same ids, bit-identical fp64 distances, same tie order (equal distance: higher
 *     id first), a short count when |E(q)| < k, and count -1 only when an ELIGIBLE row makes the reference's math.sqrt
 *     raise (a near-parallel row that is not eligible does not fail the query).
 *   Approximate: the traversal is the unrestricted one -- same pops, same search_k accounting, ids that are duplicates
 *     or not eligible included -- and the candidate set is the unrestricted one intersected with E(q); the answer is its k
 *     nearest by the same distances and tie order.  It equals the unrestricted answer with k = n_items, filtered to E(q)
 *     and cut to k.  search_k = -1 is k * n_trees as everywhere: a caller with a small allow-list passes a larger one
 *     (morna_amd.search scales its default by n / n_allowed).
 * The bitmap and the labels are copied to the handle's device and live with the restriction object.  It is bound to the
 * handle and to the handle's n_items at creation: a search after the item count changed returns MORNA_E_STATE, with
 * another handle MORNA_E_INVALID.  Free it before the handle is destroyed.
 * Query sources: q ([nq][dim], fp32 for the approximate search, fp64 for the exact one), or items ([nq] stored rows), or
 * both NULL: the staged query rows of morna_build_query_rows (nq must be their count).
 * r == NULL is MORNA_E_INVALID here, never a silent unrestricted search; so is q_group with a restriction made without
 * item_group.  Outputs as morna_get_nns_by_vector / morna_exact_search.  Not available on the row-sharded paths.
 * morna_restriction_counts: counts[0..2] = n_items, allowed items, items with a label >= 0.
 */
typedef struct morna_restriction morna_restriction;
int morna_restriction_create(morna_index *h, const uint32_t *allow_bits /* [(n_items+31)/32] or NULL */,
                             const int32_t *item_group /* [n_items] or NULL */, morna_restriction **out);
int morna_restriction_counts(const morna_restriction *r, int64_t *counts /* n_items, n_allowed, n_grouped */);
int morna_restriction_free(morna_restriction *r);
int morna_get_nns_restricted(morna_index *h, const morna_restriction *r, const float *q, const int32_t *items, int64_t nq,
                             const int32_t *q_group /* [nq] or NULL */, int32_t k, int32_t search_k,
                             int32_t *ids, float *dist, int32_t *count);
int morna_exact_search_restricted(morna_index *h, const morna_restriction *r, const double *q, const int32_t *items, int64_t nq,
                                  const int32_t *q_group, int32_t k, int32_t *ids, double *dist, int32_t *count);

/*
 * ---- label distance sums (no counterpart in the reference, whose README reads them off `search -m` output by
 * eye) ---------------------------------------------------------------------------------------------------------------------
 * For every query q and every label g, the sum of the angular distances from q to the items that carry g, from ONE scan.
 *   item_label[n_items]: the label of every item, in [-1, n_labels); -1: none.  1 <= n_labels <= MORNA_LABELS_MAX.
 *   Queries: q ([nq][dim] fp64), or items ([nq] stored rows), or both NULL: the staged query rows of morna_build_query_rows
 *     (nq must be their count; with none staged there is no query source: MORNA_E_INVALID).  q and items: MORNA_E_INVALID.
 *   r: a restriction, or NULL for none.  q_group as in the restricted search; q_group without a restriction that holds the
 *     items' groups is MORNA_E_INVALID.  E(q) is the eligible set defined above, every item when r is NULL.
 *   v(q, i): the fp32 value the exact search's scan has for (q, i) -- the MFMA scan for a batch of 32 queries or more, the
 *     vector scan below, the choice morna_exact_search makes -- 2 - 2cos, 2 where the product of the squared norms is not
 *     positive, within stats[5] of the true value.  d = sqrt((double) max(v, 0.0f)) in fp64, D = (uint64)(d * 2^32 + 0.5).
 *   Item i is COUNTED for (q, g) iff item_label[i] == g, i is in E(q), and -- for queries given as items -- i != items[q].
 *   sums_out[q][g] = the sum of D(q, i) over the counted items (fixed point, 32 fractional bits; D < 2^33, so no sum of fewer
 *     than 2^29 terms passes 2^62); counts_out[q][g] = their number.  Integer sums: the result does not depend on the order
 *     of summation, the grid or the batch; two calls give the same bytes.
 *   Domain: an index that holds a row outside the scan's domain (a non-zero row whose fp32 squared norm is below dim' 2^-96,
 *     dim' = dim rounded up to 256, above 2^126 or not finite) is refused, MORNA_E_INVALID naming the first such row.  A
 *     zero row, a zero query and a query whose fp64 sum of squares lies outside [2^-900, 2^890] are inside: every v is 2.
 *     A host query with a non-finite element or sum of squares: MORNA_E_INVALID, as morna_exact_search.
 *   Errors: MORNA_E_INVALID naming the offender for a label outside [-1, n_labels) and for n_labels outside the limits; an
 *     item outside the index: MORNA_E_RANGE; the restriction's state errors as in the restricted search; a row-sharded
 *     handle (morna_comm_init): MORNA_E_INVALID.
 *   morna_label_sums_stats  of the last call, stats[6]: scan ms (staging and scan kernels, HIP events), sums-kernel ms,
 *     queries, batches (scan values of a batch: at most 2 GiB), items counted (the sum of counts_out), the scan's error
 *     bound used (the largest over the batches).  All 0 after a call that failed or had nq = 0.
 */
#define MORNA_LABELS_MAX 4096
int morna_label_sums(morna_index *h, const morna_restriction *r /* or NULL: unrestricted */, const double *q,
                     const int32_t *items, int64_t nq, const int32_t *q_group /* [nq] or NULL */,
                     const int32_t *item_label /* [n_items] */, int32_t n_labels, uint64_t *sums_out /* [nq][n_labels] */,
                     int32_t *counts_out /* [nq][n_labels] */);
int morna_label_sums_stats(const morna_index *h, double *stats /* [6] */);

/*
 * ---- radius search (no counterpart in the reference, which only answers "the k nearest") -------------
 * Every item within the distance `radius` of a query.  The distance is the one morna_exact_search returns: sqrt(2 - 2cos) in
 * fp64, accumulated in the reference's sequential order (cosine_distance, morna.py:101-114).
 *   The answer for query q and radius r (fp64, finite, 0 <= r): the list morna_exact_search returns for q with k = n_items,
 *     cut after the last entry whose distance is <= r, compared in fp64, inclusive: the same ids, bit-identical distances,
 *     the same tie order (equal distance: higher id first).  r >= 2 returns every evaluated row.  r < 0, NaN or inf:
 *     MORNA_E_INVALID.
 *   count -1: some evaluated row gives a NaN distance, i.e. the reference raises for q.  Such a row has a scan value of
 *     about 0 and is a candidate for every r >= 0.  The list is still filled, for diagnosis: NaN entries last, by ascending id.
 *   r (the restriction) may be NULL: every item is eligible.  Else the answer is taken on the eligible set E(q) of the
 *     restricted search; q_group as there (q_group without a restriction that holds the items' groups: MORNA_E_INVALID).
 *   after ([nq] or NULL): only items with id > after[q].  Neither ineligible items nor items at or below the bound are
 *     evaluated: a near-parallel row among them does not fail the query.
 *   Pairs: every unordered pair {i, j} of stored rows with d(i, j) <= r is the search by item over all items with
 *     after[q] = items[q].  d is symmetric bit for bit (pq and pp qq are sums and products of the same terms in the same
 *     order either way).  A pair whose fp64 radicand is negative has the distance NaN and belongs to the result for every r;
 *     its query has count -1.  (The reference would raise for the whole query; a caller that looks for duplicates must not
 *     lose exactly these.)
 *   Queries: q ([nq][dim] fp64), or items ([nq] stored rows), or both NULL: the staged query rows of morna_build_query_rows
 *     (nq must be their count).  q and items: MORNA_E_INVALID.
 *   Domain, as morna_exact_search: rows outside the scan's domain are candidates of every query and get the reference's
 *     value; a query whose fp64 sum of squares lies outside [2^-900, 2^890] is compared with every row; a host query with a
 *     non-finite element or sum of squares: MORNA_E_INVALID; a row-sharded handle (morna_comm_init): MORNA_E_INVALID.
 *   Window: a row is a candidate iff its fp32 scan value v <= fl_up((float)(r * r)) + the scan's error bound (stats[7]); every
 *     candidate is then evaluated in fp64.  Queries are taken in batches (scan values of a batch: at most 2 GiB;
 *     MORNA_RADIUS_BATCH=<queries> in the environment caps a batch further).  The answer does not depend on the batch, the
 *     grid or which scan ran.  More than 2^31 - 1 result entries in one call: MORNA_E_INVALID naming the total.
 *   morna_radius_counts  count_out[nq]: the length of every list, or -1
 *   morna_radius_query   borrowed views of list q, valid until morna_radius_free: ids[len], dist[len], ordered (len is the
 *                        list's length also where the count is -1).  The lists lie one after the other in query order:
 *                        list q + 1 begins where list q ends, in both arrays
 *   morna_exact_radius_stats  of the last call, stats[8]: scan ms (staging and scan kernels, HIP events), selection ms (count,
 *     offsets and write kernels), distance ms (the fp64 pass and the ordering on the device), queries, batches, candidates
 *     (fp64 chains run), result entries, the window used (the largest over the batches).  All 0 after a call that failed.
 */
typedef struct morna_radius morna_radius;
int morna_exact_radius(morna_index *h, const morna_restriction *r /* or NULL */, const double *q, const int32_t *items,
                       int64_t nq, const int32_t *q_group /* [nq] or NULL */, const int32_t *after /* [nq] or NULL */,
                       double radius, morna_radius **out);
int morna_radius_counts(const morna_radius *r, int64_t *count_out /* [nq] */);
int morna_radius_query(const morna_radius *r, int64_t q, const int32_t **ids, const double **dist, int64_t *len);
int morna_radius_free(morna_radius *r);
int morna_exact_radius_stats(const morna_index *h, double *stats /* [8] */);

/*
 * ---- spherical k-means (no counterpart in the reference, whose grouping tables come from outside) ------
 * A partition of the stored rows into k groups by angular distance, bit-reproducible against a CPU restatement.
 *   Rows: the handle's stored fp32 rows x_i.  The eligible set E: every row, or the allowed rows of a restriction r that holds
 *     an allow-list only (a restriction that holds groups: MORNA_E_INVALID).  A row-sharded handle: MORNA_E_INVALID.
 *   Distance: d(i, c) = cosine_distance(x_i, c) of the reference (morna.py:101-114) with c an fp64 vector, accumulated in its
 *     sequential order, sqrt(2 - 2cos), 2 under the root where the product of the sums of squares is not positive; NaN where
 *     math.sqrt would raise, returned as the canonical quiet NaN (0x7ff8000000000000).
 *   Assignment: a_i = the j that minimises d(i, c_j) in fp64.  A NaN orders behind every number; ties, all-NaN included, go
 *     to the lowest j.  A row outside E gets a_i = -1 and the distance -1.0.
 *   Update: pp_i = the sequential fp64 sum of squares of row i in cosine_distance's order, s_i = 1.0 / sqrt(pp_i) (a correctly
 *     rounded sqrt, then one division).  Member i of cluster j is skipped iff not (pp_i > 0 and pp_i < inf); it stays
 *     assigned.  c_j[z] = the sum of (double) x_i[z] * s_i over the unskipped members in ascending item id, from 0.0, one
 *     rounding per multiply and one per add, no fused multiply-add, no division by the count (d does not depend on the scale
 *     of c).  A cluster without an unskipped member keeps its centroid.
 *   Loop (morna_kmeans): c0_j = the widened row of seed_items[j]; the seeds are distinct (MORNA_E_INVALID), in range
 *     (MORNA_E_RANGE) and eligible (MORNA_E_INVALID).  For t = 1 .. max_iter (>= 1): a(t) = assign(c(t-1)); if t > 1 and
 *     a(t) == a(t-1), stop as converged; otherwise c(t) = update(a(t)).  Returned: the last a(t) in assign_out[n_items], its
 *     distances to the c(t-1) it was made against in dist_out[n_items], those centroids in centroids_out[k][dim], the
 *     clusters' sizes in sizes_out[k] (skipped members included), info_out[0] = t, info_out[1] = converged (0 or 1).
 *     dist_out, centroids_out and sizes_out may be NULL.
 *   morna_kmeans_assign: one assignment against k fp64 centroids in host memory.  A centroid with a non-finite element or
 *     sum of squares: MORNA_E_INVALID, as morna_exact_search.  dist_out may be NULL.
 *   Limits: 1 <= k <= min(MORNA_LABELS_MAX, |E|), so that every output can feed morna_label_sums (morna_kmeans_assign, whose
 *     centroids are given and not drawn from E: 1 <= k <= MORNA_LABELS_MAX); k * n_items <= 2^29 (the scan values of all
 *     centroids share one batch of at most 2 GiB).  Beyond either: MORNA_E_INVALID naming the limit.  An
 *     empty index: MORNA_E_EMPTY.
 *   The result does not depend on the grid, the batch, which scan ran or the order of any launch: the fp32 scan only chooses
 *     which (row, centroid) pairs are evaluated in fp64 (the window is derived at kmeans_window, csrc/exact.hip), member lists
 *     are placed by counting, and every sum runs in ascending item id.
 *   morna_kmeans_stats  of the last call, stats[8]: ms of the scan (staging and scan kernels), of the pick (pick, offsets and
 *     list kernels), of the resolve (the fp64 chains and the minimum) and of the update (member lists and sums), HIP events,
 *     summed over the iterations; open rows (rows with more than one centroid inside the window, summed over the iterations);
 *     fp64 chains run (summed); iterations; the largest cluster of the last iteration (0 for morna_kmeans_assign).  All 0
 *     after a call that failed.
 */
int morna_kmeans(morna_index *h, const morna_restriction *r /* or NULL */, const int32_t *seed_items /* [k] */, int32_t k,
                 int32_t max_iter, int32_t *assign_out /* [n_items] */, double *dist_out /* [n_items] or NULL */,
                 double *centroids_out /* [k][dim] or NULL */, int32_t *sizes_out /* [k] or NULL */, int32_t *info_out /* [2] */);
int morna_kmeans_assign(morna_index *h, const morna_restriction *r /* or NULL */, const double *centroids /* [k][dim] */, int32_t k,
                        int32_t *assign_out /* [n_items] */, double *dist_out /* [n_items] or NULL */);
int morna_kmeans_stats(const morna_index *h, double *stats /* [8] */);

/*
 * ---- label mixture (no counterpart in the reference, whose README only names the question: "may uncover
 * significant contamination") ----------------------------------------------------------------------------------------------
 * Every query as a non-negative combination of the label centroids: a non-negative least squares fit on the unit sphere,
 * bit-reproducible against a CPU restatement.
 *   Arithmetic: fp64, one rounding per operation, no fused multiply-add; every sum starts from 0.0 and runs in ascending index.
 *   item_label[n_items] in [-1, n_labels); 1 <= n_labels <= MORNA_MIXTURE_LABELS_MAX (the normalised Gram matrix, 128 KiB at the
 *     limit, stays in the 160 KiB of LDS).  r: a restriction that holds an allow-list only, or NULL (one that holds groups:
 *     MORNA_E_INVALID, as morna_kmeans); E: the eligible rows.  Queries as in morna_label_sums: q ([nq][dim] fp64), or items, or
 *     both NULL for the staged query rows.  tol finite and >= 0; max_sweeps >= 1.
 *   Centroid sums: pp_i and sigma_i = s_i exactly as morna_kmeans defines them; a member with not (0 < pp_i < inf) is skipped.
 *     s_l[z] = morna_kmeans' update over the members {i in E : item_label[i] = l} (the zero vector without an unskipped
 *     member); m_l = the unskipped members of l.
 *   Gram: S_lm = sum_z s_l[z] * s_m[z] for l <= m, S_ml := S_lm.
 *   Per query y (by item: the widened stored row): yy = sum_z y[z]^2, t_l = sum_z s_l[z] * y[z].
 *   Own label left out: a by-item query i that is in E, unskipped, with o = item_label[i] >= 0 has tau_m = t_m * sigma_i,
 *     S'_om = S'_mo = S_om - tau_m (m != o), S'_oo = (S_oo - 2.0 * tau_o) + 1.0, t'_o = t_o - pp_i * sigma_i (pp_i is the
 *     query's yy: the same sum), m'_o = m_o - 1; everything else unchanged.  This is the centroid without the query's own unit
 *     row, obtained algebraically: no centroid is rebuilt per query.
 *   Active labels: l is active iff m'_l >= 1 and 0 < S'_ll < inf.  d_l = sqrt(S'_ll) correctly rounded,
 *     G_lm = S'_lm / (d_l * d_m) for l != m, G_ll := 1.0, b_l = t'_l / (d_l * sqrt(yy)).  A query with not (0 < yy < inf) or
 *     without an active label: all weights 0, info = 0, 0, 0, -1.  A host query with a non-finite element or sum of squares:
 *     MORNA_E_INVALID, as morna_exact_search.
 *   Solver, cyclic coordinate descent on the active labels: a = 0, g = b.  In sweep s = 1 .. max_sweeps: mx = 0; for every
 *     active l ascending: delta = g_l; if delta < -a_l, delta = -a_l; if delta != 0: a_l = a_l + delta and, for every active m,
 *     g_m = g_m - delta * G_ml; mx = max(mx, |delta|).  After a sweep with mx <= tol: stop, status 1.  After max_sweeps sweeps
 *     without that: status 0.  No step sums across labels, so the answer cannot depend on the wave, the grid or the batch.
 *   Report, sums over the active labels ascending: h_l = sum_m G_lm * a_m, w_l = b_l - h_l, kkt = the largest of |w_l| where
 *     a_l > 0 and max(w_l, 0) where a_l = 0 (the Karush-Kuhn-Tucker conditions), u = sum_l a_l * h_l, v = sum_l a_l * b_l,
 *     rr = (1.0 - 2.0 * v) + u: the squared distance from the unit query to its blend.
 *   Outputs: weights_out[nq][n_labels] (0.0 for an inactive label), info_out[nq][4] = rr, kkt, sweeps, status,
 *     active_out[nq][n_labels] bytes (may be NULL).
 *   morna_label_centroids: s, m and S alone (sums_out[L][dim], counts_out[L], gram_out[L][L] or NULL).
 *   Errors: a row-sharded handle: MORNA_E_INVALID; an empty index: MORNA_E_EMPTY; a label outside [-1, n_labels), tol,
 *     max_sweeps or n_labels outside their limits: MORNA_E_INVALID naming the offender; an item outside the index: MORNA_E_RANGE.
 *   morna_mixture_stats  of the last call, stats[8]: ms of the centroid step (member lists and sums), of the Gram (transpose,
 *     Gram and normalisation), of the query dots (staging and dots), of the solver, HIP events; queries; sweeps summed; the
 *     largest sweep count; queries with status != 1.  All 0 after a call that failed.
 */
#define MORNA_MIXTURE_LABELS_MAX 128
int morna_label_centroids(morna_index *h, const morna_restriction *r /* or NULL */, const int32_t *item_label /* [n_items] */,
                          int32_t n_labels, double *sums_out /* [n_labels][dim] */, int32_t *counts_out /* [n_labels] */,
                          double *gram_out /* [n_labels][n_labels] or NULL */);
int morna_mixture(morna_index *h, const morna_restriction *r /* or NULL */, const double *q, const int32_t *items, int64_t nq,
                  const int32_t *item_label /* [n_items] */, int32_t n_labels, double tol, int32_t max_sweeps,
                  double *weights_out /* [nq][n_labels] */, double *info_out /* [nq][4] */,
                  uint8_t *active_out /* [nq][n_labels] or NULL */);
int morna_mixture_stats(const morna_index *h, double *stats /* [8] */);

/*
 * ---- principal axes (no counterpart in the reference, whose README asks whether "a sample's global
 * expression patterns are similar to those of samples from the same tissue") ------------------------------------------------
 * The leading principal axes of the unit-scaled stored rows by a deterministic block power iteration, and the coordinates of
 * any row or query on them, bit-reproducible against a CPU restatement (tests/pca_ref.py).
 *   Arithmetic: fp64, one rounding per operation (+, -, *, /, sqrt correctly rounded), no fused multiply-add.
 *   BS, the blocked ascending sum, is the one summation rule of this contract.  BS of terms t_0 .. t_{n-1}: for every block
 *     B = 0, 1, .. of 256 consecutive indices [256 B, 256 B + 256), P_B = the terms of the block added one by one in ascending
 *     index to 0.0; BS = the P_B added one by one in ascending B to 0.0.  The index is the column z for a sum over columns and
 *     the item id i for a sum over rows.  A row that is left out of a sum over rows adds no term to its block and moves no
 *     block edge; a block without a term has P_B = 0.0 and is still added.
 *   Rows: pp_i, s_i and the skip rule not (0 < pp_i < inf) exactly as morna_kmeans defines them.  u_i[z] = (double) x_i[z] * s_i.
 *     The fitted set F: the rows that are eligible and not skipped; eligible is every row, or the allowed rows of a
 *     restriction r that holds an allow-list only (one that holds groups: MORNA_E_INVALID).  m = |F|; m < 2: MORNA_E_INVALID.
 *   Mean: mu[z] = BS_{i in F}(u_i[z]) / (double) m with center != 0; with center == 0, mu[z] = 0.0 and every formula below is
 *     used unchanged.
 *   Widths: p components, 1 <= p <= MORNA_PCA_MAX_COMPONENTS; extra >= 0; b = p + extra columns are iterated,
 *     b <= MORNA_PCA_MAX_BLOCK and b <= min(dim, m - 1).  Beyond either: MORNA_E_INVALID naming the limit.
 *   Start: G[z][j] = (double) (mix(seed * 0x9E3779B97F4A7C15 + 64 z + j) >> 11) * 2^-53 - 0.5 for z < dim, j < b, in
 *     unsigned 64-bit arithmetic modulo 2^64; mix(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 *     x *= 0x94D049BB133111EB; x ^= x >> 31.  Q = Orth(G).
 *   Orth(A), A[dim][b] -> Q[dim][b], columns j = 0 .. b - 1 in turn, a = column j of A: twice { r_k = BS_z(q_k[z] * a[z]) for
 *     every k < j, all from the same a; then for k = 0 .. j - 1 in turn and every z, a[z] = a[z] - r_k * q_k[z] }.  Then
 *     nn = BS_z(a[z] * a[z]); not (0 < nn < inf) ends the call with MORNA_E_INVALID naming column j ("fewer than b independent
 *     directions"); otherwise q_j[z] = a[z] / sqrt(nn) (one sqrt, then one division per element).
 *   Iteration t = 1 .. max_iter (>= 1):
 *     c_j = BS_z(mu[z] * Q[z][j]);  T[i][j] = BS_z(u_i[z] * Q[z][j]) - c_j for i in F;  S_j = BS_{i in F}(T[i][j]);
 *     Y[z][j] = BS_{i in F}(u_i[z] * T[i][j]);  Z[z][j] = (Y[z][j] - mu[z] * S_j) / (double) m;
 *     B_jk = BS_z(Q[z][j] * Z[z][k]) for j <= k, B_kj := B_jk.
 *     theta, W = Eig(B) (below).
 *     If t >= 2 and max over j < p of |theta_j(t) - theta_j(t-1)| <= tol * theta_0(t): stop, converged.
 *     If t == max_iter: stop, not converged.  Otherwise Q = Orth(M), M[z][j] = the sum over k = 0 .. b - 1 ascending, from 0.0,
 *     of Z[z][k] * W[k][j].
 *   Eig(B), cyclic Jacobi by rows on a copy A of B with W = the identity: a sweep visits the pairs (p, q), p = 0 .. b - 2,
 *     q = p + 1 .. b - 1, in that order.  A pair with A[p][q] == 0.0 or |A[p][q]| <= 2^-54 * (|A[p][p]| + |A[q][q]|) is passed
 *     over.  Otherwise tau = (A[q][q] - A[p][p]) / (2.0 * A[p][q]); t = 1.0 / (|tau| + sqrt(1.0 + tau * tau)), negated when
 *     tau < 0; c = 1.0 / sqrt(1.0 + t * t); s = t * c.  Columns first: for every k = 0 .. b - 1, with x = A[k][p] and
 *     y = A[k][q]: A[k][p] = c * x - s * y, A[k][q] = s * x + c * y.  Then rows: for every k, with x = A[p][k] and y = A[q][k]:
 *     A[p][k] = c * x - s * y, A[q][k] = s * x + c * y.  Then A[p][q] = A[q][p] = 0.0.  W takes the column step alone
 *     (x = W[k][p], y = W[k][q]).  The sweeps end after the first sweep that rotated nothing, or after 64 sweeps.
 *     theta_j = A[j][j] ordered descending, equal values in ascending j; the columns of W are ordered with them.
 *   Result, at the iteration that stopped: V[z][j] = the sum over k ascending, from 0.0, of Q[z][k] * W[k][j], j < p; axis j is
 *     negated when its element of largest magnitude (the lowest z among equals) is negative.  axes_out[p][dim] = V transposed,
 *     mean_out[dim] = mu, values_out[p] = theta_j, info_out[4] = iterations t, converged (0.0 or 1.0), m,
 *     tv = BS_{i in F}(BS_z((u_i[z] - mu[z]) * (u_i[z] - mu[z]))) / (double) m, the total variance.
 *   tol finite and >= 0.  A non-finite theta: MORNA_E_INVALID.
 *   morna_pca_project: queries as in morna_label_sums (q [nq][dim] fp64 in host memory, or items, or both NULL for the staged
 *     query rows).  For a query y: pp = the sequential sum of squares in cosine_distance's order, s = 1.0 / sqrt(pp),
 *     u[z] = y[z] * s (by item, y = the widened stored row, so u = u_i);
 *     coords_out[q][j] = BS_z(u[z] * axes[j][z]) - BS_z(mean[z] * axes[j][z]).  A query with not (0 < pp < inf): the canonical
 *     quiet NaN (0x7ff8000000000000) in every coordinate.  A restriction plays no part: every row can be placed.  A host query
 *     with a non-finite element or sum of squares: MORNA_E_INVALID, as morna_exact_search; a non-finite element of axes or
 *     mean: MORNA_E_INVALID; 1 <= p <= MORNA_PCA_MAX_COMPONENTS; an item outside the index: MORNA_E_RANGE.
 *   Errors of both: a row-sharded handle: MORNA_E_INVALID; an empty index: MORNA_E_EMPTY.
 *   Nothing depends on the grid, the wave or the batch: every BS is evaluated as its definition reads, partial by partial,
 *     and no atomic is used.
 *   morna_pca_stats  of the last morna_pca, stats[8]: ms of the T passes, of the Y passes (S and Z with them), of the
 *     orthonormalisations (the start's included), of the small products (c, B, Z W, Q W), HIP events, summed over the
 *     iterations; ms of Eig on the host; iterations; rows fitted m; bytes of rows read, 4 dim (n_items + m (2 + 2 iterations)):
 *     the scales, the mean and the total variance once, T and Y per iteration.  All 0 after a call that failed.
 */
#define MORNA_PCA_MAX_COMPONENTS 32
#define MORNA_PCA_MAX_BLOCK 64
int morna_pca(morna_index *h, const morna_restriction *r /* or NULL */, int32_t p, int32_t extra, int32_t center, uint64_t seed,
              double tol, int32_t max_iter, double *axes_out /* [p][dim] */, double *mean_out /* [dim] */,
              double *values_out /* [p] */, double *info_out /* [4] */);
int morna_pca_project(morna_index *h, const double *axes /* [p][dim] */, const double *mean /* [dim] */, int32_t p, const double *q,
                      const int32_t *items, int64_t nq, double *coords_out /* [nq][p] */);
int morna_pca_stats(const morna_index *h, double *stats /* [8] */);

/*
 * ---- tree-prefix search and the (tree count, search_k) sweep (no counterpart in the reference, whose
 * tests/README.md experiment 3 builds one index per tree count and compares result files by eye) -------------------------
 * Tree i of a forest does not depend on the number of trees built with it, and node ids keep their relative order when the
 * forest is cut to its first t trees; so the searches below answer, from ONE built index, what an index built with
 * n_trees = t on the same rows and seed would answer: the same ids, fp32 distance bytes and counts.
 *   morna_get_nns_prefix  morna_get_nns_by_vector / _by_item / _by_query_rows (q, or items, or both NULL: the staged
 *       query rows, as below; q and items together: MORNA_E_INVALID) over the first n_trees_used trees.  search_k = -1 is k * n_trees_used.  n_trees_used = the forest's tree
 *       count is the plain call.  n_trees_used < 1 or above the forest's: MORNA_E_RANGE naming both numbers.  An index
 *       that is not built: MORNA_E_STATE.
 *   morna_search_sweep    every cell of trees[n_t] x search_ks[n_s] at once.  Both lists strictly ascending and positive,
 *       1 <= n_t, n_s <= 64 (MORNA_E_INVALID naming the entry or the limit; -1 is not accepted in search_ks: the caller
 *       writes k * t itself), trees[n_t - 1] at most the forest's tree count (MORNA_E_RANGE naming both numbers).
 *       Outputs, host memory, each may be NULL and is then not copied: ids_out / dist_out [n_t][n_s][nq][k], count_out /
 *       ncand_out / ndots_out [n_t][n_s][nq].  Cell (i, j, q) equals morna_get_nns_prefix with n_trees_used = trees[i] and
 *       search_k = search_ks[j] for query q in ids, distance bytes and count; ncand is that call's number of unique
 *       candidates, ndots its number of hyperplane dots, the trees[i] root dots included (0 of them when the roots are
 *       leaves).  The work: the queries are staged and the root margins taken once per batch, one descent runs per
 *       (query, tree count) to the largest search_k and records where every smaller one stops, every candidate of the
 *       deepest lists gets its canonical dot once, and each cell ranks a prefix of those keys.  A batch that
 *       morna_get_nns_by_* would send through the whole-batch fp16 contraction gets that contraction, once: the canonical
 *       dots are then taken only for the candidates that the fp16 filter of some cell lets through.
 *   morna_recall_sweep    the sweep beside ONE exact search of the same queries (morna_exact_search of the fp32 queries
 *       widened to fp64, or morna_exact_search_by_item), 1 <= k <= MORNA_RECALL_MAX_K (MORNA_E_INVALID naming the limit).
 *       hits_out [n_t][n_s][nq] (required) = the number of ids cell (i, j, q) shares with the exact answer of q, counted on
 *       the device; -1 in every cell of a query whose exact count is -1 (morna_exact_search).  exact_count_out [nq],
 *       exact_ids_out [nq][k] and the sweep's outputs may each be NULL.
 *   Query sources of the prefix call and the two sweeps: q ([nq][dim] fp32), or items ([nq] stored rows), or both NULL: the staged query rows
 *       of morna_build_query_rows (nq must be their count; the exact search then takes their fp64 rows, as
 *       morna_exact_search_query_rows does).  q and items together: MORNA_E_INVALID.
 *   morna_search_sweep_stats  of the last sweep or recall sweep, stats[4]: descents run (queries x tree counts), cells
 *       answered, rows read by canonical candidate dots, whether the whole-batch fp16 contraction ran (0 or 1).  All 0
 *       after a call with nq = 0 or one that failed its checks.
 */
#define MORNA_SWEEP_MAX_LIST 64
#define MORNA_RECALL_MAX_K 256
int morna_get_nns_prefix(morna_index *h, const float *q, const int32_t *items, int64_t nq, int32_t k, int32_t search_k,
                         int32_t n_trees_used, int32_t *ids, float *dist, int32_t *count);
int morna_search_sweep(morna_index *h, const float *q, const int32_t *items, int64_t nq, int32_t k, const int32_t *trees,
                       int32_t n_t, const int32_t *search_ks, int32_t n_s, int32_t *ids_out, float *dist_out, int32_t *count_out,
                       int32_t *ncand_out, int32_t *ndots_out);
int morna_recall_sweep(morna_index *h, const float *q, const int32_t *items, int64_t nq, int32_t k, const int32_t *trees,
                       int32_t n_t, const int32_t *search_ks, int32_t n_s, int32_t *hits_out, int32_t *exact_count_out,
                       int32_t *ncand_out, int32_t *ndots_out, int32_t *ids_out, float *dist_out, int32_t *count_out,
                       int32_t *exact_ids_out);
int morna_search_sweep_stats(const morna_index *h, double *stats);

/*
 * Row-sharded search (one handle per GPU; the reference has no such path): merge of the
 * per-shard answers to the same queries after their all-gather.  ids / dist: [world][nq][kk], each
 * [kk] list as get_nns_* returns it -- ascending (distance, id), empty slots id -1 last -- with ids
 * already global.  Writes the k smallest (distance, id) pairs per query; out slots past the
 * count are id -1 / distance +inf.  Host memory, no GPU work.
 */
int morna_merge_topk(const int64_t *ids, const float *dist, int32_t world, int64_t nq, int32_t kk, int32_t k,
                     int64_t *ids_out, float *dist_out, int32_t *count_out);

/*
 * The same exchange with the answers resident in HBM (one handle per GPU, RCCL all-gather between the two calls):
 *   morna_get_nns_by_vector_packed  as morna_get_nns_by_vector (q: host or this device's memory), but the answers are
 *       written to packed_dev -- memory of the handle's device, [nq][2k] int32: the k global ids (local id + id_offset,
 *       -1 = empty) followed by the bits of the k fp32 distances: Q * k * 8 bytes per rank.  ENQUEUED on
 *       the handle's stream when the call returns (q, when it is device memory, is read there too): work the caller
 *       orders behind that stream sees the message; morna_synchronize() waits for it.
 *   morna_merge_topk_packed  gathered_dev[world][nq][2kk] (the all-gathered messages, device memory; read on the
 *       handle's stream: complete before the call, or produced by work ordered on that stream) -> the k smallest
 *       (distance, id) per query, host memory, complete when the call returns.
 *   morna_get_item_vectors_dev  rows of `ids` -> out_dev[n][dim] (device memory), enqueued on the handle's stream.
 *   morna_get_stream  the handle's HIP stream (a hipStream_t), so that the caller can put its collectives between
 *       these calls in stream order instead of waiting on the host (torch: torch.cuda.ExternalStream).
 * world <= 64, kk <= 255, global ids below 2^31.
 */
int morna_get_nns_by_vector_packed(morna_index *h, const float *q, int64_t nq, int32_t k, int32_t search_k, int64_t id_offset,
                                   int32_t *packed_dev);
int morna_get_item_vectors_dev(morna_index *h, const int32_t *ids, int64_t n, float *out_dev);
int morna_get_stream(morna_index *h, void **stream_out);
int morna_merge_topk_packed(morna_index *h, const int32_t *gathered_dev, int32_t world, int64_t nq, int32_t kk, int32_t k,
                            int32_t *ids_out, float *dist_out, int32_t *count_out);

/*
 * ---- row-sharded search with the communicator inside the library ("the RCCL communicator owned by the
 * handle"; 8e).  One handle per GPU and process; rank g holds the rows with global ids [off[g], off[g+1]) -- off from the
 * ranks' own item counts, exchanged by the library -- and its own forest.  Every function below is COLLECTIVE: all ranks
 * call it with the same nq / k / search_k (and the same queries, where queries are passed).  Data path: per-shard search
 * -> ncclAllGather of the per-shard top-k (Q * k * 8 bytes per rank; exact: Q * (12 k + 4)) on the handle's stream ->
 * merge kernel; every rank receives the same merged answer (global ids).  RCCL is loaded at run time; without it
 * morna_comm_init fails and nothing falls back to the host.  Arguments are checked before the first collective of a call;
 * as in any RCCL program, a call that fails on ONE rank only (an item number out of that shard's range) leaves the other
 * ranks waiting in the collective: validate rank-local input before calling.
 *   morna_comm_unique_id   ncclGetUniqueId: ONE rank makes the id, the caller hands the 128 bytes to the others (any
 *                          channel: a file, MPI, torch.distributed's store)
 *   morna_comm_init        ncclCommInitRank on the handle's device; world <= 64
 *   morna_comm_info        rank, world and (when offsets != NULL: collective, always exchanges) offsets[world + 1].  The
 *                          sharded calls exchange the row counts themselves at their first use and whenever THIS handle's
 *                          row count has changed; ranks that resize must do so together (or call this on every rank)
 *   *_by_item_sharded      every rank contributes stored rows of ITS shard as queries (local ids); the answers come back
 *                          for all ranks' queries, rank 0's first.  n_each[world] = every rank's query count, or NULL
 *                          (then the counts are exchanged first).  Query rows travel HBM -> xGMI -> HBM.
 *   exact variants         merged as exact_search_nn's bisect_left scan over ALL rows would (equal distance: higher global
 *                          id first); count -1 as morna_exact_search, true of the whole matrix if true of one shard
 */
#define MORNA_COMM_ID_BYTES 128
int morna_comm_unique_id(uint8_t *id_out /* [MORNA_COMM_ID_BYTES] */);
int morna_comm_init(morna_index *h, const uint8_t *id, int32_t rank, int32_t world);
int morna_comm_destroy(morna_index *h);
int morna_comm_info(morna_index *h, int32_t *rank, int32_t *world, int64_t *offsets);
int morna_get_nns_by_vector_sharded(morna_index *h, const float *q, int64_t nq, int32_t k, int32_t search_k,
                                    int32_t *ids_out, float *dist_out, int32_t *count_out);
int morna_get_nns_by_item_sharded(morna_index *h, const int32_t *local_items, int64_t n_local, const int64_t *n_each,
                                  int32_t k, int32_t search_k, int32_t *ids_out, float *dist_out, int32_t *count_out);
int morna_exact_search_sharded(morna_index *h, const double *q, int64_t nq, int32_t k,
                               int32_t *ids_out, double *dist_out, int32_t *count_out);
int morna_exact_search_by_item_sharded(morna_index *h, const int32_t *local_items, int64_t n_local, const int64_t *n_each,
                                       int32_t k, int32_t *ids_out, double *dist_out, int32_t *count_out);
/*
 * The two halves of the exact exchange on their own (a caller with its own transport; tests that lay several shards'
 * messages side by side): the per-shard answers packed in HBM -- morna_exact_packed_bytes(nq, k) bytes: ids int32
 * [nq][k] (local + id_offset, -1 = empty) | count int32 [nq] | pad to 8 | distances fp64 [nq][k]; queries: exactly one
 * of q (host fp64 [nq][dim]), q_dev (fp32 [nq][dim], this device) and items (stored rows); enqueued on the handle's
 * stream -- and the merge of `world` such messages laid end to end in device memory (host results, waits).
 */
int64_t morna_exact_packed_bytes(int64_t nq, int32_t k);
int morna_exact_search_packed(morna_index *h, const double *q, const float *q_dev, const int32_t *items, int64_t nq, int32_t k,
                              int64_t id_offset, uint8_t *packed_dev);
int morna_merge_exact_packed(morna_index *h, const uint8_t *gathered_dev, int32_t world, int64_t nq, int32_t kk, int32_t k,
                             int32_t *ids_out, double *dist_out, int32_t *count_out);

/* ---- persistence (stands in for AnnoyIndex.save / load)      morna.py:439, 544 */
int morna_save(morna_index *h, const char *path);
int morna_load(morna_index *h, const char *path);

/* ---- measurement --------------------------------------------------------- */

enum {
    MORNA_T_FEATURES = 0,   /* hash + accumulate + transpose/convert + norms   */
    MORNA_T_TWO_MEANS = 1,  /* forest: centroid kernel                         */
    MORNA_T_SPLIT = 2,      /* forest: hyperplane margin / side kernel (dominant) */
    MORNA_T_PARTITION = 3,  /* forest: stable partition                        */
    MORNA_T_QUERY = 4,      /* traversal + refine + top-k                      */
    MORNA_T_EXACT = 5,      /* exact scan + re-rank                            */
    MORNA_T_QUERY_FILTER = 6, /* part of MORNA_T_QUERY: the whole-batch fp16 contraction (bytes = its flops) */
    MORNA_T_EXACT_SCAN = 7, /* part of MORNA_T_EXACT: the fp32 scan (bytes = its flops when it ran on the matrix cores) */
    MORNA_T_SPLIT_MM = 8,   /* part of MORNA_T_SPLIT: the fp16 contraction alone (bytes = the flops of the tiles it LAUNCHED) */
    MORNA_T_TM_STRIP = 9,   /* part of MORNA_T_TWO_MEANS: levels run by two_means_strip_kernel (four waves per node), and
                               by two_means_wide_kernel (the same strips, rows past 8192 floats) */
    MORNA_T_TM_WAVE = 10,   /* part of MORNA_T_TWO_MEANS: levels run by two_means_wave_kernel (one wave per node) */
    MORNA_T_COUNT = 11
};
/* HIP-event timing of the kernels on the handle's own stream.  on: 0 off, 1 every group, otherwise a mask with bit
 * (MORNA_T_x + 1) set for each group to time (each event pair costs the stream a few microseconds of idle) */
int morna_timer_enable(morna_index *h, int32_t on);
int morna_timer_reset(morna_index *h);
/* ms = summed event time, launches, bytes = algorithmic bytes of those launches */
int morna_timer_read(morna_index *h, int32_t which, double *ms, int64_t *launches, int64_t *bytes);
int morna_synchronize(morna_index *h);

#ifdef __cplusplus
}
#endif
#endif /* MORNA_HIP_H */
