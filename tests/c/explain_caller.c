/* morna_jstore_explain from C, against include/morna_hip.h alone: a store of three samples made from arrays, weights that are
 * powers of two (every product and sum below is exact), two queries by sample explained against their lists, the same
 * queries given as arrays, and the pairs compared with the contract worked out by hand; the statistics
 * and the refusals.  Prints "explain caller ok" and returns 0 when all hold. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "morna_hip.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, morna_last_error()); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

/* sample 10: components 2 1 . 5 12 .    sample 20: 6 . 0 2 4 .    sample 30: . 2 . . . 2 */
static const int64_t ext[3] = {10, 20, 30};
static const int64_t ptr[4] = {0, 4, 8, 10};
static const int32_t line[10] = {0, 1, 3, 4, 0, 2, 3, 4, 1, 5};
static const int32_t cov[10] = {1, 2, 5, 3, 3, 7, 2, 1, 4, 2};
static const double w[6] = {2.0, 0.5, 0.0, 1.0, 4.0, 1.0};

static int pair_is(const morna_jexplained *e, int64_t q, int32_t rank, const double *want_sums, const int64_t *want_counts, int n,
                   const int32_t *want_lines, const double *want_terms, const int32_t *want_cov)
{
    double sums[6];
    int64_t counts[3];
    int32_t n_top = -1;
    const int32_t *lines = NULL, *cov_r = NULL;
    const double *terms = NULL;
    if (morna_jexplained_pair(e, q, rank, sums, counts, &n_top, &lines, &terms, &cov_r) != MORNA_OK) return 0;
    const double ppqq = want_sums[1] * want_sums[2];
    const double radicand = ppqq > 0.0 ? 2.0 - 2.0 * want_sums[0] / sqrt(ppqq) : 2.0;
    if (memcmp(sums, want_sums, 5 * sizeof(double)) != 0 || sums[5] != sqrt(radicand > 0.0 ? radicand : 0.0)) return 0;
    if (memcmp(counts, want_counts, sizeof counts) != 0 || n_top != n) return 0;
    for (int i = 0; i < n; i++)
        if (lines[i] != want_lines[i] || terms[i] != want_terms[i] || cov_r[i] != want_cov[i]) return 0;
    return 1;
}

int main(void)
{
    int32_t n_dev = 0;
    CHECK(morna_device_count(&n_dev) == MORNA_OK && n_dev >= 1);
    morna_jstore *s = NULL;
    CHECK(morna_jstore_from_arrays(0, ext, 3, ptr, line, cov, 6, &s) == MORNA_OK);
    morna_jexplained *e = NULL;
    const int64_t q_ext[2] = {10, 20};
    const int64_t results[4] = {20, 30, 10, 0};   /* [nq][k]: query 20 has one result */
    const int32_t n_results[2] = {2, 1};
    CHECK(morna_jstore_explain_by_sample(s, q_ext, 2, results, n_results, 2, 2, &e) == MORNA_E_STATE && e == NULL);   /* no weights yet */
    CHECK(morna_jstore_set_weights(s, w, 6) == MORNA_OK);
    CHECK(morna_jstore_explain_by_sample(s, q_ext, 2, results, n_results, 2, 2, &e) == MORNA_OK && e != NULL);

    /* (10, 20): terms 12 (line 0), 0, 10 (line 3), 48 (line 4) */
    const double s0[5] = {70.0, 56.0, 174.0, 56.0, 173.0};
    const int64_t c0[3] = {3, 4, 3};
    const int32_t l0[2] = {4, 0}, v0[2] = {1, 3};
    const double t0[2] = {48.0, 12.0};
    CHECK(pair_is(e, 0, 0, s0, c0, 2, l0, t0, v0));
    /* (10, 30): line 1 alone is shared */
    const double s1[5] = {2.0, 8.0, 174.0, 4.0, 1.0};
    const int64_t c1[3] = {1, 4, 2};
    const int32_t l1[1] = {1}, v1[1] = {4};
    const double t1[1] = {2.0};
    CHECK(pair_is(e, 0, 1, s1, c1, 1, l1, t1, v1));
    /* (20, 10): the first pair the other way round */
    const double s2[5] = {70.0, 174.0, 56.0, 173.0, 56.0};
    const int64_t c2[3] = {3, 3, 4};
    const int32_t l2[2] = {4, 0}, v2[2] = {3, 1};
    CHECK(pair_is(e, 1, 0, s2, c2, 2, l2, t0, v2));
    CHECK(morna_jexplained_pair(e, 1, 1, NULL, NULL, NULL, NULL, NULL, NULL) == MORNA_E_RANGE);   /* past the query's list */
    CHECK(morna_jexplained_pair(e, 2, 0, NULL, NULL, NULL, NULL, NULL, NULL) == MORNA_E_RANGE);
    CHECK(morna_jexplained_pair(e, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL) == MORNA_OK);
    CHECK(morna_jexplained_free(e) == MORNA_OK);

    double stats[6];
    CHECK(morna_jstore_explain_stats(s, stats) == MORNA_OK);
    CHECK(stats[0] == 3.0 && stats[1] == 10.0 && stats[2] == 1.0 && stats[3] > 0.0 && stats[4] == 80.0 && stats[5] == 16.0);

    /* the same queries as arrays: sample 10's row with a line of coverage 0 added, sample 20's row */
    const int64_t q_ptr[3] = {0, 5, 9};
    const int32_t q_line[9] = {0, 1, 3, 4, 5, 0, 2, 3, 4}, q_cov[9] = {1, 2, 5, 3, 0, 3, 7, 2, 1};
    e = NULL;
    CHECK(morna_jstore_explain(s, q_ptr, q_line, q_cov, 2, results, n_results, 2, 2, &e) == MORNA_OK && e != NULL);
    CHECK(pair_is(e, 0, 0, s0, c0, 2, l0, t0, v0) && pair_is(e, 0, 1, s1, c1, 1, l1, t1, v1) && pair_is(e, 1, 0, s2, c2, 2, l2, t0, v2));
    CHECK(morna_jexplained_free(e) == MORNA_OK);

    /* refusals */
    e = NULL;
    const int64_t unknown[4] = {20, 77, 10, 0};
    CHECK(morna_jstore_explain_by_sample(s, q_ext, 2, unknown, n_results, 2, 2, &e) == MORNA_E_RANGE && e == NULL);
    CHECK(strstr(morna_last_error(), "77") != NULL);
    CHECK(morna_jstore_explain_stats(s, stats) == MORNA_OK && stats[0] == 0.0 && stats[3] == 0.0);
    CHECK(morna_jstore_explain_by_sample(s, q_ext, 2, results, n_results, 2, 0, &e) == MORNA_E_INVALID);
    CHECK(morna_jstore_explain_by_sample(s, q_ext, 2, results, n_results, 2, MORNA_JEXPLAIN_MAX_TOP + 1, &e) == MORNA_E_INVALID);
    CHECK(morna_jstore_explain_by_sample(s, q_ext, 2, results, n_results, 0, 2, &e) == MORNA_E_INVALID);
    CHECK(morna_jstore_explain_by_sample(s, q_ext, 2, results, n_results, MORNA_JNEAREST_MAX_K + 1, 2, &e) == MORNA_E_INVALID);
    const int32_t too_many[2] = {3, 1};
    CHECK(morna_jstore_explain_by_sample(s, q_ext, 2, results, too_many, 2, 2, &e) == MORNA_E_INVALID);
    const int64_t q_unknown[2] = {10, 99};
    CHECK(morna_jstore_explain_by_sample(s, q_unknown, 2, results, n_results, 2, 2, &e) == MORNA_E_RANGE);
    const int32_t q_negative[9] = {1, 2, -5, 3, 0, 3, 7, 2, 1};
    CHECK(morna_jstore_explain(s, q_ptr, q_line, q_negative, 2, results, n_results, 2, 2, &e) == MORNA_E_INVALID);
    CHECK(strstr(morna_last_error(), "line 3") != NULL);
    CHECK(morna_jstore_explain_by_sample(s, q_ext, 0, NULL, NULL, 2, 2, &e) == MORNA_OK && e != NULL);   /* no query: an empty answer */
    CHECK(morna_jexplained_free(e) == MORNA_OK);
    CHECK(morna_jstore_free(s) == MORNA_OK);
    printf("explain caller ok\n");
    return 0;
}
