/* morna_jstore_thin from C, against include/morna_hip.h alone: the known answers of the contract, the
 * borrowed views, the statistics and the refusals.  Prints "thin caller ok" and returns 0 when all hold. */
#include <stdio.h>
#include <string.h>

#include "morna_hip.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, morna_last_error()); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

int main(void)
{
    /* two samples: 12 holds six lines, 21504 three */
    const int64_t ext_ids[2] = {12, 21504}, ptr[3] = {0, 6, 9};
    const int32_t line[9] = {0, 1, 2, 3, 4095, 4096, 10, 20, 30};
    const int32_t cov[9] = {5, 5, 5, 5, 64, 65, 1, 1, 100000};
    morna_jstore *store = NULL;
    CHECK(morna_jstore_from_arrays(0, ext_ids, 2, ptr, line, cov, 5000, &store) == MORNA_OK);

    const int64_t jobs[3] = {12, 12, 12};
    const uint64_t keep[3] = {(uint64_t)1 << 31, 0, (uint64_t)1 << 32};
    morna_jthinned *r = NULL;
    CHECK(morna_jstore_thin(store, jobs, keep, 3, 8675309u, &r) == MORNA_OK && r);
    int64_t counts[3];
    CHECK(morna_jthinned_counts(r, counts) == MORNA_OK);
    CHECK(counts[0] == 6 && counts[1] == 0 && counts[2] == 6);
    const int32_t *lines_out = NULL, *cov_out = NULL;
    const int32_t want[6] = {1, 3, 3, 4, 39, 25};
    CHECK(morna_jthinned_job(r, 0, &lines_out, &cov_out) == MORNA_OK);
    CHECK(memcmp(lines_out, line, sizeof(want)) == 0 && memcmp(cov_out, want, sizeof(want)) == 0);
    CHECK(morna_jthinned_job(r, 2, &lines_out, &cov_out) == MORNA_OK);
    CHECK(memcmp(lines_out, line, 6 * sizeof(int32_t)) == 0 && memcmp(cov_out, cov, 6 * sizeof(int32_t)) == 0);
    CHECK(morna_jthinned_job(r, 3, &lines_out, &cov_out) == MORNA_E_RANGE);
    CHECK(morna_jthinned_job(r, -1, NULL, NULL) == MORNA_E_RANGE);
    double stats[5];
    CHECK(morna_jstore_thin_stats(store, stats) == MORNA_OK);
    CHECK(stats[0] > 0 && stats[1] == 16.0 * 18 && stats[2] == 4.0 * 18 + 8.0 * 12 && stats[3] == 3.0 * 149 && stats[4] == 3);
    CHECK(morna_jthinned_free(r) == MORNA_OK);

    const int64_t other[1] = {21504};
    const uint64_t tenth[1] = {429496730u};
    CHECK(morna_jstore_thin(store, other, tenth, 1, 1u, &r) == MORNA_OK);
    CHECK(morna_jthinned_counts(r, counts) == MORNA_OK && counts[0] == 1);
    CHECK(morna_jthinned_job(r, 0, &lines_out, &cov_out) == MORNA_OK && lines_out[0] == 30 && cov_out[0] == 9845);
    CHECK(morna_jthinned_free(r) == MORNA_OK);

    /* refusals: nothing is launched and the statistics are cleared */
    const int64_t unknown[1] = {7};
    const uint64_t too_much[1] = {((uint64_t)1 << 32) + 1};
    CHECK(morna_jstore_thin(store, unknown, tenth, 1, 1u, &r) == MORNA_E_RANGE && strstr(morna_last_error(), "7"));
    CHECK(morna_jstore_thin(store, other, too_much, 1, 1u, &r) == MORNA_E_INVALID);
    CHECK(morna_jstore_thin(store, NULL, tenth, 1, 1u, &r) == MORNA_E_INVALID);
    CHECK(morna_jstore_thin(store, other, NULL, 1, 1u, &r) == MORNA_E_INVALID);
    CHECK(morna_jstore_thin(store, other, tenth, 1, 1u, NULL) == MORNA_E_INVALID);
    CHECK(morna_jstore_thin(NULL, other, tenth, 1, 1u, &r) == MORNA_E_INVALID);
    CHECK(morna_jstore_thin_stats(store, stats) == MORNA_OK);
    CHECK(stats[0] == 0 && stats[1] == 0 && stats[2] == 0 && stats[3] == 0 && stats[4] == 0);
    CHECK(morna_jstore_thin(store, NULL, NULL, 0, 1u, &r) == MORNA_OK && r);
    CHECK(morna_jthinned_counts(r, NULL) == MORNA_OK);
    CHECK(morna_jthinned_free(r) == MORNA_OK);
    CHECK(morna_jstore_free(store) == MORNA_OK);
    printf("thin caller ok\n");
    return 0;
}
