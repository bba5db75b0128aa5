/* morna_add_items_from_store from C, against include/morna_hip.h alone: a store from arrays, weights, one call, the rows read
 * back and compared with the contract computed here, the statistics, a refusal and the row norms.  Prints
 * "hashrows caller ok" and returns 0 when all hold. */
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

#define N_LINES 8
#define DIM 3

/* the contract: one sample's row, sequential per cell, one rounding per operation */
static void contract_row(const int32_t *line, const int32_t *cov, int64_t n, const double *w, const int32_t *hash, float *out)
{
    volatile double cell[DIM] = {0.0, 0.0, 0.0};
    for (int64_t i = 0; i < n; i++) {
        const int32_t j = line[i];
        if (w[j] == 0.0) continue;
        int32_t c = hash[j] % DIM;
        if (c < 0) c += DIM;
        volatile double term = (double)cov[i] * w[j];
        cell[c] = cell[c] + (hash[j] < 0 ? -term : term);
    }
    for (int c = 0; c < DIM; c++) out[c] = (float)cell[c];
}

int main(void)
{
    /* two samples: 12 holds five lines (one of weight 0, one negative coverage), 21504 three */
    const int64_t ext_ids[2] = {12, 21504}, ptr[3] = {0, 5, 8};
    const int32_t line[8] = {0, 1, 2, 3, 6, 4, 5, 7};
    const int32_t cov[8] = {2, 9, 3, -4, 5, 1, 2147483647, 0};
    const double w[N_LINES] = {1.5, 0.0, 2.0, 0.25, 3.0, 0.5, 1.0, 4.0};
    const int32_t hash[N_LINES] = {0, -1, 7, -8, 5, 2147483647, (int32_t)(-2147483647 - 1), 3};
    morna_jstore *store = NULL;
    morna_index *h = NULL;
    CHECK(morna_jstore_from_arrays(0, ext_ids, 2, ptr, line, cov, N_LINES, &store) == MORNA_OK);
    CHECK(morna_index_create(DIM, 0, &h) == MORNA_OK);

    /* no weights yet: refused, and the statistics say nothing ran */
    const int64_t named[3] = {21504, 12, 21504};
    double stats[4];
    CHECK(morna_add_items_from_store(h, store, named, 3, hash, N_LINES) == MORNA_E_STATE);
    CHECK(morna_jstore_set_weights(store, w, N_LINES) == MORNA_OK);
    CHECK(morna_add_items_from_store(h, store, named, 3, hash, N_LINES) == MORNA_OK);
    CHECK(morna_get_n_items(h) == 3);

    float rows[3 * DIM], want[3 * DIM], norms[3];
    CHECK(morna_get_items(h, rows) == MORNA_OK);
    contract_row(line + 5, cov + 5, 3, w, hash, want);
    contract_row(line, cov, 5, w, hash, want + DIM);
    contract_row(line + 5, cov + 5, 3, w, hash, want + 2 * DIM);
    CHECK(memcmp(rows, want, sizeof(rows)) == 0);
    /* and by hand.  12: line 0 -> cell 0, +3; line 2 (hash 7) -> cell 1, +6; line 3 (hash -8: cell 1, sign -) -(-1) = +1;
     * line 6 (INT32_MIN: cell 1, sign -) -5.  21504: line 4 (hash 5) -> cell 2, +3; line 5 (INT32_MAX: cell 1) 1073741823.5,
     * which fp32 rounds to 2^30; line 7 -> cell 0, +0 */
    const float by_hand[3 * DIM] = {0.0f, 1073741824.0f, 3.0f, 3.0f, 2.0f, 0.0f, 0.0f, 1073741824.0f, 3.0f};
    CHECK(memcmp(rows, by_hand, sizeof(rows)) == 0);
    CHECK(morna_get_norms2(h, norms) == MORNA_OK);
    CHECK(norms[1] == 13.0f && norms[0] == norms[2] && norms[0] > 1.0e18f);

    CHECK(morna_jstore_hash_rows_stats(store, stats) == MORNA_OK);
    CHECK(stats[0] > 0 && stats[1] == 8.0 * (3 + 5 + 3) + 12.0 * N_LINES && stats[2] == 4.0 * 3 * 256 && stats[3] == 3);

    /* refusals: nothing is launched, the statistics are cleared, the handle keeps its rows */
    const int64_t unknown[2] = {12, 7};
    CHECK(morna_add_items_from_store(h, store, unknown, 2, hash, N_LINES) == MORNA_E_RANGE && strstr(morna_last_error(), "7"));
    CHECK(morna_add_items_from_store(h, store, named, 3, hash, N_LINES - 1) == MORNA_E_INVALID);
    CHECK(morna_add_items_from_store(h, store, named, 0, hash, N_LINES) == MORNA_E_EMPTY);
    CHECK(morna_add_items_from_store(h, store, NULL, 3, hash, N_LINES) == MORNA_E_INVALID);
    CHECK(morna_add_items_from_store(h, store, named, 3, NULL, N_LINES) == MORNA_E_INVALID);
    CHECK(morna_add_items_from_store(NULL, store, named, 3, hash, N_LINES) == MORNA_E_INVALID);
    CHECK(morna_add_items_from_store(h, NULL, named, 3, hash, N_LINES) == MORNA_E_INVALID);
    CHECK(morna_jstore_hash_rows_stats(store, stats) == MORNA_OK);
    CHECK(stats[0] == 0 && stats[1] == 0 && stats[2] == 0 && stats[3] == 0);
    CHECK(morna_get_n_items(h) == 3 && morna_get_items(h, rows) == MORNA_OK && memcmp(rows, by_hand, sizeof(rows)) == 0);

    /* the unhashed squared norm of a row: v = cov * w, the squares added in line order */
    double pp[3];
    const int64_t twice[2] = {21504, 21504};
    volatile double v0 = 1.0 * 3.0, v1 = 2147483647.0 * 0.5, v2 = 0.0 * 4.0, sum = 0.0;
    sum = sum + v0 * v0;
    sum = sum + v1 * v1;
    sum = sum + v2 * v2;
    CHECK(morna_jstore_row_norms(store, twice, 2, pp) == MORNA_OK && pp[0] == sum && pp[1] == sum);
    CHECK(morna_jstore_row_norms(store, named, 3, pp) == MORNA_E_INVALID && strstr(morna_last_error(), "negative"));
    CHECK(morna_jstore_row_norms(store, unknown, 2, pp) == MORNA_E_RANGE);

    /* a built index takes no more items */
    CHECK(morna_build(h, 1, 0) == MORNA_OK);
    CHECK(morna_add_items_from_store(h, store, named, 3, hash, N_LINES) == MORNA_E_STATE);
    CHECK(morna_index_destroy(h) == MORNA_OK);
    CHECK(morna_jstore_free(store) == MORNA_OK);
    printf("hashrows caller ok\n");
    return 0;
}
