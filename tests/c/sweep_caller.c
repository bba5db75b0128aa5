/* Tree-prefix search, the (tree count, search_k) sweep and its recall counts from C, against include/morna_hip.h alone.
 * 64 rows of 8 features, row i = e_(i % 8) + (i / 8 + 1) / 64 * e_((i + 1) % 8), as restrict_caller.c makes them.  Every
 * cell of the sweep is compared with morna_get_nns_prefix.  Prints "sweep_caller: ok" and returns 0 when all holds. */
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

#define N 64
#define D 8
#define K 5
#define NT 3
#define NS 3
#define NQ 4

int main(void)
{
    static float rows[N][D];
    for (int i = 0; i < N; i++) {
        rows[i][i % D] = 1.0f;
        rows[i][(i + 1) % D] = (float)(i / D + 1) / 64.0f;
    }
    morna_index *h = NULL;
    CHECK(morna_index_create(D, 0, &h) == MORNA_OK && h);
    CHECK(morna_add_items_f32(h, 0, &rows[0][0], N) == MORNA_OK);
    const int32_t items[NQ] = {9, 41, 0, 63}, trees[NT] = {1, 2, 4}, search_ks[NS] = {1, 11, 300};
    static int32_t ids[NT][NS][NQ][K], count[NT][NS][NQ], ncand[NT][NS][NQ], ndots[NT][NS][NQ], hits[NT][NS][NQ];
    static float dist[NT][NS][NQ][K];
    int32_t p_ids[NQ][K], p_count[NQ], ex_count[NQ], ex_ids[NQ][K];
    float p_dist[NQ][K];
    double stats[4];

    /* an index that is not built */
    CHECK(morna_get_nns_prefix(h, NULL, items, NQ, K, -1, 1, &p_ids[0][0], &p_dist[0][0], p_count) == MORNA_E_STATE);
    CHECK(morna_search_sweep(h, NULL, items, NQ, K, trees, NT, search_ks, NS, &ids[0][0][0][0], NULL, NULL, NULL, NULL) == MORNA_E_STATE);
    CHECK(morna_build(h, 4, 1u) == MORNA_OK);

    /* by item and by vector (the rows themselves as vectors: the same queries, the same answers) */
    static float qv[NQ][D];
    for (int q = 0; q < NQ; q++) memcpy(qv[q], rows[items[q]], sizeof(qv[q]));
    for (int pass = 0; pass < 2; pass++) {
        const float *q = pass ? &qv[0][0] : NULL;
        const int32_t *it = pass ? NULL : items;
        CHECK(morna_search_sweep(h, q, it, NQ, K, trees, NT, search_ks, NS, &ids[0][0][0][0], &dist[0][0][0][0], &count[0][0][0],
                                 &ncand[0][0][0], &ndots[0][0][0]) == MORNA_OK);
        CHECK(morna_search_sweep_stats(h, stats) == MORNA_OK);
        CHECK(stats[0] == NQ * NT && stats[1] == NQ * NT * NS && stats[2] > 0);
        for (int i = 0; i < NT; i++)
            for (int j = 0; j < NS; j++) {
                CHECK(morna_get_nns_prefix(h, q, it, NQ, K, search_ks[j], trees[i], &p_ids[0][0], &p_dist[0][0], p_count) == MORNA_OK);
                CHECK(memcmp(p_ids, ids[i][j], sizeof(p_ids)) == 0);
                CHECK(memcmp(p_dist, dist[i][j], sizeof(p_dist)) == 0);
                CHECK(memcmp(p_count, count[i][j], sizeof(p_count)) == 0);
                for (int qq = 0; qq < NQ; qq++) {
                    CHECK(ncand[i][j][qq] >= count[i][j][qq] && ncand[i][j][qq] <= N && ndots[i][j][qq] >= trees[i]);
                    CHECK(j == 0 || (ncand[i][j][qq] >= ncand[i][j - 1][qq] && ndots[i][j][qq] >= ndots[i][j - 1][qq]));
                }
            }
        /* search_k 300 on all four trees visits every row: the row itself comes first */
        for (int qq = 0; qq < NQ; qq++) CHECK(ncand[NT - 1][NS - 1][qq] == N && ids[NT - 1][NS - 1][qq][0] == items[qq]);
    }
    /* the whole forest through the prefix call is the plain call */
    int32_t d_ids[NQ][K], d_count[NQ];
    float d_dist[NQ][K];
    CHECK(morna_get_nns_by_item(h, items, NQ, K, -1, &d_ids[0][0], &d_dist[0][0], d_count) == MORNA_OK);
    CHECK(morna_get_nns_prefix(h, NULL, items, NQ, K, -1, 4, &p_ids[0][0], &p_dist[0][0], p_count) == MORNA_OK);
    CHECK(memcmp(p_ids, d_ids, sizeof(p_ids)) == 0 && memcmp(p_dist, d_dist, sizeof(p_dist)) == 0 &&
          memcmp(p_count, d_count, sizeof(p_count)) == 0);

    /* recall: hits against the lists of the same call */
    CHECK(morna_recall_sweep(h, NULL, items, NQ, K, trees, NT, search_ks, NS, &hits[0][0][0], ex_count, &ncand[0][0][0], &ndots[0][0][0],
                             &ids[0][0][0][0], NULL, &count[0][0][0], &ex_ids[0][0]) == MORNA_OK);
    for (int i = 0; i < NT; i++)
        for (int j = 0; j < NS; j++)
            for (int qq = 0; qq < NQ; qq++) {
                int want = 0;
                for (int a = 0; a < count[i][j][qq]; a++)
                    for (int e = 0; e < ex_count[qq]; e++) want += ids[i][j][qq][a] == ex_ids[qq][e];
                CHECK(hits[i][j][qq] == (ex_count[qq] < 0 ? -1 : want));
            }
    CHECK(morna_recall_sweep(h, NULL, items, NQ, K, trees, NT, search_ks, NS, &hits[0][0][0], NULL, NULL, NULL, NULL, NULL, NULL, NULL) ==
          MORNA_OK);

    /* refusals */
    const int32_t unsorted[2] = {2, 1}, twice[2] = {2, 2}, past[2] = {1, 5}, zero[1] = {0};
    int32_t many[MORNA_SWEEP_MAX_LIST + 1];
    for (int i = 0; i <= MORNA_SWEEP_MAX_LIST; i++) many[i] = i + 1;
    CHECK(morna_search_sweep(h, NULL, items, NQ, K, unsorted, 2, search_ks, NS, NULL, NULL, NULL, NULL, NULL) == MORNA_E_INVALID);
    CHECK(morna_search_sweep(h, NULL, items, NQ, K, trees, NT, twice, 2, NULL, NULL, NULL, NULL, NULL) == MORNA_E_INVALID);
    CHECK(morna_search_sweep(h, NULL, items, NQ, K, zero, 1, search_ks, NS, NULL, NULL, NULL, NULL, NULL) == MORNA_E_INVALID);
    CHECK(morna_search_sweep(h, NULL, items, NQ, K, trees, 0, search_ks, NS, NULL, NULL, NULL, NULL, NULL) == MORNA_E_INVALID);
    CHECK(morna_search_sweep(h, NULL, items, NQ, K, trees, NT, many, MORNA_SWEEP_MAX_LIST + 1, NULL, NULL, NULL, NULL, NULL) ==
          MORNA_E_INVALID);
    CHECK(morna_search_sweep(h, NULL, items, NQ, K, trees, NT, many, MORNA_SWEEP_MAX_LIST, NULL, NULL, NULL, NULL, NULL) == MORNA_OK);
    CHECK(morna_search_sweep(h, NULL, items, NQ, K, past, 2, search_ks, NS, NULL, NULL, NULL, NULL, NULL) == MORNA_E_RANGE);
    CHECK(morna_search_sweep(h, &qv[0][0], items, NQ, K, trees, NT, search_ks, NS, NULL, NULL, NULL, NULL, NULL) == MORNA_E_INVALID);
    CHECK(morna_search_sweep(h, NULL, NULL, NQ, K, trees, NT, search_ks, NS, NULL, NULL, NULL, NULL, NULL) == MORNA_E_STATE);
    CHECK(morna_recall_sweep(h, NULL, items, NQ, MORNA_RECALL_MAX_K + 1, trees, NT, search_ks, NS, &hits[0][0][0], NULL, NULL, NULL, NULL,
                             NULL, NULL, NULL) == MORNA_E_INVALID);
    CHECK(morna_recall_sweep(h, NULL, items, NQ, K, trees, NT, search_ks, NS, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) ==
          MORNA_E_INVALID);
    CHECK(morna_get_nns_prefix(h, NULL, items, NQ, K, -1, 0, &p_ids[0][0], NULL, NULL) == MORNA_E_RANGE);
    CHECK(morna_get_nns_prefix(h, NULL, items, NQ, K, -1, 5, &p_ids[0][0], NULL, NULL) == MORNA_E_RANGE);
    CHECK(morna_search_sweep_stats(h, NULL) == MORNA_E_INVALID);
    CHECK(morna_index_destroy(h) == MORNA_OK);
    printf("sweep_caller: ok\n");
    return 0;
}
