/* Restricted search from C, against include/morna_hip.h alone: a restriction is made, both searches run under it, its
 * counts are read and it is freed.  64 rows of 8 features, row i = e_(i % 8) + (i / 8 + 1) / 64 * e_((i + 1) % 8): the
 * neighbours of a row are the rows of its residue class.  Prints "restrict caller ok" and returns 0 when all holds. */
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
    CHECK(morna_build(h, 4, 1u) == MORNA_OK);

    /* allowed: the odd items; groups: item i has label i / 16 */
    uint32_t allow[2] = {0xaaaaaaaau, 0xaaaaaaaau};
    int32_t group[N];
    for (int i = 0; i < N; i++) group[i] = i / 16;
    morna_restriction *r = NULL;
    CHECK(morna_restriction_create(h, allow, group, &r) == MORNA_OK && r);
    int64_t counts[3] = {0, 0, 0};
    CHECK(morna_restriction_counts(r, counts) == MORNA_OK);
    CHECK(counts[0] == N && counts[1] == N / 2 && counts[2] == N);

    /* by item: query 9 carries its own group 0, query 41 none */
    const int32_t items[2] = {9, 41}, q_group[2] = {0, -1};
    int32_t ids[2 * K], count[2], ids_e[2 * K], count_e[2];
    float dist[2 * K];
    double dist_e[2 * K];
    CHECK(morna_get_nns_restricted(h, r, NULL, items, 2, q_group, K, N * 4, ids, dist, count) == MORNA_OK);
    CHECK(morna_exact_search_restricted(h, r, NULL, items, 2, q_group, K, ids_e, dist_e, count_e) == MORNA_OK);
    for (int q = 0; q < 2; q++) {
        CHECK(count[q] == K && count_e[q] == K);
        for (int j = 0; j < K; j++) {
            const int32_t a = ids[q * K + j], e = ids_e[q * K + j];
            CHECK(a >= 0 && a < N && (a & 1) && e >= 0 && e < N && (e & 1));          /* allowed items only */
            CHECK(q_group[q] < 0 || (group[a] != q_group[q] && group[e] != q_group[q]));   /* none of the query's group */
            CHECK(j == 0 || (dist[q * K + j - 1] <= dist[q * K + j] && dist_e[q * K + j - 1] <= dist_e[q * K + j]));
        }
    }
    CHECK(ids_e[0] == 17 && ids[0] == 17);       /* 9 without its group (0..15): the nearest odd row of its class is 17 */
    CHECK(ids_e[K] == 41 && ids[K] == 41);       /* 41 is allowed and carries no group: it finds itself */

    /* by vector, no query groups: row 9 as the query finds itself */
    double qd[D];
    float qf[D];
    for (int z = 0; z < D; z++) {
        qf[z] = rows[9][z];
        qd[z] = (double)rows[9][z];
    }
    CHECK(morna_get_nns_restricted(h, r, qf, NULL, 1, NULL, K, N * 4, ids, dist, count) == MORNA_OK);
    CHECK(morna_exact_search_restricted(h, r, qd, NULL, 1, NULL, K, ids_e, dist_e, count_e) == MORNA_OK);
    CHECK(count[0] == K && count_e[0] == K && ids[0] == 9 && ids_e[0] == 9 && dist_e[0] < 1e-3);

    /* refusals */
    CHECK(morna_get_nns_restricted(h, NULL, qf, NULL, 1, NULL, K, -1, ids, dist, count) == MORNA_E_INVALID);
    CHECK(morna_exact_search_restricted(h, NULL, qd, NULL, 1, NULL, K, ids_e, dist_e, count_e) == MORNA_E_INVALID);
    CHECK(morna_exact_search_restricted(h, r, qd, items, 1, NULL, K, ids_e, dist_e, count_e) == MORNA_E_INVALID);
    CHECK(morna_exact_search_restricted(h, r, NULL, NULL, 1, NULL, K, ids_e, dist_e, count_e) == MORNA_E_STATE);
    CHECK(morna_restriction_counts(NULL, counts) == MORNA_E_INVALID);
    morna_restriction *plain = NULL;
    CHECK(morna_restriction_create(h, NULL, NULL, &plain) == MORNA_OK);
    CHECK(morna_restriction_counts(plain, counts) == MORNA_OK && counts[1] == N && counts[2] == 0);
    CHECK(morna_exact_search_restricted(h, plain, qd, NULL, 1, q_group, K, ids_e, dist_e, count_e) == MORNA_E_INVALID);
    CHECK(morna_exact_search_restricted(h, plain, qd, NULL, 1, NULL, K, ids_e, dist_e, count_e) == MORNA_OK && ids_e[0] == 9);

    CHECK(morna_restriction_free(plain) == MORNA_OK);
    CHECK(morna_restriction_free(r) == MORNA_OK);
    CHECK(morna_restriction_free(NULL) == MORNA_OK);
    CHECK(morna_index_destroy(h) == MORNA_OK);
    printf("restrict caller ok\n");
    return 0;
}
