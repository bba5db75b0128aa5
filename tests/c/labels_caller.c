/* morna_label_sums from C, against include/morna_hip.h alone: an index of small-integer rows (every fp32 dot and norm of the
 * scan exact), the sums by item, by vector and under a restriction compared with the contract computed
 * here, the statistics and the refusals.  Prints "labels caller ok" and returns 0 when all hold. */
#include <math.h>
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

#define N 70
#define DIM 6
#define L 3
#define NQ 4

static float rows[N * DIM];
static int32_t label[N], group[N];

/* the contract: v = float(2 - 2 pq / sqrt(pp qq)), 2 where pp qq is not positive; D = (uint64)(sqrt(max(v, 0)) 2^32 + 0.5) */
static uint64_t fixed_distance(const double *q, int r)
{
    double pq = 0.0, pp = 0.0, qq = 0.0;
    for (int z = 0; z < DIM; z++) {
        pq += q[z] * rows[r * DIM + z];
        pp += (double)rows[r * DIM + z] * rows[r * DIM + z];
        qq += q[z] * q[z];
    }
    volatile float v = pp * qq > 0.0 ? (float)(2.0 - 2.0 * pq / sqrt(pp * qq)) : 2.0f;
    const double d = sqrt((double)(v > 0.0f ? v : 0.0f));
    return (uint64_t)(d * 4294967296.0 + 0.5);
}

/* self: the row a by-item query skips (-1: none); allow_even: only even rows count; gq: the query's group (-1: none) */
static void contract(const double *q, int self, int allow_even, int gq, uint64_t *sums, int32_t *counts)
{
    for (int g = 0; g < L; g++) sums[g] = 0, counts[g] = 0;
    for (int r = 0; r < N; r++) {
        if (label[r] < 0 || r == self) continue;
        if (allow_even && (r & 1)) continue;
        if (gq >= 0 && group[r] == gq) continue;
        sums[label[r]] += fixed_distance(q, r);
        counts[label[r]]++;
    }
}

int main(void)
{
    uint32_t state = 12345u;
    for (int i = 0; i < N * DIM; i++) {
        state = state * 1664525u + 1013904223u;
        rows[i] = (float)((int)((state >> 16) % 17u) - 8);   /* integers in [-8, 8] */
    }
    for (int z = 0; z < DIM; z++) rows[3 * DIM + z] = 0.0f;                       /* a zero row */
    for (int z = 0; z < DIM; z++) {                                               /* row 5 = 2 * row 4: a scaled copy */
        rows[4 * DIM + z] = (float)((int)rows[4 * DIM + z] / 2);
        rows[5 * DIM + z] = 2.0f * rows[4 * DIM + z];
    }
    for (int r = 0; r < N; r++) {
        label[r] = r % 4 == 3 ? -1 : r % 4 == 2 ? 0 : r % 4;                       /* labels 0 and 1; label 2 below */
        group[r] = r < 10 ? 0 : -1;
    }
    label[0] = 2;                                                                 /* label 2: its only member is query 0 */

    morna_index *h = NULL;
    CHECK(morna_index_create(DIM, 0, &h) == MORNA_OK);
    CHECK(morna_add_items_f32(h, 0, rows, N) == MORNA_OK);

    const int32_t items[NQ] = {0, 3, 4, 69};
    double q[NQ * DIM];
    for (int i = 0; i < NQ; i++)
        for (int z = 0; z < DIM; z++) q[i * DIM + z] = rows[items[i] * DIM + z];
    uint64_t sums[NQ * L], want_s[L];
    int32_t counts[NQ * L], want_c[L];
    double stats[6];

    /* by item: the query itself is not counted */
    CHECK(morna_label_sums(h, NULL, NULL, items, NQ, NULL, label, L, sums, counts) == MORNA_OK);
    for (int i = 0; i < NQ; i++) {
        contract(q + i * DIM, items[i], 0, -1, want_s, want_c);
        CHECK(memcmp(sums + i * L, want_s, sizeof(want_s)) == 0 && memcmp(counts + i * L, want_c, sizeof(want_c)) == 0);
    }
    CHECK(counts[2] == 0 && sums[2] == 0 && counts[L + 2] == 1);
    /* the zero row as the query: every distance is sqrt(2) */
    CHECK(sums[L + 0] == (uint64_t)counts[L + 0] * (uint64_t)(sqrt(2.0) * 4294967296.0 + 0.5));
    CHECK(morna_label_sums_stats(h, stats) == MORNA_OK);
    CHECK(stats[0] > 0 && stats[1] > 0 && stats[2] == NQ && stats[3] == 1 && stats[5] > 0 && stats[5] < 1e-4);
    CHECK(stats[4] == counts[0] + counts[1] + counts[2] + counts[3] + counts[4] + counts[5] + counts[6] + counts[7] + counts[8]
                          + counts[9] + counts[10] + counts[11]);

    /* by vector: nothing is skipped */
    CHECK(morna_label_sums(h, NULL, q, NULL, NQ, NULL, label, L, sums, counts) == MORNA_OK);
    for (int i = 0; i < NQ; i++) {
        contract(q + i * DIM, -1, 0, -1, want_s, want_c);
        CHECK(memcmp(sums + i * L, want_s, sizeof(want_s)) == 0 && memcmp(counts + i * L, want_c, sizeof(want_c)) == 0);
    }
    CHECK(counts[2] == 1 && sums[2] == 0);

    /* under a restriction: even rows only, and queries 0 and 2 leave group 0 out */
    uint32_t allow[(N + 31) / 32];
    for (int w = 0; w < (N + 31) / 32; w++) allow[w] = 0x55555555u;
    const int32_t q_group[NQ] = {0, -1, 0, -1};
    morna_restriction *r = NULL;
    CHECK(morna_restriction_create(h, allow, group, &r) == MORNA_OK);
    CHECK(morna_label_sums(h, r, NULL, items, NQ, q_group, label, L, sums, counts) == MORNA_OK);
    for (int i = 0; i < NQ; i++) {
        contract(q + i * DIM, items[i], 1, q_group[i], want_s, want_c);
        CHECK(memcmp(sums + i * L, want_s, sizeof(want_s)) == 0 && memcmp(counts + i * L, want_c, sizeof(want_c)) == 0);
    }

    /* refusals; the statistics are cleared */
    int32_t bad[N];
    memcpy(bad, label, sizeof(bad));
    bad[9] = L;
    CHECK(morna_label_sums(h, NULL, NULL, items, NQ, NULL, bad, L, sums, counts) == MORNA_E_INVALID && strstr(morna_last_error(), "item 9"));
    CHECK(morna_label_sums(h, NULL, NULL, items, NQ, NULL, label, 0, sums, counts) == MORNA_E_INVALID);
    CHECK(morna_label_sums(h, NULL, NULL, items, NQ, NULL, label, MORNA_LABELS_MAX + 1, sums, counts) == MORNA_E_INVALID);
    CHECK(morna_label_sums(h, NULL, q, items, NQ, NULL, label, L, sums, counts) == MORNA_E_INVALID);
    CHECK(morna_label_sums(h, NULL, NULL, NULL, NQ, NULL, label, L, sums, counts) == MORNA_E_INVALID);
    CHECK(morna_label_sums(h, NULL, NULL, items, NQ, q_group, label, L, sums, counts) == MORNA_E_INVALID);
    CHECK(morna_label_sums(h, NULL, NULL, items, NQ, NULL, NULL, L, sums, counts) == MORNA_E_INVALID);
    CHECK(morna_label_sums(NULL, NULL, NULL, items, NQ, NULL, label, L, sums, counts) == MORNA_E_INVALID);
    CHECK(morna_label_sums_stats(h, stats) == MORNA_OK);
    CHECK(stats[0] == 0 && stats[1] == 0 && stats[2] == 0 && stats[3] == 0 && stats[4] == 0 && stats[5] == 0);
    CHECK(morna_label_sums_stats(h, NULL) == MORNA_E_INVALID);

    CHECK(morna_restriction_free(r) == MORNA_OK);
    CHECK(morna_index_destroy(h) == MORNA_OK);
    printf("labels caller ok\n");
    return 0;
}
