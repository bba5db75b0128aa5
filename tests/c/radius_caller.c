/* morna_exact_radius from C, against include/morna_hip.h alone: an index of small-integer rows, the lists by item, by vector,
 * with `after` and under a restriction compared with the contract computed here -- cosine_distance in the
 * reference's sequential fp64 order, ordered by (distance, higher id first), cut at r inclusive -- the statistics and the
 * refusals.  Prints "radius caller ok" and returns 0 when all hold. */
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

#define N 70
#define DIM 6
#define NQ 4

static float rows[N * DIM];
static int32_t group[N];

/* morna.py:101-114 */
static double cosine_distance(const float *p, const double *q)
{
    double pq = 0.0, pp = 0.0, qq = 0.0;
    for (int z = 0; z < DIM; z++) {
        const double i = (double)p[z], j = q[z];
        pp = pp + i * i;
        qq = qq + j * j;
        pq = pq + i * j;
    }
    const double ppqq = pp * qq;
    double distance = 2.0;
    if (ppqq > 0.0) distance = 2.0 - (2.0 * pq) / sqrt(ppqq);
    return sqrt(distance);
}

typedef struct { double d; int32_t id; } entry;

static int by_distance_then_higher_id(const void *a, const void *b)
{
    const entry *x = (const entry *)a, *y = (const entry *)b;
    if (x->d != y->d) return x->d < y->d ? -1 : 1;
    return x->id > y->id ? -1 : x->id < y->id ? 1 : 0;
}

/* after: only rows above it; allow_even: only even rows; gq: the query's group (-1: none).  Returns the length. */
static int contract(const double *q, double r, int after, int allow_even, int gq, entry *out)
{
    int n = 0;
    for (int i = 0; i < N; i++) {
        if (i <= after || (allow_even && (i & 1)) || (gq >= 0 && group[i] == gq)) continue;
        const double d = cosine_distance(rows + i * DIM, q);
        if (d <= r) out[n].d = d, out[n++].id = i;
    }
    qsort(out, (size_t)n, sizeof(entry), by_distance_then_higher_id);
    return n;
}

static int same(const morna_radius *res, int64_t qi, const entry *want, int n)
{
    const int32_t *ids = NULL;
    const double *dist = NULL;
    int64_t len = -1;
    if (morna_radius_query(res, qi, &ids, &dist, &len) != MORNA_OK || len != n) return 0;
    for (int t = 0; t < n; t++)
        if (ids[t] != want[t].id || memcmp(&dist[t], &want[t].d, sizeof(double)) != 0) return 0;
    return 1;
}

int main(void)
{
    uint32_t state = 2014u;
    for (int i = 0; i < N * DIM; i++) {
        state = state * 1664525u + 1013904223u;
        rows[i] = (float)((int)((state >> 16) % 17u) - 8);   /* integers in [-8, 8] */
    }
    for (int z = 0; z < DIM; z++) rows[3 * DIM + z] = 0.0f;                       /* a zero row */
    for (int z = 0; z < DIM; z++) {                                               /* row 5 = 2 * row 4, row 60 = row 4 */
        rows[4 * DIM + z] = (float)((int)rows[4 * DIM + z] / 2);
        rows[5 * DIM + z] = 2.0f * rows[4 * DIM + z];
        rows[60 * DIM + z] = rows[4 * DIM + z];
    }
    rows[4 * DIM] = 3.0f;                                                         /* (not a zero row) */
    rows[5 * DIM] = 6.0f;
    rows[60 * DIM] = 3.0f;
    for (int r = 0; r < N; r++) group[r] = r < 10 ? 0 : -1;

    morna_index *h = NULL;
    CHECK(morna_index_create(DIM, 0, &h) == MORNA_OK);
    CHECK(morna_add_items_f32(h, 0, rows, N) == MORNA_OK);

    const int32_t items[NQ] = {0, 3, 4, 69};
    double q[NQ * DIM];
    for (int i = 0; i < NQ; i++)
        for (int z = 0; z < DIM; z++) q[i * DIM + z] = rows[items[i] * DIM + z];
    entry want[N];
    int64_t counts[NQ];
    double stats[8];
    morna_radius *res = NULL;
    const double radii[5] = {0.0, 0.9, 1.3, sqrt(2.0), 2.5};

    for (int k = 0; k < 5; k++) {
        /* by item and by vector: the same lists (the query's own row leads at distance 0) */
        for (int by_vector = 0; by_vector < 2; by_vector++) {
            CHECK(morna_exact_radius(h, NULL, by_vector ? q : NULL, by_vector ? NULL : items, NQ, NULL, NULL, radii[k], &res) == MORNA_OK);
            CHECK(morna_radius_counts(res, counts) == MORNA_OK);
            int64_t total = 0;
            for (int i = 0; i < NQ; i++) {
                const int n = contract(q + i * DIM, radii[k], -1, 0, -1, want);
                CHECK(counts[i] == n && same(res, i, want, n));
                total += n;
            }
            CHECK(morna_exact_radius_stats(h, stats) == MORNA_OK);
            CHECK(stats[0] > 0 && stats[1] > 0 && stats[3] == NQ && stats[4] == 1 && stats[5] >= stats[6] && stats[6] == (double)total);
            CHECK(stats[7] >= radii[k] * radii[k] && stats[7] < radii[k] * radii[k] * (1 + 1e-6) + 1e-4);
            CHECK(morna_radius_free(res) == MORNA_OK);
        }
    }
    /* the copies of row 4 at distance 0, higher id first; everything at 2.5; the zero row as the query: sqrt(2) or nothing */
    CHECK(morna_exact_radius(h, NULL, NULL, items, NQ, NULL, NULL, 0.0, &res) == MORNA_OK);
    CHECK(morna_radius_counts(res, counts) == MORNA_OK && counts[2] == 3 && counts[1] == 0);
    want[0].id = 60, want[1].id = 5, want[2].id = 4;
    want[0].d = want[1].d = want[2].d = 0.0;
    CHECK(same(res, 2, want, 3));
    CHECK(morna_radius_free(res) == MORNA_OK);
    CHECK(morna_exact_radius(h, NULL, NULL, items, NQ, NULL, NULL, 2.5, &res) == MORNA_OK);
    CHECK(morna_radius_counts(res, counts) == MORNA_OK && counts[0] == N && counts[1] == N && counts[3] == N);
    {   /* the lists lie one after the other */
        const int32_t *i0 = NULL, *i1 = NULL;
        const double *d0 = NULL, *d1 = NULL;
        int64_t n0 = 0, n1 = 0;
        CHECK(morna_radius_query(res, 0, &i0, &d0, &n0) == MORNA_OK && morna_radius_query(res, 1, &i1, &d1, &n1) == MORNA_OK);
        CHECK(i1 == i0 + n0 && d1 == d0 + n0 && n1 == N);
    }
    CHECK(morna_radius_free(res) == MORNA_OK);

    /* ids above; under a restriction: even rows only, and queries 0 and 2 leave group 0 out; both together */
    const int32_t after[NQ] = {0, -1, 40, 68};
    uint32_t allow[(N + 31) / 32];
    for (int w = 0; w < (N + 31) / 32; w++) allow[w] = 0x55555555u;
    const int32_t q_group[NQ] = {0, -1, 0, -1};
    morna_restriction *r = NULL;
    CHECK(morna_restriction_create(h, allow, group, &r) == MORNA_OK);
    for (int mode = 0; mode < 3; mode++) {
        CHECK(morna_exact_radius(h, mode ? r : NULL, NULL, items, NQ, mode ? q_group : NULL, mode == 1 ? NULL : after, 1.3, &res) == MORNA_OK);
        CHECK(morna_radius_counts(res, counts) == MORNA_OK);
        for (int i = 0; i < NQ; i++) {
            const int n = contract(q + i * DIM, 1.3, mode == 1 ? -1 : after[i], mode != 0, mode ? q_group[i] : -1, want);
            CHECK(counts[i] == n && same(res, i, want, n));
        }
        CHECK(morna_radius_free(res) == MORNA_OK);
    }

    /* refusals; the statistics are cleared; the exact search answers as before */
    res = (morna_radius *)h;
    CHECK(morna_exact_radius(h, NULL, NULL, items, NQ, NULL, NULL, -0.5, &res) == MORNA_E_INVALID && res == NULL);
    CHECK(morna_exact_radius(h, NULL, NULL, items, NQ, NULL, NULL, NAN, &res) == MORNA_E_INVALID);
    CHECK(morna_exact_radius(h, NULL, NULL, items, NQ, NULL, NULL, INFINITY, &res) == MORNA_E_INVALID);
    CHECK(morna_exact_radius(h, NULL, q, items, NQ, NULL, NULL, 1.0, &res) == MORNA_E_INVALID);
    CHECK(morna_exact_radius(h, NULL, NULL, NULL, NQ, NULL, NULL, 1.0, &res) == MORNA_E_INVALID);
    CHECK(morna_exact_radius(h, NULL, NULL, items, NQ, q_group, NULL, 1.0, &res) == MORNA_E_INVALID);
    CHECK(morna_exact_radius(h, NULL, NULL, items, NQ, NULL, NULL, 1.0, NULL) == MORNA_E_INVALID);
    CHECK(morna_exact_radius(NULL, NULL, NULL, items, NQ, NULL, NULL, 1.0, &res) == MORNA_E_INVALID);
    CHECK(morna_exact_radius_stats(h, stats) == MORNA_OK);
    for (int i = 0; i < 8; i++) CHECK(stats[i] == 0);
    CHECK(morna_exact_radius_stats(h, NULL) == MORNA_E_INVALID);
    CHECK(morna_radius_counts(NULL, counts) == MORNA_E_INVALID);
    int32_t ids[NQ * 3], cnt[NQ];
    double dist[NQ * 3];
    CHECK(morna_exact_search_by_item(h, items, NQ, 3, ids, dist, cnt) == MORNA_OK);
    CHECK(cnt[2] == 3 && ids[6] == 60 && ids[7] == 5 && ids[8] == 4 && dist[8] == 0.0);

    CHECK(morna_restriction_free(r) == MORNA_OK);
    CHECK(morna_index_destroy(h) == MORNA_OK);
    printf("radius caller ok\n");
    return 0;
}
