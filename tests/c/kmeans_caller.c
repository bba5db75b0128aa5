/* morna_kmeans and morna_kmeans_assign from C, against include/morna_hip.h alone: an index of small-integer rows, the loop with
 * and without an allow-list and one assignment against given centroids compared with the contract computed
 * here -- cosine_distance in the reference's sequential fp64 order, the lowest centroid of the smallest distance, the members'
 * scaled rows added in ascending id with one rounding per multiply and per add -- the statistics and the refusals.  Prints
 * "kmeans caller ok" and returns 0 when all hold. */
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
#define K 4

static float rows[N * DIM];

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

static void assign(const double *cent, int k, const int *allow, int32_t *a, double *d)
{
    for (int i = 0; i < N; i++) {
        if (allow && !allow[i]) {
            a[i] = -1, d[i] = -1.0;
            continue;
        }
        int bj = 0;
        double bd = cosine_distance(rows + i * DIM, cent);
        for (int j = 1; j < k; j++) {
            const double dj = cosine_distance(rows + i * DIM, cent + j * DIM);
            if (dj < bd || (bd != bd && dj == dj)) bd = dj, bj = j;
        }
        a[i] = bj, d[i] = bd;
    }
}

/* the contract's loop; returns the iterations, *converged set */
static int contract(const int32_t *seeds, int k, int max_iter, const int *allow, int32_t *a, double *d, double *cent, int32_t *sizes,
                    int *converged)
{
    int32_t prev[N];
    double next[K * DIM];
    for (int j = 0; j < k; j++)
        for (int z = 0; z < DIM; z++) cent[j * DIM + z] = (double)rows[seeds[j] * DIM + z];
    *converged = 0;
    int t = 0;
    for (;;) {
        t++;
        assign(cent, k, allow, a, d);
        if (t > 1 && memcmp(a, prev, sizeof prev) == 0) {
            *converged = 1;
            break;
        }
        if (t == max_iter) break;
        memcpy(next, cent, sizeof(double) * (size_t)k * DIM);
        for (int j = 0; j < k; j++) {
            double acc[DIM] = {0};
            int any = 0;
            for (int i = 0; i < N; i++) {
                if (a[i] != j) continue;
                double pp = 0.0;
                for (int z = 0; z < DIM; z++) pp = pp + (double)rows[i * DIM + z] * (double)rows[i * DIM + z];
                if (!(pp > 0.0 && pp < INFINITY)) continue;
                const double s = 1.0 / sqrt(pp);
                for (int z = 0; z < DIM; z++) acc[z] = acc[z] + (double)rows[i * DIM + z] * s;
                any = 1;
            }
            if (any) memcpy(next + j * DIM, acc, sizeof acc);
        }
        memcpy(prev, a, sizeof prev);
        memcpy(cent, next, sizeof(double) * (size_t)k * DIM);
    }
    for (int j = 0; j < k; j++) sizes[j] = 0;
    for (int i = 0; i < N; i++)
        if (a[i] >= 0) sizes[a[i]]++;
    return t;
}

int main(void)
{
    uint32_t state = 2015u;
    for (int i = 0; i < N * DIM; i++) {
        state = state * 1664525u + 1013904223u;
        rows[i] = (float)((int)((state >> 16) % 17u) - 8);   /* integers in [-8, 8] */
    }
    for (int z = 0; z < DIM; z++) rows[3 * DIM + z] = 0.0f;                       /* a zero row */
    rows[4 * DIM] = 3.0f;                                                         /* (not a zero row) */
    for (int z = 0; z < DIM; z++) rows[5 * DIM + z] = 2.0f * rows[4 * DIM + z];   /* row 5 = 2 * row 4 */

    morna_index *h = NULL;
    CHECK(morna_index_create(DIM, 0, &h) == MORNA_OK);
    CHECK(morna_add_items_f32(h, 0, rows, N) == MORNA_OK);

    const int32_t seeds[K] = {0, 9, 21, 40};
    int32_t a[N], want_a[N], sizes[K], want_sizes[K], info[2];
    double d[N], want_d[N], cent[K * DIM], want_cent[K * DIM], stats[8];
    int converged = 0;

    /* the loop to convergence, and cut after 1 and 2 assignments */
    const int max_iters[3] = {50, 1, 2};
    for (int m = 0; m < 3; m++) {
        const int t = contract(seeds, K, max_iters[m], NULL, want_a, want_d, want_cent, want_sizes, &converged);
        CHECK(morna_kmeans(h, NULL, seeds, K, max_iters[m], a, d, cent, sizes, info) == MORNA_OK);
        CHECK(info[0] == t && info[1] == converged);
        CHECK(memcmp(a, want_a, sizeof a) == 0 && memcmp(d, want_d, sizeof d) == 0);
        CHECK(memcmp(cent, want_cent, sizeof cent) == 0 && memcmp(sizes, want_sizes, sizeof sizes) == 0);
        CHECK(morna_kmeans_stats(h, stats) == MORNA_OK);
        int largest = 0;
        for (int j = 0; j < K; j++) largest = sizes[j] > largest ? sizes[j] : largest;
        CHECK(stats[0] > 0 && stats[1] > 0 && stats[2] > 0 && stats[5] >= (double)N * t && stats[6] == t && stats[7] == largest);
        if (m == 0) CHECK(converged == 1 && t > 2);
    }
    /* the optional outputs may be NULL */
    CHECK(morna_kmeans(h, NULL, seeds, K, 50, a, NULL, NULL, NULL, info) == MORNA_OK);
    (void)contract(seeds, K, 50, NULL, want_a, want_d, want_cent, want_sizes, &converged);
    CHECK(memcmp(a, want_a, sizeof a) == 0);

    /* one assignment against those centroids: the same answer; a doubled copy behind a centroid loses the tie */
    CHECK(morna_kmeans_assign(h, NULL, want_cent, K, a, d) == MORNA_OK);
    CHECK(memcmp(a, want_a, sizeof a) == 0 && memcmp(d, want_d, sizeof d) == 0);
    CHECK(morna_kmeans_stats(h, stats) == MORNA_OK && stats[6] == 1 && stats[7] == 0);
    double five[5 * DIM];
    memcpy(five, want_cent, sizeof want_cent);
    for (int z = 0; z < DIM; z++) five[4 * DIM + z] = 2.0 * want_cent[1 * DIM + z];
    CHECK(morna_kmeans_assign(h, NULL, five, 5, a, NULL) == MORNA_OK && memcmp(a, want_a, sizeof a) == 0);

    /* an allow-list: even rows only */
    uint32_t allow_bits[(N + 31) / 32];
    int allow[N];
    for (int w = 0; w < (N + 31) / 32; w++) allow_bits[w] = 0x55555555u;
    for (int i = 0; i < N; i++) allow[i] = !(i & 1);
    morna_restriction *r = NULL;
    CHECK(morna_restriction_create(h, allow_bits, NULL, &r) == MORNA_OK);
    const int32_t even_seeds[3] = {0, 22, 40};
    const int t = contract(even_seeds, 3, 50, allow, want_a, want_d, want_cent, want_sizes, &converged);
    CHECK(morna_kmeans(h, r, even_seeds, 3, 50, a, d, cent, sizes, info) == MORNA_OK && info[0] == t && info[1] == converged);
    CHECK(memcmp(a, want_a, sizeof a) == 0 && memcmp(d, want_d, sizeof d) == 0 && a[1] == -1 && d[1] == -1.0);
    CHECK(memcmp(cent, want_cent, sizeof(double) * 3 * DIM) == 0 && memcmp(sizes, want_sizes, sizeof(int32_t) * 3) == 0);

    /* refusals; the statistics are cleared; the exact search answers as before */
    int32_t group[N];
    for (int i = 0; i < N; i++) group[i] = i < 10 ? 0 : -1;
    morna_restriction *grouped = NULL;
    CHECK(morna_restriction_create(h, NULL, group, &grouped) == MORNA_OK);
    const int32_t twice[2] = {7, 7}, odd[2] = {0, 9}, outside[2] = {0, N};
    CHECK(morna_kmeans(h, NULL, seeds, 0, 50, a, d, cent, sizes, info) == MORNA_E_INVALID);
    CHECK(morna_kmeans(h, NULL, seeds, K, 0, a, d, cent, sizes, info) == MORNA_E_INVALID);
    CHECK(morna_kmeans(h, NULL, twice, 2, 50, a, d, cent, sizes, info) == MORNA_E_INVALID);
    CHECK(morna_kmeans(h, NULL, outside, 2, 50, a, d, cent, sizes, info) == MORNA_E_RANGE);
    CHECK(morna_kmeans(h, r, odd, 2, 50, a, d, cent, sizes, info) == MORNA_E_INVALID);
    CHECK(morna_kmeans(h, grouped, seeds, K, 50, a, d, cent, sizes, info) == MORNA_E_INVALID);
    CHECK(morna_kmeans(h, NULL, NULL, K, 50, a, d, cent, sizes, info) == MORNA_E_INVALID);
    CHECK(morna_kmeans(h, NULL, seeds, K, 50, NULL, d, cent, sizes, info) == MORNA_E_INVALID);
    CHECK(morna_kmeans(NULL, NULL, seeds, K, 50, a, d, cent, sizes, info) == MORNA_E_INVALID);
    five[2] = NAN;
    CHECK(morna_kmeans_assign(h, NULL, five, 5, a, d) == MORNA_E_INVALID);
    CHECK(morna_kmeans_assign(h, NULL, NULL, 5, a, d) == MORNA_E_INVALID);
    CHECK(morna_kmeans_stats(h, stats) == MORNA_OK);
    for (int i = 0; i < 8; i++) CHECK(stats[i] == 0);
    CHECK(morna_kmeans_stats(h, NULL) == MORNA_E_INVALID);
    const int32_t items[1] = {4};
    int32_t ids[3], cnt[1];
    double dist[3];
    CHECK(morna_exact_search_by_item(h, items, 1, 3, ids, dist, cnt) == MORNA_OK);
    CHECK(cnt[0] == 3 && ids[0] == 5 && ids[1] == 4 && dist[1] == 0.0);

    CHECK(morna_restriction_free(grouped) == MORNA_OK);
    CHECK(morna_restriction_free(r) == MORNA_OK);
    CHECK(morna_index_destroy(h) == MORNA_OK);
    printf("kmeans caller ok\n");
    return 0;
}
