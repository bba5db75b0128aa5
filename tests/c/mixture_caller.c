/* morna_label_centroids and morna_mixture from C, against include/morna_hip.h alone: an index of small-integer rows, the centroid
 * sums, their counts and Gram matrix, and the fit of queries by item (the own label left out), by vector and under an allow-list
 * compared with the contract computed here -- every sum sequential in fp64 with one rounding per multiply and
 * per add, the cyclic coordinate descent label by label -- the statistics and the refusals.  Prints "mixture caller ok" and
 * returns 0 when all hold. */
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
#define L 5

static float rows[N * DIM];
static int32_t label[N];
static double pp[N], sigma[N], s[L * DIM], S[L * L];
static int32_t m[L];

static void centroids(const int *allow)
{
    memset(s, 0, sizeof s);
    memset(m, 0, sizeof m);
    for (int i = 0; i < N; i++) {
        pp[i] = 0.0;
        for (int z = 0; z < DIM; z++) pp[i] = pp[i] + (double)rows[i * DIM + z] * (double)rows[i * DIM + z];
        sigma[i] = pp[i] > 0.0 && pp[i] < INFINITY ? 1.0 / sqrt(pp[i]) : -1.0;
        if (label[i] < 0 || (allow && !allow[i]) || sigma[i] < 0.0) continue;
        for (int z = 0; z < DIM; z++) s[label[i] * DIM + z] = s[label[i] * DIM + z] + (double)rows[i * DIM + z] * sigma[i];
        m[label[i]]++;
    }
    for (int a = 0; a < L; a++)
        for (int b = a; b < L; b++) {
            double acc = 0.0;
            for (int z = 0; z < DIM; z++) acc = acc + s[a * DIM + z] * s[b * DIM + z];
            S[a * L + b] = S[b * L + a] = acc;
        }
}

/* one query of the contract: y, and `item` >= 0 when it is that stored row (centroids() ran with the same allow-list) */
static void fit(const double *y, int item, const int *allow, double tol, int max_sweeps, double *w, double *info, uint8_t *act)
{
    double yy = 0.0, t[L], Sp[L * L], G[L * L], d[L], b[L], a[L], g[L], hsum[L];
    int mm[L], o = -1;
    memcpy(Sp, S, sizeof Sp);
    for (int l = 0; l < L; l++) {
        t[l] = 0.0;
        mm[l] = m[l];
    }
    for (int z = 0; z < DIM; z++) {
        yy = yy + y[z] * y[z];
        for (int l = 0; l < L; l++) t[l] = t[l] + s[l * DIM + z] * y[z];
    }
    if (item >= 0 && label[item] >= 0 && (!allow || allow[item]) && sigma[item] > 0.0) {
        o = label[item];
        double tau[L];
        for (int l = 0; l < L; l++) tau[l] = t[l] * sigma[item];
        for (int l = 0; l < L; l++)
            if (l != o) Sp[o * L + l] = Sp[l * L + o] = S[o * L + l] - tau[l];
        Sp[o * L + o] = (S[o * L + o] - 2.0 * tau[o]) + 1.0;
        t[o] = t[o] - pp[item] * sigma[item];
        mm[o]--;
    }
    int any = 0;
    for (int l = 0; l < L; l++) {
        act[l] = mm[l] >= 1 && Sp[l * L + l] > 0.0 && Sp[l * L + l] < INFINITY;
        d[l] = act[l] ? sqrt(Sp[l * L + l]) : 0.0;
        any |= act[l];
        w[l] = 0.0;
    }
    info[0] = info[1] = info[2] = 0.0;
    info[3] = -1.0;
    if (!(yy > 0.0 && yy < INFINITY) || !any) return;
    for (int l = 0; l < L; l++) {
        for (int k = 0; k < L; k++) G[l * L + k] = l == k ? 1.0 : act[l] && act[k] ? Sp[l * L + k] / (d[l] * d[k]) : 0.0;
        b[l] = act[l] ? t[l] / (d[l] * sqrt(yy)) : 0.0;
        a[l] = 0.0;
        g[l] = b[l];
    }
    int sweeps = 0, status = 0;
    for (int sw = 1; sw <= max_sweeps; sw++) {
        double mx = 0.0;
        for (int l = 0; l < L; l++) {
            if (!act[l]) continue;
            double delta = g[l];
            if (delta < -a[l]) delta = -a[l];
            if (delta != 0.0) {
                a[l] = a[l] + delta;
                for (int k = 0; k < L; k++)
                    if (act[k]) g[k] = g[k] - delta * G[k * L + l];
            }
            if (fabs(delta) > mx) mx = fabs(delta);
        }
        sweeps = sw;
        if (mx <= tol) {
            status = 1;
            break;
        }
    }
    double kkt = 0.0, u = 0.0, v = 0.0;
    for (int l = 0; l < L; l++) {
        hsum[l] = 0.0;
        for (int k = 0; k < L; k++)
            if (act[k]) hsum[l] = hsum[l] + G[l * L + k] * a[k];
    }
    for (int l = 0; l < L; l++) {
        if (!act[l]) continue;
        const double wl = b[l] - hsum[l], kl = a[l] > 0.0 ? fabs(wl) : (wl > 0.0 ? wl : 0.0);
        if (kl > kkt) kkt = kl;
        u = u + a[l] * hsum[l];
        v = v + a[l] * b[l];
        w[l] = a[l];
    }
    info[0] = (1.0 - 2.0 * v) + u;
    info[1] = kkt;
    info[2] = sweeps;
    info[3] = status;
}

#define NQ 12

int main(void)
{
    uint32_t state = 2016u;
    for (int i = 0; i < N * DIM; i++) {
        state = state * 1664525u + 1013904223u;
        rows[i] = (float)((int)((state >> 16) % 17u) - 8);   /* integers in [-8, 8] */
    }
    for (int i = 0; i < N; i++) label[i] = i % 7 == 6 ? -1 : i % 4;               /* labels 0..3; label 4 stays empty */
    label[9] = 4;                                                                 /* but for one member */
    for (int i = 0; i < N; i++)                                                   /* the rows lean towards their label */
        if (label[i] >= 0) rows[i * DIM + label[i]] += 20.0f;
    for (int z = 0; z < DIM; z++) rows[3 * DIM + z] = 0.0f;                       /* a zero row, a member of label 3 */

    morna_index *h = NULL;
    CHECK(morna_index_create(DIM, 0, &h) == MORNA_OK);
    CHECK(morna_add_items_f32(h, 0, rows, N) == MORNA_OK);

    double sums[L * DIM], gram[L * L], stats[8];
    int32_t counts[L];
    centroids(NULL);
    CHECK(morna_label_centroids(h, NULL, label, L, sums, counts, gram) == MORNA_OK);
    CHECK(memcmp(sums, s, sizeof s) == 0 && memcmp(counts, m, sizeof m) == 0 && memcmp(gram, S, sizeof S) == 0);
    CHECK(m[4] == 1 && m[0] + m[1] + m[2] + m[3] + m[4] == N - N / 7 - 1);        /* (the zero row 3 is skipped) */
    CHECK(morna_label_centroids(h, NULL, label, L, sums, counts, NULL) == MORNA_OK && memcmp(sums, s, sizeof s) == 0);
    CHECK(morna_mixture_stats(h, stats) == MORNA_OK && stats[0] > 0 && stats[1] > 0 && stats[4] == 0);

    /* by item: the lone member of label 4, the zero row, an item without a label, and others */
    const int32_t items[NQ] = {9, 3, 6, 0, 1, 2, 4, 5, 7, 8, 40, 69};
    double w[NQ * L], info[NQ * 4], want_w[L], want_info[4], y[DIM];
    uint8_t act[NQ * L], want_act[L];
    const double tols[3] = {1e-12, 1e-12, 0.0};
    const int sweeps[3] = {1000, 2, 50};
    for (int c = 0; c < 3; c++) {
        CHECK(morna_mixture(h, NULL, NULL, items, NQ, label, L, tols[c], sweeps[c], w, info, act) == MORNA_OK);
        double total = 0.0, largest = 0.0, open = 0.0;
        for (int q = 0; q < NQ; q++) {
            for (int z = 0; z < DIM; z++) y[z] = (double)rows[items[q] * DIM + z];
            fit(y, items[q], NULL, tols[c], sweeps[c], want_w, want_info, want_act);
            CHECK(memcmp(w + q * L, want_w, sizeof want_w) == 0 && memcmp(info + q * 4, want_info, sizeof want_info) == 0);
            CHECK(memcmp(act + q * L, want_act, sizeof want_act) == 0);
            total += want_info[2];
            largest = want_info[2] > largest ? want_info[2] : largest;
            open += want_info[3] != 1.0;
        }
        CHECK(act[4] == 0 && act[L + 4] == 1 && info[4 + 3] == -1.0);             /* label 4 without item 9; the zero row */
        CHECK(morna_mixture_stats(h, stats) == MORNA_OK);
        CHECK(stats[2] > 0 && stats[3] > 0 && stats[4] == NQ && stats[5] == total && stats[6] == largest && stats[7] == open);
        if (c == 0) CHECK(open == 1);
        if (c == 1) CHECK(largest == 2 && open > 1);
    }
    /* the active flags may be NULL; by vector nothing is left out */
    double Q[3 * DIM];
    for (int q = 0; q < 3; q++)
        for (int z = 0; z < DIM; z++) Q[q * DIM + z] = q == 2 ? (z == 1 ? 2.5 : -0.5) : (double)rows[items[q] * DIM + z];
    CHECK(morna_mixture(h, NULL, Q, NULL, 3, label, L, 1e-12, 1000, w, info, NULL) == MORNA_OK);
    for (int q = 0; q < 3; q++) {
        fit(Q + q * DIM, -1, NULL, 1e-12, 1000, want_w, want_info, want_act);
        CHECK(memcmp(w + q * L, want_w, sizeof want_w) == 0 && memcmp(info + q * 4, want_info, sizeof want_info) == 0);
    }
    CHECK(w[2 * L + 1] > 0.5);                                                    /* a vector along label 1 */

    /* an allow-list: even rows only; an odd query gets no patch */
    uint32_t allow_bits[(N + 31) / 32];
    int allow[N];
    for (int k = 0; k < (N + 31) / 32; k++) allow_bits[k] = 0x55555555u;
    for (int i = 0; i < N; i++) allow[i] = !(i & 1);
    morna_restriction *r = NULL;
    CHECK(morna_restriction_create(h, allow_bits, NULL, &r) == MORNA_OK);
    centroids(allow);
    CHECK(morna_label_centroids(h, r, label, L, sums, counts, gram) == MORNA_OK);
    CHECK(memcmp(sums, s, sizeof s) == 0 && memcmp(counts, m, sizeof m) == 0 && memcmp(gram, S, sizeof S) == 0 && m[4] == 0);
    CHECK(morna_mixture(h, r, NULL, items, NQ, label, L, 1e-12, 1000, w, info, act) == MORNA_OK);
    for (int q = 0; q < NQ; q++) {
        for (int z = 0; z < DIM; z++) y[z] = (double)rows[items[q] * DIM + z];
        fit(y, items[q], allow, 1e-12, 1000, want_w, want_info, want_act);
        CHECK(memcmp(w + q * L, want_w, sizeof want_w) == 0 && memcmp(info + q * 4, want_info, sizeof want_info) == 0);
        CHECK(memcmp(act + q * L, want_act, sizeof want_act) == 0 && act[q * L + 4] == 0);
    }

    /* refusals; the statistics are cleared; the exact search answers as before */
    int32_t group[N], bad[N];
    for (int i = 0; i < N; i++) group[i] = i < 10 ? 0 : -1;
    morna_restriction *grouped = NULL;
    CHECK(morna_restriction_create(h, NULL, group, &grouped) == MORNA_OK);
    memcpy(bad, label, sizeof bad);
    bad[11] = L;
    const int32_t outside[2] = {0, N};
    CHECK(morna_mixture(h, grouped, NULL, items, NQ, label, L, 1e-9, 100, w, info, act) == MORNA_E_INVALID);
    CHECK(morna_label_centroids(h, grouped, label, L, sums, counts, gram) == MORNA_E_INVALID);
    CHECK(morna_mixture(h, NULL, NULL, items, NQ, bad, L, 1e-9, 100, w, info, act) == MORNA_E_INVALID);
    CHECK(strstr(morna_last_error(), "item 11") != NULL);
    CHECK(morna_mixture(h, NULL, NULL, items, NQ, label, 0, 1e-9, 100, w, info, act) == MORNA_E_INVALID);
    CHECK(morna_mixture(h, NULL, NULL, items, NQ, label, MORNA_MIXTURE_LABELS_MAX + 1, 1e-9, 100, w, info, act) == MORNA_E_INVALID);
    CHECK(strstr(morna_last_error(), "129 labels") != NULL);
    CHECK(morna_mixture(h, NULL, NULL, items, NQ, label, L, -1.0, 100, w, info, act) == MORNA_E_INVALID);
    CHECK(morna_mixture(h, NULL, NULL, items, NQ, label, L, NAN, 100, w, info, act) == MORNA_E_INVALID);
    CHECK(morna_mixture(h, NULL, NULL, items, NQ, label, L, 1e-9, 0, w, info, act) == MORNA_E_INVALID);
    CHECK(strstr(morna_last_error(), "max_sweeps") != NULL);
    CHECK(morna_mixture(h, NULL, Q, items, 3, label, L, 1e-9, 100, w, info, act) == MORNA_E_INVALID);
    CHECK(morna_mixture(h, NULL, NULL, outside, 2, label, L, 1e-9, 100, w, info, act) == MORNA_E_RANGE);
    CHECK(morna_mixture(h, NULL, NULL, NULL, 2, label, L, 1e-9, 100, w, info, act) == MORNA_E_INVALID);    /* nothing is staged */
    CHECK(morna_mixture(h, NULL, NULL, items, NQ, NULL, L, 1e-9, 100, w, info, act) == MORNA_E_INVALID);
    CHECK(morna_mixture(h, NULL, NULL, items, NQ, label, L, 1e-9, 100, NULL, info, act) == MORNA_E_INVALID);
    CHECK(morna_mixture(NULL, NULL, NULL, items, NQ, label, L, 1e-9, 100, w, info, act) == MORNA_E_INVALID);
    Q[4] = NAN;
    CHECK(morna_mixture(h, NULL, Q, NULL, 3, label, L, 1e-9, 100, w, info, act) == MORNA_E_INVALID);
    CHECK(morna_mixture_stats(h, stats) == MORNA_OK);
    for (int i = 0; i < 8; i++) CHECK(stats[i] == 0);
    CHECK(morna_mixture_stats(h, NULL) == MORNA_E_INVALID);
    morna_index *empty = NULL;
    CHECK(morna_index_create(DIM, 0, &empty) == MORNA_OK);
    CHECK(morna_mixture(empty, NULL, NULL, items, 1, label, L, 1e-9, 100, w, info, act) == MORNA_E_EMPTY);
    CHECK(morna_label_centroids(empty, NULL, label, L, sums, counts, gram) == MORNA_E_EMPTY);
    CHECK(morna_index_destroy(empty) == MORNA_OK);
    const int32_t one[1] = {4};
    int32_t ids[3], cnt[1];
    double dist[3];
    CHECK(morna_exact_search_by_item(h, one, 1, 3, ids, dist, cnt) == MORNA_OK);
    CHECK(cnt[0] == 3 && ids[0] == 4 && dist[0] == 0.0);

    CHECK(morna_restriction_free(grouped) == MORNA_OK);
    CHECK(morna_restriction_free(r) == MORNA_OK);
    CHECK(morna_index_destroy(h) == MORNA_OK);
    printf("mixture caller ok\n");
    return 0;
}
