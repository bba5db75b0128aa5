/* morna_pca and morna_pca_project from C, against include/morna_hip.h alone: an index of small-integer rows (300 of them, so
 * the sums over rows cross a block edge), the fit with and without centring and under an allow-list, and the coordinates by
 * item and by vector, compared byte for byte with the contract computed here -- the blocked ascending sum,
 * the splitmix64 start, Gram-Schmidt twice, the cyclic Jacobi -- then the statistics and the refusals.  Prints "pca caller ok"
 * and returns 0 when all hold. */
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

#define N 300
#define DIM 6
#define BMAX 5

static float rows[N * DIM];
static double U[N * DIM];   /* the unit rows */
static int skipped[N];

/* BS of term(i, ctx), i < n, over the indices with keep[i] (keep null: all) */
typedef double (*term_fn)(int i, const void *ctx);
static double bs(int n, term_fn term, const void *ctx, const int *keep)
{
    double total = 0.0;
    for (int b0 = 0; b0 < n; b0 += 256) {
        double part = 0.0;
        for (int i = b0; i < n && i < b0 + 256; i++)
            if (!keep || keep[i]) part = part + term(i, ctx);
        total = total + part;
    }
    return total;
}

struct dot {
    const double *a, *b;
    int sa, sb;   /* strides */
};
static double dot_term(int i, const void *ctx)
{
    const struct dot *d = (const struct dot *)ctx;
    return d->a[i * d->sa] * d->b[i * d->sb];
}
static double bs_dot(int n, const double *a, int sa, const double *b, int sb, const int *keep)
{
    const struct dot d = {a, b, sa, sb};
    return bs(n, dot_term, &d, keep);
}
static double one_term(int i, const void *ctx) { return ((const double *)ctx)[i]; }

static uint64_t mix(uint64_t x)
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

/* Q[DIM][b] = Orth(A); 0, or 1 + the column without a direction */
static int orth(const double *A, int b, double *Q)
{
    for (int j = 0; j < b; j++) {
        double a[DIM], r[BMAX];
        for (int z = 0; z < DIM; z++) a[z] = A[z * b + j];
        for (int pass = 0; pass < 2; pass++) {
            for (int k = 0; k < j; k++) r[k] = bs_dot(DIM, Q + k, b, a, 1, NULL);
            for (int k = 0; k < j; k++)
                for (int z = 0; z < DIM; z++) a[z] = a[z] - r[k] * Q[z * b + k];
        }
        const double nn = bs_dot(DIM, a, 1, a, 1, NULL);
        if (!(nn > 0.0 && nn < INFINITY)) return j + 1;
        const double root = sqrt(nn);
        for (int z = 0; z < DIM; z++) Q[z * b + j] = a[z] / root;
    }
    return 0;
}

static void jacobi(double *A, int b, double *theta, double *W)
{
    double R[BMAX * BMAX];
    for (int i = 0; i < b * b; i++) R[i] = 0.0;
    for (int i = 0; i < b; i++) R[i * b + i] = 1.0;
    const double tiny = ldexp(1.0, -54);
    for (int sweep = 0; sweep < 64; sweep++) {
        int rotated = 0;
        for (int p = 0; p + 1 < b; p++)
            for (int q = p + 1; q < b; q++) {
                const double apq = A[p * b + q], app = A[p * b + p], aqq = A[q * b + q];
                if (apq == 0.0 || fabs(apq) <= tiny * (fabs(app) + fabs(aqq))) continue;
                rotated = 1;
                const double tau = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (fabs(tau) + sqrt(1.0 + tau * tau));
                if (tau < 0.0) t = -t;
                const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < b; k++) {
                    const double x = A[k * b + p], y = A[k * b + q];
                    A[k * b + p] = c * x - s * y;
                    A[k * b + q] = s * x + c * y;
                }
                for (int k = 0; k < b; k++) {
                    const double x = A[p * b + k], y = A[q * b + k];
                    A[p * b + k] = c * x - s * y;
                    A[q * b + k] = s * x + c * y;
                }
                A[p * b + q] = 0.0;
                A[q * b + p] = 0.0;
                for (int k = 0; k < b; k++) {
                    const double x = R[k * b + p], y = R[k * b + q];
                    R[k * b + p] = c * x - s * y;
                    R[k * b + q] = s * x + c * y;
                }
            }
        if (!rotated) break;
    }
    int order[BMAX];
    for (int i = 0; i < b; i++) order[i] = i;
    for (int i = 1; i < b; i++)   /* a stable insertion sort, descending */
        for (int j = i; j > 0 && A[order[j] * b + order[j]] > A[order[j - 1] * b + order[j - 1]]; j--) {
            const int t = order[j];
            order[j] = order[j - 1];
            order[j - 1] = t;
        }
    for (int j = 0; j < b; j++) {
        theta[j] = A[order[j] * b + order[j]];
        for (int k = 0; k < b; k++) W[k * b + j] = R[k * b + order[j]];
    }
}

/* the contract; F: the rows fitted.  Returns the iterations */
static int contract(int p, int extra, int center, uint64_t seed, double tol, int max_iter, const int *F, double *axes, double *mu,
                    double *values, double *info)
{
    const int b = p + extra;
    int m = 0;
    for (int i = 0; i < N; i++) m += F[i];
    static double col[N], T[N * BMAX];
    for (int z = 0; z < DIM; z++) {
        for (int i = 0; i < N; i++) col[i] = U[i * DIM + z];
        mu[z] = center ? bs(N, one_term, col, F) / (double)m : 0.0;
    }
    double G[DIM * BMAX], Q[DIM * BMAX], Y[DIM * BMAX], Z[DIM * BMAX], B[BMAX * BMAX], W[BMAX * BMAX], theta[BMAX], prev[BMAX], c[BMAX], S[BMAX];
    const uint64_t base = seed * 0x9E3779B97F4A7C15ull;
    for (int z = 0; z < DIM; z++)
        for (int j = 0; j < b; j++) G[z * b + j] = (double)(mix(base + 64ull * (uint64_t)z + (uint64_t)j) >> 11) * 0x1p-53 - 0.5;
    if (orth(G, b, Q) != 0) return -1;
    int t = 0, converged = 0;
    for (t = 1;; t++) {
        for (int j = 0; j < b; j++) c[j] = bs_dot(DIM, mu, 1, Q + j, b, NULL);
        for (int i = 0; i < N; i++)
            for (int j = 0; j < b; j++) T[i * b + j] = F[i] ? bs_dot(DIM, U + i * DIM, 1, Q + j, b, NULL) - c[j] : 0.0;
        for (int j = 0; j < b; j++) {
            for (int i = 0; i < N; i++) col[i] = T[i * b + j];
            S[j] = bs(N, one_term, col, F);
        }
        for (int z = 0; z < DIM; z++)
            for (int j = 0; j < b; j++) {
                Y[z * b + j] = bs_dot(N, U + z, DIM, T + j, b, F);
                Z[z * b + j] = (Y[z * b + j] - mu[z] * S[j]) / (double)m;
            }
        for (int j = 0; j < b; j++)
            for (int k = j; k < b; k++) B[j * b + k] = B[k * b + j] = bs_dot(DIM, Q + j, b, Z + k, b, NULL);
        memcpy(prev, theta, sizeof prev);
        jacobi(B, b, theta, W);
        if (t >= 2) {
            double worst = 0.0;
            for (int j = 0; j < p; j++) worst = fabs(theta[j] - prev[j]) > worst ? fabs(theta[j] - prev[j]) : worst;
            converged = worst <= tol * theta[0];
        }
        if (converged || t == max_iter) break;
        for (int z = 0; z < DIM; z++)
            for (int j = 0; j < b; j++) {
                double a = 0.0;
                for (int k = 0; k < b; k++) a = a + Z[z * b + k] * W[k * b + j];
                G[z * b + j] = a;
            }
        if (orth(G, b, Q) != 0) return -1;
    }
    for (int j = 0; j < p; j++) {
        double v[DIM];
        int big = 0;
        for (int z = 0; z < DIM; z++) {
            double a = 0.0;
            for (int k = 0; k < b; k++) a = a + Q[z * b + k] * W[k * b + j];
            v[z] = a;
            if (fabs(v[z]) > fabs(v[big])) big = z;
        }
        for (int z = 0; z < DIM; z++) axes[j * DIM + z] = v[big] < 0.0 ? -v[z] : v[z];
        values[j] = theta[j];
    }
    for (int i = 0; i < N; i++) {
        double d[DIM];
        for (int z = 0; z < DIM; z++) d[z] = U[i * DIM + z] - mu[z];
        col[i] = bs_dot(DIM, d, 1, d, 1, NULL);
    }
    info[0] = t, info[1] = converged, info[2] = m, info[3] = bs(N, one_term, col, F) / (double)m;
    return t;
}

/* the coordinates of the unit vector u */
static void place(const double *axes, const double *mu, int p, const double *u, double *out)
{
    for (int j = 0; j < p; j++) out[j] = bs_dot(DIM, u, 1, axes + j * DIM, 1, NULL) - bs_dot(DIM, mu, 1, axes + j * DIM, 1, NULL);
}

int main(void)
{
    uint32_t state = 2018u;
    for (int i = 0; i < N * DIM; i++) {
        state = state * 1664525u + 1013904223u;
        rows[i] = (float)((int)((state >> 16) % 17u) - 8) + (i % DIM == (i / DIM) % 3 ? 6.0f : 0.0f);   /* three loose groups */
    }
    for (int z = 0; z < DIM; z++) rows[3 * DIM + z] = 0.0f;                       /* a zero row: skipped */
    for (int z = 0; z < DIM; z++) rows[5 * DIM + z] = 2.0f * rows[4 * DIM + z];   /* row 5 = 2 * row 4: the same unit row */
    int all[N], even[N];
    for (int i = 0; i < N; i++) {
        double pp = 0.0;
        for (int z = 0; z < DIM; z++) pp = pp + (double)rows[i * DIM + z] * (double)rows[i * DIM + z];
        skipped[i] = !(pp > 0.0 && pp < INFINITY);
        const double s = skipped[i] ? 0.0 : 1.0 / sqrt(pp);
        for (int z = 0; z < DIM; z++) U[i * DIM + z] = (double)rows[i * DIM + z] * s;
        all[i] = !skipped[i];
        even[i] = !skipped[i] && !(i & 1);
    }
    CHECK(skipped[3] && !skipped[4]);

    morna_index *h = NULL;
    CHECK(morna_index_create(DIM, 0, &h) == MORNA_OK);
    CHECK(morna_add_items_f32(h, 0, rows, N) == MORNA_OK);
    uint32_t allow_bits[(N + 31) / 32];
    for (int w = 0; w < (N + 31) / 32; w++) allow_bits[w] = 0x55555555u;
    morna_restriction *r = NULL;
    CHECK(morna_restriction_create(h, allow_bits, NULL, &r) == MORNA_OK);

    double axes[BMAX * DIM], mean[DIM], values[BMAX], info[4], stats[8];
    double want_axes[BMAX * DIM], want_mean[DIM], want_values[BMAX], want_info[4];
    /* p, extra, center, seed, max_iter, allow-list */
    const int cases[6][6] = {{2, 2, 1, 0, 1, 0}, {2, 2, 1, 0, 2, 0}, {2, 3, 1, 7, 200, 0}, {3, 0, 0, 1, 5, 0}, {1, 1, 1, 2, 3, 1}, {2, 1, 0, 3, 200, 1}};
    for (int m = 0; m < 6; m++) {
        const int p = cases[m][0], extra = cases[m][1], center = cases[m][2], max_iter = cases[m][4];
        const uint64_t seed = (uint64_t)cases[m][3];
        const int t = contract(p, extra, center, seed, 1e-9, max_iter, cases[m][5] ? even : all, want_axes, want_mean, want_values, want_info);
        CHECK(t >= 1);
        CHECK(morna_pca(h, cases[m][5] ? r : NULL, p, extra, center, seed, 1e-9, max_iter, axes, mean, values, info) == MORNA_OK);
        CHECK(memcmp(info, want_info, sizeof info) == 0);
        CHECK(memcmp(mean, want_mean, sizeof mean) == 0);
        CHECK(memcmp(values, want_values, sizeof(double) * (size_t)p) == 0);
        CHECK(memcmp(axes, want_axes, sizeof(double) * (size_t)p * DIM) == 0);
        CHECK(morna_pca_stats(h, stats) == MORNA_OK);
        CHECK(stats[0] > 0 && stats[1] > 0 && stats[2] > 0 && stats[3] > 0 && stats[5] == t && stats[6] == want_info[2]);
        CHECK(stats[7] == 4.0 * DIM * (N + want_info[2] * (2.0 + 2.0 * t)));
        if (max_iter == 200) CHECK(info[1] == 1.0 && t > 2 && t < 200);
        if (!center) CHECK(mean[0] == 0.0 && mean[DIM - 1] == 0.0);
    }
    CHECK(want_info[2] == 150.0);   /* the even rows, all with a direction: the zero row is odd */

    /* coordinates on the last axes: by item (rows the allow-list left out too), by vector, the zero row */
    const int32_t items[5] = {0, 1, 3, 4, 5};
    double coords[5 * 2], want[2], vecs[2 * DIM];
    CHECK(morna_pca_project(h, axes, mean, 2, NULL, items, 5, coords) == MORNA_OK);
    for (int q = 0; q < 5; q++) {
        if (items[q] == 3) {
            CHECK(coords[q * 2] != coords[q * 2] && coords[q * 2 + 1] != coords[q * 2 + 1]);
            continue;
        }
        place(axes, mean, 2, U + items[q] * DIM, want);
        CHECK(memcmp(coords + q * 2, want, sizeof want) == 0);
    }
    CHECK(memcmp(coords + 3 * 2, coords + 4 * 2, sizeof want) == 0);
    for (int z = 0; z < DIM; z++) vecs[z] = (double)rows[4 * DIM + z], vecs[DIM + z] = 3.0 * (double)rows[9 * DIM + z];
    CHECK(morna_pca_project(h, axes, mean, 2, vecs, NULL, 2, coords + 6) == MORNA_OK);
    CHECK(memcmp(coords + 6, coords + 3 * 2, sizeof want) == 0);

    /* refusals; the statistics are cleared */
    int32_t group[N];
    for (int i = 0; i < N; i++) group[i] = i < 10 ? 0 : -1;
    morna_restriction *grouped = NULL;
    CHECK(morna_restriction_create(h, NULL, group, &grouped) == MORNA_OK);
    CHECK(morna_pca(h, grouped, 2, 2, 1, 0, 1e-9, 5, axes, mean, values, info) == MORNA_E_INVALID);
    CHECK(morna_pca(h, NULL, 0, 2, 1, 0, 1e-9, 5, axes, mean, values, info) == MORNA_E_INVALID);
    CHECK(morna_pca(h, NULL, MORNA_PCA_MAX_COMPONENTS + 1, 0, 1, 0, 1e-9, 5, axes, mean, values, info) == MORNA_E_INVALID);
    CHECK(morna_pca(h, NULL, 2, MORNA_PCA_MAX_BLOCK - 1, 1, 0, 1e-9, 5, axes, mean, values, info) == MORNA_E_INVALID);
    CHECK(morna_pca(h, NULL, 2, DIM - 1, 1, 0, 1e-9, 5, axes, mean, values, info) == MORNA_E_INVALID);   /* b = dim + 1 */
    CHECK(morna_pca(h, NULL, 2, 2, 1, 0, -1.0, 5, axes, mean, values, info) == MORNA_E_INVALID);
    CHECK(morna_pca(h, NULL, 2, 2, 1, 0, 1e-9, 0, axes, mean, values, info) == MORNA_E_INVALID);
    CHECK(morna_pca(h, NULL, 2, 2, 1, 0, 1e-9, 5, NULL, mean, values, info) == MORNA_E_INVALID);
    CHECK(morna_pca(NULL, NULL, 2, 2, 1, 0, 1e-9, 5, axes, mean, values, info) == MORNA_E_INVALID);
    CHECK(morna_pca_stats(h, stats) == MORNA_OK);
    for (int i = 0; i < 8; i++) CHECK(stats[i] == 0);
    CHECK(morna_pca_stats(h, NULL) == MORNA_E_INVALID);
    const int32_t outside[1] = {N};
    CHECK(morna_pca_project(h, want_axes, want_mean, 2, NULL, outside, 1, coords) == MORNA_E_RANGE);
    CHECK(morna_pca_project(h, want_axes, want_mean, 2, vecs, items, 2, coords) == MORNA_E_INVALID);
    CHECK(morna_pca_project(h, want_axes, want_mean, 2, NULL, NULL, 2, coords) == MORNA_E_INVALID);
    want_axes[DIM + 1] = INFINITY;
    CHECK(morna_pca_project(h, want_axes, want_mean, 2, NULL, items, 5, coords) == MORNA_E_INVALID);
    want_axes[DIM + 1] = 0.0;
    want_mean[2] = NAN;
    CHECK(morna_pca_project(h, want_axes, want_mean, 2, NULL, items, 5, coords) == MORNA_E_INVALID);
    morna_index *empty = NULL;
    CHECK(morna_index_create(DIM, 0, &empty) == MORNA_OK);
    CHECK(morna_pca(empty, NULL, 2, 2, 1, 0, 1e-9, 5, axes, mean, values, info) == MORNA_E_EMPTY);
    CHECK(morna_index_destroy(empty) == MORNA_OK);

    CHECK(morna_restriction_free(grouped) == MORNA_OK);
    CHECK(morna_restriction_free(r) == MORNA_OK);
    CHECK(morna_index_destroy(h) == MORNA_OK);
    printf("pca caller ok\n");
    return 0;
}
