/* A host without Python on the point-location grid of the sampling engine
 * (include/stk.h "sampling the trial space"): a sheared grid of 2 side^2 triangles, its
 * bucket grid from stk_sample_grid_build / _sizes / _copy / _free -- host code of
 * libstk.so, no GPU touched -- checked in the program: the lists ascend, every triangle is
 * listed in the bin of its centroid and of each vertex, every listed triangle's widened
 * box touches its bin, and bad meshes are refused.  Plain C99:
 *     gcc -std=c99 sample_host.c -lstk -lm        usage: sample_host <side> */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "stk.h"

#define CHECK(call)                                                                   \
    do {                                                                              \
        if ((call) != 0) {                                                            \
            fprintf(stderr, "%s:%d: %s failed: %s\n", __FILE__, __LINE__, #call, stk_last_error()); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)
#define REQUIRE(cond)                                                                 \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond);  \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static int32_t bin_of(double x, double lo, double inv_w, int32_t nb)
{
    const double t = floor((x - lo) * inv_w);
    if (!(t >= 0.0)) return 0;
    if (t >= (double)nb) return nb - 1;
    return (int32_t)t;
}

static int listed(const int32_t *ptr, const int32_t *lst, int64_t bin, int32_t cell)
{
    for (int32_t s = ptr[bin]; s < ptr[bin + 1]; ++s)
        if (lst[s] == cell) return 1;
    return 0;
}

int main(int argc, char **argv)
{
    const int side = argc > 1 ? atoi(argv[1]) : 8;
    REQUIRE(side >= 1 && side <= 2000);
    const int64_t nv = (int64_t)(side + 1) * (side + 1), nt = 2 * (int64_t)side * side;
    double *pts = malloc(sizeof(double) * 2 * nv);
    int64_t *tris = malloc(sizeof(int64_t) * 3 * nt);
    REQUIRE(pts && tris);
    for (int j = 0; j <= side; ++j)
        for (int i = 0; i <= side; ++i) {
            const int64_t v = (int64_t)j * (side + 1) + i;
            pts[2 * v] = -1.0 + (3.0 * i + 0.9 * j) / side; /* sheared: boxes overlap */
            pts[2 * v + 1] = 2.0 * j / side;
        }
    for (int j = 0; j < side; ++j)
        for (int i = 0; i < side; ++i) {
            const int64_t v = (int64_t)j * (side + 1) + i, t = 2 * ((int64_t)j * side + i);
            const int64_t a[6] = {v, v + 1, v + side + 2, v, v + side + 2, v + side + 1};
            for (int k = 0; k < 6; ++k) tris[3 * t + k] = a[k];
        }

    stk_sample_grid *grid = NULL;
    CHECK(stk_sample_grid_build(2, nv, nt, pts, tris, &grid));
    int32_t bins[3];
    double lo[3], inv_w[3], widen;
    int64_t entries = 0;
    CHECK(stk_sample_grid_sizes(grid, bins, lo, inv_w, &widen, &entries));
    const int32_t want = (int32_t)floor(sqrt((double)nt) + 0.5);
    REQUIRE(bins[0] == want && bins[1] == want && bins[2] == 1);
    REQUIRE(fabs(widen - 3.9e-12) < 1e-24); /* the box is 3.9 x 2 */
    REQUIRE(fabs(lo[0] - (-1.0 - widen)) < 1e-15 && fabs(lo[1] - (0.0 - widen)) < 1e-15);
    const int64_t n_bins = (int64_t)bins[0] * bins[1];
    int32_t *ptr = malloc(sizeof(int32_t) * (n_bins + 1)), *lst = malloc(sizeof(int32_t) * (entries ? entries : 1));
    REQUIRE(ptr && lst);
    CHECK(stk_sample_grid_copy(grid, ptr, lst));
    CHECK(stk_sample_grid_free(grid));
    REQUIRE(ptr[0] == 0 && ptr[n_bins] == entries && entries >= nt);

    const double slack = 4.0 * 2.3e-16 * 3.9;
    for (int64_t b = 0; b < n_bins; ++b) {
        REQUIRE(ptr[b] <= ptr[b + 1]);
        const int32_t ix = (int32_t)(b % bins[0]), iy = (int32_t)(b / bins[0]);
        const double blo[2] = {lo[0] + ix / inv_w[0], lo[1] + iy / inv_w[1]};
        const double bhi[2] = {lo[0] + (ix + 1) / inv_w[0], lo[1] + (iy + 1) / inv_w[1]};
        for (int32_t s = ptr[b]; s < ptr[b + 1]; ++s) {
            const int32_t t = lst[s];
            REQUIRE(t >= 0 && t < nt);
            REQUIRE(s == ptr[b] || lst[s - 1] < t); /* ascending */
            for (int k = 0; k < 2; ++k) { /* the widened box touches the bin */
                double cl = pts[2 * tris[3 * t] + k], ch = cl;
                for (int a = 1; a < 3; ++a) {
                    const double x = pts[2 * tris[3 * t + a] + k];
                    cl = x < cl ? x : cl, ch = x > ch ? x : ch;
                }
                REQUIRE(cl - widen <= bhi[k] + slack && ch + widen >= blo[k] - slack);
            }
        }
    }
    for (int64_t t = 0; t < nt; ++t) { /* centroid and vertices */
        double c[2] = {0.0, 0.0};
        for (int a = 0; a < 3; ++a) {
            const double *p = pts + 2 * tris[3 * t + a];
            c[0] += p[0] / 3.0, c[1] += p[1] / 3.0;
            const int64_t b = (int64_t)bin_of(p[1], lo[1], inv_w[1], bins[1]) * bins[0] + bin_of(p[0], lo[0], inv_w[0], bins[0]);
            REQUIRE(listed(ptr, lst, b, (int32_t)t));
        }
        const int64_t b = (int64_t)bin_of(c[1], lo[1], inv_w[1], bins[1]) * bins[0] + bin_of(c[0], lo[0], inv_w[0], bins[0]);
        REQUIRE(listed(ptr, lst, b, (int32_t)t));
    }

    /* refused: a vertex index out of range, a mesh without extent */
    grid = NULL;
    tris[1] = nv;
    REQUIRE(stk_sample_grid_build(2, nv, nt, pts, tris, &grid) != 0 && grid == NULL);
    tris[1] = 1;
    for (int64_t v = 0; v < 2 * nv; ++v) pts[v] = 0.25;
    REQUIRE(stk_sample_grid_build(2, nv, nt, pts, tris, &grid) != 0 && grid == NULL);

    printf("sample_host ok: %lld vertices, %lld triangles, %d x %d bins, %lld list entries\n", (long long)nv,
           (long long)nt, bins[0], bins[1], (long long)entries);
    free(pts), free(tris), free(ptr), free(lst);
    return 0;
}
