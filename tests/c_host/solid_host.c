/* A host without Python on the plan side of the solidification maps (include/stk.h
 * "solidification maps"): a grid of 2 side^2 triangles whose cells are listed in a scattered
 * order, its Z-curve order from stk_solid_cell_order and the tiles' row lists from
 * stk_solid_tile_rows -- host code of libstk.so, no GPU touched -- checked in the program:
 * the order is a permutation, every list ascends strictly and holds rows only, every
 * position leads back to the row of its vertex, every listed row is used, the ordered cells
 * list fewer rows than the scattered ones, and bad arguments are refused.  Plain C99:
 *     gcc -std=c99 solid_host.c -lstk -lm        usage: solid_host <side> */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

/* the lists of `cells`, checked; returns the number of rows listed or -1 */
static int64_t checked_lists(int64_t nv, int64_t nc, const int64_t *cells, const int32_t *row_of, int64_t n_free)
{
    const int64_t n_tiles = (nc + 255) / 256;
    int32_t *ptr = malloc(sizeof(int32_t) * (size_t)(n_tiles + 1));
    int32_t *rows = malloc(sizeof(int32_t) * (size_t)(3 * nc));
    uint16_t *pos = malloc(sizeof(uint16_t) * (size_t)(3 * nc));
    char *used = malloc((size_t)(3 * nc));
    int64_t listed = -1;
    if (!ptr || !rows || !pos || !used) goto done;
    if (stk_solid_tile_rows(2, nv, nc, cells, row_of, ptr, rows, pos) != 0) goto done;
    if (ptr[0] != 0) goto done;
    memset(used, 0, (size_t)(3 * nc));
    for (int64_t i = 0; i < n_tiles; ++i) {
        const int32_t len = ptr[i + 1] - ptr[i];
        if (len < 0 || len > 768) goto done;
        for (int32_t s = ptr[i]; s < ptr[i + 1]; ++s) {
            if (rows[s] < 0 || rows[s] >= n_free) goto done;
            if (s > ptr[i] && rows[s] <= rows[s - 1]) goto done; /* strictly ascending: distinct */
        }
        const int64_t t1 = 256 * (i + 1) < nc ? 256 * (i + 1) : nc;
        for (int64_t q = 3 * 256 * i; q < 3 * t1; ++q) {
            const int32_t row = row_of[cells[q]];
            if (row < 0) {
                if (pos[q] != 0xFFFF) goto done;
            } else {
                if (pos[q] >= len || rows[ptr[i] + pos[q]] != row) goto done;
                used[ptr[i] + pos[q]] = 1;
            }
        }
    }
    for (int32_t s = 0; s < ptr[n_tiles]; ++s)
        if (!used[s]) goto done;
    listed = ptr[n_tiles];
done:
    free(ptr), free(rows), free(pos), free(used);
    return listed;
}

int main(int argc, char **argv)
{
    const int side = argc > 1 ? atoi(argv[1]) : 16;
    REQUIRE(side >= 1 && side <= 2000);
    const int64_t nv = (int64_t)(side + 1) * (side + 1), nc = 2 * (int64_t)side * side;
    double *pts = malloc(sizeof(double) * 2 * (size_t)nv);
    int64_t *cells = malloc(sizeof(int64_t) * 3 * (size_t)nc), *placed = malloc(sizeof(int64_t) * 3 * (size_t)nc);
    int32_t *row_of = malloc(sizeof(int32_t) * (size_t)nv), *order = malloc(sizeof(int32_t) * (size_t)nc);
    char *seen = calloc((size_t)nc, 1);
    REQUIRE(pts && cells && placed && row_of && order && seen);
    int64_t n_free = 0;
    for (int j = 0; j <= side; ++j)
        for (int i = 0; i <= side; ++i) {
            const int64_t v = (int64_t)j * (side + 1) + i;
            pts[2 * v] = (double)i / side, pts[2 * v + 1] = (double)j / side;
            row_of[v] = i > 0 && i < side && j > 0 && j < side ? (int32_t)n_free++ : -1;
        }
    /* square s goes to the places 2 ((s * stride) mod side^2) and the next: consecutive cells
     * lie far apart, as after a refinement that appends the children level by level */
    const int64_t ns = (int64_t)side * side;
    int64_t stride = ns / 2 + 1;
    for (;; ++stride) { /* coprime with ns */
        int64_t a = stride, b = ns;
        while (b) {
            const int64_t r = a % b;
            a = b, b = r;
        }
        if (a == 1) break;
    }
    for (int64_t s = 0; s < ns; ++s) {
        const int64_t i = s % side, j = s / side, v = j * (side + 1) + i, at = 2 * ((s * stride) % ns);
        const int64_t tri[2][3] = {{v, v + 1, v + side + 2}, {v, v + side + 2, v + side + 1}};
        memcpy(cells + 3 * at, tri, sizeof tri);
    }

    CHECK(stk_solid_cell_order(2, nv, nc, pts, cells, order));
    for (int64_t t = 0; t < nc; ++t) {
        REQUIRE(order[t] >= 0 && order[t] < nc && !seen[order[t]]);
        seen[order[t]] = 1;
        memcpy(placed + 3 * t, cells + 3 * (int64_t)order[t], 3 * sizeof(int64_t));
    }
    const int64_t scattered = checked_lists(nv, nc, cells, row_of, n_free);
    const int64_t ordered = checked_lists(nv, nc, placed, row_of, n_free);
    REQUIRE(scattered >= 0 && ordered >= 0 && ordered <= scattered);
    if (nc >= 4 * 256) REQUIRE(2 * ordered < scattered);

    /* refusals: the argument is named and nothing is written */
    int32_t ptr[2] = {77, 77}, rows[3] = {77, 77, 77};
    uint16_t pos[3] = {77, 77, 77};
    REQUIRE(stk_solid_tile_rows(4, nv, 1, cells, row_of, ptr, rows, pos) != 0 && strstr(stk_last_error(), "d = 4"));
    REQUIRE(stk_solid_tile_rows(2, nv, 1, NULL, row_of, ptr, rows, pos) != 0 && strstr(stk_last_error(), "cells is null"));
    REQUIRE(stk_solid_tile_rows(2, nv, 1, cells, NULL, ptr, rows, pos) != 0 && strstr(stk_last_error(), "row_of is null"));
    REQUIRE(stk_solid_cell_order(2, nv, nc, pts, cells, NULL) != 0 && strstr(stk_last_error(), "order is null"));
    REQUIRE(ptr[0] == 77 && ptr[1] == 77 && rows[0] == 77 && pos[0] == 77);
    REQUIRE(stk_solid_rows(2) == STK_SOLID_ROWS(2) && stk_solid_rows(3) == STK_SOLID_ROWS(3) && stk_solid_rows(1) == 0);

    printf("solid_host ok: %lld cells, %lld free dofs, %lld rows listed in the scattered order, %lld along the Z-curve\n",
           (long long)nc, (long long)n_free, (long long)scattered, (long long)ordered);
    free(pts), free(cells), free(placed), free(row_of), free(order), free(seen);
    return 0;
}
