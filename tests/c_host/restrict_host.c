/* A host without Python on the plan side of the restriction (include/stk.h "restriction"): the
 * free vertices of a grid of side^2 squares cut into triangles and refined once, in the
 * hierarchical numbering (the coarse vertices first), their parents table, and its transposed
 * table from stk_transfer_children -- host code of libstk.so, no GPU touched -- checked in the
 * program: ptr starts at 0 and ascends, every list ascends strictly, every entry leads back to
 * a parent pair that names its coarse row with the entry's weight, every parent reference is
 * listed exactly once, an interior coarse row lists 7 rows, and bad arguments are refused with
 * nothing written.  Plain C99:
 *     gcc -std=c99 restrict_host.c -lstk -lm        usage: restrict_host <side> */
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

/* the coarse row of the fine-grid vertex (x, y), both even; -1 on the boundary */
static int32_t coarse_row(int side, int x, int y)
{
    if (x <= 0 || y <= 0 || x >= 2 * side || y >= 2 * side) return -1;
    return (int32_t)((y / 2 - 1) * (side - 1) + (x / 2 - 1));
}

int main(int argc, char **argv)
{
    const int side = argc > 1 ? atoi(argv[1]) : 8;
    REQUIRE(side >= 1 && side <= 2000);
    const int64_t M_c = (int64_t)(side - 1) * (side - 1), M_f = (int64_t)(2 * side - 1) * (2 * side - 1);
    int32_t *parents = malloc(sizeof(int32_t) * 2 * (size_t)(M_f + 1));
    int64_t *ptr = malloc(sizeof(int64_t) * (size_t)(M_c + 1));
    int32_t *entries = malloc(sizeof(int32_t) * (size_t)(2 * M_f + 1));
    char *listed = calloc((size_t)(2 * M_f + 1), 1);
    REQUIRE(parents && ptr && entries && listed);
    /* the coarse vertices first, then the new ones row by row: on a horizontal edge, a vertical
     * one, or the diagonal of a square */
    int64_t at = M_c, references = 0;
    for (int y = 1; y < 2 * side; ++y)
        for (int x = 1; x < 2 * side; ++x) {
            int32_t p0, p1;
            int64_t i;
            if (!(x & 1) && !(y & 1)) {
                i = coarse_row(side, x, y), p0 = p1 = (int32_t)i;
            } else {
                i = at++;
                const int dx = x & 1, dy = y & 1;
                p0 = coarse_row(side, x - dx, y - dy), p1 = coarse_row(side, x + dx, y + dy);
            }
            parents[2 * i] = p0, parents[2 * i + 1] = p1;
            references += p0 == p1 ? (p0 >= 0) : (p0 >= 0) + (p1 >= 0);
        }
    REQUIRE(at == M_f);

    CHECK(stk_transfer_children(M_f, M_c, parents, ptr, entries));
    REQUIRE(ptr[0] == 0 && ptr[M_c] == references);
    int64_t longest = 0;
    for (int64_t j = 0; j < M_c; ++j) {
        REQUIRE(ptr[j + 1] >= ptr[j]);
        if (ptr[j + 1] - ptr[j] > longest) longest = ptr[j + 1] - ptr[j];
        for (int64_t e = ptr[j]; e < ptr[j + 1]; ++e) {
            const int64_t i = entries[e] >> 1;
            const int half = entries[e] & 1;
            REQUIRE(entries[e] >= 0 && i < M_f);
            REQUIRE(e == ptr[j] || entries[e] >> 1 > entries[e - 1] >> 1); /* strictly ascending fine rows */
            const int32_t p0 = parents[2 * i], p1 = parents[2 * i + 1];
            if (half) {
                REQUIRE(p0 != p1 && (p0 == j || p1 == j));
                const int which = p1 == j;
                REQUIRE(!listed[2 * i + which]);
                listed[2 * i + which] = 1;
            } else {
                REQUIRE(p0 == j && p1 == j && i == j && !listed[2 * i]);
                listed[2 * i] = 1;
            }
        }
    }
    /* every reference once: with the count above, none is missing */
    int64_t seen = 0;
    for (int64_t s = 0; s < 2 * M_f; ++s) seen += listed[s];
    REQUIRE(seen == references);
    if (side >= 4) REQUIRE(longest == 7); /* an interior vertex: itself and six edge midpoints */

    /* refusals: the argument is named and nothing is written */
    int64_t small_ptr[3] = {77, 77, 77};
    int32_t small_entries[4] = {77, 77, 77, 77};
    const int32_t bad[4] = {0, 0, 2, 0}, hole[4] = {-1, -1, 0, 0};
    REQUIRE(stk_transfer_children(2, 2, bad, small_ptr, small_entries) != 0 && strstr(stk_last_error(), "parents[1]"));
    REQUIRE(stk_transfer_children(2, 2, hole, small_ptr, small_entries) != 0 &&
            strstr(stk_last_error(), "a copy pair without a row to copy"));
    REQUIRE(stk_transfer_children(-1, 2, bad, small_ptr, small_entries) != 0 && strstr(stk_last_error(), "M_fine"));
    REQUIRE(stk_transfer_children(2, 2, NULL, small_ptr, small_entries) != 0 && strstr(stk_last_error(), "parents is null"));
    REQUIRE(stk_transfer_children(2, 1, bad, NULL, small_entries) != 0);
    REQUIRE(stk_transfer_children((int64_t)STK_RESTRICT_MAX_M_FINE + 1, 1, NULL, small_ptr, small_entries) != 0);
    REQUIRE(small_ptr[0] == 77 && small_ptr[2] == 77 && small_entries[0] == 77 && small_entries[3] == 77);
    /* no fine rows: every coarse row is empty */
    CHECK(stk_transfer_children(0, 2, NULL, small_ptr, NULL));
    REQUIRE(small_ptr[0] == 0 && small_ptr[1] == 0 && small_ptr[2] == 0);

    printf("restrict_host ok: %lld fine rows, %lld coarse rows, %lld entries, the longest list %lld\n", (long long)M_f,
           (long long)M_c, (long long)references, (long long)longest);
    free(parents), free(ptr), free(entries), free(listed);
    return 0;
}
