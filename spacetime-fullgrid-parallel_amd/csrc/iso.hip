// Isotherms (include/stk.h "isotherms"): per time node of a trial-space slab the pieces of
// the level set {u_h = threshold} -- segments in 2-D, triangles in 3-D -- as records of
// vertices, gradient and cell index.  The faces of the time curves' zone pieces (curves.hip)
// that lie on the level set, from the same cut (curves_plan.h), on the time curves' plan.
//
//  * stk_iso_count   n_cols columns of a slab -> counts [n_cols][n_tiles], pieces per tile
//  * stk_iso_fill    the same columns, with the caller's exclusive prefix `first` of the
//                    counts -> the records, in place
//
// A variable-length result without atomics: tile t is the 256 consecutive cells [256 t,
// 256 t + 256), one lane per cell, and a workgroup takes a tile and a chunk of columns (the
// launch form of curves_cells_kernel).  A row's columns of a chunk are one run of the slab; a
// lane asks for them in groups (8 columns in count, 4 in fill), so a line of the run is
// fetched once.  A lane has 0, 1 or 2 pieces; its rank in the tile
// comes from two ballots per wavefront and the four wavefront totals in LDS.  The caller
// scans the counts (column, then tile), so record i is what it is whatever the grid, the
// chunk and the number of ranks.  `fill` looks at a (column, tile)'s count before it asks for
// a slab row -- on a real isotherm almost every tile is empty -- recomputes the lanes' counts,
// stages the tile's records in LDS, 256 at a time, and stores them as one run, consecutive
// lanes on consecutive doubles.  A record is stored iff its index is in [0, n_out): tables
// that do not belong together can misplace records, never write out of bounds.
//
// ARITHMETIC: every product, quotient and sum rounded on its own -- contraction is SWITCHED
// OFF for this file, curves_plan.h and p1_mesh.h (their pragmas and -ffp-contract=off in the
// Makefile), and no kernel here calls fma.  No square root: the lengths are the caller's.
#include <algorithm>

#include "curves_plan.h"

#pragma clang fp contract(off)

namespace {

constexpr int BS = 256, WAVES = BS / 64;
constexpr int32_t CHUNK_COLS = 16, CHUNK_MAX = 32;
constexpr int64_t GRID_CHUNKS = 32768;  // chunks of columns per launch: the grid's second dimension
constexpr int ROUND = 256;              // records staged at a time
constexpr int GROUP = 8, FILL_GROUP = 4;  // columns of a row asked for together by count and by fill
std::atomic<int32_t> g_chunk_cols{CHUNK_COLS};

constexpr int width(int D) { return D * D + D + 1; }

// pieces of a cell with n vertices above: the table of include/stk.h
template <int D>
__device__ inline int pieces_of(int n)
{
    return n == 0 || n == D + 1 ? 0 : (D == 3 && n == 2 ? 2 : 1);
}

// the slab offsets of a lane's d + 1 rows, -1 on the boundary and for a lane without a cell
template <int D>
__device__ inline void rows_of_cell(bool live, int64_t t, const int32_t *__restrict__ cells,
                                    const int32_t *__restrict__ row_of, int64_t ld, int64_t (&off)[D + 1])
{
#pragma unroll
    for (int a = 0; a <= D; ++a) {
        off[a] = -1;
        if (live) {
            const int32_t row = row_of[cells[(D + 1) * t + a]];
            off[a] = row >= 0 ? (int64_t)row * ld : -1;
        }
    }
}

// The lane's count k and, from two ballots, the pieces of the lanes below it in its wavefront
// and of the whole wavefront.
__device__ inline void wave_rank(int k, int lane, int &below, int &total)
{
    const unsigned long long one = __ballot(k >= 1), two = __ballot(k == 2);
    const unsigned long long lower = lane ? ~0ull >> (64 - lane) : 0ull;
    below = __popcll(one & lower) + __popcll(two & lower);
    total = __popcll(one) + __popcll(two);
}

// grid: (tile, chunk of columns).  LDS: the wavefront totals of every column of the chunk, so
// one barrier serves the chunk.
template <int D>
__global__ __launch_bounds__(BS) void iso_count_kernel(int64_t nc, int64_t n_tiles, int32_t n_cols, int32_t cw,
                                                      const int32_t *__restrict__ cells,
                                                      const int32_t *__restrict__ row_of, const double *__restrict__ u,
                                                      int64_t ld, double theta, int64_t *__restrict__ counts)
{
    __shared__ int wsum[CHUNK_MAX][WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x;
    const int32_t c_first = (int32_t)blockIdx.y * cw;
    const int32_t c_end = c_first + cw < n_cols ? c_first + cw : n_cols;
    const int64_t t = tile * BS + tid;
    const bool live = t < nc;
    int64_t off[D + 1];
    rows_of_cell<D>(live, t, cells, row_of, ld, off);
    // a row's columns of the chunk are one run of the slab: GROUP of them are asked for
    // together, so the run is fetched once while its lines are still near
    for (int32_t c0 = c_first; c0 < c_end; c0 += GROUP) {
        double Ug[GROUP][D + 1];
#pragma unroll
        for (int a = 0; a <= D; ++a)
#pragma unroll
            for (int q = 0; q < GROUP; ++q) Ug[q][a] = off[a] >= 0 && c0 + q < c_end ? u[off[a] + c0 + q] : 0.0;
#pragma unroll
        for (int q = 0; q < GROUP; ++q) {
            if (c0 + q >= c_end) break;  // (the workgroup's)
            const int k = live ? pieces_of<D>(cut_above<D>(Ug[q], theta)) : 0;
            int below, total;
            wave_rank(k, lane, below, total);
            if (lane == 0) wsum[c0 + q - c_first][wave] = total;
        }
    }
    __syncthreads();
    if (tid < c_end - c_first) {
        int64_t sum = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) sum += wsum[tid][w];
        counts[(int64_t)(c_first + tid) * n_tiles + tile] = sum;
    }
}

// One column of a tile: the lanes' counts once more, their ranks in the tile, their records
// through LDS into the run that starts at record `base`.  Every lane of the workgroup calls it.
template <int D>
__device__ inline void fill_column(const double (&U)[D + 1], const double (*P)[D], const double (*g)[D], bool live,
                                   int64_t t, double theta, int tid, double *stage, int *wsum, int64_t base,
                                   int64_t n_out, double *__restrict__ out)
{
    constexpr int W = width(D);
    const int lane = tid & 63, wave = tid >> 6;
    const int n = cut_above<D>(U, theta);
    const int k = live ? pieces_of<D>(n) : 0;
    int below, total;
    wave_rank(k, lane, below, total);
    if (lane == 0) wsum[wave] = total;
    __syncthreads();
    int rank = below, in_tile = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int s = wsum[w];
        rank += w < wave ? s : 0;
        in_tile += s;
    }
    __syncthreads();  // wsum has been read: the next column may write it
    // the lane's records: the vertices of the table of include/stk.h, G and the cell
    pt<D> X[2][D];
    double G[D];
    if (k > 0) {
        const cell_cut<D> q(U, P, theta);
        if constexpr (D == 2) {
            if (n == 1)
                X[0][0] = q.cut(0, 1), X[0][1] = q.cut(0, 2);
            else
                X[0][0] = q.cut(1, 2), X[0][1] = q.cut(0, 2);
            X[1][0] = X[0][0], X[1][1] = X[0][1];  // (never stored: k is 1)
        } else {
            if (n == 1) {
                X[0][0] = q.cut(0, 1), X[0][1] = q.cut(0, 2), X[0][2] = q.cut(0, 3);
                X[1][0] = X[0][0], X[1][1] = X[0][1], X[1][2] = X[0][2];
            } else if (n == 2) {
                X[0][0] = q.cut(0, 2), X[0][1] = q.cut(0, 3), X[0][2] = q.cut(1, 2);
                X[1][0] = X[0][1], X[1][1] = X[0][2], X[1][2] = q.cut(1, 3);
            } else {
                X[0][0] = q.cut(0, 3), X[0][1] = q.cut(1, 3), X[0][2] = q.cut(2, 3);
                X[1][0] = X[0][0], X[1][1] = X[0][1], X[1][2] = X[0][2];
            }
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            G[j] = U[0] * g[0][j];
#pragma unroll
            for (int a = 1; a <= D; ++a) G[j] = G[j] + U[a] * g[a][j];
        }
    }
    for (int r0 = 0; r0 < in_tile; r0 += ROUND) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int at = rank + p - r0;
            if (p < k && at >= 0 && at < ROUND) {
                double *rec = stage + at * W;
#pragma unroll
                for (int r = 0; r < D; ++r)
#pragma unroll
                    for (int j = 0; j < D; ++j) rec[r * D + j] = X[p][r].x[j];
#pragma unroll
                for (int j = 0; j < D; ++j) rec[D * D + j] = G[j];
                rec[D * D + D] = (double)t;
            }
        }
        __syncthreads();
        const int here = (in_tile - r0 < ROUND ? in_tile - r0 : ROUND) * W;
        for (int j = tid; j < here; j += BS) {
            const int rec = j / W;
            const int64_t i = base + r0 + rec;
            if ((uint64_t)i < (uint64_t)n_out) out[i * W + (j - rec * W)] = stage[j];
        }
        __syncthreads();  // the run has left: the next round may stage
    }
}

// grid: (tile, chunk of columns).  LDS: ROUND records and the wavefront totals.
template <int D>
__global__ __launch_bounds__(BS) void iso_fill_kernel(int64_t nc, int64_t n_tiles, int32_t n_cols, int32_t cw,
                                                     const double *__restrict__ pts, const int32_t *__restrict__ cells,
                                                     const int32_t *__restrict__ row_of, const double *__restrict__ grad,
                                                     const double *__restrict__ u, int64_t ld, double theta,
                                                     const int64_t *__restrict__ counts, const int64_t *__restrict__ first,
                                                     int64_t n_out, double *__restrict__ out)
{
    __shared__ double stage[ROUND * width(D)];
    __shared__ int wsum[WAVES];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int32_t c_first = (int32_t)blockIdx.y * cw;
    const int32_t c_end = c_first + cw < n_cols ? c_first + cw : n_cols;
    const int64_t t = tile * BS + tid;
    const bool live = t < nc;
    bool loaded = false;  // (the workgroup's: the cell is read for the first column that has a piece)
    double g[D + 1][D], P[D + 1][D];
    int64_t off[D + 1];
    for (int32_t c0 = c_first; c0 < c_end; c0 += FILL_GROUP) {
        // the columns of the group that have a piece in this tile (the workgroup's): their part
        // of every row's run is asked for together, before any of them is worked on
        bool wanted[FILL_GROUP], any = false;
#pragma unroll
        for (int q = 0; q < FILL_GROUP; ++q) {
            wanted[q] = c0 + q < c_end && counts[(int64_t)(c0 + q) * n_tiles + tile] != 0;
            any = any || wanted[q];
        }
        if (!any) continue;  // before any slab row is asked for
        if (!loaded) {
            loaded = true;
            rows_of_cell<D>(live, t, cells, row_of, ld, off);
#pragma unroll
            for (int a = 0; a <= D; ++a) {
                const int64_t vert = live ? cells[(D + 1) * t + a] : 0;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    g[a][j] = live ? grad[((D + 1) * t + a) * D + j] : 0.0;
                    P[a][j] = live ? pts[D * vert + j] : 0.0;
                }
            }
        }
        double Ug[FILL_GROUP][D + 1];
#pragma unroll
        for (int a = 0; a <= D; ++a)
#pragma unroll
            for (int q = 0; q < FILL_GROUP; ++q) Ug[q][a] = wanted[q] && off[a] >= 0 ? u[off[a] + c0 + q] : 0.0;
        for (int q = 0; q < FILL_GROUP; ++q) {  // (not unrolled: one copy of the column's code)
            bool mine = false;
            double U[D + 1];
#pragma unroll
            for (int p = 0; p < FILL_GROUP; ++p) {  // selects, no indexed access
#pragma unroll
                for (int a = 0; a <= D; ++a) U[a] = p == 0 || p == q ? Ug[p][a] : U[a];
                mine = p == q ? wanted[p] : mine;
            }
            if (!mine) continue;
            const int64_t slot = (int64_t)(c0 + q) * n_tiles + tile;
            fill_column<D>(U, P, g, live, t, theta, tid, stage, wsum, first[slot], n_out, out);
        }
    }
}

int check(const char *who, const stk_curves_plan *plan, int64_t M, int32_t n_cols, const double *slab, int64_t row_stride,
          double threshold, const int64_t *counts)
{
    STK_REQUIRE(plan != nullptr, "%s: plan is null", who);
    STK_REQUIRE(slab != nullptr, "%s: slab is null", who);
    STK_REQUIRE(counts != nullptr, "%s: counts is null", who);
    STK_REQUIRE(n_cols >= 1, "%s: n_cols = %d is below 1", who, n_cols);
    STK_REQUIRE(M == plan->n_free, "%s: M = %lld, the plan has %lld free dofs", who, (long long)M, (long long)plan->n_free);
    STK_REQUIRE(row_stride >= n_cols, "%s: row_stride = %lld is below n_cols = %d", who, (long long)row_stride, n_cols);
    STK_REQUIRE(!std::isnan(threshold), "%s: threshold is NaN", who);
    return 0;
}

}  // namespace

extern "C" int stk_iso_width(int32_t d) { return d == 2 || d == 3 ? width(d) : 0; }

extern "C" int stk_iso_count(void *stream, stk_curves_plan *plan, int64_t M, int32_t n_cols, const double *slab,
                             int64_t row_stride, double threshold, int64_t *counts)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    if (int rc = check("stk_iso_count", plan, M, n_cols, slab, row_stride, threshold, counts)) return rc;
    hipStream_t st = stk_stream(stream);
    if (std::isinf(threshold)) {  // no vertex, or every vertex, is above: no piece
        STK_HIP(hipMemsetAsync(counts, 0, (size_t)n_cols * plan->n_tiles * sizeof(int64_t), st));
        return 0;
    }
    const int32_t cw = g_chunk_cols.load(std::memory_order_relaxed);
    const int64_t batch = GRID_CHUNKS * cw;
    for (int64_t c0 = 0; c0 < n_cols; c0 += batch) {
        const int32_t here = (int32_t)std::min<int64_t>(batch, n_cols - c0);
        const dim3 grid((unsigned)plan->n_tiles, (unsigned)((here + cw - 1) / cw));
#define STK_ISO_LAUNCH(D)                                                                                              \
    hipLaunchKernelGGL(iso_count_kernel<D>, grid, dim3(BS), 0, st, plan->nc, plan->n_tiles, here, cw, plan->mesh.cells, \
                       plan->mesh.row_of, slab + c0, row_stride, threshold, counts + c0 * plan->n_tiles)
        if (plan->d == 2)
            STK_ISO_LAUNCH(2);
        else
            STK_ISO_LAUNCH(3);
#undef STK_ISO_LAUNCH
        STK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int stk_iso_fill(void *stream, stk_curves_plan *plan, int64_t M, int32_t n_cols, const double *slab,
                            int64_t row_stride, double threshold, const int64_t *counts, const int64_t *first,
                            int64_t n_out, double *out)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    if (int rc = check("stk_iso_fill", plan, M, n_cols, slab, row_stride, threshold, counts)) return rc;
    STK_REQUIRE(first != nullptr, "stk_iso_fill: first is null");
    STK_REQUIRE(out != nullptr, "stk_iso_fill: out is null");
    STK_REQUIRE(n_out >= 0, "stk_iso_fill: n_out = %lld is below 0", (long long)n_out);
    if (std::isinf(threshold) || n_out == 0) return 0;  // no piece, or no place for one
    hipStream_t st = stk_stream(stream);
    const int32_t cw = g_chunk_cols.load(std::memory_order_relaxed);
    const int64_t batch = GRID_CHUNKS * cw;
    for (int64_t c0 = 0; c0 < n_cols; c0 += batch) {
        const int32_t here = (int32_t)std::min<int64_t>(batch, n_cols - c0);
        const dim3 grid((unsigned)plan->n_tiles, (unsigned)((here + cw - 1) / cw));
#define STK_ISO_LAUNCH(D)                                                                                             \
    hipLaunchKernelGGL(iso_fill_kernel<D>, grid, dim3(BS), 0, st, plan->nc, plan->n_tiles, here, cw, plan->mesh.points, \
                       plan->mesh.cells, plan->mesh.row_of, plan->grad, slab + c0, row_stride, threshold,              \
                       counts + c0 * plan->n_tiles, first + c0 * plan->n_tiles, n_out, out)
        if (plan->d == 2)
            STK_ISO_LAUNCH(2);
        else
            STK_ISO_LAUNCH(3);
#undef STK_ISO_LAUNCH
        STK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int stk_iso_tile(int32_t cols)
{
    STK_REQUIRE(cols >= 0 && cols <= CHUNK_MAX, "stk_iso_tile: cols = %d not in 0..%d", cols, CHUNK_MAX);
    g_chunk_cols.store(cols ? cols : CHUNK_COLS, std::memory_order_relaxed);
    return 0;
}
