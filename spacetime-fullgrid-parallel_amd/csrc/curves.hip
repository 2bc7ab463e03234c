// Time curves (include/stk.h "time curves"): per time node of a trial-space slab the
// reductions over SPACE -- the heat content, the squares of the L2 and H1 norms, the outflow
// through the boundary, the hottest free dof, and with a threshold the measure, the first
// moment and the bounding box of the zone {u_h > threshold} -- from one pass over the cells.
// The complement of the history maps (history.hip), which reduce along time per point.
//
//  * stk_curves_boundary_faces  host only: which faces of a cell belong to no other cell,
//                               from a sort of the face keys
//  * stk_curves_plan_create     uploads the mesh and the vertex -> slab-row map, computes |T|
//                               and grad lambda_a per cell (p1_geometry_kernel), uploads the
//                               face masks, owns the workspace of the tile partials
//  * stk_curves_eval            n_cols columns of a slab -> out [rows][n_cols]
//
// Two launches per column batch.  `cells`: a workgroup takes tile i -- the 256 consecutive
// cells [256 i, 256 i + 256), one lane per cell, and the 256 consecutive slab rows of the same
// index for the peak -- and a chunk of columns.  A lane keeps the geometry of its cell in
// registers and gathers its d + 1 slab rows column by column (a row is contiguous in time: the
// chunk is one run of 8 cols bytes per row; the loads of column c + 1 are issued before the
// tree of column c).  Per column the lane's terms go through ONE pairwise tree -- sums add,
// the box takes min / max, the peak the larger value and on a tie the lower row; the terms are
// laid out in LDS, a wavefront takes a row and does the steps inside a wavefront with
// cross-lane moves: two barriers per column -- and leave as one partial per tile in
// work[row][col][tile].  `finish`: one workgroup per (row,
// column) runs the same tree over the tile index.  No atomics: tile i is what it is whatever
// the grid, the chunk and the batch, so every sum has one shape, fixed by nc alone.
//
// ARITHMETIC: every product, quotient and sum rounded on its own -- contraction is SWITCHED
// OFF for this file and for p1_mesh.h (their pragmas and -ffp-contract=off in the Makefile),
// and no kernel here calls fma.
#include <algorithm>

#include "curves_plan.h"

#pragma clang fp contract(off)

namespace {

constexpr int BS = 256;
// the workspace of a plan: the columns of a call are evaluated in batches whose tile partials
// stay at or below this (one column where not even one fits)
constexpr int64_t BATCH_BYTES = 8 << 20;
constexpr int32_t CHUNK_COLS = 8, CHUNK_MAX = 32;
std::atomic<int32_t> g_chunk_cols{CHUNK_COLS};
std::atomic<int64_t> g_batch_bytes{BATCH_BYTES};

constexpr int n_sums(int D) { return STK_CURVES_MOMENT + D; }
constexpr int n_rows(int D) { return STK_CURVES_MOMENT + 3 * D + 2; }

// The tree of a tile: x[j] (+) x[j + s], s = 128, 64, .., 1, over the BS values of a row in
// LDS.  A wavefront takes a row: lane l holds x[l], x[l + 64], x[l + 128], x[l + 192], does the
// steps s = 128 (for j = l and j = l + 64) and s = 64 in registers and the steps s = 32 .. 1 with
// cross-lane moves -- the same pairs in the same order as a walk over LDS with a barrier per
// step, the four wavefronts on four rows at once.  Rows [0, NS) add; peak and peak_row are a
// pair: the larger value, on a tie the lower row; then D rows of minima and D rows of maxima.
// Lane 0 of the wavefront gets the result of row q through put(q, value).
__device__ inline double join_min(double a, double b) { return b < a ? b : a; }
__device__ inline double join_max(double a, double b) { return b > a ? b : a; }

template <int D, class Put>
__device__ inline void tile_tree(const double *red, int tid, Put put)
{
    constexpr int NS = n_sums(D), R = n_rows(D);
    const int lane = tid & 63;
    for (int q = tid >> 6; q < R; q += BS / 64) {  // (q is the wavefront's: no divergence)
        if (q == NS + 1) continue;               // peak_row travels with the peak
        const double *x = red + q * BS;
        const double a0 = x[lane], a1 = x[lane + 64], a2 = x[lane + 128], a3 = x[lane + 192];
        if (q < NS) {
            double z = (a0 + a2) + (a1 + a3);
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) z = z + __shfl_down(z, s);
            if (lane == 0) put(q, z);
        } else if (q == NS) {
            const double *y = red + (NS + 1) * BS;
            double p = a0, r = y[lane];
            const auto join = [&](double pb, double rb) {
                if (pb > p || (pb == p && rb < r)) p = pb, r = rb;
            };
            double p1 = a1, r1 = y[lane + 64];
            join(a2, y[lane + 128]);  // s = 128, j = lane
            if (a3 > p1 || (a3 == p1 && y[lane + 192] < r1)) p1 = a3, r1 = y[lane + 192];  // s = 128, j = lane + 64
            join(p1, r1);             // s = 64
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const double pb = __shfl_down(p, s), rb = __shfl_down(r, s);
                join(pb, rb);
            }
            if (lane == 0) put(NS, p), put(NS + 1, r);
        } else if (q < NS + 2 + D) {
            double z = join_min(join_min(a0, a2), join_min(a1, a3));
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) z = join_min(z, __shfl_down(z, s));
            if (lane == 0) put(q, z);
        } else {
            double z = join_max(join_max(a0, a2), join_max(a1, a3));
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) z = join_max(z, __shfl_down(z, s));
            if (lane == 0) put(q, z);
        }
    }
}

// |det| of the edge vectors x_r - x_0 of a sub-simplex, over d!: the expressions of
// p1_simplex_of and p1_volume (x3 is not read for a triangle)
template <int D>
__device__ inline double sub_volume(const pt<D> &x0, const pt<D> &x1, const pt<D> &x2, const pt<D> &x3)
{
    double e[D][D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        e[0][k] = x1.x[k] - x0.x[k];
        e[1][k] = x2.x[k] - x0.x[k];
        if constexpr (D == 3) e[2][k] = x3.x[k] - x0.x[k];
    }
    if constexpr (D == 2) {
        (void)x3;
        return fabs(e[0][0] * e[1][1] - e[0][1] * e[1][0]) / 2.0;
    } else {
        const double c0 = e[1][1] * e[2][2] - e[1][2] * e[2][1];
        const double c1 = e[1][2] * e[2][0] - e[1][0] * e[2][2];
        const double c2 = e[1][0] * e[2][1] - e[1][1] * e[2][0];
        return fabs((e[0][0] * c0 + e[0][1] * c1) + e[0][2] * c2) / 6.0;
    }
}

// The zone {u_h > theta} of one cell: measure, first moment and box.  The vertices are put in
// the order q_0 .. q_d: those above (U_a > theta, strictly) in ascending a, then the others in
// ascending a; n of them are above.  C(a, b) = q_a + s (q_b - q_a), s = (W_a - theta) /
// (W_a - W_b), is the cut on the edge from an above vertex to one that is not.  The zone is
//   d = 2   n = 1: X = (q0, C01, C02)            the triangle X0 X1 X2
//           n = 2: X = (q0, q1, C12, C02)        X0 X1 X2 and X0 X2 X3
//   d = 3   n = 1: X = (q0, C01, C02, C03)       the tetrahedron X0 X1 X2 X3
//           n = 2: X = (q0, C02, C03, q1, C12, C13)   a prism: X0 X1 X2 X3, X1 X2 X3 X4, X2 X3 X4 X5
//           n = 3: X = (q0, q1, q2, C03, C13, C23)    the same three
//   n = d + 1: the cell itself with its own |T| and its own vertices.
// Every piece adds |piece| >= 0 and |piece| (sum of its vertices) / (d + 1).
template <int D>
__device__ inline void zone_of_cell(const double (&U)[D + 1], const double (*P)[D], double v, double theta,
                                    double &measure, double (&moment)[D], double (&lo)[D], double (&hi)[D])
{
    const int n = cut_above<D>(U, theta);
    measure = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) moment[j] = 0.0, lo[j] = __builtin_inf(), hi[j] = -__builtin_inf();
    if (n == 0) return;
    if (n == D + 1) {
        measure = v;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double s = P[0][j] + P[1][j];
#pragma unroll
            for (int a = 2; a <= D; ++a) s = s + P[a][j];
            moment[j] = (v * s) / (double)(D + 1);
#pragma unroll
            for (int a = 0; a <= D; ++a) {
                if (P[a][j] < lo[j]) lo[j] = P[a][j];
                if (P[a][j] > hi[j]) hi[j] = P[a][j];
            }
        }
        return;
    }
    // the order q_0 .. q_d and the cuts: curves_plan.h, shared with the isotherms
    const cell_cut<D> q(U, P, theta);
    const auto vertex = [&](int a) { return q.vertex(a); };
    const auto cut = [&](int a, int b) { return q.cut(a, b); };
    const auto widen = [&](const pt<D> &x) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (x.x[j] < lo[j]) lo[j] = x.x[j];
            if (x.x[j] > hi[j]) hi[j] = x.x[j];
        }
    };
    const auto piece = [&](const pt<D> &x0, const pt<D> &x1, const pt<D> &x2, const pt<D> &x3) {
        const double m = sub_volume<D>(x0, x1, x2, x3);
        measure = measure + m;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double s = (x0.x[j] + x1.x[j]) + x2.x[j];
            if constexpr (D == 3) s = s + x3.x[j];
            moment[j] = moment[j] + (m * s) / (double)(D + 1);
        }
    };
    if constexpr (D == 2) {
        if (n == 1) {
            const pt<D> x0 = vertex(0), x1 = cut(0, 1), x2 = cut(0, 2);
            widen(x0), widen(x1), widen(x2);
            piece(x0, x1, x2, x0);
        } else {
            const pt<D> x0 = vertex(0), x1 = vertex(1), x2 = cut(1, 2), x3 = cut(0, 2);
            widen(x0), widen(x1), widen(x2), widen(x3);
            piece(x0, x1, x2, x0);
            piece(x0, x2, x3, x0);
        }
    } else {
        if (n == 1) {
            const pt<D> x0 = vertex(0), x1 = cut(0, 1), x2 = cut(0, 2), x3 = cut(0, 3);
            widen(x0), widen(x1), widen(x2), widen(x3);
            piece(x0, x1, x2, x3);
        } else {
            // both prisms: the staircase of three tetrahedra over (x0 x1 x2) -> (x3 x4 x5)
            pt<D> x0 = vertex(0), x1, x2, x3, x4, x5;
            if (n == 2)
                x1 = cut(0, 2), x2 = cut(0, 3), x3 = vertex(1), x4 = cut(1, 2), x5 = cut(1, 3);
            else
                x1 = vertex(1), x2 = vertex(2), x3 = cut(0, 3), x4 = cut(1, 3), x5 = cut(2, 3);
            widen(x0), widen(x1), widen(x2), widen(x3), widen(x4), widen(x5);
            piece(x0, x1, x2, x3);
            piece(x1, x2, x3, x4);
            piece(x2, x3, x4, x5);
        }
    }
}

// LDS: the n_rows(D) BS doubles of the tree.  grid: (tile, chunk of columns)
template <int D>
__global__ __launch_bounds__(BS) void curves_cells_kernel(int64_t nc, int64_t n_tiles, int64_t n_work, int64_t M,
                                                         int32_t n_cols, int32_t cw, const double *__restrict__ pts,
                                                         const int32_t *__restrict__ cells,
                                                         const int32_t *__restrict__ row_of,
                                                         const double *__restrict__ vol,
                                                         const double *__restrict__ grad,
                                                         const uint8_t *__restrict__ faces,
                                                         const double *__restrict__ u, int64_t ld, double theta,
                                                         double *__restrict__ work)
{
    constexpr int NS = n_sums(D), R = n_rows(D);
    __shared__ double red[R * BS];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int32_t c_first = (int32_t)blockIdx.y * cw;
    const int32_t c_end = c_first + cw < n_cols ? c_first + cw : n_cols;
    const int64_t t = tile * BS + tid;
    const bool live = tile < n_tiles && t < nc;  // a cell of mine
    const bool has_row = t < M;                  // a slab row of mine, for the peak
    double v = 0.0, g[D + 1][D], P[D + 1][D];
    int64_t off[D + 1];  // the slab offset of vertex a's row, -1 on the boundary
    int mask = 0;
#pragma unroll
    for (int a = 0; a <= D; ++a) {
        off[a] = -1;
#pragma unroll
        for (int j = 0; j < D; ++j) g[a][j] = 0.0, P[a][j] = 0.0;
    }
    if (live) {
        v = vol[t];
        mask = faces[t];
#pragma unroll
        for (int a = 0; a <= D; ++a) {
            const int32_t vert = cells[(D + 1) * t + a];
            const int32_t row = row_of[vert];
            off[a] = row >= 0 ? (int64_t)row * ld : -1;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                g[a][j] = grad[((D + 1) * t + a) * D + j];
                P[a][j] = pts[D * (int64_t)vert + j];
            }
        }
    }
    const int64_t own = has_row ? t * ld : -1;
    double Un[D + 1], pn = 0.0;  // the column ahead
    auto fetch = [&](int32_t c) {
#pragma unroll
        for (int a = 0; a <= D; ++a) Un[a] = off[a] >= 0 ? u[off[a] + c] : 0.0;
        pn = own >= 0 ? u[own + c] : 0.0;
    };
    if (c_first < c_end) fetch(c_first);
    for (int32_t c = c_first; c < c_end; ++c) {
        double U[D + 1];
#pragma unroll
        for (int a = 0; a <= D; ++a) U[a] = Un[a];
        const double mine = pn;
        if (c + 1 < c_end) fetch(c + 1);
        double term[R];
#pragma unroll
        for (int q = 0; q < R; ++q) term[q] = 0.0;
        term[NS] = -__builtin_inf(), term[NS + 1] = (double)M;
#pragma unroll
        for (int j = 0; j < D; ++j) term[NS + 2 + j] = __builtin_inf(), term[NS + 2 + D + j] = -__builtin_inf();
        if (has_row && mine == mine) term[NS] = mine, term[NS + 1] = (double)t;
        if (live) {
            double S = U[0] + U[1], Q2 = U[0] * U[0] + U[1] * U[1];
#pragma unroll
            for (int a = 2; a <= D; ++a) S = S + U[a], Q2 = Q2 + U[a] * U[a];
            term[STK_CURVES_HEAT] = (v * S) / (double)(D + 1);
            term[STK_CURVES_L2] = (v * (S * S + Q2)) / (double)((D + 1) * (D + 2));
            double G[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                G[j] = U[0] * g[0][j];
#pragma unroll
                for (int a = 1; a <= D; ++a) G[j] = G[j] + U[a] * g[a][j];
            }
            double GG = G[0] * G[0] + G[1] * G[1];
            if constexpr (D == 3) GG = GG + G[2] * G[2];
            term[STK_CURVES_H1] = v * GG;
            double flow = 0.0;
#pragma unroll
            for (int a = 0; a <= D; ++a) {
                double dot = G[0] * g[a][0] + G[1] * g[a][1];
                if constexpr (D == 3) dot = dot + G[2] * g[a][2];
                if (mask >> a & 1) flow = flow + dot;
            }
            term[STK_CURVES_OUTFLOW] = ((double)D * v) * flow;
            double moment[D], lo[D], hi[D];
            zone_of_cell<D>(U, P, v, theta, term[STK_CURVES_MEASURE], moment, lo, hi);
#pragma unroll
            for (int j = 0; j < D; ++j)
                term[STK_CURVES_MOMENT + j] = moment[j], term[NS + 2 + j] = lo[j], term[NS + 2 + D + j] = hi[j];
        }
        __syncthreads();  // the tree of the column before has been read
#pragma unroll
        for (int q = 0; q < R; ++q) red[q * BS + tid] = term[q];
        __syncthreads();
        tile_tree<D>(red, tid, [&](int q, double value) { work[((int64_t)q * n_cols + c) * n_work + tile] = value; });
    }
}

// one workgroup per (row q, column c): partial i and partial i + s for s = P / 2, .., 1.  The
// sums run over the n_tiles cell tiles with P the power of two at or above n_tiles (an absent
// partner adds nothing): the shape of err_finish_kernel.  The peak and the box run over all
// n_work tiles.  In place on the workspace down to BS partials, then in LDS.  An empty box
// (lo = +inf, hi = -inf) leaves as NaN.
template <int D>
__global__ __launch_bounds__(BS) void curves_finish_kernel(int64_t n_tiles, int64_t n_work, int32_t n_cols,
                                                          double *__restrict__ work, int64_t ld_out,
                                                          double *__restrict__ out)
{
    constexpr int NS = n_sums(D), R = n_rows(D);
    __shared__ double red[2 * BS];
    const int tid = threadIdx.x;
    const int q = blockIdx.x, c = blockIdx.y;
    const int kind = q < NS ? 0 : q < NS + 2 ? 1 : q < NS + 2 + D ? 2 : 3;  // sum, peak pair, min, max
    if (q == NS + 1) return;                                                // the pair travels with the peak
    double *w = work + ((int64_t)q * n_cols + c) * n_work;
    double *w2 = work + ((int64_t)(q + 1) * n_cols + c) * n_work;  // peak_row beside peak (kind 1 only)
    const int64_t n = kind == 0 ? n_tiles : n_work;
    int64_t Pw = 1;
    while (Pw < n) Pw <<= 1;
    auto join = [&](double &a, double &ar, double b, double br) {
        if (kind == 0)
            a = a + b;
        else if (kind == 1) {
            if (b > a || (b == a && br < ar)) a = b, ar = br;
        } else if (kind == 2) {
            if (b < a) a = b;
        } else {
            if (b > a) a = b;
        }
    };
    for (int64_t s = Pw / 2; s >= BS; s >>= 1) {
        for (int64_t i = tid; i < s && i + s < n; i += BS) {
            double a = w[i], ar = kind == 1 ? w2[i] : 0.0;
            join(a, ar, w[i + s], kind == 1 ? w2[i + s] : 0.0);
            w[i] = a;
            if (kind == 1) w2[i] = ar;
        }
        __syncthreads();
    }
    const double neutral = kind == 0 ? 0.0 : kind == 2 ? __builtin_inf() : -__builtin_inf();
    red[tid] = tid < n ? w[tid] : neutral;
    red[BS + tid] = kind == 1 && tid < n ? w2[tid] : __builtin_inf();
    for (int s = BS / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) join(red[tid], red[BS + tid], red[tid + s], red[BS + tid + s]);
    }
    __syncthreads();
    if (tid == 0) {
        double r = red[0];
        if ((kind == 2 && r == __builtin_inf()) || (kind == 3 && r == -__builtin_inf())) r = __builtin_nan("");
        out[(int64_t)q * ld_out + c] = r;
        if (kind == 1) out[(int64_t)(q + 1) * ld_out + c] = red[BS];
    }
    (void)R;
}

struct face_key {
    int32_t v[3];  // the face's vertices, ascending; -1 in the last place of an edge
    int32_t slot;  // (d + 1) cell + a
};

inline bool same_face(const face_key &a, const face_key &b)
{
    return a.v[0] == b.v[0] && a.v[1] == b.v[1] && a.v[2] == b.v[2];
}

}  // namespace

extern "C" int stk_curves_rows(int32_t d) { return d == 2 || d == 3 ? n_rows(d) : 0; }

extern "C" int stk_curves_boundary_faces(int32_t d, int64_t nc, const int64_t *cells, uint8_t *mask)
{
    STK_REQUIRE(d == 2 || d == 3, "stk_curves_boundary_faces: d = %d is neither 2 nor 3", d);
    STK_REQUIRE(nc > 0 && (int64_t)(d + 1) * nc < ((int64_t)1 << 31), "stk_curves_boundary_faces: nc = %lld out of range",
                (long long)nc);
    STK_REQUIRE(cells != nullptr, "stk_curves_boundary_faces: cells is null");
    STK_REQUIRE(mask != nullptr, "stk_curves_boundary_faces: mask is null");
    const int64_t ns = (int64_t)(d + 1) * nc;
    for (int64_t q = 0; q < ns; ++q)
        STK_REQUIRE(cells[q] >= 0 && cells[q] < ((int64_t)1 << 31), "stk_curves_boundary_faces: cell %lld names vertex %lld",
                    (long long)(q / (d + 1)), (long long)cells[q]);
    // one key per (cell, a): the other d vertices in ascending order.  Sorted by the vertices
    // and then by the slot -- a total order, so the result is the same on every run -- a face
    // that belongs to exactly one cell is a run of length one.
    std::vector<face_key> keys((size_t)ns);
    for (int64_t t = 0; t < nc; ++t) {
        for (int a = 0; a <= d; ++a) {
            face_key k = {{0, 0, -1}, (int32_t)((d + 1) * t + a)};
            int m = 0;
            for (int b = 0; b <= d; ++b)
                if (b != a) k.v[m++] = (int32_t)cells[(d + 1) * t + b];
            std::sort(k.v, k.v + d);
            keys[(size_t)((d + 1) * t + a)] = k;
        }
    }
    std::sort(keys.begin(), keys.end(), [](const face_key &a, const face_key &b) {
        for (int i = 0; i < 3; ++i)
            if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
        return a.slot < b.slot;
    });
    for (int64_t t = 0; t < nc; ++t) mask[t] = 0;
    for (size_t i = 0; i < keys.size();) {
        size_t j = i + 1;
        while (j < keys.size() && same_face(keys[i], keys[j])) ++j;
        if (j == i + 1) mask[keys[i].slot / (d + 1)] |= (uint8_t)(1u << (keys[i].slot % (d + 1)));
        i = j;
    }
    return 0;
}

extern "C" int stk_curves_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points, const int64_t *cells,
                                      int64_t n_free, const int64_t *free_vertices, stk_curves_plan **out)
{
    const char *who = "stk_curves_plan_create";
    std::vector<int32_t> row_of;
    if (int rc = p1_plan_open(who, d, nv, nc, points, cells, n_free, free_vertices, out, &row_of)) return rc;
    std::vector<uint8_t> faces((size_t)nc);
    if (int rc = stk_curves_boundary_faces(d, nc, cells, faces.data())) return rc;

    stk_curves_plan *p = new stk_curves_plan();
    p->d = d, p->nv = nv, p->nc = nc, p->n_free = n_free;
    p->n_tiles = (nc + BS - 1) / BS;
    const int64_t row_tiles = (n_free + BS - 1) / BS;
    p->n_work = p->n_tiles > row_tiles ? p->n_tiles : row_tiles;  // (below 2^23 by the checks above: one grid takes it)
    const int64_t one_column = (int64_t)n_rows(d) * p->n_work;
    p->work_doubles = std::max(one_column, BATCH_BYTES / 8);
    int rc = p1_mesh_upload(p->dev, &p->mesh, d, nv, nc, points, cells, &row_of);
    if (!rc) rc = !(p->faces = p->dev.upload(faces));
    if (!rc) rc = p1_geometry(who, p->dev, p, &p->vol);
    if (!rc && !(p->work = p->dev.alloc<double>((size_t)p->work_doubles))) rc = p1_no_array(who);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return 0;
}

extern "C" int stk_curves_plan_destroy(stk_curves_plan *plan)
{
    delete plan;
    return 0;
}

extern "C" int stk_curves_eval(void *stream, stk_curves_plan *plan, int64_t M, int32_t n_cols, const double *slab,
                               int64_t row_stride, double threshold, int64_t ld_out, double *out)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan != nullptr, "stk_curves_eval: plan is null");
    STK_REQUIRE(slab != nullptr, "stk_curves_eval: slab is null");
    STK_REQUIRE(out != nullptr, "stk_curves_eval: out is null");
    STK_REQUIRE(n_cols >= 1, "stk_curves_eval: n_cols = %d is below 1", n_cols);
    STK_REQUIRE(M == plan->n_free, "stk_curves_eval: M = %lld, the plan has %lld free dofs", (long long)M,
                (long long)plan->n_free);
    STK_REQUIRE(row_stride >= n_cols, "stk_curves_eval: row_stride = %lld is below n_cols = %d", (long long)row_stride,
                n_cols);
    STK_REQUIRE(!std::isnan(threshold), "stk_curves_eval: threshold is NaN");
    STK_REQUIRE(ld_out >= n_cols, "stk_curves_eval: ld_out = %lld is below n_cols = %d", (long long)ld_out, n_cols);
    hipStream_t st = stk_stream(stream);
    const int32_t R = n_rows(plan->d);
    const int32_t cw = g_chunk_cols.load(std::memory_order_relaxed);
    // the columns of a batch: what the cap holds, a whole number of chunks where it holds one
    int64_t limit = std::min(g_batch_bytes.load(std::memory_order_relaxed) / 8, plan->work_doubles);
    int64_t batch = limit / ((int64_t)R * plan->n_work);
    if (batch < 1) batch = 1;
    if (batch > 32768) batch = 32768;  // the finish grid's second dimension
    if (batch > cw) batch -= batch % cw;
    for (int64_t c0 = 0; c0 < n_cols; c0 += batch) {
        const int32_t here = (int32_t)std::min<int64_t>(batch, n_cols - c0);
        const dim3 grid((unsigned)plan->n_work, (unsigned)((here + cw - 1) / cw));
        const dim3 fgrid((unsigned)R, (unsigned)here);
#define STK_CURVES_LAUNCH(D)                                                                                              \
    hipLaunchKernelGGL(curves_cells_kernel<D>, grid, dim3(BS), 0, st, plan->nc, plan->n_tiles, plan->n_work, M, here, cw,  \
                       plan->mesh.points, plan->mesh.cells, plan->mesh.row_of, plan->vol, plan->grad, plan->faces,         \
                       slab + c0, row_stride, threshold, plan->work);                                                      \
    STK_LAUNCH_CHECK();                                                                                                   \
    hipLaunchKernelGGL(curves_finish_kernel<D>, fgrid, dim3(BS), 0, st, plan->n_tiles, plan->n_work, here, plan->work,     \
                       ld_out, out + c0);                                                                                  \
    STK_LAUNCH_CHECK()
        if (plan->d == 2) {
            STK_CURVES_LAUNCH(2);
        } else {
            STK_CURVES_LAUNCH(3);
        }
#undef STK_CURVES_LAUNCH
    }
    return 0;
}

extern "C" int stk_curves_tile(int32_t cols)
{
    STK_REQUIRE(cols >= 0 && cols <= CHUNK_MAX, "stk_curves_tile: cols = %d not in 0..%d", cols, CHUNK_MAX);
    g_chunk_cols.store(cols ? cols : CHUNK_COLS, std::memory_order_relaxed);
    return 0;
}

extern "C" int stk_curves_batch(int64_t bytes)
{
    STK_REQUIRE(bytes >= 0 && bytes <= BATCH_BYTES, "stk_curves_batch: bytes = %lld not in 0..%lld", (long long)bytes,
                (long long)BATCH_BYTES);
    g_batch_bytes.store(bytes ? bytes : BATCH_BYTES, std::memory_order_relaxed);
    return 0;
}
