// The evaluation operator of the trial space (include/stk.h "sampling the trial space"):
// u_h(t_k, x_p) of a slab of nodal values for arbitrary points of a simplicial P1 mesh
// and arbitrary times -- rasters, probes and line cuts without downloading the slab.
//
//  * stk_sample_grid_build  HOST: a uniform bucket grid over the bounding box, every cell
//                           listed (CSR, ascending) in every bin its widened box touches.
//                           On the host threads of the library; no GPU touched.
//  * stk_sample_plan_create uploads the mesh, the vertex -> slab-row map and that grid
//  * stk_sample_locate      one lane per point: the cells of the point's bin, barycentric
//                           coordinates by the signed-area / cofactor expressions
//                           (p1_barycentric, p1_mesh.h), the cell with the largest smallest
//                           coordinate
//  * stk_sample_eval        out[k][p] = w0 s_p(c0) + w1 s_p(c1) with the spatial sums
//                           s_p(c) = ((l0 u[v0][c] + l1 u[v1][c]) + l2 u[v2][c]) [+ ...]
//  * stk_sample_pairs       paired requests (t_p, x_p): one lane per point, u_h, its time
//                           derivative and its gradient from 2 (d + 1) slab entries
//  * stk_sample_grad_coeffs the gradients of the barycentric coordinates (p1_gradients,
//                           p1_mesh.h) per located point:
//                           as `lam` of stk_sample_eval they give the blocks of the gradient
//  * stk_sample_pairs_adjoint  E^T of the pairs: numbers at (t_p, x_p) onto the slab, as
//                           store, stable sort by destination (sample_adj_sort.hip) and one
//                           summing pass -- no float atomics, one order per entry
//
// THE EVAL KERNEL.  A slab row is contiguous in time and a point needs d + 1 whole rows, so
// the pass is a row gather, and its output is time-major: points x times turned through
// LDS.  A workgroup takes 64 consecutive points.  Pass 1 walks (point, needed column) with
// the column on neighbouring lanes -- a wavefront reads its rows in whole lines, every
// needed entry of a row once per call -- and leaves s_p(c) in an LDS tile
// [point][column] (odd row length: pass 2's column reads are conflict-free).  Pass 2
// walks (request, point) with the point on neighbouring lanes: a wavefront is one request,
// reads its two columns of the tile and stores 512 contiguous bytes of out.  The spatial
// sum does not depend on the request, so it is formed once per column however many
// requests read it.  No atomics; every sum has one owner and one order.
//
// ARITHMETIC: every product and every sum rounded on its own -- contraction is SWITCHED
// OFF for this file and for p1_mesh.h (their pragmas and -ffp-contract=off in the Makefile), as
// for the load engine, and no kernel here calls fma.
#include <algorithm>

#include "host_threads.h"
#include "p1_mesh.h"
#include "sample_adj_sort.h"

#pragma clang fp contract(off)

struct stk_sample_grid {
    int32_t d;
    int32_t nb[3];
    double lo[3], inv_w[3];  // bin of x along k: floor((x - lo[k]) * inv_w[k]), clamped
    double widen;
    std::vector<int32_t> bin_ptr, bin_cells;
};

namespace {

constexpr int BS = 256;
constexpr int TP = 64;         // points of an eval tile = one wavefront of pass 2
constexpr int UNROLL = 4;      // steps of pass 1 whose loads are in flight together
constexpr int MAX_COLS = 96;   // distinct columns of one launch: the tile stays below 50 KB
constexpr double INSIDE = -1e-12;

struct grid_desc {
    int32_t nb[3];
    double lo[3], inv_w[3];
};

// The bin of a coordinate: the SAME expression files the cells (host) and looks the points
// up (device); it is monotone in x, so a point between two corners of a box lands between
// their bins whatever the rounding.
__host__ __device__ inline int32_t bin_of(double x, double lo, double inv_w, int32_t nb)
{
    const double t = floor((x - lo) * inv_w);
    if (!(t >= 0.0)) return 0;  // below the box, or not a number
    if (t >= (double)nb) return nb - 1;
    return (int32_t)t;
}

// one lane per point
template <int D>
__global__ __launch_bounds__(BS) void sample_locate_kernel(int64_t n_p, const double *__restrict__ x, grid_desc g,
                                                           const int32_t *__restrict__ bin_ptr,
                                                           const int32_t *__restrict__ bin_cells,
                                                           const double *__restrict__ pts,
                                                           const int32_t *__restrict__ cells, int32_t *__restrict__ cell_out,
                                                           double *__restrict__ lam_out)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t p = (int64_t)blockIdx.x * BS + threadIdx.x; p < n_p; p += stride) {
        double xp[D];
        int64_t bin = 0;
#pragma unroll
        for (int k = D - 1; k >= 0; --k) {
            xp[k] = x[k * n_p + p];
            bin = bin * g.nb[k] + bin_of(xp[k], g.lo[k], g.inv_w[k], g.nb[k]);
        }
        const double nan = __builtin_nan("");
        double best = -__builtin_inf(), lb[D + 1];
        int32_t cb = -1;
#pragma unroll
        for (int a = 0; a <= D; ++a) lb[a] = nan;
        const int32_t begin = bin_ptr[bin], end = bin_ptr[bin + 1];
        for (int32_t s = begin; s < end; ++s) {  // ascending cells: `>` keeps the lowest on a tie
            const int32_t t = bin_cells[s];
            double l[D + 1];
            p1_barycentric(p1_simplex_of<D>(pts, cells + (D + 1) * (int64_t)t), xp, l);
            double m = l[0];
#pragma unroll
            for (int a = 1; a <= D; ++a) m = l[a] < m ? l[a] : m;
            bool any_nan = false;
#pragma unroll
            for (int a = 0; a <= D; ++a) any_nan = any_nan || l[a] != l[a];
            if (!any_nan && m > best) {
                best = m, cb = t;
#pragma unroll
                for (int a = 0; a <= D; ++a) lb[a] = l[a];
            }
        }
        cell_out[p] = best >= INSIDE ? cb : -1;
#pragma unroll
        for (int a = 0; a <= D; ++a) lam_out[(D + 1) * p + a] = lb[a];
    }
}

// LDS of the eval kernel: the tile [TP][stride] of spatial sums, then per point its
// coordinates [TP][D + 1] and slab rows [TP][D + 1] (-1 = boundary vertex, -2 = outside)
template <int D>
__global__ __launch_bounds__(BS) void sample_eval_kernel(int64_t n_p, int64_t nc, const int32_t *__restrict__ cell,
                                                         const double *__restrict__ lam,
                                                         const int32_t *__restrict__ cells,
                                                         const int32_t *__restrict__ row_of, int32_t ld,
                                                         const double *__restrict__ u, int32_t n_c,
                                                         const int32_t *__restrict__ cols, int32_t n_k,
                                                         const int32_t *__restrict__ req_col,
                                                         const double *__restrict__ req_w, int64_t ld_out,
                                                         double *__restrict__ out)
{
    extern __shared__ double lds[];
    const int stride = n_c | 1;
    double *tile = lds;
    double *pl = lds + TP * stride;
    int32_t *pr = reinterpret_cast<int32_t *>(pl + TP * (D + 1));
    const int tid = threadIdx.x;
    const int64_t n_tiles = (n_p + TP - 1) / TP;
    for (int64_t tile_id = blockIdx.x; tile_id < n_tiles; tile_id += gridDim.x) {
        const int64_t p0 = tile_id * TP;
        const int here = (int)(n_p - p0 < TP ? n_p - p0 : TP);
        if (tid < here) {
            const int32_t t = cell[p0 + tid];
#pragma unroll
            for (int a = 0; a <= D; ++a) {
                pl[tid * (D + 1) + a] = lam[(D + 1) * (p0 + tid) + a];
                pr[tid * (D + 1) + a] = t < 0 || t >= nc ? -2 : row_of[cells[(D + 1) * (int64_t)t + a]];
            }
        }
        __syncthreads();
        // pass 1: (point, column), the column on neighbouring lanes; the loads of UNROLL
        // steps are issued before the first sum needs one (a step alone waits out a whole
        // memory round trip per (d + 1) loads)
        const int total = here * n_c;
        for (int base = tid; base < total; base += BS * UNROLL) {
            double v[UNROLL][D + 1], l[UNROLL][D + 1];
            int at[UNROLL];
#pragma unroll
            for (int s = 0; s < UNROLL; ++s) {
                const int idx = base + s * BS;
                at[s] = -1;
                if (idx < total) {
                    const int p = idx / n_c, j = idx - p * n_c;
                    if (pr[p * (D + 1)] != -2) {
                        at[s] = p * stride + j;
                        const int32_t c = cols[j];
#pragma unroll
                        for (int a = 0; a <= D; ++a) {
                            const int32_t r = pr[p * (D + 1) + a];
                            l[s][a] = pl[p * (D + 1) + a];
                            v[s][a] = r >= 0 ? u[(int64_t)r * ld + c] : 0.0;
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < UNROLL; ++s) {
                if (at[s] < 0) continue;
                double sum = l[s][0] * v[s][0];
#pragma unroll
                for (int a = 1; a <= D; ++a) sum = sum + l[s][a] * v[s][a];
                tile[at[s]] = sum;
            }
        }
        __syncthreads();
        // pass 2: (request, point), the point on neighbouring lanes
        for (int idx = tid; idx < n_k * TP; idx += BS) {
            const int k = idx / TP, p = idx % TP;
            if (p >= here) continue;
            double v;
            if (pr[p * (D + 1)] == -2) {
                v = __builtin_nan("");
            } else {
                const int32_t j0 = req_col[2 * k], j1 = req_col[2 * k + 1];
                const double a0 = j0 >= 0 ? req_w[2 * k] * tile[p * stride + j0] : 0.0;
                const double a1 = j1 >= 0 ? req_w[2 * k + 1] * tile[p * stride + j1] : 0.0;
                v = a0 + a1;
            }
            out[(int64_t)k * ld_out + p0 + p] = v;
        }
        __syncthreads();
    }
}

// one lane per point: out [D][n_p][D + 1], the coefficients stk_sample_eval takes as `lam`
template <int D>
__global__ __launch_bounds__(BS) void sample_grad_coeffs_kernel(int64_t n_p, int64_t nc, const int32_t *__restrict__ cell,
                                                                const double *__restrict__ pts,
                                                                const int32_t *__restrict__ cells,
                                                                double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t p = (int64_t)blockIdx.x * BS + threadIdx.x; p < n_p; p += stride) {
        const int32_t t = cell[p];
        double G[D + 1][D];
        if (t >= 0 && t < nc) {
            int32_t v[D + 1];
#pragma unroll
            for (int a = 0; a <= D; ++a) v[a] = cells[(D + 1) * (int64_t)t + a];
            p1_gradients(p1_simplex_of<D>(pts, v), G);
        } else {
#pragma unroll
            for (int a = 0; a <= D; ++a)
#pragma unroll
                for (int j = 0; j < D; ++j) G[a][j] = __builtin_nan("");
        }
#pragma unroll
        for (int j = 0; j < D; ++j)
#pragma unroll
            for (int a = 0; a <= D; ++a) out[((int64_t)j * n_p + p) * (D + 1) + a] = G[a][j];
    }
}

template <int D>
__device__ inline double spatial_sum(const double *k, const double *v)
{
    double sum = k[0] * v[0];
#pragma unroll
    for (int a = 1; a <= D; ++a) sum = sum + k[a] * v[a];
    return sum;
}

// THE PAIRS KERNEL: one lane per (t_p, x_p).  A point reads 2 (D + 1) slab entries -- the
// two time columns of its D + 1 rows -- and nothing is shared between points, so there are
// no tiles and no LDS.  All addresses are formed first and all loads issued before the
// first sum: an absent column's address is replaced by the present one's and a boundary
// vertex's row by row 0 (both values are then dropped), so no load sits behind a branch of
// its own.  WIDE (even ld, 16-byte aligned slab): where both columns are present and the
// first is even, the two adjacent doubles of a row come in one 16-byte load.  Every field
// row of out is stored coalesced.
template <int D, bool WIDE>
__global__ __launch_bounds__(BS) void sample_pairs_kernel(int64_t n_p, int64_t nc, const int32_t *__restrict__ cell,
                                                          const double *__restrict__ lam, const double *__restrict__ t,
                                                          double h, double t_last, int32_t N, int32_t t_begin,
                                                          int32_t n_loc, int32_t ld, const double *__restrict__ u,
                                                          const double *__restrict__ pts,
                                                          const int32_t *__restrict__ cells,
                                                          const int32_t *__restrict__ row_of, int32_t fields,
                                                          int64_t ld_out, double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    const bool want_u = fields & 1, want_dt = fields & 2, want_grad = fields & 4;
    for (int64_t p = (int64_t)blockIdx.x * BS + threadIdx.x; p < n_p; p += stride) {
        const int32_t tc = cell[p];
        const double tp = t[p];
        const double nan = __builtin_nan("");
        double val_u = nan, val_dt = nan, val_g[D];
#pragma unroll
        for (int j = 0; j < D; ++j) val_g[j] = nan;
        if (tc >= 0 && tc < nc && tp >= 0.0 && tp <= t_last) {  // a NaN time fails both comparisons
            const auto [w0, w1, c0, c1, have0, have1] = p1_time_bracket(tp, h, N, t_begin, n_loc);
            int32_t v[D + 1], r[D + 1];
#pragma unroll
            for (int a = 0; a <= D; ++a) v[a] = cells[(D + 1) * (int64_t)tc + a];
#pragma unroll
            for (int a = 0; a <= D; ++a) r[a] = row_of[v[a]];
            double l[D + 1], G[D + 1][D], u0[D + 1], u1[D + 1];
#pragma unroll
            for (int a = 0; a <= D; ++a) l[a] = lam[(D + 1) * p + a], u0[a] = u1[a] = 0.0;
            if (have0 || have1) {
                const double *row[D + 1];
#pragma unroll
                for (int a = 0; a <= D; ++a) row[a] = u + (int64_t)(r[a] < 0 ? 0 : r[a]) * ld;
                if (WIDE && have0 && have1 && !(c0 & 1)) {
#pragma unroll
                    for (int a = 0; a <= D; ++a) {
                        const double2 w = *reinterpret_cast<const double2 *>(row[a] + c0);
                        u0[a] = w.x, u1[a] = w.y;
                    }
                } else {
                    const int64_t ca = have0 ? c0 : c1, cb = have1 ? c1 : c0;
#pragma unroll
                    for (int a = 0; a <= D; ++a) u0[a] = row[a][ca], u1[a] = row[a][cb];
                }
#pragma unroll
                for (int a = 0; a <= D; ++a)
                    if (r[a] < 0) u0[a] = u1[a] = 0.0;
            }
            if (want_grad) p1_gradients(p1_simplex_of<D>(pts, v), G);
            if (want_u || want_dt) {
                const double s0 = spatial_sum<D>(l, u0), s1 = spatial_sum<D>(l, u1);
                const double a0 = have0 ? w0 * s0 : 0.0, a1 = have1 ? w1 * s1 : 0.0;
                val_u = a0 + a1;
                const double d0 = have0 ? -(s0 / h) : 0.0, d1 = have1 ? s1 / h : 0.0;
                val_dt = d0 + d1;
            }
            if (want_grad) {
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    double k[D + 1];
#pragma unroll
                    for (int a = 0; a <= D; ++a) k[a] = G[a][j];
                    const double a0 = have0 ? w0 * spatial_sum<D>(k, u0) : 0.0;
                    const double a1 = have1 ? w1 * spatial_sum<D>(k, u1) : 0.0;
                    val_g[j] = a0 + a1;
                }
            }
        }
        int64_t at = p;
        if (want_u) out[at] = val_u, at += ld_out;
        if (want_dt) out[at] = val_dt, at += ld_out;
        if (want_grad) {
#pragma unroll
            for (int j = 0; j < D; ++j) out[at + j * ld_out] = val_g[j];
        }
    }
}

// ---- the adjoint of the pairs kernel: store, group, sum -----------------------------------
// E^T w as the store-and-sum form of a scatter-add: no float atomics, one fixed order per
// entry.  (1) One lane per point writes its 2 (D + 1) records (destination key, term) at
// p K + a (D + 1) + b, K = 2 (D + 1): ascending p, then a, then b.  The key of a kept term is
// row n_loc + column (64-bit); a dropped term -- an unused point, a column of another rank,
// a boundary vertex -- gets the key M n_loc, one past the last entry, and sorts behind them
// all.  (2) A stable sort by key (sample_adj_sort.hip) makes every entry's terms a run in
// that order.  (3) The run is cut into chunks of STK_SAMPLE_ADJ_CHUNK terms from its start;
// the lane AT the first record of a chunk sums it from the left.  A run of one chunk is
// stored at once; the chunk sums of a longer one are parked on the chunk's first record and
// added from the left, by the lane at the run's start, in a second launch.  Which lane sums
// what depends on the sorted records alone, never on the launch shape.
constexpr int ADJ_CHUNK = STK_SAMPLE_ADJ_CHUNK;

template <int D>
__global__ __launch_bounds__(BS) void sample_adj_records_kernel(
    int64_t n_p, int64_t nc, const int32_t *__restrict__ cell, const double *__restrict__ lam, const double *__restrict__ t,
    double h, double t_last, int32_t N, int32_t t_begin, int32_t n_loc, uint64_t none, const double *__restrict__ w,
    int64_t ld_w, int32_t field, const double *__restrict__ pts, const int32_t *__restrict__ cells,
    const int32_t *__restrict__ row_of, uint64_t *__restrict__ keys, double *__restrict__ vals,
    unsigned char *__restrict__ used)
{
    constexpr int K = 2 * (D + 1);
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t p = (int64_t)blockIdx.x * BS + threadIdx.x; p < n_p; p += stride) {
        const int32_t tc = cell[p];
        const double tp = t[p];
        const bool ok = tc >= 0 && tc < nc && tp >= 0.0 && tp <= t_last;  // a NaN time fails both comparisons
        uint64_t key[K];
        double term[K];
#pragma unroll
        for (int k = 0; k < K; ++k) key[k] = none, term[k] = 0.0;
        if (ok) {
            const auto [w0, w1, c0, c1, have0, have1] = p1_time_bracket(tp, h, N, t_begin, n_loc);
            int32_t v[D + 1];
#pragma unroll
            for (int b = 0; b <= D; ++b) v[b] = cells[(D + 1) * (int64_t)tc + b];
            if (field == 4) {
                double G[D + 1][D], wj[D];
                p1_gradients(p1_simplex_of<D>(pts, v), G);
#pragma unroll
                for (int j = 0; j < D; ++j) wj[j] = w[j * ld_w + p];
#pragma unroll
                for (int b = 0; b <= D; ++b) {
                    double q = wj[0] * G[b][0];
#pragma unroll
                    for (int j = 1; j < D; ++j) q = q + wj[j] * G[b][j];
                    term[b] = w0 * q, term[D + 1 + b] = w1 * q;
                }
            } else {
                const double wp = w[p];
                double k0, k1;
                if (field == 1) {
                    k0 = wp * w0, k1 = wp * w1;
                } else {
                    k1 = wp / h, k0 = -k1;
                }
#pragma unroll
                for (int b = 0; b <= D; ++b) {
                    const double l = lam[(D + 1) * p + b];
                    term[b] = k0 * l, term[D + 1 + b] = k1 * l;
                }
            }
#pragma unroll
            for (int b = 0; b <= D; ++b) {
                const int32_t r = row_of[v[b]];
                if (r >= 0 && have0) key[b] = (uint64_t)r * (uint64_t)n_loc + (uint64_t)c0;
                if (r >= 0 && have1) key[D + 1 + b] = (uint64_t)r * (uint64_t)n_loc + (uint64_t)c1;
            }
        }
        used[p] = ok ? 1 : 0;
#pragma unroll
        for (int k = 0; k < K; ++k) keys[K * p + k] = key[k], vals[K * p + k] = term[k];
    }
}

// every valid column +0.0; the padding column of an odd n_loc is not touched
__global__ __launch_bounds__(BS) void sample_adj_zero_kernel(int64_t entries, int32_t n_loc, int32_t ld,
                                                             double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < entries; i += stride) {
        const int64_t row = i / n_loc;
        out[row * ld + (i - row * n_loc)] = 0.0;
    }
}

__device__ inline void adj_store(uint64_t key, double sum, int32_t n_loc, int32_t ld, int32_t accumulate,
                                 double *__restrict__ out)
{
    const uint64_t row = key / (uint64_t)n_loc;
    double *at = out + (int64_t)row * ld + (int64_t)(key - row * (uint64_t)n_loc);
    *at = accumulate ? *at + sum : sum;
}

// one lane per sorted record; works where the record opens a chunk of its run
__global__ __launch_bounds__(BS) void sample_adj_chunks_kernel(int64_t n, uint64_t none,
                                                               const uint64_t *__restrict__ keys, double *vals,
                                                               int32_t n_loc, int32_t ld, int32_t accumulate,
                                                               double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += stride) {
        const uint64_t k = keys[i];
        if (k >= none) continue;
        const bool opens_run = i == 0 || keys[i - 1] != k;
        bool opens_chunk = opens_run;
        if (!opens_run && i >= ADJ_CHUNK && keys[i - ADJ_CHUNK] == k) {
            // ADJ_CHUNK or more records of this run lie before i: find its start, the first
            // record whose key is not below k
            int64_t lo = 0, hi = i - ADJ_CHUNK;  // keys[hi] == k
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (keys[mid] < k) lo = mid + 1;
                else hi = mid;
            }
            opens_chunk = (i - lo) % ADJ_CHUNK == 0;
        }
        if (!opens_chunk) continue;
        double sum = vals[i];
        int64_t j = i + 1;
        const int64_t end = i + ADJ_CHUNK < n ? i + ADJ_CHUNK : n;
        for (; j < end && keys[j] == k; ++j) sum = sum + vals[j];
        const bool more = j == i + ADJ_CHUNK && j < n && keys[j] == k;
        if (opens_run && !more) adj_store(k, sum, n_loc, ld, accumulate, out);
        else vals[i] = sum;  // read by this lane alone in this launch
    }
}

// the runs of more than one chunk: the parked chunk sums, added from the left
__global__ __launch_bounds__(BS) void sample_adj_runs_kernel(int64_t n, uint64_t none,
                                                             const uint64_t *__restrict__ keys,
                                                             const double *__restrict__ vals, int32_t n_loc, int32_t ld,
                                                             int32_t accumulate, double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i + ADJ_CHUNK < n; i += stride) {
        const uint64_t k = keys[i];
        if (k >= none || keys[i + ADJ_CHUNK] != k || (i > 0 && keys[i - 1] == k)) continue;
        double total = vals[i];
        for (int64_t j = i + ADJ_CHUNK; j < n && keys[j] == k; j += ADJ_CHUNK) total = total + vals[j];
        adj_store(k, total, n_loc, ld, accumulate, out);
    }
}

inline size_t adj_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// workspace: keys [2][n_rec] (uint64), terms [2][n_rec] (double), the sort's scratch; every
// part on a 256-byte boundary
int adj_layout(int64_t n_p, int32_t d, size_t *part, size_t *sort_bytes, size_t *total)
{
    STK_REQUIRE(n_p >= 0 && (d == 2 || d == 3), "stk_sample_pairs_adjoint: n_p=%lld d=%d", (long long)n_p, d);
    STK_REQUIRE(n_p <= (((int64_t)1 << 31) - 1) / (2 * (d + 1)),
                "stk_sample_pairs_adjoint: %lld points are 2 (d + 1) n_p >= 2^31 records, more than one call indexes; "
                "split the list and accumulate",
                (long long)n_p);
    const int64_t n_rec = 2 * (int64_t)(d + 1) * n_p;
    *part = adj_align((size_t)n_rec * 8);
    *sort_bytes = 0;
    if (n_rec)
        if (int rc = stk_adj_sort_temp_bytes(n_rec, sort_bytes)) return rc;
    *total = 4 * *part + adj_align(*sort_bytes);
    return 0;
}

}  // namespace

struct stk_sample_plan {
    int32_t d;
    int64_t nv, nc, n_free;
    grid_desc g;
    p1_mesh_dev mesh;
    int32_t *bin_ptr;    // [bins + 1]
    int32_t *bin_cells;  // cells of bin b: bin_ptr[b] .. bin_ptr[b + 1], ascending
    // request tables of stk_sample_eval: written into pinned host memory, copied on the
    // caller's stream; `copied` guards the host side against the next call
    char *req_host, *req_dev;
    size_t req_bytes;
    hipEvent_t copied;
    bool copy_pending;
    stk_dev_arrays dev;  // owns every device array above (req_host and the event go by hand)
    ~stk_sample_plan()
    {
        if (req_host) (void)hipHostFree(req_host);
        if (copied) (void)hipEventDestroy(copied);
    }
};

extern "C" int stk_sample_grid_build(int32_t d, int64_t nv, int64_t nc, const double *points, const int64_t *cells,
                                     stk_sample_grid **out)
{
    STK_REQUIRE(out, "stk_sample_grid_build: null pointer");
    if (int rc = p1_check_mesh("stk_sample_grid_build", d, nv, nc, points, cells)) return rc;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int k = 0; k < d; ++k) lo[k] = hi[k] = points[k];
    for (int64_t v = 0; v < nv; ++v)
        for (int k = 0; k < d; ++k) {
            const double x = points[d * v + k];
            STK_REQUIRE(std::isfinite(x), "stk_sample_grid_build: vertex %lld is not finite", (long long)v);
            lo[k] = std::min(lo[k], x), hi[k] = std::max(hi[k], x);
        }
    double extent = 0.0;
    for (int k = 0; k < d; ++k) extent = std::max(extent, hi[k] - lo[k]);
    STK_REQUIRE(extent > 0.0, "stk_sample_grid_build: the mesh has no extent");
    stk_sample_grid *g = new stk_sample_grid();
    g->d = d, g->widen = 1e-12 * extent;
    const int32_t nb = (int32_t)std::max(1.0, std::floor(std::pow((double)nc, 1.0 / d) + 0.5));
    int64_t n_bins = 1;
    for (int k = 0; k < 3; ++k) {
        g->nb[k] = k < d ? nb : 1;
        g->lo[k] = k < d ? lo[k] - g->widen : 0.0;
        g->inv_w[k] = k < d ? (double)nb / ((hi[k] - lo[k]) + 2.0 * g->widen) : 0.0;
        n_bins *= g->nb[k];
    }
    if (n_bins >= ((int64_t)1 << 31)) {
        delete g;
        stk_set_error("stk_sample_grid_build: too many bins for 32-bit tables");
        return 2;
    }
    // pass 1, over the cells: the bins each widened box reaches, per axis
    std::vector<int32_t> range((size_t)nc * 6);
    const int T = host_threads(nc);
    on_threads(T, [&](int k) {
        for (int64_t t = share(nc, T, k); t < share(nc, T, k + 1); ++t) {
            int32_t *r = &range[(size_t)t * 6];
            for (int a = 0; a < 3; ++a) r[2 * a] = r[2 * a + 1] = 0;
            for (int a = 0; a < d; ++a) {
                double bl = points[d * cells[(d + 1) * t] + a], bh = bl;
                for (int j = 1; j <= d; ++j) {
                    const double x = points[d * cells[(d + 1) * t + j] + a];
                    bl = std::min(bl, x), bh = std::max(bh, x);
                }
                r[2 * a] = bin_of(bl - g->widen, g->lo[a], g->inv_w[a], g->nb[a]);
                r[2 * a + 1] = bin_of(bh + g->widen, g->lo[a], g->inv_w[a], g->nb[a]);
            }
        }
    });
    // passes 2 and 3, over slabs of bins along the last axis: every thread counts, then
    // files, the cells of ITS bins in ascending cell order -- one owner per list, the
    // result does not depend on the number of threads
    const int last = d - 1;
    const int TB = std::min<int>(T, g->nb[last]);
    g->bin_ptr.assign((size_t)n_bins + 1, 0);
    auto for_bins = [&](int k, auto &&visit) {
        const int32_t s0 = (int32_t)share(g->nb[last], TB, k), s1 = (int32_t)share(g->nb[last], TB, k + 1);
        for (int64_t t = 0; t < nc; ++t) {
            int32_t r[6];
            for (int a = 0; a < 6; ++a) r[a] = range[(size_t)t * 6 + a];
            r[2 * last] = std::max(r[2 * last], s0), r[2 * last + 1] = std::min(r[2 * last + 1], s1 - 1);
            for (int32_t iz = r[4]; iz <= r[5]; ++iz)
                for (int32_t iy = r[2]; iy <= r[3]; ++iy)
                    for (int32_t ix = r[0]; ix <= r[1]; ++ix)
                        visit(((int64_t)iz * g->nb[1] + iy) * g->nb[0] + ix, (int32_t)t);
        }
    };
    on_threads(TB, [&](int k) { for_bins(k, [&](int64_t b, int32_t) { ++g->bin_ptr[(size_t)b + 1]; }); });
    int64_t total = 0;
    for (int64_t b = 0; b < n_bins; ++b) {
        total += g->bin_ptr[(size_t)b + 1];
        if (total >= ((int64_t)1 << 31)) {
            delete g;
            stk_set_error("stk_sample_grid_build: bin lists too large for 32-bit tables");
            return 2;
        }
        g->bin_ptr[(size_t)b + 1] = (int32_t)total;
    }
    g->bin_cells.resize((size_t)total);
    std::vector<int32_t> cursor(g->bin_ptr.begin(), g->bin_ptr.end() - 1);
    on_threads(TB, [&](int k) { for_bins(k, [&](int64_t b, int32_t t) { g->bin_cells[(size_t)cursor[(size_t)b]++] = t; }); });
    *out = g;
    return 0;
}

extern "C" int stk_sample_grid_sizes(const stk_sample_grid *grid, int32_t *bins, double *lo, double *inv_width,
                                     double *widen, int64_t *n_entries)
{
    STK_REQUIRE(grid, "stk_sample_grid_sizes: null pointer");
    for (int k = 0; k < 3; ++k) {
        if (bins) bins[k] = grid->nb[k];
        if (lo) lo[k] = grid->lo[k];
        if (inv_width) inv_width[k] = grid->inv_w[k];
    }
    if (widen) *widen = grid->widen;
    if (n_entries) *n_entries = (int64_t)grid->bin_cells.size();
    return 0;
}

extern "C" int stk_sample_grid_copy(const stk_sample_grid *grid, int32_t *bin_ptr, int32_t *bin_cells)
{
    STK_REQUIRE(grid && bin_ptr && bin_cells, "stk_sample_grid_copy: null pointer");
    std::copy(grid->bin_ptr.begin(), grid->bin_ptr.end(), bin_ptr);
    std::copy(grid->bin_cells.begin(), grid->bin_cells.end(), bin_cells);
    return 0;
}

extern "C" int stk_sample_grid_free(stk_sample_grid *grid)
{
    delete grid;
    return 0;
}

extern "C" int stk_sample_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points, const int64_t *cells,
                                      int64_t n_free, const int64_t *free_vertices, stk_sample_plan **out)
{
    STK_REQUIRE(out && n_free > 0 && free_vertices, "stk_sample_plan_create: bad arguments");
    stk_sample_grid *grid = nullptr;
    if (int rc = stk_sample_grid_build(d, nv, nc, points, cells, &grid)) return rc;
    std::vector<int32_t> row_of;
    if (int rc = p1_row_of("stk_sample_plan_create", nv, n_free, free_vertices, &row_of)) {
        stk_sample_grid_free(grid);
        return rc;
    }

    stk_sample_plan *p = new stk_sample_plan();
    p->d = d, p->nv = nv, p->nc = nc, p->n_free = n_free;
    for (int k = 0; k < 3; ++k) p->g.nb[k] = grid->nb[k], p->g.lo[k] = grid->lo[k], p->g.inv_w[k] = grid->inv_w[k];
    int rc = p1_mesh_upload(p->dev, &p->mesh, d, nv, nc, points, cells, &row_of);
    if (!rc) rc = !(p->bin_ptr = p->dev.upload(grid->bin_ptr)) || !(p->bin_cells = p->dev.upload(grid->bin_cells));
    stk_sample_grid_free(grid);
    if (!rc && hipEventCreateWithFlags(&p->copied, hipEventDisableTiming) != hipSuccess) {
        stk_set_error("stk_sample_plan_create: no event");
        rc = 1;
    }
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return 0;
}

extern "C" int stk_sample_plan_destroy(stk_sample_plan *plan)
{
    delete plan;
    return 0;
}

extern "C" int stk_sample_locate(void *stream, const stk_sample_plan *plan, int64_t n_p, const double *x, int32_t *cell,
                                 double *lam)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan && n_p >= 0 && (n_p == 0 || (x && cell && lam)), "stk_sample_locate: bad arguments");
    if (n_p == 0) return 0;
    const dim3 grid(stk_flat_grid(n_p, BS));
    hipStream_t st = stk_stream(stream);
    if (plan->d == 2)
        hipLaunchKernelGGL(sample_locate_kernel<2>, grid, dim3(BS), 0, st, n_p, x, plan->g, plan->bin_ptr, plan->bin_cells,
                           plan->mesh.points, plan->mesh.cells, cell, lam);
    else
        hipLaunchKernelGGL(sample_locate_kernel<3>, grid, dim3(BS), 0, st, n_p, x, plan->g, plan->bin_ptr, plan->bin_cells,
                           plan->mesh.points, plan->mesh.cells, cell, lam);
    STK_LAUNCH_CHECK();
    return 0;
}

extern "C" int stk_sample_eval(void *stream, stk_sample_plan *plan, int64_t n_p, const int32_t *cell, const double *lam,
                               int32_t M, int32_t n_loc, int32_t ld, const double *slab, int32_t n_k, const int32_t *columns,
                               const double *weights, int64_t ld_out, double *out)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan && n_p >= 0 && n_k >= 0, "stk_sample_eval: bad arguments");
    if (n_p == 0 || n_k == 0) return 0;
    STK_REQUIRE(cell && lam && slab && columns && weights && out, "stk_sample_eval: null pointer");
    STK_REQUIRE(M == plan->n_free, "stk_sample_eval: a slab of %d rows on a plan of %lld free dofs", M,
                (long long)plan->n_free);
    STK_REQUIRE(n_loc >= 1 && ld >= n_loc && ld_out >= n_p, "stk_sample_eval: n_loc=%d ld=%d ld_out=%lld n_p=%lld", n_loc, ld,
                (long long)ld_out, (long long)n_p);
    for (int k = 0; k < 2 * n_k; ++k)
        STK_REQUIRE(columns[k] >= -1 && columns[k] < n_loc, "stk_sample_eval: request %d names column %d of %d", k / 2,
                    columns[k], n_loc);
    // launches: consecutive requests whose distinct columns fit one tile.  Per launch
    // [n_c columns | n_kc x 2 indices into them (int32) | pad to 8 | n_kc x 2 weights]
    struct launch {
        int32_t k0, n_kc, n_c;
        size_t off_cols, off_req, off_w;
    };
    std::vector<launch> launches;
    std::vector<int32_t> slot((size_t)n_loc, -1), used;
    size_t bytes = 0;
    std::vector<char> image;
    auto flush = [&](int32_t k0, int32_t k1) {
        launch L;
        L.k0 = k0, L.n_kc = k1 - k0, L.n_c = (int32_t)used.size();  // 0: all "not on this rank"
        std::vector<int32_t> head(used);
        for (int32_t k = k0; k < k1; ++k)
            for (int a = 0; a < 2; ++a) head.push_back(columns[2 * k + a] < 0 ? -1 : slot[(size_t)columns[2 * k + a]]);
        if (head.size() & 1) head.push_back(0);
        L.off_cols = bytes, L.off_req = bytes + 4 * (size_t)L.n_c;
        L.off_w = bytes + 4 * head.size();
        image.resize(L.off_w + 16 * (size_t)L.n_kc);
        std::copy((const char *)head.data(), (const char *)(head.data() + head.size()), image.begin() + L.off_cols);
        std::copy((const char *)(weights + 2 * k0), (const char *)(weights + 2 * k1), image.begin() + L.off_w);
        bytes = image.size();
        launches.push_back(L);
        for (int32_t c : used) slot[(size_t)c] = -1;
        used.clear();
    };
    int32_t k0 = 0;
    for (int32_t k = 0; k < n_k; ++k) {
        int fresh = 0;
        for (int a = 0; a < 2; ++a) {
            const int32_t c = columns[2 * k + a];
            fresh += c >= 0 && slot[(size_t)c] < 0 && !(a == 1 && c == columns[2 * k]);
        }
        if ((int)used.size() + fresh > MAX_COLS) flush(k0, k), k0 = k;
        for (int a = 0; a < 2; ++a) {
            const int32_t c = columns[2 * k + a];
            if (c >= 0 && slot[(size_t)c] < 0) slot[(size_t)c] = (int32_t)used.size(), used.push_back(c);
        }
    }
    flush(k0, n_k);

    hipStream_t st = stk_stream(stream);
    if (plan->copy_pending) STK_HIP(hipEventSynchronize(plan->copied));  // the host image is free again
    if (bytes > plan->req_bytes) {
        // the device image may still be read by an earlier call's kernels
        STK_HIP(hipStreamSynchronize(st));
        plan->dev.release(plan->req_dev);
        if (plan->req_host) (void)hipHostFree(plan->req_host);
        plan->req_dev = plan->req_host = nullptr, plan->req_bytes = 0;
        const size_t room = std::max<size_t>(2 * bytes, 4096);
        if (!(plan->req_dev = plan->dev.alloc<char>(room))) return 1;
        STK_HIP(hipHostMalloc((void **)&plan->req_host, room, hipHostMallocDefault));
        plan->req_bytes = room;
    }
    std::copy(image.begin(), image.end(), plan->req_host);
    STK_HIP(hipMemcpyAsync(plan->req_dev, plan->req_host, bytes, hipMemcpyHostToDevice, st));
    STK_HIP(hipEventRecord(plan->copied, st));
    plan->copy_pending = true;

    const int d = plan->d;
    const int64_t n_tiles = (n_p + TP - 1) / TP;
    const dim3 grid((unsigned)std::min<int64_t>(n_tiles, 256 * 16));
    for (const launch &L : launches) {
        const size_t lds = (size_t)TP * (L.n_c | 1) * sizeof(double) + (size_t)TP * (d + 1) * (sizeof(double) + sizeof(int32_t));
        const int32_t *cols = (const int32_t *)(plan->req_dev + L.off_cols);
        const int32_t *req = (const int32_t *)(plan->req_dev + L.off_req);
        const double *w = (const double *)(plan->req_dev + L.off_w);
        double *o = out + (int64_t)L.k0 * ld_out;
        if (d == 2)
            hipLaunchKernelGGL(sample_eval_kernel<2>, grid, dim3(BS), lds, st, n_p, plan->nc, cell, lam, plan->mesh.cells, plan->mesh.row_of, ld,
                               slab, L.n_c, cols, L.n_kc, req, w, ld_out, o);
        else
            hipLaunchKernelGGL(sample_eval_kernel<3>, grid, dim3(BS), lds, st, n_p, plan->nc, cell, lam, plan->mesh.cells, plan->mesh.row_of, ld,
                               slab, L.n_c, cols, L.n_kc, req, w, ld_out, o);
        STK_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int stk_sample_grad_coeffs(void *stream, const stk_sample_plan *plan, int64_t n_p, const int32_t *cell,
                                      double *out)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan && n_p >= 0 && (n_p == 0 || (cell && out)), "stk_sample_grad_coeffs: bad arguments");
    if (n_p == 0) return 0;
    const dim3 grid(stk_flat_grid(n_p, BS));
    hipStream_t st = stk_stream(stream);
    if (plan->d == 2)
        hipLaunchKernelGGL(sample_grad_coeffs_kernel<2>, grid, dim3(BS), 0, st, n_p, plan->nc, cell, plan->mesh.points, plan->mesh.cells,
                           out);
    else
        hipLaunchKernelGGL(sample_grad_coeffs_kernel<3>, grid, dim3(BS), 0, st, n_p, plan->nc, cell, plan->mesh.points, plan->mesh.cells,
                           out);
    STK_LAUNCH_CHECK();
    return 0;
}

extern "C" int stk_sample_pairs(void *stream, const stk_sample_plan *plan, int64_t n_p, const int32_t *cell,
                                const double *lam, const double *t, double h, int32_t N, int32_t t_begin, int32_t M,
                                int32_t n_loc, int32_t ld, const double *slab, int32_t fields, int64_t ld_out, double *out)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan && n_p >= 0, "stk_sample_pairs: bad arguments");
    STK_REQUIRE(fields >= 1 && fields <= 7, "stk_sample_pairs: fields=%d is no mask of u (1), dt (2) and grad (4)", fields);
    if (n_p == 0) return 0;
    STK_REQUIRE(cell && lam && t && slab && out, "stk_sample_pairs: null pointer");
    STK_REQUIRE(M == plan->n_free, "stk_sample_pairs: a slab of %d rows on a plan of %lld free dofs", M,
                (long long)plan->n_free);
    STK_REQUIRE(h > 0.0 && N >= 2 && t_begin >= 0, "stk_sample_pairs: h=%g N=%d t_begin=%d", h, N, t_begin);
    STK_REQUIRE(n_loc >= 1 && ld >= n_loc && ld_out >= n_p, "stk_sample_pairs: n_loc=%d ld=%d ld_out=%lld n_p=%lld", n_loc, ld,
                (long long)ld_out, (long long)n_p);
    const bool wide = !(ld & 1) && !((uintptr_t)slab & 15);
    const double t_last = (double)(N - 1) * h;
    const dim3 grid(stk_flat_grid(n_p, BS));
    hipStream_t st = stk_stream(stream);
#define STK_PAIRS(D, W)                                                                                                     \
    hipLaunchKernelGGL((sample_pairs_kernel<D, W>), grid, dim3(BS), 0, st, n_p, plan->nc, cell, lam, t, h, t_last, N, t_begin, \
                       n_loc, ld, slab, plan->mesh.points, plan->mesh.cells, plan->mesh.row_of, fields, ld_out, out)
    if (plan->d == 2) {
        if (wide) STK_PAIRS(2, true);
        else STK_PAIRS(2, false);
    } else {
        if (wide) STK_PAIRS(3, true);
        else STK_PAIRS(3, false);
    }
#undef STK_PAIRS
    STK_LAUNCH_CHECK();
    return 0;
}

extern "C" int stk_sample_pairs_adjoint_work_size(int64_t n_p, int32_t d, int64_t *bytes)
{
    STK_REQUIRE(bytes, "stk_sample_pairs_adjoint_work_size: null pointer");
    size_t part, sort_bytes, total;
    if (int rc = adj_layout(n_p, d, &part, &sort_bytes, &total)) return rc;
    *bytes = (int64_t)total;
    return 0;
}

extern "C" int stk_sample_pairs_adjoint(void *stream, const stk_sample_plan *plan, int64_t n_p, const int32_t *cell,
                                        const double *lam, const double *t, double h, int32_t N, int32_t t_begin, int32_t M,
                                        int32_t n_loc, int32_t ld, double *slab, const double *w, int64_t ld_w, int32_t field,
                                        int32_t accumulate, unsigned char *used, void *work, int64_t work_bytes)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan && n_p >= 0 && slab, "stk_sample_pairs_adjoint: bad arguments");
    STK_REQUIRE(field == 1 || field == 2 || field == 4, "stk_sample_pairs_adjoint: field=%d is none of u (1), dt (2), grad (4)",
                field);
    STK_REQUIRE(accumulate == 0 || accumulate == 1, "stk_sample_pairs_adjoint: accumulate=%d", accumulate);
    STK_REQUIRE(M == plan->n_free, "stk_sample_pairs_adjoint: a slab of %d rows on a plan of %lld free dofs", M,
                (long long)plan->n_free);
    STK_REQUIRE(h > 0.0 && N >= 2 && t_begin >= 0, "stk_sample_pairs_adjoint: h=%g N=%d t_begin=%d", h, N, t_begin);
    STK_REQUIRE(n_loc >= 1 && ld >= n_loc && ld_w >= n_p, "stk_sample_pairs_adjoint: n_loc=%d ld=%d ld_w=%lld n_p=%lld", n_loc,
                ld, (long long)ld_w, (long long)n_p);
    size_t part, sort_bytes, total;
    if (int rc = adj_layout(n_p, plan->d, &part, &sort_bytes, &total)) return rc;
    if (n_p > 0) {
        STK_REQUIRE(cell && lam && t && w && used && work, "stk_sample_pairs_adjoint: null pointer");
        STK_REQUIRE(!((uintptr_t)work & 255) && work_bytes >= (int64_t)total,
                    "stk_sample_pairs_adjoint: a workspace of %lld bytes at %p; %lld on a 256-byte boundary are needed",
                    (long long)work_bytes, work, (long long)total);
    }
    hipStream_t st = stk_stream(stream);
    const int64_t entries = (int64_t)M * n_loc;
    if (!accumulate) {
        hipLaunchKernelGGL(sample_adj_zero_kernel, dim3(stk_flat_grid(entries, BS)), dim3(BS), 0, st, entries, n_loc, ld, slab);
        STK_LAUNCH_CHECK();
    }
    if (n_p == 0) return 0;
    char *base = static_cast<char *>(work);
    uint64_t *const keys[2] = {reinterpret_cast<uint64_t *>(base), reinterpret_cast<uint64_t *>(base + part)};
    double *const vals[2] = {reinterpret_cast<double *>(base + 2 * part), reinterpret_cast<double *>(base + 3 * part)};
    const int64_t n_rec = 2 * (int64_t)(plan->d + 1) * n_p;
    const uint64_t none = (uint64_t)entries;  // the key of a dropped term: one past the last entry
    int key_bits = 1;
    while (key_bits < 64 && (none >> key_bits)) ++key_bits;
    const double t_last = (double)(N - 1) * h;
    const dim3 grid(stk_flat_grid(n_p, BS));
    if (plan->d == 2)
        hipLaunchKernelGGL(sample_adj_records_kernel<2>, grid, dim3(BS), 0, st, n_p, plan->nc, cell, lam, t, h, t_last, N, t_begin,
                           n_loc, none, w, ld_w, field, plan->mesh.points, plan->mesh.cells, plan->mesh.row_of, keys[0], vals[0], used);
    else
        hipLaunchKernelGGL(sample_adj_records_kernel<3>, grid, dim3(BS), 0, st, n_p, plan->nc, cell, lam, t, h, t_last, N, t_begin,
                           n_loc, none, w, ld_w, field, plan->mesh.points, plan->mesh.cells, plan->mesh.row_of, keys[0], vals[0], used);
    STK_LAUNCH_CHECK();
    int half = 0;
    if (int rc = stk_adj_sort(st, base + 4 * part, adj_align(sort_bytes), keys, vals, n_rec, key_bits, &half)) return rc;
    const dim3 grid_rec(stk_flat_grid(n_rec, BS));
    hipLaunchKernelGGL(sample_adj_chunks_kernel, grid_rec, dim3(BS), 0, st, n_rec, none, keys[half], vals[half], n_loc, ld,
                       accumulate, slab);
    STK_LAUNCH_CHECK();
    if (n_rec > ADJ_CHUNK) {
        hipLaunchKernelGGL(sample_adj_runs_kernel, grid_rec, dim3(BS), 0, st, n_rec, none, keys[half], vals[half], n_loc, ld,
                           accumulate, slab);
        STK_LAUNCH_CHECK();
    }
    return 0;
}
