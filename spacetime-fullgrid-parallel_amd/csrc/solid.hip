// Solidification maps (include/stk.h "solidification maps"): per CELL of a trial-space slab
// the last time its mean dropped to or below a threshold, the cooling rate and the gradient
// of u_h at that moment, the number of such crossings, and the largest |grad u_h|^2 with its
// earliest node -- from ONE scan over the cells' rows with a carried state of 6 + 2 d doubles
// per cell (STK_SOLID_ROWS).  Mean and gradient of a cell are linear in time per element, so a
// scan of columns [k0, k1) followed by one of [k1, k2) is the scan of [k0, k2), double for
// double.  The history maps (history.hip) see dofs; the gradient lives on cells.
//
//  * stk_solid_cell_order    host only: the cells along the Z-curve of their centroids, so that
//                            256 consecutive ones are a compact patch that shares its rows
//  * stk_solid_tile_rows     host only: per tile of 256 consecutive cells the ascending list of
//                            the DISTINCT slab rows its cells touch (sort and unique, no hash)
//                            and per cell the d + 1 positions in that list as 16-bit indices
//  * stk_solid_plan_create   uploads the mesh and the lists, computes grad lambda_a per cell
//                            (p1_geometry_kernel)
//  * stk_solid_scan          n_cols columns of a slab -> state [6 + 2 d][nc], in/out
//
// One launch.  A workgroup of 256 lanes takes tile i -- the cells order[256 i .. 256 i + 256) of
// the plan's order, one lane per cell; a cell's numbers are its own, so the order changes no
// double, and the state is read and written at the cell's own index -- and walks the columns
// in chunks of cw.  Per chunk it requests the runs
// [row][c0 .. c0 + cw) of the WHOLE list into LDS at once, the lanes running along time first
// (the flat index j = r cw + c over the lanes: a wavefront's request covers whole row
// segments), so a row shared by several cells of the tile is fetched once per tile and chunk,
// not d + 1 or six times.  The LDS rows are re-strided to an ODD length (history.hip), so the
// 8-byte reads of lanes on different rows spread over the banks.  After one barrier every lane
// walks its d + 1 rows through the chunk's columns out of LDS.  The state stays in registers
// over the chunks and is read and written once per cell.  cw follows from the LDS budget and
// the longest list of the plan and is at least 1 (stk_solid_tile overrides both).
//
// 64-bit offsets, 8-byte loads only (the pointer is only 8-byte aligned), no atomics, nothing
// allocated per call, no synchronisation.
//
// ARITHMETIC: every product, quotient and sum rounded on its own -- contraction is SWITCHED
// OFF for this file and for p1_mesh.h (their pragmas and -ffp-contract=off in the Makefile),
// and no kernel here calls fma.
#include <algorithm>

#include "p1_mesh.h"

#pragma clang fp contract(off)

struct stk_solid_plan {
    int32_t d;
    int64_t nv, nc, n_free, n_tiles;
    int32_t longest;  // the longest tile list
    p1_mesh_dev mesh;
    double *grad;        // [nc][d + 1][d], in the plan's order of the cells
    int32_t *cell_of;    // [nc]: the cell a place of the plan's order holds
    int32_t *tile_ptr;   // [n_tiles + 1]
    int32_t *tile_rows;  // [tile_ptr[n_tiles]]
    uint16_t *cell_pos;  // [nc][d + 1]: the position in the tile's list, SOLID_NO_ROW on the boundary
    stk_dev_arrays dev;  // owns every device array above
};

namespace {

constexpr int BS = 256;
constexpr uint16_t SOLID_NO_ROW = 0xFFFF;
// the chunk of the default: 16 KiB of LDS per workgroup, the fastest of the budgets measured on
// the 65-column slab, and what stk_solid_tile accepts
constexpr int32_t TILE_KIB = 16, TILE_KIB_MAX = 64, TILE_COLS_MAX = 128;
std::atomic<int32_t> g_tile_cols{0}, g_tile_kib{TILE_KIB}, g_caller_order{0};

template <int D>
struct solid_state {
    double t_solid, cooling, n_solid, max_q, t_max, last_mean, grad_solid[D], last_grad[D];
};

// mean, gradient and |gradient|^2 of a cell at one node: the expressions of the contract
template <int D>
__device__ inline void solid_cell(const double (&U)[D + 1], const double (&g)[D + 1][D], double &m, double (&G)[D],
                                  double &Q)
{
    double s = U[0] + U[1];
#pragma unroll
    for (int a = 2; a <= D; ++a) s = s + U[a];
    m = s / (double)(D + 1);
#pragma unroll
    for (int j = 0; j < D; ++j) {
        G[j] = U[0] * g[0][j] + U[1] * g[1][j];
#pragma unroll
        for (int a = 2; a <= D; ++a) G[j] = G[j] + U[a] * g[a][j];
    }
    Q = G[0] * G[0] + G[1] * G[1];
    if constexpr (D == 3) Q = Q + G[2] * G[2];
}

template <int D>
__device__ inline void solid_fresh(solid_state<D> &s, double m, const double (&G)[D], double Q, int64_t k, double h)
{
    s.t_solid = s.cooling = __builtin_nan("");
    s.n_solid = 0.0;
    s.max_q = Q;
    s.t_max = (double)k * h;
    s.last_mean = m;
#pragma unroll
    for (int j = 0; j < D; ++j) s.grad_solid[j] = __builtin_nan(""), s.last_grad[j] = G[j];
}

template <int D>
__device__ inline void solid_step(solid_state<D> &s, double b, const double (&G)[D], double Q, int64_t k, double h,
                                  double theta)
{
    const double a = s.last_mean;
    if (Q > s.max_q) {
        s.max_q = Q;
        s.t_max = (double)k * h;
    }
    if (a > theta && b <= theta) {
        const double x = (theta - a) / (b - a);
        s.t_solid = ((double)(k - 1) + x) * h;
        s.cooling = (a - b) / h;
#pragma unroll
        for (int j = 0; j < D; ++j) s.grad_solid[j] = s.last_grad[j] + x * (G[j] - s.last_grad[j]);
        s.n_solid = s.n_solid + 1.0;
    }
    s.last_mean = b;
#pragma unroll
    for (int j = 0; j < D; ++j) s.last_grad[j] = G[j];
}

template <int D>
__device__ inline void solid_read(solid_state<D> &s, const double *state, int64_t nc, int64_t t)
{
    s.t_solid = state[t];
    s.cooling = state[nc + t];
    s.n_solid = state[2 * nc + t];
    s.max_q = state[3 * nc + t];
    s.t_max = state[4 * nc + t];
    s.last_mean = state[5 * nc + t];
#pragma unroll
    for (int j = 0; j < D; ++j) s.grad_solid[j] = state[(6 + j) * nc + t], s.last_grad[j] = state[(6 + D + j) * nc + t];
}

template <int D>
__device__ inline void solid_write(const solid_state<D> &s, double *state, int64_t nc, int64_t t)
{
    state[t] = s.t_solid;
    state[nc + t] = s.cooling;
    state[2 * nc + t] = s.n_solid;
    state[3 * nc + t] = s.max_q;
    state[4 * nc + t] = s.t_max;
    state[5 * nc + t] = s.last_mean;
#pragma unroll
    for (int j = 0; j < D; ++j) state[(6 + j) * nc + t] = s.grad_solid[j], state[(6 + D + j) * nc + t] = s.last_grad[j];
}

// grid: one workgroup per tile.  LDS image [rows of the tile's list][ldp], ldp = cw | 1; the
// launch sizes it for the longest list.  (r, c) of the loading lanes advance by (BS / cw,
// BS % cw) per step, as in history_slab_kernel: no division in the loop.
template <int D>
__global__ __launch_bounds__(BS) void solid_scan_kernel(int64_t nc, int32_t n_cols, const double *__restrict__ u,
                                                        int64_t ld, int64_t k_first, double h, double theta,
                                                        int32_t fresh, double *__restrict__ state, int32_t cw,
                                                        const int32_t *__restrict__ tile_ptr,
                                                        const int32_t *__restrict__ tile_rows,
                                                        const uint16_t *__restrict__ cell_pos,
                                                        const double *__restrict__ grad,
                                                        const int32_t *__restrict__ cell_of)
{
    extern __shared__ double image[];
    const int ldp = cw | 1;
    const int tid = threadIdx.x;
    const int64_t place = (int64_t)blockIdx.x * BS + tid;  // in the plan's order
    const bool mine = place < nc;
    const int64_t t = mine ? cell_of[place] : 0;  // the cell: where its state lives
    const int32_t list_first = tile_ptr[blockIdx.x];
    const int n_rows = tile_ptr[blockIdx.x + 1] - list_first;
    const int32_t *__restrict__ rows = tile_rows + list_first;
    const int r_first = tid / cw, c_first = tid - r_first * cw;
    const int dr = BS / cw, dc = BS - dr * cw;

    double g[D + 1][D];
    int at[D + 1];  // where vertex a's row starts in the image, -1 on the boundary
    solid_state<D> s;
#pragma unroll
    for (int a = 0; a <= D; ++a) {
        at[a] = -1;
#pragma unroll
        for (int j = 0; j < D; ++j) g[a][j] = 0.0;
    }
    if (mine) {
#pragma unroll
        for (int a = 0; a <= D; ++a) {
            const uint16_t p = cell_pos[(D + 1) * place + a];
            at[a] = p == SOLID_NO_ROW ? -1 : (int)p * ldp;
#pragma unroll
            for (int j = 0; j < D; ++j) g[a][j] = grad[((D + 1) * place + a) * D + j];
        }
        if (!fresh) solid_read<D>(s, state, nc, t);
    }
    for (int32_t c0 = 0; c0 < n_cols; c0 += cw) {
        const int here = n_cols - c0 < cw ? n_cols - c0 : cw;
        if (c0) __syncthreads();  // the walk of the chunk before is over
        for (int r = r_first, c = c_first; r < n_rows;) {
            if (c < here) image[r * ldp + c] = u[(int64_t)rows[r] * ld + c0 + c];
            r += dr;
            c += dc;
            if (c >= cw) {
                c -= cw;
                ++r;
            }
        }
        __syncthreads();
        if (mine) {
            const int64_t k0 = k_first + c0;
            for (int c = 0; c < here; ++c) {
                double U[D + 1], m, G[D], Q;
#pragma unroll
                for (int a = 0; a <= D; ++a) U[a] = at[a] >= 0 ? image[at[a] + c] : 0.0;
                solid_cell<D>(U, g, m, G, Q);
                if (fresh && c0 == 0 && c == 0)
                    solid_fresh<D>(s, m, G, Q, k0, h);
                else
                    solid_step<D>(s, m, G, Q, k0 + c, h, theta);
            }
        }
    }
    if (mine) solid_write<D>(s, state, nc, t);
}

}  // namespace

extern "C" int stk_solid_rows(int32_t d) { return d == 2 || d == 3 ? STK_SOLID_ROWS(d) : 0; }

extern "C" int stk_solid_cell_order(int32_t d, int64_t nv, int64_t nc, const double *points, const int64_t *cells,
                                    int32_t *order)
{
    if (int rc = p1_check_mesh("stk_solid_cell_order", d, nv, nc, points, cells)) return rc;
    STK_REQUIRE(order != nullptr, "stk_solid_cell_order: order is null");
    // the key of a cell: its centroid ((p_0 + p_1) + p_2 [+ p_3]) / (d + 1), per axis the 16 bits
    // trunc((c - lo) / (hi - lo) * 65535) over the box [lo, hi] of all points (0 on an axis
    // of no extent), the bits interleaved with axis 0 lowest; sorted by (key, cell): a total
    // order, the same on every run
    double lo[3], hi[3];
    for (int j = 0; j < d; ++j) lo[j] = hi[j] = points[j];
    for (int64_t v = 1; v < nv; ++v)
        for (int j = 0; j < d; ++j) {
            lo[j] = std::min(lo[j], points[d * v + j]);
            hi[j] = std::max(hi[j], points[d * v + j]);
        }
    std::vector<std::pair<uint64_t, int32_t>> keyed((size_t)nc);
    for (int64_t t = 0; t < nc; ++t) {
        const int64_t *c = cells + (d + 1) * t;
        uint64_t key = 0;
        for (int j = 0; j < d; ++j) {
            double x = points[d * c[0] + j] + points[d * c[1] + j];
            for (int a = 2; a <= d; ++a) x = x + points[d * c[a] + j];
            x = x / (double)(d + 1);
            const double extent = hi[j] - lo[j];
            double q = extent > 0.0 ? (x - lo[j]) / extent * 65535.0 : 0.0;
            if (!(q >= 0.0)) q = 0.0;  // (also a NaN coordinate)
            if (q > 65535.0) q = 65535.0;
            const uint64_t bits = (uint64_t)q;
            for (int b = 0; b < 16; ++b) key |= ((bits >> b) & 1) << (d * b + j);
        }
        keyed[(size_t)t] = {key, (int32_t)t};
    }
    std::sort(keyed.begin(), keyed.end());
    for (int64_t t = 0; t < nc; ++t) order[t] = keyed[(size_t)t].second;
    return 0;
}

extern "C" int stk_solid_tile_rows(int32_t d, int64_t nv, int64_t nc, const int64_t *cells, const int32_t *row_of,
                                   int32_t *tile_ptr, int32_t *tile_rows, uint16_t *cell_pos)
{
    STK_REQUIRE(d == 2 || d == 3, "stk_solid_tile_rows: d = %d is neither 2 nor 3", d);
    STK_REQUIRE(nv > 0 && nv < ((int64_t)1 << 31), "stk_solid_tile_rows: nv = %lld out of range", (long long)nv);
    STK_REQUIRE(nc > 0 && (int64_t)(d + 1) * nc < ((int64_t)1 << 31), "stk_solid_tile_rows: nc = %lld out of range",
                (long long)nc);
    STK_REQUIRE(cells != nullptr, "stk_solid_tile_rows: cells is null");
    STK_REQUIRE(row_of != nullptr, "stk_solid_tile_rows: row_of is null");
    STK_REQUIRE(tile_ptr != nullptr, "stk_solid_tile_rows: tile_ptr is null");
    STK_REQUIRE(tile_rows != nullptr, "stk_solid_tile_rows: tile_rows is null");
    STK_REQUIRE(cell_pos != nullptr, "stk_solid_tile_rows: cell_pos is null");
    const int nl = d + 1;
    for (int64_t q = 0; q < nl * nc; ++q)
        STK_REQUIRE(cells[q] >= 0 && cells[q] < nv, "stk_solid_tile_rows: cell %lld names vertex %lld", (long long)(q / nl),
                    (long long)cells[q]);
    for (int64_t v = 0; v < nv; ++v)
        STK_REQUIRE(row_of[v] >= -1, "stk_solid_tile_rows: row_of[%lld] = %d is below -1", (long long)v, row_of[v]);
    // per tile: the rows of its cells' free vertices, sorted, the duplicates dropped -- a list
    // of at most 256 (d + 1) entries, so a position fits 16 bits beside the reserved value --
    // and per (cell, a) the place of its row by bisection
    const int64_t n_tiles = (nc + BS - 1) / BS;
    std::vector<int32_t> list;
    list.reserve((size_t)BS * nl);
    int32_t filled = 0;
    for (int64_t tile = 0; tile < n_tiles; ++tile) {
        const int64_t t0 = tile * BS, t1 = std::min<int64_t>(t0 + BS, nc);
        list.clear();
        for (int64_t q = nl * t0; q < nl * t1; ++q) {
            const int32_t row = row_of[cells[q]];
            if (row >= 0) list.push_back(row);
        }
        std::sort(list.begin(), list.end());
        list.erase(std::unique(list.begin(), list.end()), list.end());
        tile_ptr[tile] = filled;
        for (size_t i = 0; i < list.size(); ++i) tile_rows[filled + (int32_t)i] = list[i];
        for (int64_t q = nl * t0; q < nl * t1; ++q) {
            const int32_t row = row_of[cells[q]];
            cell_pos[q] = row < 0 ? SOLID_NO_ROW : (uint16_t)(std::lower_bound(list.begin(), list.end(), row) - list.begin());
        }
        filled += (int32_t)list.size();
    }
    tile_ptr[n_tiles] = filled;
    return 0;
}

extern "C" int stk_solid_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points, const int64_t *cells,
                                     int64_t n_free, const int64_t *free_vertices, stk_solid_plan **out)
{
    const char *who = "stk_solid_plan_create";
    std::vector<int32_t> row_of;
    if (int rc = p1_plan_open(who, d, nv, nc, points, cells, n_free, free_vertices, out, &row_of)) return rc;
    const int64_t ns = (int64_t)(d + 1) * nc, n_tiles = (nc + BS - 1) / BS;
    // the plan's order of the cells and the cells in that order: tiles, geometry and positions
    // are all taken from `placed`
    std::vector<int32_t> order((size_t)nc);
    if (g_caller_order.load(std::memory_order_relaxed)) {
        for (int64_t t = 0; t < nc; ++t) order[(size_t)t] = (int32_t)t;
    } else if (int rc = stk_solid_cell_order(d, nv, nc, points, cells, order.data())) {
        return rc;
    }
    std::vector<int64_t> placed((size_t)ns);
    for (int64_t i = 0; i < nc; ++i)
        for (int a = 0; a <= d; ++a) placed[(size_t)((d + 1) * i + a)] = cells[(d + 1) * (int64_t)order[(size_t)i] + a];
    std::vector<int32_t> tile_ptr((size_t)n_tiles + 1), tile_rows((size_t)ns);
    std::vector<uint16_t> cell_pos((size_t)ns);
    if (int rc = stk_solid_tile_rows(d, nv, nc, placed.data(), row_of.data(), tile_ptr.data(), tile_rows.data(),
                                     cell_pos.data()))
        return rc;

    stk_solid_plan *p = new stk_solid_plan();
    p->d = d, p->nv = nv, p->nc = nc, p->n_free = n_free, p->n_tiles = n_tiles;
    p->longest = 0;
    for (int64_t i = 0; i < n_tiles; ++i) p->longest = std::max(p->longest, tile_ptr[(size_t)i + 1] - tile_ptr[(size_t)i]);
    stk_dev_arrays &dev = p->dev;
    int rc = p1_mesh_upload(dev, &p->mesh, d, nv, nc, points, placed.data(), nullptr);
    if (!rc) rc = !(p->cell_of = dev.upload(order)) || !(p->tile_ptr = dev.upload(tile_ptr));
    if (!rc) rc = !(p->tile_rows = dev.upload(tile_rows.data(), (size_t)tile_ptr[(size_t)n_tiles]));
    if (!rc) rc = !(p->cell_pos = dev.upload(cell_pos));
    if (!rc) rc = p1_geometry(who, dev, p, nullptr);  // (the scan has no use for |T|)
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return 0;
}

extern "C" int stk_solid_plan_destroy(stk_solid_plan *plan)
{
    delete plan;
    return 0;
}

extern "C" int stk_solid_scan(void *stream, stk_solid_plan *plan, int64_t M, int32_t n_cols, const double *slab,
                              int64_t row_stride, int64_t k_first, double h, double threshold, int32_t fresh,
                              double *state)
{
    STK_REQUIRE(plan != nullptr, "stk_solid_scan: plan is null");
    STK_REQUIRE(slab != nullptr, "stk_solid_scan: slab is null");
    STK_REQUIRE(state != nullptr, "stk_solid_scan: state is null");
    STK_REQUIRE(M == plan->n_free, "stk_solid_scan: M = %lld, the plan has %lld free dofs", (long long)M,
                (long long)plan->n_free);
    STK_REQUIRE(n_cols >= 0, "stk_solid_scan: n_cols = %d is negative", n_cols);
    STK_REQUIRE(!(fresh && n_cols == 0), "stk_solid_scan: fresh with n_cols = 0: no column to start from");
    STK_REQUIRE(k_first >= 0, "stk_solid_scan: k_first = %lld is negative", (long long)k_first);
    STK_REQUIRE(std::isfinite(h) && h > 0.0, "stk_solid_scan: h = %g is not a positive finite step", h);
    STK_REQUIRE(!std::isnan(threshold), "stk_solid_scan: threshold is NaN");
    STK_REQUIRE(row_stride >= n_cols, "stk_solid_scan: row_stride = %lld is below n_cols = %d", (long long)row_stride,
                n_cols);
    if (n_cols == 0) return 0;
    hipStream_t st = stk_stream(stream);
    // the widest chunk whose odd-strided image of the longest list fits -- the budget, or the
    // columns asked for under the largest budget -- then the columns spread evenly over that
    // many chunks
    const int64_t longest = plan->longest > 0 ? plan->longest : 1;
    const int32_t asked = g_tile_cols.load(std::memory_order_relaxed);
    const int64_t budget = (int64_t)(asked ? TILE_KIB_MAX : g_tile_kib.load(std::memory_order_relaxed)) * 1024;
    int64_t widest = budget / (8 * longest) - 1;
    if (asked && widest > asked) widest = asked;
    if (widest > TILE_COLS_MAX) widest = TILE_COLS_MAX;
    if (widest < 1) widest = 1;
    const int32_t n_chunks = (int32_t)((n_cols + widest - 1) / widest);
    const int32_t cw = (n_cols + n_chunks - 1) / n_chunks;
    const size_t lds = (size_t)longest * (cw | 1) * sizeof(double);
    const dim3 grid((unsigned)plan->n_tiles);  // (below 2^23 by the checks of the plan)
    if (plan->d == 2)
        hipLaunchKernelGGL(solid_scan_kernel<2>, grid, dim3(BS), lds, st, plan->nc, n_cols, slab, row_stride, k_first, h,
                           threshold, fresh, state, cw, plan->tile_ptr, plan->tile_rows, plan->cell_pos, plan->grad,
                           plan->cell_of);
    else
        hipLaunchKernelGGL(solid_scan_kernel<3>, grid, dim3(BS), lds, st, plan->nc, n_cols, slab, row_stride, k_first, h,
                           threshold, fresh, state, cw, plan->tile_ptr, plan->tile_rows, plan->cell_pos, plan->grad,
                           plan->cell_of);
    STK_LAUNCH_CHECK();
    return 0;
}

extern "C" int stk_solid_order(int32_t caller_order)
{
    STK_REQUIRE(caller_order == 0 || caller_order == 1, "stk_solid_order: caller_order = %d is neither 0 nor 1", caller_order);
    g_caller_order.store(caller_order, std::memory_order_relaxed);
    return 0;
}

extern "C" int stk_solid_tile(int32_t cols, int32_t lds_kib)
{
    STK_REQUIRE(cols >= 0 && cols <= TILE_COLS_MAX, "stk_solid_tile: cols = %d not in 0..%d", cols, TILE_COLS_MAX);
    STK_REQUIRE(lds_kib >= 0 && lds_kib <= TILE_KIB_MAX, "stk_solid_tile: lds_kib = %d not in 0..%d", lds_kib, TILE_KIB_MAX);
    g_tile_cols.store(cols, std::memory_order_relaxed);
    g_tile_kib.store(lds_kib ? lds_kib : TILE_KIB, std::memory_order_relaxed);
    return 0;
}
