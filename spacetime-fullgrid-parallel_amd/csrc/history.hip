// Thermal history maps (include/stk.h "history maps"): per row -- a spatial dof of a
// trial-space slab, or a sampled point -- the peak and its time, the dose (the integral over
// time), the time above a threshold with the first and last crossing, and the largest and
// smallest rate, all from ONE pass over the node values.  The function is piecewise linear
// in time, so every one of them is a reduction along the row; the state of nine doubles
// (STK_HISTORY_STATE) is carried from call to call, so a scan of columns [k0, k1) followed
// by one of [k1, k2) is the scan of [k0, k2), double for double.
//
//  * history_slab_kernel   rows contiguous in time (u[i*ld + c]): a workgroup of R lanes takes
//                          a tile of R consecutive rows -- one run of R*ld doubles -- and
//                          streams it through LDS in chunks of cw columns, every lane loading
//                          along the run (8-byte loads: the pointer is only 8-byte aligned),
//                          then lane r walks row r in ascending k.  The LDS rows are
//                          re-strided to an ODD length, so the 8-byte reads of 32 neighbouring
//                          lanes fall on 32 distinct pairs of the 64 banks.  The state stays in
//                          registers over the chunks of a tile.
//  * history_cols_kernel   rows strided (u[i + c*ld]: the (n_k, n_p) block of the sampler): one
//                          lane per row, every load and every state access coalesced, no LDS.
//
// Grid-stride over tiles, 64-bit offsets, no atomics, nothing allocated, no synchronisation.
//
// ARITHMETIC: every operation rounded on its own -- contraction is SWITCHED OFF for this file
// (the pragma and -ffp-contract=off in the Makefile), and no kernel here calls fma.
#include <cmath>

#include "stk_common.h"

#pragma clang fp contract(off)

namespace {

struct hist_state {
    double peak, t_peak, dose, above, t_first, t_last, max_rate, min_rate, last;
};

__device__ inline void hist_fresh(hist_state &s, double v, int64_t k, double h, double theta)
{
    const double tk = (double)k * h;
    s.peak = s.last = v;
    s.t_peak = tk;
    s.dose = s.above = 0.0;
    s.t_first = s.t_last = v > theta ? tk : __builtin_nan("");
    s.max_rate = -__builtin_inf();
    s.min_rate = __builtin_inf();
}

// inv_h: 1 / h where that is exact (h a power of two: the product is then the quotient, bit
// for bit, and costs no division), else 0.0
__device__ inline void hist_step(hist_state &s, double b, int64_t k, double h, double half_h, double inv_h,
                                 double theta)
{
    const double a = s.last;
    const double tk = (double)k * h;
    if (b > s.peak) {
        s.peak = b;
        s.t_peak = tk;
    }
    s.dose = s.dose + (a + b) * half_h;
    const double rate = inv_h != 0.0 ? (b - a) * inv_h : (b - a) / h;
    if (rate > s.max_rate) s.max_rate = rate;
    if (rate < s.min_rate) s.min_rate = rate;
    const bool a_up = a > theta, b_up = b > theta;
    if (a_up && b_up) {
        s.above = s.above + h;
        s.t_last = tk;
    } else if (b_up) {
        const double x = (theta - a) / (b - a);
        s.above = s.above + h * (1.0 - x);
        if (s.t_first != s.t_first) s.t_first = ((double)(k - 1) + x) * h;
        s.t_last = tk;
    } else if (a_up) {
        const double x = (theta - a) / (b - a);
        s.above = s.above + h * x;
        s.t_last = ((double)(k - 1) + x) * h;
    }
    s.last = b;
}

__device__ inline void hist_read(hist_state &s, const double *state, int64_t M, int64_t i)
{
    s.peak = state[i];
    s.t_peak = state[M + i];
    s.dose = state[2 * M + i];
    s.above = state[3 * M + i];
    s.t_first = state[4 * M + i];
    s.t_last = state[5 * M + i];
    s.max_rate = state[6 * M + i];
    s.min_rate = state[7 * M + i];
    s.last = state[8 * M + i];
}

__device__ inline void hist_write(const hist_state &s, double *state, int64_t M, int64_t i)
{
    state[i] = s.peak;
    state[M + i] = s.t_peak;
    state[2 * M + i] = s.dose;
    state[3 * M + i] = s.above;
    state[4 * M + i] = s.t_first;
    state[5 * M + i] = s.t_last;
    state[6 * M + i] = s.max_rate;
    state[7 * M + i] = s.min_rate;
    state[8 * M + i] = s.last;
}

// Tile of R rows by chunks of cw columns; LDS image [R][ldp], ldp = cw | 1.  The flat index
// j = r * cw + c of a chunk runs over the lanes: consecutive lanes read consecutive doubles
// of a row piece, and with cw = n_cols the pieces of a tile are the run of the rows itself
// (less the padding column).  (r, c) advance by (R / cw, R % cw) per step: no division in
// the loop.
template <int R>
__global__ __launch_bounds__(R) void history_slab_kernel(int64_t M, int32_t n_cols, const double *__restrict__ u,
                                                         int64_t ld, int64_t k_first, double h, double inv_h,
                                                         double theta, int32_t fresh,
                                                         double *__restrict__ state, int32_t cw,
                                                         int64_t n_tiles)
{
    extern __shared__ double tile[];
    const int ldp = cw | 1;
    const int tid = threadIdx.x;
    const int r_first = tid / cw, c_first = tid - r_first * cw;
    const int dr = R / cw, dc = R - dr * cw;
    const int64_t dg = (int64_t)dr * ld + dc;
    const int dl = dr * ldp + dc;
    const double half_h = 0.5 * h;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t row0 = t * R;
        const int rows = (int)(M - row0 < R ? M - row0 : R);
        const bool mine = tid < rows;
        hist_state s;
        if (mine && !fresh) hist_read(s, state, M, row0 + tid);
        const double *base = u + row0 * ld;
        for (int32_t c0 = 0; c0 < n_cols; c0 += cw) {
            const int here = n_cols - c0 < cw ? n_cols - c0 : cw;
            if (c0) __syncthreads();  // the walk of the chunk before is over
            // global and LDS offsets advance with (r, c): no multiplication per element
            int64_t g = (int64_t)r_first * ld + c_first + c0;
            int l = r_first * ldp + c_first;
            for (int r = r_first, c = c_first; r < rows;) {
                if (c < here) tile[l] = base[g];
                r += dr;
                c += dc;
                g += dg;
                l += dl;
                if (c >= cw) {
                    c -= cw;
                    ++r;
                    g += ld - cw;
                    l += ldp - cw;
                }
            }
            __syncthreads();
            if (mine) {
                const double *row = tile + tid * ldp;
                int c = 0;
                if (fresh && c0 == 0) {
                    hist_fresh(s, row[0], k_first, h, theta);
                    c = 1;
                }
                const int64_t k0 = k_first + c0;
                for (; c + 4 <= here; c += 4) {  // four LDS reads in flight ahead of their steps
                    const double v0 = row[c], v1 = row[c + 1], v2 = row[c + 2], v3 = row[c + 3];
                    hist_step(s, v0, k0 + c, h, half_h, inv_h, theta);
                    hist_step(s, v1, k0 + c + 1, h, half_h, inv_h, theta);
                    hist_step(s, v2, k0 + c + 2, h, half_h, inv_h, theta);
                    hist_step(s, v3, k0 + c + 3, h, half_h, inv_h, theta);
                }
                for (; c < here; ++c) hist_step(s, row[c], k0 + c, h, half_h, inv_h, theta);
            }
        }
        if (mine) hist_write(s, state, M, row0 + tid);
        __syncthreads();  // the next tile's loads overwrite this one
    }
}

constexpr int COLS_BS = 256;

__global__ __launch_bounds__(COLS_BS) void history_cols_kernel(int64_t M, int32_t n_cols,
                                                               const double *__restrict__ u, int64_t ld,
                                                               int64_t k_first, double h, double inv_h, double theta,
                                                               int32_t fresh, double *__restrict__ state)
{
    const double half_h = 0.5 * h;
    const int64_t stride = (int64_t)gridDim.x * COLS_BS;
    for (int64_t i = (int64_t)blockIdx.x * COLS_BS + threadIdx.x; i < M; i += stride) {
        hist_state s;
        int32_t c = 0;
        if (fresh) {
            hist_fresh(s, u[i], k_first, h, theta);
            c = 1;
        } else {
            hist_read(s, state, M, i);
        }
        for (; c < n_cols; ++c) hist_step(s, u[i + (int64_t)c * ld], k_first + c, h, half_h, inv_h, theta);
        hist_write(s, state, M, i);
    }
}

// 1 / h if h is a power of two whose reciprocal is a normal number, else 0.0
double exact_reciprocal(double h)
{
    int e = 0;
    if (std::frexp(h, &e) != 0.5 || e < -1000 || e > 1000) return 0.0;
    return 1.0 / h;
}

// the tile of the slab form (stk_history_tile): rows per workgroup and its LDS in KiB.  The
// default -- chunks of 9 columns, up to eight workgroups resident per CU -- is the fastest of those
// measured on the 65-column slab
constexpr int TILE_ROWS = 256, TILE_KIB = 20;
std::atomic<int32_t> g_tile_rows{TILE_ROWS}, g_tile_kib{TILE_KIB};

template <int R>
int launch_slab(hipStream_t st, int64_t M, int32_t n_cols, const double *u, int64_t ld, int64_t k_first, double h,
                double theta, int32_t fresh, double *state)
{
    // the widest chunk whose odd-strided image fits, then the columns spread evenly over
    // that many chunks
    int32_t widest = g_tile_kib.load(std::memory_order_relaxed) * 1024 / (8 * R) - 1;
    if (widest < 1) widest = 1;
    const int32_t n_chunks = (n_cols + widest - 1) / widest;
    const int32_t cw = (n_cols + n_chunks - 1) / n_chunks;
    const size_t lds = (size_t)R * (cw | 1) * sizeof(double);
    const int64_t n_tiles = (M + R - 1) / R;
    const int64_t cap = (int64_t)stk_cu_count() * 16;  // grid-stride beyond that
    const unsigned grid = (unsigned)(n_tiles < cap ? n_tiles : cap);
    hipLaunchKernelGGL((history_slab_kernel<R>), dim3(grid), dim3(R), lds, st, M, n_cols, u, ld, k_first, h,
                       exact_reciprocal(h), theta, fresh, state, cw, n_tiles);
    STK_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int stk_history_scan(void *stream, int64_t M, int32_t n_cols, const double *u, int64_t row_stride,
                                int64_t col_stride, int64_t k_first, double h, double threshold, int32_t fresh,
                                double *state)
{
    STK_REQUIRE(u != nullptr, "stk_history_scan: u is null");
    STK_REQUIRE(state != nullptr, "stk_history_scan: state is null");
    STK_REQUIRE(M >= 0, "stk_history_scan: M = %lld is negative", (long long)M);
    STK_REQUIRE(n_cols >= 0, "stk_history_scan: n_cols = %d is negative", n_cols);
    STK_REQUIRE(!(fresh && n_cols == 0), "stk_history_scan: fresh with n_cols = 0: no column to start from");
    STK_REQUIRE(k_first >= 0, "stk_history_scan: k_first = %lld is negative", (long long)k_first);
    STK_REQUIRE(std::isfinite(h) && h > 0.0, "stk_history_scan: h = %g is not a positive finite step", h);
    STK_REQUIRE(!std::isnan(threshold), "stk_history_scan: threshold is NaN");
    const bool slab = col_stride == 1 && row_stride >= (n_cols > 0 ? n_cols : 1);
    const bool cols = !slab && row_stride == 1 && col_stride >= (M > 0 ? M : 1);
    STK_REQUIRE(slab || cols,
                "stk_history_scan: row_stride = %lld, col_stride = %lld is neither a slab (col_stride 1, "
                "row_stride >= n_cols) nor a time-major block (row_stride 1, col_stride >= M)",
                (long long)row_stride, (long long)col_stride);
    if (M == 0 || n_cols == 0) return 0;
    hipStream_t st = stk_stream(stream);
    if (cols) {
        hipLaunchKernelGGL(history_cols_kernel, dim3(stk_flat_grid(M, COLS_BS)), dim3(COLS_BS), 0, st, M, n_cols, u,
                           col_stride, k_first, h, exact_reciprocal(h), threshold, fresh, state);
        STK_LAUNCH_CHECK();
        return 0;
    }
    switch (g_tile_rows.load(std::memory_order_relaxed)) {
    case 64:
        return launch_slab<64>(st, M, n_cols, u, row_stride, k_first, h, threshold, fresh, state);
    case 128:
        return launch_slab<128>(st, M, n_cols, u, row_stride, k_first, h, threshold, fresh, state);
    case 512:
        return launch_slab<512>(st, M, n_cols, u, row_stride, k_first, h, threshold, fresh, state);
    default:
        return launch_slab<256>(st, M, n_cols, u, row_stride, k_first, h, threshold, fresh, state);
    }
}

extern "C" int stk_history_tile(int32_t rows, int32_t lds_kib)
{
    STK_REQUIRE(rows == 0 || rows == 64 || rows == 128 || rows == 256 || rows == 512,
                "stk_history_tile: rows = %d is none of 0, 64, 128, 256, 512", rows);
    STK_REQUIRE(lds_kib >= 0 && lds_kib <= 64, "stk_history_tile: lds_kib = %d not in 0..64", lds_kib);
    g_tile_rows.store(rows ? rows : TILE_ROWS, std::memory_order_relaxed);
    g_tile_kib.store(lds_kib ? lds_kib : TILE_KIB, std::memory_order_relaxed);
    return 0;
}
