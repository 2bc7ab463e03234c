// Level transfer (include/stk.h "level transfer"): the trial-space slab of a coarser
// discretisation -- one space level fewer and/or 2^a times fewer time elements -- prolonged to
// the slab of the finer one that represents the same function.  ONE kernel reads the coarse
// slab once and writes the fine slab once:
//
//  * prolong_kernel   a workgroup of 256 lanes takes a tile of R consecutive fine rows for the
//                     columns of the call, in chunks of cw fine columns where the LDS budget
//                     asks for it.  Phase 1: the coarse runs of the tile's parents, lanes along
//                     time (a run of 33 doubles is 264 contiguous bytes), the spatial rule
//                     applied on the way, the rows s_i(q) left in LDS at an ODD stride.
//                     Phase 2: lanes walk the tile's output in pairs of columns, row after row
//                     (rows lie back to back in the slab, so the stores of a wave stay one run
//                     across row ends); the rule in time from two LDS reads; a 16-byte store
//                     where the pair is aligned, 8-byte stores elsewhere.  The pad column of
//                     an odd n_cols is never written.
//
// The parents of a tile are staged in LDS first, so that the loads of phase 1 depend on LDS,
// not on a second global load.  Grid-stride over tiles, 64-bit offsets, no atomics, nothing
// allocated, no synchronisation.
//
// ARITHMETIC: every operation rounded on its own -- contraction is SWITCHED OFF for this file
// (the pragma and -ffp-contract=off in the Makefile), and no kernel here calls fma.
#include <string>
#include <vector>

#include "host_threads.h"
#include "stk_common.h"

#pragma clang fp contract(off)

struct stk_transfer_plan {
    int64_t M_fine, M_coarse;
    int32_t *parents;  // device, [M_fine][2]
    stk_dev_arrays dev;
};

namespace {

constexpr int BS = 256;

// (r, c) of the flat index j = r * w + c advance by (BS / w, BS % w) per step: no division
// in the loops (the walk of history.hip)
template <int R>
__global__ __launch_bounds__(BS) void prolong_kernel(int64_t M, const int32_t *__restrict__ parents, int32_t a,
                                                     const double *__restrict__ uc, int64_t ldc, int64_t qc_first,
                                                     double *__restrict__ out, int64_t ld, int64_t k_first,
                                                     int32_t n_cols, int32_t cw, int32_t ldq, int32_t wide,
                                                     int64_t n_tiles)
{
    extern __shared__ double tile[];  // [R][ldq]: s_i(q) of the chunk
    __shared__ int32_t par[R][2];
    const int tid = threadIdx.x;
    const int64_t mask = ((int64_t)1 << a) - 1;
    const double scale = 1.0 / (double)((int64_t)1 << a);  // a power of two: rem * scale is exact
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t row0 = t * R;
        const int rows = (int)(M - row0 < R ? M - row0 : R);
        if (tid < rows) {
            par[tid][0] = parents[2 * (row0 + tid)];
            par[tid][1] = parents[2 * (row0 + tid) + 1];
        }
        for (int32_t c0 = 0; c0 < n_cols; c0 += cw) {
            const int here = n_cols - c0 < cw ? n_cols - c0 : cw;
            const int64_t k0 = k_first + c0, k_last = k0 + here - 1;
            const int64_t q_lo = k0 >> a;
            const int nq = (int)((k_last >> a) + ((k_last & mask) != 0 ? 1 : 0) - q_lo) + 1;  // <= ldq
            __syncthreads();  // the parents are there; the walk of the chunk before is over
            {
                const int64_t col0 = q_lo - qc_first;
                const int dr = BS / nq, dc = BS - dr * nq;
                int r = tid / nq, c = tid - r * nq;
                while (r < rows) {
                    const int32_t p0 = par[r][0], p1 = par[r][1];
                    double v;
                    if (p0 == p1 && p0 >= 0) {
                        v = uc[(int64_t)p0 * ldc + col0 + c];
                    } else {
                        const double A = p0 >= 0 ? uc[(int64_t)p0 * ldc + col0 + c] : 0.0;
                        const double B = p1 >= 0 ? uc[(int64_t)p1 * ldc + col0 + c] : 0.0;
                        v = (A + B) * 0.5;
                    }
                    tile[r * ldq + c] = v;
                    r += dr;
                    c += dc;
                    if (c >= nq) {
                        c -= nq;
                        ++r;
                    }
                }
            }
            __syncthreads();
            {
                const int np = (here + 1) >> 1;  // pairs of columns per row
                const int dr = BS / np, dc = BS - dr * np;
                int r = tid / np, pp = tid - r * np;
                double *base = out + row0 * ld + c0;
                while (r < rows) {
                    const int c = 2 * pp;
                    const bool two = c + 1 < here;
                    double v[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        v[e] = 0.0;
                        if (e == 1 && !two) continue;  // past the chunk: neither read nor stored
                        const int64_t k = k0 + c + e;
                        const int64_t rem = k & mask;
                        const int at = r * ldq + (int)((k >> a) - q_lo);
                        const double s0 = tile[at];
                        if (rem == 0) {
                            v[e] = s0;
                        } else {
                            const double w1 = (double)rem * scale, w0 = 1.0 - w1;
                            v[e] = w0 * s0 + w1 * tile[at + 1];
                        }
                    }
                    double *dst = base + (int64_t)r * ld + c;
                    if (wide && two) {
                        *reinterpret_cast<double2 *>(dst) = make_double2(v[0], v[1]);
                    } else {
                        dst[0] = v[0];
                        if (two) dst[1] = v[1];
                    }
                    r += dr;
                    pp += dc;
                    if (pp >= np) {
                        pp -= np;
                        ++r;
                    }
                }
            }
        }
        __syncthreads();  // the next tile's parents overwrite this one's
    }
}

// the launch form (stk_transfer_tile): fine rows per workgroup and its LDS in KiB
constexpr int TILE_ROWS = 64, TILE_KIB = 64;
std::atomic<int32_t> g_tile_rows{TILE_ROWS}, g_tile_kib{TILE_KIB};

template <int R>
int launch(hipStream_t st, const stk_transfer_plan *plan, int32_t a, const double *uc, int64_t ldc, int64_t qc_first,
           double *out, int64_t ld, int64_t k_first, int32_t n_cols)
{
    // the odd LDS stride the budget allows (at least 3: a chunk of one column reads two), the
    // widest chunk whose coarse window fits it -- ((cw - 1) >> a) + 3 doubles bound the window
    // of ANY cw consecutive fine columns -- then the columns spread evenly over the chunks
    // (the budget covers the staged parents too: 8 R bytes)
    int32_t ldq_max = (g_tile_kib.load(std::memory_order_relaxed) * 1024 - 8 * R) / (8 * R);
    if (!(ldq_max & 1)) --ldq_max;
    if (ldq_max < 3) ldq_max = 3;
    const int64_t widest = (int64_t)(ldq_max - 2) << a;
    int32_t cw = n_cols, n_chunks = 1;
    if (widest < n_cols) {
        n_chunks = (int32_t)((n_cols + widest - 1) / widest);
        cw = (n_cols + n_chunks - 1) / n_chunks;
        if ((cw & 1) && cw + 1 <= widest) ++cw;  // even chunks keep the pairs of a row aligned
    }
    const int32_t ldq = (((cw - 1) >> a) + 3) | 1;
    // 16-byte stores: every pair of every row and chunk on a 16-byte address
    const int32_t wide = ((uintptr_t)out % 16 == 0) && !(ld & 1) && (n_chunks == 1 || !(cw & 1));
    const size_t lds = (size_t)R * ldq * sizeof(double);
    const int64_t n_tiles = (plan->M_fine + R - 1) / R;
    const int64_t cap = (int64_t)stk_cu_count() * 16;  // grid-stride beyond that
    const unsigned grid = (unsigned)(n_tiles < cap ? n_tiles : cap);
    hipLaunchKernelGGL((prolong_kernel<R>), dim3(grid), dim3(BS), lds, st, plan->M_fine, plan->parents, a, uc, ldc,
                       qc_first, out, ld, k_first, n_cols, cw, ldq, wide, n_tiles);
    STK_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// the checks of a parents table, shared by the creators of both directions (`who` names the caller)
static int check_parents(const char *who, int64_t M_fine, int64_t M_coarse, const int32_t *parents)
{
    STK_REQUIRE(M_fine >= 0, "%s: M_fine = %lld is negative", who, (long long)M_fine);
    STK_REQUIRE(M_coarse >= 0 && M_coarse <= INT32_MAX, "%s: M_coarse = %lld not in 0..2^31-1", who,
                (long long)M_coarse);
    STK_REQUIRE(parents != nullptr || M_fine == 0, "%s: parents is null", who);
    for (int64_t i = 0; i < M_fine; ++i) {
        const int32_t p0 = parents[2 * i], p1 = parents[2 * i + 1];
        STK_REQUIRE(p0 >= -1 && p0 < M_coarse && p1 >= -1 && p1 < M_coarse,
                    "%s: parents[%lld] = (%d, %d) not in [-1, M_coarse = %lld)", who, (long long)i, p0, p1,
                    (long long)M_coarse);
        // the coarse level's own vertices come first (the hierarchical numbering) and copy
        STK_REQUIRE(!(p0 == -1 && p1 == -1 && i < M_coarse),
                    "%s: parents[%lld] = (-1, -1) in a row below M_coarse = %lld, a vertex of "
                    "the coarse level: a copy pair without a row to copy",
                    who, (long long)i, (long long)M_coarse);
    }
    return 0;
}

extern "C" int stk_transfer_plan_create(int64_t M_fine, int64_t M_coarse, const int32_t *parents,
                                        stk_transfer_plan **out)
{
    STK_REQUIRE(out != nullptr, "stk_transfer_plan_create: out is null");
    *out = nullptr;
    if (const int rc = check_parents("stk_transfer_plan_create", M_fine, M_coarse, parents)) return rc;
    stk_transfer_plan *plan = new stk_transfer_plan();
    plan->M_fine = M_fine, plan->M_coarse = M_coarse;
    if (M_fine > 0 && !(plan->parents = plan->dev.upload(parents, (size_t)M_fine * 2))) {
        const std::string why = stk_last_error();
        stk_set_error("stk_transfer_plan_create: the upload of the parents failed: %s", why.c_str());
        delete plan;
        return 1;
    }
    *out = plan;
    return 0;
}

extern "C" int stk_transfer_plan_destroy(stk_transfer_plan *plan)
{
    delete plan;
    return 0;
}

extern "C" int stk_transfer_tile(int32_t rows, int32_t lds_kib)
{
    STK_REQUIRE(rows == 0 || rows == 64 || rows == 128 || rows == 256,
                "stk_transfer_tile: rows = %d is none of 0, 64, 128, 256", rows);
    STK_REQUIRE(lds_kib >= 0 && lds_kib <= 64, "stk_transfer_tile: lds_kib = %d not in 0..64", lds_kib);
    g_tile_rows.store(rows ? rows : TILE_ROWS, std::memory_order_relaxed);
    g_tile_kib.store(lds_kib ? lds_kib : TILE_KIB, std::memory_order_relaxed);
    return 0;
}

extern "C" int stk_transfer_prolong(void *stream, const stk_transfer_plan *plan, int32_t a, const double *uc,
                                    int64_t ldc, int64_t qc_first, int32_t n_cc, double *out, int64_t ld,
                                    int64_t k_first, int32_t n_cols)
{
    STK_REQUIRE(plan != nullptr, "stk_transfer_prolong: plan is null");
    STK_REQUIRE(uc != nullptr, "stk_transfer_prolong: uc is null");
    STK_REQUIRE(out != nullptr, "stk_transfer_prolong: out is null");
    STK_REQUIRE(a >= 0 && a <= STK_TRANSFER_MAX_A, "stk_transfer_prolong: a = %d not in 0..%d", a, STK_TRANSFER_MAX_A);
    STK_REQUIRE(n_cc >= 0, "stk_transfer_prolong: n_cc = %d is negative", n_cc);
    STK_REQUIRE(n_cols >= 0, "stk_transfer_prolong: n_cols = %d is negative", n_cols);
    STK_REQUIRE(qc_first >= 0, "stk_transfer_prolong: qc_first = %lld is negative", (long long)qc_first);
    STK_REQUIRE(k_first >= 0, "stk_transfer_prolong: k_first = %lld is negative", (long long)k_first);
    STK_REQUIRE(ldc >= n_cc, "stk_transfer_prolong: ldc = %lld is below n_cc = %d", (long long)ldc, n_cc);
    STK_REQUIRE(ld >= n_cols, "stk_transfer_prolong: ld = %lld is below n_cols = %d", (long long)ld, n_cols);
    if (n_cols == 0 || plan->M_fine == 0) return 0;
    const int64_t mask = ((int64_t)1 << a) - 1;
    const int64_t k_last = k_first + n_cols - 1;
    const int64_t q_first = k_first >> a, q_last = (k_last >> a) + ((k_last & mask) != 0 ? 1 : 0);
    STK_REQUIRE(q_first >= qc_first && q_last < qc_first + n_cc,
                "stk_transfer_prolong: the coarse window [qc_first, qc_first + n_cc) = [%lld, %lld) does not cover "
                "the columns [%lld, %lld] that the fine columns [%lld, %lld] read at a = %d",
                (long long)qc_first, (long long)(qc_first + n_cc), (long long)q_first, (long long)q_last,
                (long long)k_first, (long long)k_last, a);
    hipStream_t st = stk_stream(stream);
    switch (g_tile_rows.load(std::memory_order_relaxed)) {
    case 128:
        return launch<128>(st, plan, a, uc, ldc, qc_first, out, ld, k_first, n_cols);
    case 256:
        return launch<256>(st, plan, a, uc, ldc, qc_first, out, ld, k_first, n_cols);
    default:
        return launch<64>(st, plan, a, uc, ldc, qc_first, out, ld, k_first, n_cols);
    }
}

// ---- restriction P^T: the adjoint of the above (include/stk.h "restriction") ---------------------
// A coarse row gathers its own fine row and its children through a host-built transposed table
// (stk_transfer_children: CSR per coarse row, fine rows ascending, the weight in bit 0 of an
// entry), so every sum has ONE order -- no float atomics, no scatter.
//
//  * restrict_kernel  a workgroup of 256 lanes takes a tile of `R` consecutive coarse rows, in
//                     chunks of whole time stencils where the LDS budget asks for it.  Phase 1:
//                     lanes along time over the fine runs of each entry's row, the entries of a
//                     row folded in list order, g_j(k) left in LDS at an ODD stride.  Phase 2:
//                     lanes over (row, q) fold the up to 2^(a+1) - 1 LDS values of the stencil
//                     of q in ascending k and store out, one run across row ends.  IDENT: the
//                     time-only form, g_j = f_j, no table read.
struct stk_restrict_plan {
    int64_t M_fine, M_coarse;
    int64_t *ptr;  // device, [M_coarse + 1]
    int32_t *ent;  // device, [ptr[M_coarse]]: (fine row << 1) | (1 where the weight is 0.5)
    stk_dev_arrays dev;
};

namespace {

template <bool IDENT>
__global__ __launch_bounds__(BS) void restrict_kernel(int64_t M, int32_t R, const int64_t *__restrict__ ptr,
                                                      const int32_t *__restrict__ ent, int32_t a,
                                                      const double *__restrict__ f, int64_t ld, int64_t k_first,
                                                      int64_t n_fine, double *__restrict__ out, int64_t ldc,
                                                      int64_t q_first, int32_t n_qc, int32_t qw, int32_t ldk,
                                                      int64_t n_tiles)
{
    extern __shared__ double tile[];  // [R][ldk]: g_j(k) of the chunk's fine window
    const int tid = threadIdx.x;
    const int64_t two_a = (int64_t)1 << a;
    const double scale = 1.0 / (double)two_a;  // a power of two: rem * scale is exact
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t row0 = t * R;
        const int rows = (int)(M - row0 < R ? M - row0 : R);
        for (int32_t c0 = 0; c0 < n_qc; c0 += qw) {
            const int here = n_qc - c0 < qw ? n_qc - c0 : qw;
            const int64_t qa = q_first + c0, qb = qa + here - 1;
            int64_t k_lo = (qa - 1) * two_a + 1, k_hi = (qb + 1) * two_a - 1;
            if (k_lo < 0) k_lo = 0;
            if (k_hi > n_fine - 1) k_hi = n_fine - 1;
            const int nk = (int)(k_hi - k_lo) + 1;  // <= ldk
            __syncthreads();                        // the walk of the chunk before is over
            {
                const int64_t col0 = k_lo - k_first;
                const int dr = BS / nk, dc = BS - dr * nk;
                int r = tid / nk, c = tid - r * nk;
                while (r < rows) {
                    double g;
                    if (IDENT) {
                        g = f[(row0 + r) * ld + col0 + c];
                    } else {
                        int64_t e = ptr[row0 + r];
                        const int64_t e1 = ptr[row0 + r + 1];
                        g = 0.0;
                        if (e < e1) {
                            int32_t en = ent[e];
                            g = ((en & 1) ? 0.5 : 1.0) * f[(int64_t)(en >> 1) * ld + col0 + c];
                            for (++e; e < e1; ++e) {
                                en = ent[e];
                                g = g + ((en & 1) ? 0.5 : 1.0) * f[(int64_t)(en >> 1) * ld + col0 + c];
                            }
                        }
                    }
                    tile[r * ldk + c] = g;
                    r += dr;
                    c += dc;
                    if (c >= nk) {
                        c -= nk;
                        ++r;
                    }
                }
            }
            __syncthreads();
            {
                const int dr = BS / here, dc = BS - dr * here;
                int r = tid / here, c = tid - r * here;
                while (r < rows) {
                    const int64_t kc = (qa + c) * two_a;
                    int64_t lo = kc - two_a + 1, hi = kc + two_a - 1;
                    if (lo < 0) lo = 0;
                    if (hi > n_fine - 1) hi = n_fine - 1;
                    const double *g = tile + r * ldk;
                    double acc = 0.0;
                    for (int64_t k = lo; k <= hi; ++k) {
                        const double w = k < kc ? (double)(k - (kc - two_a)) * scale
                                                : (k == kc ? 1.0 : 1.0 - (double)(k - kc) * scale);
                        const double term = w * g[k - k_lo];
                        acc = k == lo ? term : acc + term;
                    }
                    out[(row0 + r) * ldc + c0 + c] = acc;
                    r += dr;
                    c += dc;
                    if (c >= here) {
                        c -= here;
                        ++r;
                    }
                }
            }
        }
    }
}

// the launch form (stk_restrict_tile): coarse rows per workgroup and its LDS in KiB
constexpr int RTILE_ROWS = 32, RTILE_KIB = 64;
std::atomic<int32_t> g_rtile_rows{RTILE_ROWS}, g_rtile_kib{RTILE_KIB};

int launch_restrict(hipStream_t st, int64_t M, const int64_t *ptr, const int32_t *ent, int32_t a, const double *f,
                    int64_t ld, int64_t k_first, int64_t n_fine, double *out, int64_t ldc, int64_t q_first,
                    int32_t n_qc)
{
    // qw coarse columns read at most ((qw + 1) << a) - 1 fine ones.  The rows of a tile stay and the
    // chunk shrinks while one whole stencil fits the budget; below that the rows shrink, down to
    // one row of one stencil (4 088 bytes at a = 8), which every budget is allowed
    const int64_t budget = (int64_t)g_rtile_kib.load(std::memory_order_relaxed) * 1024 / 8;  // doubles
    int32_t R = g_rtile_rows.load(std::memory_order_relaxed);
    if ((int64_t)R > M) R = (int32_t)M;
    int64_t ldk_max = budget / R;
    if (!(ldk_max & 1)) --ldk_max;
    int64_t widest = ((ldk_max + 1) >> a) - 1;
    if (widest < 1) {
        widest = 1;
        const int64_t fit = budget / (((int64_t)2 << a) - 1);
        R = (int32_t)(fit < 1 ? 1 : (fit < R ? fit : R));
    }
    int32_t qw = n_qc;
    if (widest < n_qc) {
        const int32_t n_chunks = (int32_t)((n_qc + widest - 1) / widest);
        qw = (n_qc + n_chunks - 1) / n_chunks;
    }
    const int32_t ldk = (int32_t)((((int64_t)(qw + 1) << a) - 1) | 1);
    const size_t lds = (size_t)R * ldk * sizeof(double);
    const int64_t n_tiles = (M + R - 1) / R;
    const int64_t cap = (int64_t)stk_cu_count() * 16;  // grid-stride beyond that
    const unsigned grid = (unsigned)(n_tiles < cap ? n_tiles : cap);
    if (ent)
        hipLaunchKernelGGL((restrict_kernel<false>), dim3(grid), dim3(BS), lds, st, M, R, ptr, ent, a, f, ld, k_first,
                           n_fine, out, ldc, q_first, n_qc, qw, ldk, n_tiles);
    else
        hipLaunchKernelGGL((restrict_kernel<true>), dim3(grid), dim3(BS), lds, st, M, R, ptr, ent, a, f, ld, k_first,
                           n_fine, out, ldc, q_first, n_qc, qw, ldk, n_tiles);
    STK_LAUNCH_CHECK();
    return 0;
}

// the checks both restrictions share, after the pointers'; 1 in *noop where nothing is to be done
int check_restrict(const char *who, int32_t a, int64_t ld, int64_t k_first, int32_t n_cols, int64_t n_fine,
                   int64_t ldc, int64_t q_first, int32_t n_qc)
{
    STK_REQUIRE(a >= 0 && a <= STK_TRANSFER_MAX_A, "%s: a = %d not in 0..%d", who, a, STK_TRANSFER_MAX_A);
    STK_REQUIRE(n_cols >= 0, "%s: n_cols = %d is negative", who, n_cols);
    STK_REQUIRE(n_qc >= 0, "%s: n_qc = %d is negative", who, n_qc);
    STK_REQUIRE(n_fine >= 0, "%s: n_fine = %lld is negative", who, (long long)n_fine);
    STK_REQUIRE(k_first >= 0, "%s: k_first = %lld is negative", who, (long long)k_first);
    STK_REQUIRE(q_first >= 0, "%s: q_first = %lld is negative", who, (long long)q_first);
    STK_REQUIRE(ld >= n_cols, "%s: ld = %lld is below n_cols = %d", who, (long long)ld, n_cols);
    STK_REQUIRE(ldc >= n_qc, "%s: ldc = %lld is below n_qc = %d", who, (long long)ldc, n_qc);
    if (n_qc == 0) return 0;
    const int64_t two_a = (int64_t)1 << a;
    STK_REQUIRE(n_fine >= 1 && (n_fine - 1) % two_a == 0,
                "%s: n_fine = %lld: n_fine - 1 is no multiple of 2^a = %lld (or there is no node)", who,
                (long long)n_fine, (long long)two_a);
    const int64_t q_last = q_first + n_qc - 1;
    STK_REQUIRE(q_last <= (n_fine - 1) >> a,
                "%s: the coarse columns [q_first, q_first + n_qc) = [%lld, %lld) reach beyond the last coarse node "
                "%lld of n_fine = %lld at a = %d",
                who, (long long)q_first, (long long)(q_last + 1), (long long)((n_fine - 1) >> a), (long long)n_fine, a);
    int64_t k_lo = (q_first - 1) * two_a + 1, k_hi = (q_last + 1) * two_a - 1;
    if (k_lo < 0) k_lo = 0;
    if (k_hi > n_fine - 1) k_hi = n_fine - 1;
    STK_REQUIRE(k_first <= k_lo && k_hi < k_first + n_cols,
                "%s: the fine window [k_first, k_first + n_cols) = [%lld, %lld) does not cover the columns "
                "[%lld, %lld] that the coarse columns [%lld, %lld] read at a = %d",
                who, (long long)k_first, (long long)(k_first + n_cols), (long long)k_lo, (long long)k_hi,
                (long long)q_first, (long long)q_last, a);
    return 0;
}

}  // namespace

extern "C" int stk_transfer_children(int64_t M_fine, int64_t M_coarse, const int32_t *parents, int64_t *ptr,
                                     int32_t *entries)
{
    if (const int rc = check_parents("stk_transfer_children", M_fine, M_coarse, parents)) return rc;
    STK_REQUIRE(M_fine <= STK_RESTRICT_MAX_M_FINE,
                "stk_transfer_children: M_fine = %lld is above %lld, what an entry (fine row << 1 | half) can hold",
                (long long)M_fine, (long long)STK_RESTRICT_MAX_M_FINE);
    STK_REQUIRE(ptr != nullptr, "stk_transfer_children: ptr is null");
    STK_REQUIRE(entries != nullptr || M_fine == 0, "stk_transfer_children: entries is null");
    // a stable counting sort by coarse row.  Thread k owns the coarse rows [share(k), share(k + 1)):
    // it counts and later places the entries of ITS rows only, walking all fine rows in ascending
    // order -- so a row's entries ascend and the result does not depend on the number of threads
    const int T = host_threads(M_fine);
    auto each = [&](int k, auto put) {
        const int64_t j0 = share(M_coarse, T, k), j1 = share(M_coarse, T, k + 1);
        for (int64_t i = 0; i < M_fine; ++i) {
            const int32_t p0 = parents[2 * i], p1 = parents[2 * i + 1];
            if (p0 == p1) {
                if (p0 >= j0 && p0 < j1) put(p0, (int32_t)(i << 1));
            } else {
                if (p0 >= j0 && p0 < j1) put(p0, (int32_t)(i << 1) | 1);
                if (p1 >= j0 && p1 < j1) put(p1, (int32_t)(i << 1) | 1);
            }
        }
    };
    for (int64_t j = 0; j <= M_coarse; ++j) ptr[j] = 0;
    on_threads(T, [&](int k) { each(k, [&](int32_t j, int32_t) { ++ptr[j + 1]; }); });
    for (int64_t j = 0; j < M_coarse; ++j) ptr[j + 1] += ptr[j];
    std::vector<int64_t> at(ptr, ptr + M_coarse);
    on_threads(T, [&](int k) { each(k, [&](int32_t j, int32_t e) { entries[at[j]++] = e; }); });
    return 0;
}

extern "C" int stk_restrict_plan_create(int64_t M_fine, int64_t M_coarse, const int32_t *parents,
                                        stk_restrict_plan **out)
{
    STK_REQUIRE(out != nullptr, "stk_restrict_plan_create: out is null");
    *out = nullptr;
    if (const int rc = check_parents("stk_restrict_plan_create", M_fine, M_coarse, parents)) return rc;
    STK_REQUIRE(M_fine <= STK_RESTRICT_MAX_M_FINE, "stk_restrict_plan_create: M_fine = %lld is above %lld",
                (long long)M_fine, (long long)STK_RESTRICT_MAX_M_FINE);
    std::vector<int64_t> ptr((size_t)M_coarse + 1);
    std::vector<int32_t> ent((size_t)M_fine * 2 + 1);
    if (const int rc = stk_transfer_children(M_fine, M_coarse, parents, ptr.data(), ent.data())) return rc;
    ent.resize((size_t)ptr[M_coarse]);
    stk_restrict_plan *plan = new stk_restrict_plan();
    plan->M_fine = M_fine, plan->M_coarse = M_coarse;
    if (!(plan->ptr = plan->dev.upload(ptr)) || !(plan->ent = plan->dev.upload(ent))) {
        const std::string why = stk_last_error();
        stk_set_error("stk_restrict_plan_create: the upload of the transposed table failed: %s", why.c_str());
        delete plan;
        return 1;
    }
    *out = plan;
    return 0;
}

extern "C" int stk_restrict_plan_destroy(stk_restrict_plan *plan)
{
    delete plan;
    return 0;
}

extern "C" int stk_restrict_tile(int32_t rows, int32_t lds_kib)
{
    STK_REQUIRE(rows >= 0 && rows <= 256, "stk_restrict_tile: rows = %d not in 0..256", rows);
    STK_REQUIRE(lds_kib >= 0 && lds_kib <= 64, "stk_restrict_tile: lds_kib = %d not in 0..64", lds_kib);
    g_rtile_rows.store(rows ? rows : RTILE_ROWS, std::memory_order_relaxed);
    g_rtile_kib.store(lds_kib ? lds_kib : RTILE_KIB, std::memory_order_relaxed);
    return 0;
}

extern "C" int stk_transfer_restrict(void *stream, const stk_restrict_plan *plan, int32_t a, const double *f,
                                     int64_t ld, int64_t k_first, int32_t n_cols, int64_t n_fine, double *out,
                                     int64_t ldc, int64_t q_first, int32_t n_qc)
{
    STK_REQUIRE(plan != nullptr, "stk_transfer_restrict: plan is null");
    STK_REQUIRE(f != nullptr, "stk_transfer_restrict: f is null");
    STK_REQUIRE(out != nullptr, "stk_transfer_restrict: out is null");
    if (const int rc = check_restrict("stk_transfer_restrict", a, ld, k_first, n_cols, n_fine, ldc, q_first, n_qc))
        return rc;
    if (n_qc == 0 || plan->M_coarse == 0) return 0;
    return launch_restrict(stk_stream(stream), plan->M_coarse, plan->ptr, plan->ent, a, f, ld, k_first, n_fine, out,
                           ldc, q_first, n_qc);
}

extern "C" int stk_transfer_restrict_time(void *stream, int64_t M, int32_t a, const double *f, int64_t ld,
                                          int64_t k_first, int32_t n_cols, int64_t n_fine, double *out, int64_t ldc,
                                          int64_t q_first, int32_t n_qc)
{
    STK_REQUIRE(M >= 0, "stk_transfer_restrict_time: M = %lld is negative", (long long)M);
    STK_REQUIRE(f != nullptr, "stk_transfer_restrict_time: f is null");
    STK_REQUIRE(out != nullptr, "stk_transfer_restrict_time: out is null");
    if (const int rc =
            check_restrict("stk_transfer_restrict_time", a, ld, k_first, n_cols, n_fine, ldc, q_first, n_qc))
        return rc;
    if (n_qc == 0 || M == 0) return 0;
    return launch_restrict(stk_stream(stream), M, nullptr, nullptr, a, f, ld, k_first, n_fine, out, ldc, q_first,
                           n_qc);
}
