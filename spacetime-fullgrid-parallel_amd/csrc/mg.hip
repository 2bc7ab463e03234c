// Spatial multigrid V-cycle with Gauss-Seidel smoothing, batched over the
// n_loc time slices of a slab.  Replaces MultiGrid._matvec / MGM
// (reference source/multigrid.py:168-193) and the PETSc MatSOR calls of
// PETScSMoother (multigrid.py:100-127), whose semantics are the sequential
// sweep of Smoother (multigrid.py:83-97).
//
// Gauss-Seidel on a GPU without changing the result: rows are grouped by depth
// in the dependency DAG of the sweep (row i waits for its neighbours j < i in a
// forward sweep, j > i in a backward one).  Groups run in order, one launch
// each; inside a group every (row, time slice) pair is independent.  Each row
// performs exactly the arithmetic of the sequential sweep
//     u_i += (1 / a_ii) * (f_i - sum_j a_ij u_j)        (CSR order, j = i included)
// on exactly the same inputs, so the sweep is the reference's sweep, not a
// re-coloured variant.  With the build's vertex numbering (source/mesh.py)
// the DAG has 4 groups for the 7-point matrices of the square and 3 for its
// stiffness matrix alone.  Around that: the restricted residual is formed as
// (R A) u - R f from precomputed products, the first sweep of a level visit
// (u = 0) runs on per-group matrices without the zero products and without
// zeroing u, and the coarsest levels run as one job-list launch
// (mg_coarse.hip).
//
// Matrix entries may depend on the time slice: a(t) = ca*vals_a + cm[t]*vals_m.
// That is how the block-diagonal preconditioner's matrices 2^j M_x + alpha A_x
// (reference heateq_mpi.py:97-98) share one stored hierarchy: Galerkin
// coarsening is linear, so R(2^j M + alpha A)P = 2^j RMP + alpha RAP.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "csr_spmm.h"
#include "stk_common.h"

namespace {

constexpr int GBS = 256;

__global__ __launch_bounds__(GBS) void gs_group_kernel(int64_t total, const int32_t *__restrict__ rows,
                                                       int32_t n_loc, int32_t ld,
                                                       const int32_t *__restrict__ indptr,
                                                       const int32_t *__restrict__ indices,
                                                       const double *__restrict__ va, double ca,
                                                       const double *__restrict__ vm,
                                                       const double *__restrict__ cm,
                                                       const int32_t *__restrict__ diag,
                                                       const double *__restrict__ f, double *u, int diag_free)
{
    const int64_t stride = (int64_t)gridDim.x * GBS;
    for (int64_t idx = (int64_t)blockIdx.x * GBS + threadIdx.x; idx < total; idx += stride) {
        const int q = (int)(idx / n_loc);
        const int t = (int)(idx - (int64_t)q * n_loc);
        const int i = rows[q];
        const int e0 = indptr[i], e1 = indptr[i + 1];
        const double *ut = u + t;
        const double c = (vm != nullptr) ? cm[t] : 0.0;
        double ax = 0.0;
        const int ed = diag[i];
        // batches of independent gathers (clamped past the row end), the entries
        // summed in CSR order like the sequential sweep, in the form of the plan's
        // ELL copies (stk_ell_rows.diag_free): u_i = (f_i - sum_{j != i} a_ij u_j) / a_ii,
        // or with the diagonal in the sum and u_i += (f_i - row_i u) / a_ii
        // (reference multigrid.py:89-97)
        for (int eb = e0; eb < e1; eb += 8) {
            double uv[8], av[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int e = min(eb + q, e1 - 1);
                uv[q] = ut[(size_t)indices[e] * ld];
                av[q] = (vm != nullptr) ? fma(c, vm[e], ca * va[e]) : ca * va[e];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (eb + q < e1 && (!diag_free || eb + q != ed)) ax = fma(av[q], uv[q], ax);
        }
        const double d = (vm != nullptr) ? fma(c, vm[ed], ca * va[ed]) : ca * va[ed];
        const size_t o = (size_t)i * ld + t;
        u[o] = (diag_free ? 0.0 : u[o]) + (1.0 / d) * (f[o] - ax);
    }
}

// u0[i, t] = sum_j inv[kind[t]][i][j] f0[j, t]   (exact coarse solve,
// multigrid.py:161-165, 169-170; the inverse is formed on the host at setup)
__global__ __launch_bounds__(GBS) void coarse_kernel(int32_t n0, int32_t n_loc, int32_t ld,
                                                     const double *__restrict__ inv, double ca_inv,
                                                     const int32_t *__restrict__ kind,
                                                     const double *__restrict__ f, double *__restrict__ u)
{
    const int idx = blockIdx.x * GBS + threadIdx.x;
    if (idx >= n0 * n_loc) return;
    const int i = idx / n_loc, t = idx - i * n_loc;
    const double *A = inv + (size_t)(kind ? kind[t] : 0) * n0 * n0 + (size_t)i * n0;
    double s = 0.0;
    for (int j = 0; j < n0; ++j) s = fma(A[j], f[(size_t)j * ld + t], s);
    u[(size_t)i * ld + t] = ca_inv * s;
}

}  // namespace

// levels up to this many rows may be fused into the coarse sub-V-cycle (larger ones fill the GPU by themselves)
constexpr int64_t COARSE_MAX_ROWS = 4096;

struct EllLevel {
    bool has_a = false, has_gs = false, has_p = false, has_r = false, has_ra = false, has_alt = false;
    bool ra_rows_as_r = false;  // R A and R list the same rows in the same order (checked at plan creation)
    stk_ell_rows a, fwd, bwd, p, r, ra;
    stk_ell_rows fwd_alt, bwd_alt;  // the sweeps' copies in the other row form (early V-cycles)
    std::vector<stk_ell_rows> fwd0;  // per forward group: entries towards earlier groups only
    std::vector<int32_t> fwd_pos, bwd_pos;
    // strip-wise sweeps: tile row of every position, and per strip count S the
    // position ranges [S][groups][2] (built on first use)
    std::vector<int32_t> fwd_trow, bwd_trow;
    int n_tile_rows = 0;
    mutable std::map<int, std::vector<int32_t>> fwd_strips, bwd_strips;
};

struct stk_mg {
    std::vector<stk_mg_level> lv;
    std::vector<EllLevel> ell;
    std::vector<std::vector<int32_t>> fwd_ptr, bwd_ptr;
    int smoothsteps, vcycles, n_kinds, max_ld;
    const double *coarse_inv;
    // workspaces per level (level J uses the caller's u, f)
    std::vector<double *> u, f, r;
    // fused coarse sub-V-cycle: levels 0..Lc in one launch (Lc < 0: none)
    stk_coarse_plan *coarse = nullptr;
    int Lc = -1;
    // device arrays the plan owns: the workspaces, and what stk_mg_create_from_csr built
    stk_dev_arrays dev;
    ~stk_mg() { stk_coarse_plan_free(coarse); }
    // -1: follow the process-wide tuning key "mg_fuse_restrict"; 0 / 1: this plan's
    // own choice (stk_mg_set_option; 0 is part of the reference-arithmetic mode)
    int fuse_restrict = -1;
    // levels on which the fused form may be used (the others take the two steps)
    int fuse_min_level = 0, fuse_max_level = 1 << 30;
    // V-cycles with index < fast_until_cycle run the fast forms: the alternative
    // copies of the sweeps where a level has them, the fused restricted residual
    // on every level
    int fast_until_cycle = 0;
    // ... and in the later V-cycles: bit 0 = the pre-smoothing, bit 1 = the restricted
    // residual also take the fast forms (the post-smoothing never does)
    int fast_parts = 0;
    int strip_pct = 100;  // this plan's strips as a percentage of the tuning key "mg_strip_mb"
};

// The ELL row engine needs 16-byte time pairs (even ld) and slabs below 64 GiB.
static inline bool ell_slab_ok(int64_t rows, int ld)
{
    return (ld & 1) == 0 && rows * ld * 8 < ((int64_t)1 << 36);
}

// A level visit starts from u = 0 (multigrid.py:176, 187).  With the per-group
// matrices of stk_mg_level.ell_fwd0 the first forward sweep neither needs u
// zeroed in memory nor gathers the zeros.
static bool can_zero_start(const stk_mg *mg, int level, int ld)
{
    const EllLevel &E = mg->ell[level];
    return stk_tune(g_tuning.mg_zero_start) && level >= 1 && mg->smoothsteps >= 1 && E.has_gs && !E.fwd0.empty() &&
           E.fwd0.size() + 1 == E.fwd_pos.size() && ell_slab_ok(mg->lv[level].n, ld);
}

// Strip-wise smoothing.  On a large level one group pass streams the whole level
// through the caches, so the next pass finds nothing of it there: `its` sweeps
// of `ng` dependency groups cost its*ng passes over u (and its passes over f)
// from HBM.  The plan knows a BAND of every row (stk_mg_level.*_tile_row_host:
// ascending inside every group; coupled rows lie at most one band apart --
// mesh rows of a structured mesh).  The level is cut into S strips of bands and
// ALL stages q = it*ng + g (sweep it, group g) run on strip s before strip s+1,
// stage q shifted down by q bands against stage 0.  A row of stage q in band b
// then finds
//   * every row of an earlier group of the same sweep that it reads (band
//     b-1..b+1, stage q' < q, so b' + q' <= b + q: same strip earlier, or an
//     earlier strip) already updated, and
//   * every row of a later group (stage q'' > q of this sweep, b'' + q'' >= b + q:
//     same strip later, or a later strip) still holding the value of the previous
//     sweep, whose stage q'' - ng < q has run by the same argument,
// i.e. exactly the operands of the level-wide passes: the order of updates, and
// with it the result bit for bit, is unchanged, while u and f of a strip
// (`strip_mb` MB) are read from HBM once per smoothing call, not once per pass.
// Returns the [S][its*ng][2] position table (positions of group q % ng), or NULL.
static const std::vector<int32_t> *strip_table(const EllLevel &E, bool backward, int64_t rows, int ld, int its,
                                               double strip_mb)
{
    if (strip_mb <= 0 || E.n_tile_rows < 2 || its < 1) return nullptr;
    const double level_mb = 2.0 * (double)rows * ld * 8.0 / 1.0e6;  // u and f
    int S = (int)(level_mb / strip_mb + 0.999);
    const std::vector<int32_t> &pos = backward ? E.bwd_pos : E.fwd_pos;
    const int ng = (int)pos.size() - 1;
    const int Q = its * ng;
    // Strips partition the axis band + stage, 0 .. T + Q - 2.  Any width is
    // correct; a strip touches its own bands plus the skew of its Q stages, so it
    // should be a few times wider than Q (tuning key mg_strip_width: in units of Q;
    // tests set 0 to force many thin strips).
    const int T = E.n_tile_rows, span = T + Q - 1;
    const int strip_width = stk_tune(g_tuning.mg_strip_width);
    const int min_width = strip_width > 0 ? strip_width * Q : 2;
    if (S > span / min_width) S = span / min_width;
    if (S < 2) return nullptr;
    auto &cache = backward ? E.bwd_strips : E.fwd_strips;
    const int key = S * 1024 + its;
    auto it = cache.find(key);
    if (it != cache.end()) return &it->second;
    const std::vector<int32_t> &tr = backward ? E.bwd_trow : E.fwd_trow;
    std::vector<int32_t> tab((size_t)S * Q * 2);
    for (int s = 0; s < S; ++s)
        for (int q = 0; q < Q; ++q) {
            const int g = q % ng;
            const int32_t *b = tr.data() + pos[g], *e = tr.data() + pos[g + 1];
            // rows of stage q with lo <= band + q < hi
            const int lo_row = (int)((int64_t)s * span / S) - q, hi_row = (int)((int64_t)(s + 1) * span / S) - q;
            const int32_t *lo = (s == 0) ? b : std::lower_bound(b, e, lo_row);
            const int32_t *hi = (s == S - 1) ? e : std::lower_bound(b, e, hi_row);
            tab[((size_t)s * Q + q) * 2] = (int32_t)(lo - tr.data());
            tab[((size_t)s * Q + q) * 2 + 1] = (int32_t)(hi - tr.data());
        }
    return &cache.emplace(key, std::move(tab)).first->second;
}

static int smooth_level(stk_mg *mg, hipStream_t st, int level, int n_loc, int ld, double ca, const double *cm,
                        int its, bool backward, const double *f, double *u, bool zero_start = false, int cycle = 1 << 30)
{
    const stk_mg_level &L = mg->lv[level];
    const EllLevel &E = mg->ell[level];
    if (E.has_gs && ell_slab_ok(L.n, ld)) {
        const bool alt = E.has_alt && cycle < mg->fast_until_cycle;
        const stk_ell_rows &e = alt ? (backward ? E.bwd_alt : E.fwd_alt) : (backward ? E.bwd : E.fwd);
        const std::vector<int32_t> &pos = backward ? E.bwd_pos : E.fwd_pos;
        const int ng = (int)pos.size() - 1;
        const bool zs = zero_start && !backward && its >= 1;
        const std::vector<int32_t> *strips =
            strip_table(E, backward, L.n, ld, its, stk_tune(g_tuning.mg_strip_mb) * (mg->strip_pct / 100.0));
        const int S = strips ? (int)(strips->size() / (2 * (size_t)ng * its)) : 1;
        const int Q = its * ng;
        for (int s = 0; s < S; ++s)
            for (int q = 0; q < Q; ++q) {
                const int g = q % ng;
                const int p0 = strips ? (*strips)[((size_t)s * Q + q) * 2] : pos[g];
                const int p1 = strips ? (*strips)[((size_t)s * Q + q) * 2 + 1] : pos[g + 1];
                if (strips) g_tuning.mg_strips_used.fetch_add(1, std::memory_order_relaxed);
                int rc;
                if (zs && q < ng) {
                    // first sweep of a level visit: u is NOT initialised.  Group 0
                    // has no entries left and gathers its (zero-weighted) padding
                    // slots from f; later groups only read rows of earlier groups,
                    // which this sweep has written.  Positions of a per-group
                    // matrix count from the start of its group.
                    rc = stk_rows_ell_launch(st, 1, &E.fwd0[g], p0 - pos[g], p1 - pos[g], n_loc, ld, L.n, L.n, ca, cm,
                                             g == 0 ? f : u, 0.0, 0.0, f, u, /*zero_own=*/1);
                } else {
                    rc = stk_rows_ell_launch(st, 1, &e, p0, p1, n_loc, ld, L.n, L.n, ca, cm, u, 0.0, 0.0, f, u);
                }
                if (rc) return rc;
            }
        return 0;
    }
    const std::vector<int32_t> &ptr = backward ? mg->bwd_ptr[level] : mg->fwd_ptr[level];
    const int32_t *rows = backward ? L.bwd_rows : L.fwd_rows;
    const int ngroups = (int)ptr.size() - 1;
    for (int it = 0; it < its; ++it) {
        for (int g = 0; g < ngroups; ++g) {
            const int nr = ptr[g + 1] - ptr[g];
            if (nr == 0) continue;
            const int64_t total = (int64_t)nr * n_loc;
            hipLaunchKernelGGL(gs_group_kernel, dim3(stk_flat_grid(total, GBS)), dim3(GBS), 0, st, total,
                               rows + ptr[g], n_loc, ld, L.indptr, L.indices, L.vals_a, ca,
                               cm ? L.vals_m : nullptr, cm, L.diag, f, u, E.has_gs ? E.fwd.diag_free : 1);
            STK_LAUNCH_CHECK();
        }
    }
    return 0;
}

// multigrid.py:168-182
// u_zero: u_j is zero by definition but its memory has NOT been written.
static int mgm(stk_mg *mg, hipStream_t st, int j, int n_loc, int ld, double ca, const double *cm,
               const int32_t *kind, const double *f_j, double *u_j, bool u_zero, int cycle)
{
    const stk_mg_level &L = mg->lv[j];
    if (stk_tune(g_tuning.mg_fuse_coarse) && mg->coarse && j == mg->Lc && (ld & 1) == 0 && f_j == mg->f[j] && u_j == mg->u[j]) {
        // (the job list starts from zero itself when its vectors live in LDS;
        // the global-memory variant reads u)
        if (u_zero && !stk_coarse_plan_in_lds(mg->coarse))
            STK_HIP(hipMemsetAsync(u_j, 0, sizeof(double) * (size_t)L.n * ld, st));
        return stk_coarse_plan_run(mg->coarse, st, n_loc, ld, ca, cm, kind, mg->coarse_inv);
    }
    const bool zero_start = u_zero && j >= 1 && can_zero_start(mg, j, ld);
    // (only the n_loc columns of this call, rounded up to a pair: the caller's slab may be a
    // column range of a wider one whose other columns another stream is working on)
    if (u_zero && j >= 1 && !zero_start) {
        const int cols = std::min(ld, (n_loc + 1) & ~1);
        if (cols == ld)
            STK_HIP(hipMemsetAsync(u_j, 0, sizeof(double) * (size_t)L.n * ld, st));
        else
            STK_HIP(hipMemset2DAsync(u_j, sizeof(double) * (size_t)ld, 0, sizeof(double) * (size_t)cols, (size_t)L.n,
                                     st));
    }
    if (j == 0) {
        const int total = L.n * n_loc;
        // the stored inverses are those of (vals_a + cm*vals_m) for cm != NULL,
        // and of vals_a alone otherwise; ca scales the latter
        hipLaunchKernelGGL(coarse_kernel, dim3((total + GBS - 1) / GBS), dim3(GBS), 0, st, L.n, n_loc, ld,
                           mg->coarse_inv, cm ? 1.0 : 1.0 / ca, cm ? kind : nullptr, f_j, u_j);
        STK_LAUNCH_CHECK();
        return 0;
    }
    int rc = smooth_level(mg, st, j, n_loc, ld, ca, cm, mg->smoothsteps, false, f_j, u_j, zero_start,
                          (mg->fast_parts & 1) ? -1 : cycle);
    if (rc) return rc;
    const stk_mg_level &C = mg->lv[j - 1];
    double *r_j = mg->r[j], *d_c = mg->f[j - 1], *u_c = mg->u[j - 1];
    const EllLevel &E = mg->ell[j];
    const bool even = ell_slab_ok(L.n, ld);
    // The flat kernels of a level without ELL copies keep to this call's columns like the row
    // engine: the pair of an even ld (the padding column written as zero), every column of an
    // odd one.
    const int flat_cols = (ld & 1) ? ld : std::min(ld, (n_loc + 1) & ~1);
    const bool fuse_restrict = (mg->fuse_restrict >= 0 ? mg->fuse_restrict != 0 : stk_tune(g_tuning.mg_fuse_restrict) != 0) &&
                               ((j >= mg->fuse_min_level && j <= mg->fuse_max_level) || cycle < mg->fast_until_cycle ||
                                (mg->fast_parts & 2));
    if (fuse_restrict && E.has_ra && E.has_r && even) {
        // d_c = R (A_j u_j - f_j) = (R A_j) u_j - R f_j: the fine residual is never written.
        // One pass where the two matrices list the same rows (tuning key mg_restrict_one_pass;
        // the very roundings of the two passes), else d_c = R f_j, then d_c = (R A_j) u_j - d_c.
        // Key 1 (default): only for matrices with per-slice coefficients (the preconditioner
        // family: P 5.54 -> 5.39 ms on 9-step slabs, 21.7 -> 21.5 ms on 65); K's plans, which run
        // two at a time inside S, measure SLOWER with it (S 3.31 -> 3.37 ms, 16.9 -> 17.2 ms:
        // profiles/r04_restrict_one_pass_ab.log).  Key 2: every plan.
        const int one_pass = stk_tune(g_tuning.mg_restrict_one_pass);
        rc = (one_pass && E.ra_rows_as_r && (cm != nullptr || one_pass >= 2))
                 ? stk_rows_ell2_launch(st, &E.ra, &E.r, n_loc, ld, L.n, C.n, ca, cm, u_j, f_j, d_c)
                 : -1;
        if (rc == -1) {
            rc = stk_rows_ell_launch(st, 0, &E.r, 0, E.r.n_pos, n_loc, ld, L.n, C.n, 1.0, nullptr, f_j, 1.0, 0.0,
                                     nullptr, d_c);
            if (rc) return rc;
            rc = stk_rows_ell_launch(st, 0, &E.ra, 0, E.ra.n_pos, n_loc, ld, L.n, C.n, ca, cm, u_j, 1.0, -1.0, d_c,
                                     d_c);
        }
        if (rc) return rc;
    } else {
        // r_j = A_j u_j - f_j
        if (E.has_a && even)
            rc = stk_rows_ell_launch(st, 0, &E.a, 0, E.a.n_pos, n_loc, ld, L.n, L.n, ca, cm, u_j, 1.0, -1.0, f_j,
                                     r_j);
        else
            rc = stk_csr_spmm_cols(st, L.n, n_loc, ld, flat_cols, L.indptr, L.indices, L.vals_a, ca,
                                   cm ? L.vals_m : nullptr, cm, u_j, 1.0, -1.0, f_j, r_j);
        if (rc) return rc;
        // d_c = R r_j
        if (E.has_r && even)
            rc = stk_rows_ell_launch(st, 0, &E.r, 0, E.r.n_pos, n_loc, ld, L.n, C.n, 1.0, nullptr, r_j, 1.0, 0.0,
                                     nullptr, d_c);
        else
            rc = stk_csr_spmm_cols(st, C.n, n_loc, ld, flat_cols, L.r_indptr, L.r_indices, L.r_vals, 1.0, nullptr,
                                   nullptr, r_j, 1.0, 0.0, nullptr, d_c);
        if (rc) return rc;
    }
    rc = mgm(mg, st, j - 1, n_loc, ld, ca, cm, kind, d_c, u_c, /*u_zero=*/true, cycle);
    if (rc) return rc;
    // u_j -= P u_c
    if (E.has_p && even)
        rc = stk_rows_ell_launch(st, 0, &E.p, 0, E.p.n_pos, n_loc, ld, C.n, L.n, 1.0, nullptr, u_c, -1.0, 1.0, u_j,
                                 u_j);
    else
        rc = stk_csr_spmm_cols(st, L.n, n_loc, ld, flat_cols, L.p_indptr, L.p_indices, L.p_vals, 1.0, nullptr, nullptr,
                               u_c, -1.0, 1.0, u_j, u_j);
    if (rc) return rc;
    return smooth_level(mg, st, j, n_loc, ld, ca, cm, mg->smoothsteps, true, f_j, u_j, false, cycle);
}

extern "C" int stk_mg_create(int32_t n_levels, const stk_mg_level *levels, int32_t smoothsteps, int32_t vcycles,
                             int32_t n_kinds, const double *coarse_inv, int32_t max_ld, stk_mg **out)
{
    STK_REQUIRE(n_levels >= 1 && levels && out, "stk_mg_create: bad arguments");
    STK_REQUIRE(smoothsteps >= 0 && vcycles >= 1 && max_ld >= 1, "stk_mg_create: bad parameters");
    STK_REQUIRE(coarse_inv && n_kinds >= 1, "stk_mg_create: coarse inverse missing");
    stk_mg *mg = new stk_mg();
    mg->smoothsteps = smoothsteps;
    mg->vcycles = vcycles;
    mg->n_kinds = n_kinds;
    mg->max_ld = max_ld;
    mg->coarse_inv = coarse_inv;
    mg->lv.assign(levels, levels + n_levels);
    mg->fwd_ptr.resize(n_levels);
    mg->bwd_ptr.resize(n_levels);
    mg->ell.resize(n_levels);
    for (int j = 1; j < n_levels; ++j) {
        const stk_mg_level &L = mg->lv[j];
        EllLevel &E = mg->ell[j];
        if (L.ell_a) { E.a = *L.ell_a; E.has_a = true; }
        if (L.ell_p) { E.p = *L.ell_p; E.has_p = true; }
        if (L.ell_r) { E.r = *L.ell_r; E.has_r = true; }
        if (L.ell_ra) { E.ra = *L.ell_ra; E.has_ra = true; }
        if (E.has_ra && E.has_r && E.ra.n_pos == E.r.n_pos && E.ra.n_pos > 0) {
            // the one-pass restricted residual pairs position p of R A with position p of R
            if (E.ra.row_ids == E.r.row_ids) {
                E.ra_rows_as_r = true;
            } else if (E.ra.row_ids && E.r.row_ids) {
                std::vector<int32_t> ra_rows(E.ra.n_pos), r_rows(E.r.n_pos);
                if (hipMemcpy(ra_rows.data(), E.ra.row_ids, sizeof(int32_t) * ra_rows.size(), hipMemcpyDeviceToHost) ==
                        hipSuccess &&
                    hipMemcpy(r_rows.data(), E.r.row_ids, sizeof(int32_t) * r_rows.size(), hipMemcpyDeviceToHost) ==
                        hipSuccess)
                    E.ra_rows_as_r = ra_rows == r_rows;
            }
        }
        if (L.ell_fwd0 && L.n_fwd > 0) E.fwd0.assign(L.ell_fwd0, L.ell_fwd0 + L.n_fwd);
        if (L.ell_fwd && L.ell_bwd && L.fwd_pos_host && L.bwd_pos_host) {
            E.fwd = *L.ell_fwd;
            E.bwd = *L.ell_bwd;
            E.fwd_pos.assign(L.fwd_pos_host, L.fwd_pos_host + L.n_fwd + 1);
            E.bwd_pos.assign(L.bwd_pos_host, L.bwd_pos_host + L.n_bwd + 1);
            E.has_gs = true;
        }
        if (E.has_gs && L.ell_fwd_alt && L.ell_bwd_alt && L.ell_fwd_alt->n_pos == E.fwd.n_pos &&
            L.ell_bwd_alt->n_pos == E.bwd.n_pos) {
            E.fwd_alt = *L.ell_fwd_alt;
            E.bwd_alt = *L.ell_bwd_alt;
            E.has_alt = true;
        }
        if (E.has_gs && L.n_tile_rows > 1 && L.fwd_tile_row_host && L.bwd_tile_row_host) {
            E.fwd_trow.assign(L.fwd_tile_row_host, L.fwd_tile_row_host + E.fwd.n_pos);
            E.bwd_trow.assign(L.bwd_tile_row_host, L.bwd_tile_row_host + E.bwd.n_pos);
            E.n_tile_rows = L.n_tile_rows;
        }
        mg->lv[j].ell_a = mg->lv[j].ell_fwd = mg->lv[j].ell_bwd = mg->lv[j].ell_p = mg->lv[j].ell_r = nullptr;
        mg->lv[j].ell_ra = mg->lv[j].ell_fwd0 = nullptr;
        mg->lv[j].ell_fwd_alt = mg->lv[j].ell_bwd_alt = nullptr;
    }
    mg->u.assign(n_levels, nullptr);
    mg->f.assign(n_levels, nullptr);
    mg->r.assign(n_levels, nullptr);
    for (int j = 0; j < n_levels; ++j) {
        const stk_mg_level &L = mg->lv[j];
        if (L.n <= 0 || !L.indptr || !L.indices || !L.vals_a || !L.diag) {
            stk_set_error("stk_mg_create: level %d incomplete", j);
            stk_mg_destroy(mg);
            return 2;
        }
        if (j > 0) {
            if (!L.fwd_ptr_host || !L.bwd_ptr_host || !L.fwd_rows || !L.bwd_rows || !L.p_indptr ||
                !L.r_indptr) {
                stk_set_error("stk_mg_create: level %d lacks schedule or transfer operators", j);
                stk_mg_destroy(mg);
                return 2;
            }
            mg->fwd_ptr[j].assign(L.fwd_ptr_host, L.fwd_ptr_host + L.n_fwd + 1);
            mg->bwd_ptr[j].assign(L.bwd_ptr_host, L.bwd_ptr_host + L.n_bwd + 1);
        }
        const size_t doubles = (size_t)L.n * max_ld;
        bool ok = true;
        if (j < n_levels - 1)
            ok = (mg->u[j] = mg->dev.alloc<double>(doubles)) && (mg->f[j] = mg->dev.alloc<double>(doubles));
        if (ok && j > 0) ok = (mg->r[j] = mg->dev.alloc<double>(doubles));
        if (!ok) {
            const std::string why = stk_last_error();
            stk_set_error("stk_mg_create: level %d: %s", j, why.c_str());
            delete mg;
            return 1;
        }
    }
    // fuse the coarse end of the V-cycle when every level there has its ELL pieces
    {
        // as many levels as keep all their vectors (u, f, residual: one double per
        // row and time step) in the 144 KiB LDS arena of mg_coarse.hip
        int Lc = -1;
        int64_t arena_rows = 3 * (int64_t)mg->lv[0].n;
        for (int j = 1; j < n_levels - 1; ++j) {
            const EllLevel &E = mg->ell[j];
            arena_rows += 3 * (int64_t)mg->lv[j].n;
            if (mg->lv[j].n > COARSE_MAX_ROWS || arena_rows * (int64_t)sizeof(double) > 144 * 1024 ||
                !(E.has_a && E.has_gs && E.has_p && E.has_r))
                break;
            Lc = j;
        }
        if (Lc >= 1) {
            std::vector<stk_coarse_level> cl(Lc + 1);
            for (int j = 0; j <= Lc; ++j) {
                const EllLevel &E = mg->ell[j];
                cl[j].n = mg->lv[j].n;
                cl[j].ok = true;
                if (j >= 1) {
                    cl[j].a = E.a;
                    cl[j].fwd = E.fwd;
                    cl[j].bwd = E.bwd;
                    cl[j].p = E.p;
                    cl[j].r = E.r;
                    cl[j].fwd_pos = E.fwd_pos.data();
                    cl[j].bwd_pos = E.bwd_pos.data();
                    cl[j].n_fwd = (int)E.fwd_pos.size() - 1;
                    cl[j].n_bwd = (int)E.bwd_pos.size() - 1;
                }
                cl[j].u = mg->u[j];
                cl[j].f = mg->f[j];
                cl[j].res = mg->r[j];
            }
            mg->coarse = stk_coarse_plan_build(cl.data(), Lc, smoothsteps);
            if (mg->coarse) mg->Lc = Lc;
        }
    }
    *out = mg;
    return 0;
}

extern "C" int stk_mg_coarse_levels(const stk_mg *mg)
{
    return mg ? stk_coarse_plan_levels(mg->coarse) : 0;
}

extern "C" int stk_mg_set_member_matrices(stk_mg *mg, int32_t level, int32_t n_kinds,
                                          const int32_t *const *indptr_host, const int32_t *const *indices_host,
                                          const double *const *data_host)
{
    STK_REQUIRE(mg && indptr_host && indices_host && data_host, "stk_mg_set_member_matrices: null argument");
    STK_REQUIRE(n_kinds == mg->n_kinds, "stk_mg_set_member_matrices: %d matrices for a plan of %d kinds", n_kinds,
                mg->n_kinds);
    STK_REQUIRE(mg->coarse && level >= 1 && level <= mg->Lc,
                "stk_mg_set_member_matrices: level %d is not inside the fused coarse end (levels 1..%d)", level, mg->Lc);
    return stk_coarse_plan_set_members(mg->coarse, level, n_kinds, mg->lv[level].n, indptr_host, indices_host,
                                       data_host);
}

stk_dev_arrays &stk_mg_arrays(stk_mg *mg) { return mg->dev; }

extern "C" int stk_mg_destroy(stk_mg *mg)
{
    delete mg;
    return 0;
}

extern "C" int stk_mg_set_option(stk_mg *mg, const char *key, int32_t value)
{
    STK_REQUIRE(mg && key, "stk_mg_set_option: null pointer");
    if (std::strcmp(key, "fuse_restrict") == 0) {
        mg->fuse_restrict = value < 0 ? -1 : (value != 0);
        return 0;
    }
    if (std::strcmp(key, "fuse_restrict_min_level") == 0) {
        mg->fuse_min_level = value;
        return 0;
    }
    if (std::strcmp(key, "fuse_restrict_max_level") == 0) {
        mg->fuse_max_level = value;
        return 0;
    }
    if (std::strcmp(key, "fast_until_cycle") == 0) {
        mg->fast_until_cycle = value;
        return 0;
    }
    if (std::strcmp(key, "fast_parts") == 0) {
        mg->fast_parts = value;
        return 0;
    }
    if (std::strcmp(key, "strip_pct") == 0) {
        STK_REQUIRE(value >= 1 && value <= 10000, "stk_mg_set_option: strip_pct=%d not in 1..10000", value);
        mg->strip_pct = value;
        return 0;
    }
    stk_set_error("stk_mg_set_option: unknown key '%s' (fuse_restrict, fuse_restrict_min_level, fuse_restrict_max_level, fast_until_cycle, fast_parts, strip_pct)", key);
    return 2;
}

extern "C" int stk_mg_apply(stk_mg *mg, void *stream, int32_t n_loc, int32_t ld, double ca, const double *cm,
                            const int32_t *kind, const double *f, double *u)
{
    const stk_timed timed_(STK_OP_MULTIGRID, stream);
    STK_REQUIRE(mg && f && u && f != u, "stk_mg_apply: bad pointers");
    STK_REQUIRE(n_loc > 0 && ld >= n_loc && ld <= mg->max_ld, "stk_mg_apply: ld=%d exceeds plan max_ld=%d", ld,
                mg->max_ld);
    STK_REQUIRE(cm == nullptr || mg->lv[0].vals_m != nullptr, "stk_mg_apply: cm given but plan has no vals_m");
    STK_REQUIRE(ca != 0.0 || cm, "stk_mg_apply: zero matrix");
    hipStream_t st = stk_stream(stream);
    const int J = (int)mg->lv.size() - 1;
    for (int v = 0; v < mg->vcycles; ++v) {
        int rc = mgm(mg, st, J, n_loc, ld, ca, cm, kind, f, u, /*u_zero=*/v == 0, v);  // multigrid.py:187
        if (rc) return rc;
    }
    return 0;
}

extern "C" int stk_mg_smooth(stk_mg *mg, void *stream, int32_t level, int32_t n_loc, int32_t ld, double ca,
                             const double *cm, int32_t its, int32_t backward, const double *f, double *u)
{
    const stk_timed timed_(STK_OP_MULTIGRID, stream);
    STK_REQUIRE(mg && f && u, "stk_mg_smooth: null pointer");
    STK_REQUIRE(level >= 1 && level < (int)mg->lv.size(), "stk_mg_smooth: level %d out of range", level);
    STK_REQUIRE(n_loc > 0 && ld >= n_loc, "stk_mg_smooth: bad sizes");
    return smooth_level(mg, stk_stream(stream), level, n_loc, ld, ca, cm, its, backward != 0, f, u);
}
