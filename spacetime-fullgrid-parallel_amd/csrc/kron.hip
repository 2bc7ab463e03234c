// Single-factor Kronecker applies on the space-major slab layout x[i*ld + t].
// The Kronecker sums themselves live in kron_ell.hip, kron_pack.hip and
// kron_pack_multi.hip.
//
//  spmm_kernel       : y = alpha*(I kron A) x + beta*z, A general CSR with
//                      optional per-time-slice values (mpi_kron.py:143-150,
//                      multigrid.py:174-180).
//  time_csr_kernel   : y = (A_t kron I) x (+ x) for a small sparse time matrix
//                      with remote rows (mpi_kron.py:285-317).
//  time_dense_kernel : y = (T kron I) x for a dense n_out x n_in time factor.
//
// Work decomposition: one lane per (space row i, time index t).  Consecutive
// lanes walk t, so the gather of a CSR neighbour j is one contiguous run of
// n_loc doubles (coalesced whatever the spatial dof order is), and the CSR
// entries of row i are wave-broadcast loads.  HBM-bound; no MFMA.
#include "csr_spmm.h"
#include "stk_common.h"

namespace {

constexpr int SBS = 256;

__global__ __launch_bounds__(SBS) void spmm_kernel(int64_t total, int32_t n_loc, int32_t ld, int32_t cols,
                                                   const int32_t *__restrict__ indptr,
                                                   const int32_t *__restrict__ indices,
                                                   const double *__restrict__ va, double ca,
                                                   const double *__restrict__ vm, const double *__restrict__ cm,
                                                   const double *__restrict__ x, double alpha, double beta,
                                                   const double *z, double *y)
{
    const int64_t stride = (int64_t)gridDim.x * SBS;
    for (int64_t idx = (int64_t)blockIdx.x * SBS + threadIdx.x; idx < total; idx += stride) {
        const int row = (int)(idx / ld);
        const int t = (int)(idx - (int64_t)row * ld);
        if (t >= n_loc) {  // padding stays zero; columns from `cols` on are not this call's
            if (t < cols) y[idx] = 0.0;
            continue;
        }
        const int e0 = indptr[row], e1 = indptr[row + 1];
        const double *xt = x + t;
        const double c = (vm != nullptr) ? cm[t] : 0.0;
        double s = 0.0;
        // batches of independent gathers; entries past the row end are clamped
        // to its last entry and dropped (one memory round trip per batch)
        for (int eb = e0; eb < e1; eb += 8) {
            double xv[8], av[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = min(eb + u, e1 - 1);
                xv[u] = xt[(size_t)indices[e] * ld];
                av[u] = (vm != nullptr) ? fma(c, vm[e], ca * va[e]) : ca * va[e];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (eb + u < e1) s = fma(av[u], xv[u], s);
        }
        double out = alpha * s;
        if (beta != 0.0) out = fma(beta, z[idx], out);
        y[idx] = out;
    }
}

__global__ __launch_bounds__(SBS) void time_csr_kernel(int64_t total, int32_t M, int32_t n_loc, int32_t ld,
                                                       const int32_t *__restrict__ t_indptr,
                                                       const int32_t *__restrict__ t_cols,
                                                       const double *__restrict__ t_vals,
                                                       const double *__restrict__ x,
                                                       const double *__restrict__ recv, int add_identity,
                                                       double *__restrict__ y)
{
    const int64_t stride = (int64_t)gridDim.x * SBS;
    for (int64_t idx = (int64_t)blockIdx.x * SBS + threadIdx.x; idx < total; idx += stride) {
        const int i = (int)(idx / ld);
        const int t = (int)(idx - (int64_t)i * ld);
        if (t >= n_loc) {
            y[idx] = 0.0;
            continue;
        }
        const double *xi = x + (size_t)i * ld;
        double acc = add_identity ? xi[t] : 0.0;
        for (int e = t_indptr[t]; e < t_indptr[t + 1]; ++e) {
            const int c = t_cols[e];
            const double v = (c < n_loc) ? xi[c] : recv[(size_t)(c - n_loc) * M + i];
            acc = fma(t_vals[e], v, acc);
        }
        y[idx] = acc;
    }
}

}  // namespace

// stk_csr_spmm on the first `cols` columns of the slab (csr_spmm.h).
int stk_csr_spmm_cols(void *stream, int32_t rows, int32_t n_loc, int32_t ld, int32_t cols, const int32_t *indptr,
                      const int32_t *indices, const double *vals_a, double ca, const double *vals_m, const double *cm,
                      const double *x, double alpha, double beta, const double *z, double *y)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    if (rows == 0) return 0;
    STK_REQUIRE(rows > 0 && n_loc > 0 && ld >= n_loc && cols >= n_loc && cols <= ld, "stk_csr_spmm: bad sizes");
    STK_REQUIRE(indptr && indices && vals_a && x && y, "stk_csr_spmm: null pointer");
    STK_REQUIRE((vals_m == nullptr) == (cm == nullptr), "stk_csr_spmm: vals_m and cm go together");
    STK_REQUIRE(beta == 0.0 || z, "stk_csr_spmm: beta != 0 needs z");
    STK_REQUIRE(x != y, "stk_csr_spmm: input aliases output");
    const int64_t total = (int64_t)rows * ld;
    hipLaunchKernelGGL(spmm_kernel, dim3(stk_flat_grid(total, SBS)), dim3(SBS), 0, stk_stream(stream), total,
                       n_loc, ld, cols, indptr, indices, vals_a, ca, vals_m, cm, x, alpha, beta, z, y);
    STK_LAUNCH_CHECK();
    return 0;
}

extern "C" int stk_csr_spmm(void *stream, int32_t rows, int32_t n_loc, int32_t ld, const int32_t *indptr,
                            const int32_t *indices, const double *vals_a, double ca, const double *vals_m,
                            const double *cm, const double *x, double alpha, double beta, const double *z,
                            double *y)
{
    return stk_csr_spmm_cols(stream, rows, n_loc, ld, ld, indptr, indices, vals_a, ca, vals_m, cm, x, alpha, beta, z,
                             y);
}

namespace {
// y[i, r] = sum_c T[r, c] x[i, c]: a dense (n_out x n_in) time factor on every
// spatial row.  One thread per output; T and the x row come through the caches.
__global__ __launch_bounds__(256) void time_dense_kernel(int64_t total, int32_t n_in, int32_t ld_in, int32_t n_out,
                                                         int32_t ld_out, const double *__restrict__ T,
                                                         const double *__restrict__ x, double *__restrict__ y)
{
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx / ld_out;
        const int r = (int)(idx - i * ld_out);
        double s = 0.0;
        if (r < n_out) {
            const double *xi = x + (size_t)i * ld_in;
            const double *Tr = T + (size_t)r * n_in;
            for (int c = 0; c < n_in; ++c) s = fma(Tr[c], xi[c], s);
        }
        y[idx] = s;  // padding columns are written as zero
    }
}
}  // namespace

extern "C" int stk_time_dense_apply(void *stream, int32_t M, int32_t n_in, int32_t ld_in, int32_t n_out,
                                    int32_t ld_out, const double *T, const double *x, double *y)
{
    const stk_timed timed_(STK_OP_TIME, stream);
    STK_REQUIRE(M > 0 && n_in > 0 && n_out > 0 && ld_in >= n_in && ld_out >= n_out,
                "stk_time_dense_apply: bad sizes M=%d n_in=%d ld_in=%d n_out=%d ld_out=%d", M, n_in, ld_in, n_out,
                ld_out);
    STK_REQUIRE(T && x && y && x != y, "stk_time_dense_apply: null or aliased pointer");
    const int64_t total = (int64_t)M * ld_out;
    hipLaunchKernelGGL(time_dense_kernel, dim3(stk_flat_grid(total, 256)), dim3(256), 0, stk_stream(stream), total,
                       n_in, ld_in, n_out, ld_out, T, x, y);
    STK_LAUNCH_CHECK();
    return 0;
}

extern "C" int stk_time_csr_apply(void *stream, int32_t M, int32_t n_loc, int32_t ld, const int32_t *t_indptr,
                                  const int32_t *t_cols, const double *t_vals, const double *x,
                                  const double *recv, int32_t add_identity, double *y)
{
    const stk_timed timed_(STK_OP_TIME, stream);
    STK_REQUIRE(M > 0 && n_loc > 0 && ld >= n_loc, "stk_time_csr_apply: bad sizes");
    STK_REQUIRE(t_indptr && t_cols && t_vals && x && y, "stk_time_csr_apply: null pointer");
    STK_REQUIRE(x != y, "stk_time_csr_apply: input aliases output");  // mpi_kron.py:296
    const int64_t total = (int64_t)M * ld;
    hipLaunchKernelGGL(time_csr_kernel, dim3(stk_flat_grid(total, SBS)), dim3(SBS), 0, stk_stream(stream),
                       total, M, n_loc, ld, t_indptr, t_cols, t_vals, x, recv, add_identity, y);
    STK_LAUNCH_CHECK();
    return 0;
}
