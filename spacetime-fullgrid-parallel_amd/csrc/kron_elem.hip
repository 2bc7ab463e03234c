// Time stages of the element-block operators between the trial space (continuous P1 in
// time: a node slab) and the test space (discontinuous P1 in time: two columns per
// time element), include/stk.h "test-space slabs":
//
//  * stk_elem_time_apply    y_{e,a} = sum_k sum_b blk_k[e][a][b] z_k[node(e) + b]
//  * stk_elem_time_apply_t  x_n     = sum_k (element n-1, then element n) sum_a blk_k[e][a][n-e] w_k[e,a]
//  * stk_elem_block_mix     y_{e,a} = sum_b blk[e][a][b] x_{e,b}
//
// z_k / w_k are the space factors' images X_k x of the input slab, made by the caller
// with the row engine (stk_ell_spmm, one pass per matrix): these kernels are the time
// side alone, one lane per (space dof, element) or (space dof, node), element pairs
// moved as aligned 16-byte words.  Every output is one chain of fused multiply-adds in
// an order that depends on the global element alone (written down in stk.h), so a result
// does not depend on which rank holds the element.
#include "stk_common.h"

namespace {

constexpr int BS = 256;

struct elem_terms {
    const double *z[STK_ELEM_MAX_TERMS];    // space-factor images, one slab per term
    const double *zg[STK_ELEM_MAX_TERMS];   // ... of the interleaved ghost pair (forward only)
    const double *blk[STK_ELEM_MAX_TERMS];  // 4 * n_el doubles: blk[e][a][b]
};

__device__ inline void store_pair_nt(double *dst, double2 v)
{
    __builtin_nontemporal_store(v.x, dst);
    __builtin_nontemporal_store(v.y, dst + 1);
}

// one lane per (i, e): e fastest, so a wavefront reads consecutive nodes of a row and
// writes consecutive pairs
template <int NT>
__global__ __launch_bounds__(BS) void elem_time_kernel(int64_t total, int32_t n_el, int32_t n_loc, int32_t ld_z,
                                                       int32_t first_node, elem_terms t, double beta,
                                                       double *__restrict__ y)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t idx = (int64_t)blockIdx.x * BS + threadIdx.x; idx < total; idx += stride) {
        const int64_t i = idx / n_el;
        const int e = (int)(idx - i * n_el);
        const int n0 = first_node + e, n1 = n0 + 1;
        double2 acc = make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const double z0 = n0 < 0 ? t.zg[k][2 * i] : t.z[k][i * ld_z + n0];
            const double z1 = n1 >= n_loc ? t.zg[k][2 * i + 1] : t.z[k][i * ld_z + n1];
            const double2 b0 = *reinterpret_cast<const double2 *>(t.blk[k] + 4 * (int64_t)e);
            const double2 b1 = *reinterpret_cast<const double2 *>(t.blk[k] + 4 * (int64_t)e + 2);
            acc.x = fma(b0.y, z1, fma(b0.x, z0, acc.x));
            acc.y = fma(b1.y, z1, fma(b1.x, z0, acc.y));
        }
        double *dst = y + 2 * idx;  // ld_y = 2 * n_el: the pairs of all rows are one array
        if (beta != 0.0) {
            const double2 old = *reinterpret_cast<const double2 *>(dst);
            acc.x = fma(beta, old.x, acc.x);
            acc.y = fma(beta, old.y, acc.y);
        }
        store_pair_nt(dst, acc);
    }
}

// one lane per (i, n), n < ld_x (the padding column is written as zero)
template <int NT>
__global__ __launch_bounds__(BS) void elem_time_t_kernel(int64_t total, int32_t n_el, int32_t n_loc, int32_t ld_x,
                                                         int32_t first_node, elem_terms t, double beta,
                                                         double *__restrict__ x)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t idx = (int64_t)blockIdx.x * BS + threadIdx.x; idx < total; idx += stride) {
        const int64_t i = idx / ld_x;
        const int n = (int)(idx - i * ld_x);
        if (n >= n_loc) {
            x[idx] = 0.0;
            continue;
        }
        const int e_left = n - first_node - 1, e_right = e_left + 1;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const double2 *w = reinterpret_cast<const double2 *>(t.z[k]) + i * n_el;
            // (an element range shorter than the slab: the nodes behind it have no element)
            if (e_left >= 0 && e_left < n_el) {  // this node is the element's second one: column b = 1
                const double2 v = w[e_left];
                const double *b = t.blk[k] + 4 * (int64_t)e_left;
                acc = fma(b[3], v.y, fma(b[1], v.x, acc));
            }
            if (e_right < n_el) {  // ... its first one: column b = 0
                const double2 v = w[e_right];
                const double *b = t.blk[k] + 4 * (int64_t)e_right;
                acc = fma(b[2], v.y, fma(b[0], v.x, acc));
            }
        }
        if (beta != 0.0) acc = fma(beta, x[idx], acc);
        x[idx] = acc;
    }
}

__global__ __launch_bounds__(BS) void elem_block_mix_kernel(int64_t total, int32_t n_el,
                                                            const double *__restrict__ blk, const double *x,
                                                            double *y)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t idx = (int64_t)blockIdx.x * BS + threadIdx.x; idx < total; idx += stride) {
        const int e = (int)(idx % n_el);
        const double2 v = *reinterpret_cast<const double2 *>(x + 2 * idx);
        const double2 b0 = *reinterpret_cast<const double2 *>(blk + 4 * (int64_t)e);
        const double2 b1 = *reinterpret_cast<const double2 *>(blk + 4 * (int64_t)e + 2);
        double2 out;
        out.x = fma(b0.y, v.y, b0.x * v.x);
        out.y = fma(b1.y, v.y, b1.x * v.x);
        *reinterpret_cast<double2 *>(y + 2 * idx) = out;
    }
}

bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

extern "C" int stk_elem_time_apply(void *stream, int32_t M, int32_t n_el, int32_t n_loc, int32_t ld_z,
                                   int32_t first_node, int32_t n_terms, const double *const *z_host,
                                   const double *const *zg_host, const double *const *blocks_host, double beta,
                                   double *y)
{
    const stk_timed timed_(STK_OP_TIME, stream);
    STK_REQUIRE(M > 0 && n_el > 0 && n_loc > 0 && ld_z >= n_loc, "stk_elem_time_apply: bad sizes M=%d n_el=%d n_loc=%d ld=%d",
                M, n_el, n_loc, ld_z);
    STK_REQUIRE(n_terms >= 1 && n_terms <= STK_ELEM_MAX_TERMS, "stk_elem_time_apply: %d terms (1..%d)", n_terms,
                STK_ELEM_MAX_TERMS);
    STK_REQUIRE((first_node == 0 || first_node == -1) && first_node + n_el <= n_loc,
                "stk_elem_time_apply: elements from node %d, %d of them, on %d local nodes", first_node, n_el, n_loc);
    STK_REQUIRE(z_host && blocks_host && y && aligned16(y), "stk_elem_time_apply: null or unaligned pointer");
    const bool ghosts = first_node < 0 || first_node + n_el == n_loc;
    elem_terms t = {};
    for (int k = 0; k < n_terms; ++k) {
        t.z[k] = z_host[k], t.blk[k] = blocks_host[k];
        t.zg[k] = ghosts && zg_host ? zg_host[k] : nullptr;
        STK_REQUIRE(t.z[k] && t.blk[k] && aligned16(t.blk[k]), "stk_elem_time_apply: term %d: null or unaligned pointer", k);
        STK_REQUIRE(!ghosts || t.zg[k], "stk_elem_time_apply: term %d reads a ghost node and has no ghost pair", k);
    }
    const int64_t total = (int64_t)M * n_el;
    const dim3 grid(stk_flat_grid(total, BS));
    hipStream_t st = stk_stream(stream);
    if (n_terms == 1)
        hipLaunchKernelGGL(elem_time_kernel<1>, grid, dim3(BS), 0, st, total, n_el, n_loc, ld_z, first_node, t, beta, y);
    else if (n_terms == 2)
        hipLaunchKernelGGL(elem_time_kernel<2>, grid, dim3(BS), 0, st, total, n_el, n_loc, ld_z, first_node, t, beta, y);
    else
        hipLaunchKernelGGL(elem_time_kernel<3>, grid, dim3(BS), 0, st, total, n_el, n_loc, ld_z, first_node, t, beta, y);
    STK_LAUNCH_CHECK();
    return 0;
}

extern "C" int stk_elem_time_apply_t(void *stream, int32_t M, int32_t n_el, int32_t n_loc, int32_t ld_x,
                                     int32_t first_node, int32_t n_terms, const double *const *w_host,
                                     const double *const *blocks_host, double beta, double *x)
{
    const stk_timed timed_(STK_OP_TIME, stream);
    STK_REQUIRE(M > 0 && n_el > 0 && n_loc > 0 && ld_x >= n_loc, "stk_elem_time_apply_t: bad sizes M=%d n_el=%d n_loc=%d ld=%d",
                M, n_el, n_loc, ld_x);
    STK_REQUIRE(n_terms >= 1 && n_terms <= STK_ELEM_MAX_TERMS, "stk_elem_time_apply_t: %d terms (1..%d)", n_terms,
                STK_ELEM_MAX_TERMS);
    STK_REQUIRE((first_node == 0 || first_node == -1) && first_node + n_el <= n_loc,
                "stk_elem_time_apply_t: elements from node %d, %d of them, on %d local nodes", first_node, n_el, n_loc);
    STK_REQUIRE(w_host && blocks_host && x, "stk_elem_time_apply_t: null pointer");
    elem_terms t = {};
    for (int k = 0; k < n_terms; ++k) {
        t.z[k] = w_host[k], t.blk[k] = blocks_host[k];
        STK_REQUIRE(t.z[k] && t.blk[k] && aligned16(t.z[k]), "stk_elem_time_apply_t: term %d: null or unaligned pointer", k);
    }
    const int64_t total = (int64_t)M * ld_x;
    const dim3 grid(stk_flat_grid(total, BS));
    hipStream_t st = stk_stream(stream);
    if (n_terms == 1)
        hipLaunchKernelGGL(elem_time_t_kernel<1>, grid, dim3(BS), 0, st, total, n_el, n_loc, ld_x, first_node, t, beta, x);
    else if (n_terms == 2)
        hipLaunchKernelGGL(elem_time_t_kernel<2>, grid, dim3(BS), 0, st, total, n_el, n_loc, ld_x, first_node, t, beta, x);
    else
        hipLaunchKernelGGL(elem_time_t_kernel<3>, grid, dim3(BS), 0, st, total, n_el, n_loc, ld_x, first_node, t, beta, x);
    STK_LAUNCH_CHECK();
    return 0;
}

extern "C" int stk_elem_block_mix(void *stream, int32_t M, int32_t n_el, const double *blocks, const double *x,
                                  double *y)
{
    const stk_timed timed_(STK_OP_TIME, stream);
    STK_REQUIRE(M > 0 && n_el > 0, "stk_elem_block_mix: bad sizes M=%d n_el=%d", M, n_el);
    STK_REQUIRE(blocks && x && y && aligned16(blocks) && aligned16(x) && aligned16(y),
                "stk_elem_block_mix: null or unaligned pointer");
    const int64_t total = (int64_t)M * n_el;
    hipLaunchKernelGGL(elem_block_mix_kernel, dim3(stk_flat_grid(total, BS)), dim3(BS), 0, stk_stream(stream), total,
                       n_el, blocks, x, y);
    STK_LAUNCH_CHECK();
    return 0;
}
