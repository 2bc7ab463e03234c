// Load vectors of a simplicial P1 mesh ON THE DEVICE, written into test-space slabs
// (include/stk.h "space-time load vectors"): what a right-hand side g(t, x) that is no
// short separable sum needs -- int g(t_k, .) phi_i for every time quadrature point t_k,
// hundreds of load vectors per problem, where the host routines stk_p1_load_points_2d /
// stk_p1_load_sum_2d (mesh_refine.hip) serve the single one of u0.
//
//  * stk_load_plan_create  uploads the mesh, computes |T| per cell and builds the
//                          vertex -> (cell, local vertex) incidence of the free dofs, every
//                          list in ascending (cell, local vertex)
//  * stk_load_points       the quadrature points of every cell, [d][nc][nq]
//  * stk_load_columns      f [n_k][nc][nq] at those points -> one pair of slab columns,
//                          out[i ld + a] (+)= sum_k c[k][a] L_k[i]
//
// Two passes per call.  `shares`: a workgroup takes 256 cells, copies their nq values of
// f into LDS with unit-stride loads, one lane per cell forms the d + 1 shares
// (sum_q (f_q w_q) l_qa) |T| and the shares leave through LDS with unit-stride stores,
// [k][cell][a].  `gather`: one lane per free dof (in the caller's mesh-tile order, so the
// lanes of a workgroup read neighbouring cells) sums its shares per time point and
// stores the pair of columns as one 16-byte word.  No atomics: every sum has one owner
// and one order, so a slab does not depend on the launch shape or on the rank that
// builds it.
//
// ARITHMETIC: the doubles of the host routines, bit for bit -- every product and every
// sum is rounded on its own.  hipcc contracts a * b + c into a fused multiply-add in
// device code by default; contraction is SWITCHED OFF for this file and for p1_mesh.h (their
// pragmas and -ffp-contract=off in the Makefile), and no kernel here calls fma.
#include "p1_mesh.h"

#pragma clang fp contract(off)

struct stk_load_plan {
    int32_t d, max_k;
    int64_t nv, nc, n_free, ns;  // ns = (d + 1) nc slots (cell, local vertex)
    p1_mesh_dev mesh;            // no row_of: the incidence lists below take its place
    double *vol;                 // [nc]
    int32_t *inc_ptr;            // [n_free + 1]
    int32_t *inc_slot;           // slots of free dof i: inc_ptr[i] .. inc_ptr[i + 1], ascending
    int32_t *order;              // processing order of the free dofs, or null
    double *shares;              // [max_k][ns] workspace of stk_load_columns
    stk_dev_arrays dev;          // owns every device array above
};

namespace {

constexpr int BS = 256;

struct load_coef {
    double c[STK_LOAD_MAX_K * 2];
};

// |T| per cell (p1_volume)
template <int D>
__global__ __launch_bounds__(BS) void load_volume_kernel(int64_t nc, const double *__restrict__ p,
                                                         const int32_t *__restrict__ cells, double *__restrict__ vol)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t t = (int64_t)blockIdx.x * BS + threadIdx.x; t < nc; t += stride)
        vol[t] = p1_volume(p1_simplex_of<D>(p, cells + (D + 1) * t));
}

// blockIdx.y = time point; a workgroup walks tiles of BS cells.  LDS: BS max(nq, D + 1)
// doubles, the values of f on the way in and the shares on the way out.
template <int D>
__global__ __launch_bounds__(BS) void load_shares_kernel(int64_t nc, int32_t nq, const double *__restrict__ f,
                                                         const double *__restrict__ vol, p1_rule r,
                                                         double *__restrict__ shares)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x;
    const double *fk = f + (int64_t)blockIdx.y * nc * nq;
    double *sk = shares + (int64_t)blockIdx.y * nc * (D + 1);
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t cell0 = (int64_t)blockIdx.x * BS; cell0 < nc; cell0 += stride) {
        const int here = (int)(nc - cell0 < BS ? nc - cell0 : BS);
        const double *src = fk + cell0 * nq;
        for (int j = tid; j < here * nq; j += BS) lds[j] = src[j];
        __syncthreads();
        double s[D + 1];
#pragma unroll
        for (int a = 0; a <= D; ++a) s[a] = 0.0;
        if (tid < here) {
            for (int q = 0; q < nq; ++q) {
                const double fw = lds[tid * nq + q] * r.w[q];
#pragma unroll
                for (int a = 0; a <= D; ++a) s[a] = s[a] + fw * r.l[q * (D + 1) + a];
            }
        }
        __syncthreads();
        if (tid < here) {
            const double v = vol[cell0 + tid];
#pragma unroll
            for (int a = 0; a <= D; ++a) lds[tid * (D + 1) + a] = s[a] * v;
        }
        __syncthreads();
        double *dst = sk + cell0 * (D + 1);
        for (int j = tid; j < here * (D + 1); j += BS) dst[j] = lds[j];
        __syncthreads();
    }
}

// one lane per free dof: L_k = its shares in ascending (cell, local vertex), then the
// pair sum_k c[k][a] L_k with k ascending, moved as one 16-byte word
__global__ __launch_bounds__(BS) void load_gather_kernel(int64_t n_free, int64_t ns, int32_t n_k,
                                                         const int32_t *__restrict__ inc_ptr,
                                                         const int32_t *__restrict__ inc_slot,
                                                         const int32_t *__restrict__ order,
                                                         const double *__restrict__ shares, load_coef c,
                                                         int32_t accumulate, int64_t ld, double *out)
{
    const int64_t stride = (int64_t)gridDim.x * BS;
    for (int64_t idx = (int64_t)blockIdx.x * BS + threadIdx.x; idx < n_free; idx += stride) {
        const int64_t i = order ? order[idx] : idx;
        const int32_t begin = inc_ptr[i], end = inc_ptr[i + 1];
        double2 acc = make_double2(0.0, 0.0);
        for (int k = 0; k < n_k; ++k) {
            const double *sk = shares + (int64_t)k * ns;
            double L = 0.0;
            for (int32_t s = begin; s < end; ++s) L = L + sk[inc_slot[s]];
            const double t0 = c.c[2 * k] * L, t1 = c.c[2 * k + 1] * L;
            acc.x = k ? acc.x + t0 : t0;
            acc.y = k ? acc.y + t1 : t1;
        }
        double2 *dst = reinterpret_cast<double2 *>(out + i * ld);
        if (accumulate) {
            const double2 old = *dst;
            acc.x = old.x + acc.x;
            acc.y = old.y + acc.y;
        }
        *dst = acc;
    }
}

}  // namespace

extern "C" int stk_load_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points, const int64_t *cells,
                                    int64_t n_free, const int64_t *free_vertices, const int32_t *row_order,
                                    int32_t max_k, stk_load_plan **out)
{
    STK_REQUIRE((d == 2 || d == 3) && nv > 0 && nc > 0 && points && cells && n_free > 0 && free_vertices && out,
                "stk_load_plan_create: bad arguments");
    STK_REQUIRE(max_k >= 1 && max_k <= STK_LOAD_MAX_K, "stk_load_plan_create: %d time points per call (1..%d)", max_k,
                STK_LOAD_MAX_K);
    if (int rc = p1_check_mesh("stk_load_plan_create", d, nv, nc, points, cells)) return rc;
    const int64_t ns = (int64_t)(d + 1) * nc;
    for (int64_t i = 0; i < n_free; ++i)
        STK_REQUIRE(free_vertices[i] >= 0 && free_vertices[i] < nv, "stk_load_plan_create: free dof %lld is vertex %lld",
                    (long long)i, (long long)free_vertices[i]);
    std::vector<int32_t> order;
    if (row_order) {
        std::vector<uint8_t> seen((size_t)n_free, 0);
        for (int64_t i = 0; i < n_free; ++i) {
            const int32_t r = row_order[i];
            STK_REQUIRE(r >= 0 && r < n_free && !seen[r], "stk_load_plan_create: row_order is no permutation at %lld",
                        (long long)i);
            seen[r] = 1;
        }
        order.assign(row_order, row_order + n_free);
    }
    // slots of every vertex: a counting sort over ascending slot numbers leaves every
    // list ascending
    std::vector<int64_t> start((size_t)nv + 1, 0);
    for (int64_t q = 0; q < ns; ++q) ++start[cells[q] + 1];
    for (int64_t v = 0; v < nv; ++v) start[v + 1] += start[v];
    std::vector<int32_t> slot((size_t)ns), fill((size_t)nv, 0);
    for (int64_t q = 0; q < ns; ++q) slot[start[cells[q]] + fill[cells[q]]++] = (int32_t)q;
    std::vector<int32_t> inc_ptr((size_t)n_free + 1, 0);
    int64_t total = 0;
    for (int64_t i = 0; i < n_free; ++i) {
        total += start[free_vertices[i] + 1] - start[free_vertices[i]];
        STK_REQUIRE(total < ((int64_t)1 << 31), "stk_load_plan_create: incidence too large for 32-bit tables");
        inc_ptr[i + 1] = (int32_t)total;
    }
    std::vector<int32_t> inc_slot((size_t)total);
    for (int64_t i = 0; i < n_free; ++i) {
        const int64_t v = free_vertices[i];
        std::copy(slot.begin() + start[v], slot.begin() + start[v + 1], inc_slot.begin() + inc_ptr[i]);
    }

    stk_load_plan *p = new stk_load_plan();
    p->d = d, p->max_k = max_k, p->nv = nv, p->nc = nc, p->n_free = n_free, p->ns = ns;
    int rc = p1_mesh_upload(p->dev, &p->mesh, d, nv, nc, points, cells, nullptr);
    if (!rc) rc = !(p->inc_ptr = p->dev.upload(inc_ptr)) || !(p->inc_slot = p->dev.upload(inc_slot));
    if (!rc && row_order) rc = !(p->order = p->dev.upload(order));
    if (!rc) {
        p->vol = p->dev.alloc<double>((size_t)nc);
        p->shares = p->vol ? p->dev.alloc<double>((size_t)max_k * ns) : nullptr;
        if (!p->shares) rc = p1_no_array("stk_load_plan_create");
    }
    if (!rc) {
        const dim3 grid(stk_flat_grid(nc, BS));
        if (d == 2)
            hipLaunchKernelGGL(load_volume_kernel<2>, grid, dim3(BS), 0, 0, nc, p->mesh.points, p->mesh.cells, p->vol);
        else
            hipLaunchKernelGGL(load_volume_kernel<3>, grid, dim3(BS), 0, 0, nc, p->mesh.points, p->mesh.cells, p->vol);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        rc = p1_hip("stk_load_plan_create", e);
    }
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return 0;
}

extern "C" int stk_load_plan_destroy(stk_load_plan *plan)
{
    delete plan;
    return 0;
}

extern "C" int stk_load_points(void *stream, const stk_load_plan *plan, int32_t nq, const double *rule_points,
                               double *q_points)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan && q_points, "stk_load_points: null pointer");
    return p1_points("stk_load_points", stream, plan, nq, rule_points, q_points);
}

extern "C" int stk_load_columns(void *stream, const stk_load_plan *plan, int32_t nq, const double *rule_weights,
                                const double *rule_points, int32_t n_k, const double *f, const double *coef,
                                int32_t accumulate, int32_t ld, double *out_pair)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan && rule_weights && f && coef && out_pair, "stk_load_columns: null pointer");
    STK_REQUIRE(n_k >= 1 && n_k <= plan->max_k, "stk_load_columns: %d time points on a plan made for %d", n_k, plan->max_k);
    STK_REQUIRE(ld >= 2 && (ld & 1) == 0 && (((uintptr_t)out_pair) & 15) == 0,
                "stk_load_columns: the column pair must be 16-byte aligned in a slab of even leading dimension (ld=%d)", ld);
    p1_rule r = {};
    if (int rc = p1_fill_rule("stk_load_columns", plan->d, nq, rule_weights, rule_points, &r)) return rc;
    load_coef c = {};
    for (int k = 0; k < 2 * n_k; ++k) c.c[k] = coef[k];
    hipStream_t st = stk_stream(stream);
    const int d = plan->d;
    const size_t lds = (size_t)BS * (nq > d + 1 ? nq : d + 1) * sizeof(double);
    const dim3 grid(stk_flat_grid(plan->nc, BS) < 2048 ? stk_flat_grid(plan->nc, BS) : 2048, n_k);
    if (d == 2)
        hipLaunchKernelGGL(load_shares_kernel<2>, grid, dim3(BS), lds, st, plan->nc, nq, f, plan->vol, r, plan->shares);
    else
        hipLaunchKernelGGL(load_shares_kernel<3>, grid, dim3(BS), lds, st, plan->nc, nq, f, plan->vol, r, plan->shares);
    STK_LAUNCH_CHECK();
    hipLaunchKernelGGL(load_gather_kernel, dim3(stk_flat_grid(plan->n_free, BS)), dim3(BS), 0, st, plan->n_free, plan->ns,
                       n_k, plan->inc_ptr, plan->inc_slot, plan->order, plan->shares, c, accumulate, (int64_t)ld, out_pair);
    STK_LAUNCH_CHECK();
    return 0;
}
