// Error norms against an exact solution ON THE DEVICE (include/stk.h "space-time error
// norms"): || u - u_h || and || grad (u - u_h) || in L2 of one time element times the
// mesh, by quadrature, for a slab of nodal values of the trial space -- without
// downloading the slab and without a nodal interpolant standing in for u.
//
//  * stk_err_plan_create  uploads the mesh and the vertex -> slab-row map, computes |T| and
//                         the gradients of the barycentric coordinates per cell
//                         (p1_geometry_kernel of p1_mesh.h, shared with the time curves)
//  * stk_err_points       the quadrature points of every cell, [d][nc][nq]: the kernel of
//                         stk_load_points (p1_mesh.h)
//  * stk_err_element      f [n_k][nc][nq] (and gf [n_k][d][nc][nq]) at those points for the
//                         n_k time points of ONE time element + the two rows of nodal values
//                         at its ends -> four sums over the mesh
//
// Two launches per call.  `cells`: a workgroup takes a tile of 256 consecutive cells, one
// lane per cell.  A lane keeps the d + 1 nodal values of its cell at both ends of the
// element in registers (a row gather, read once per call); the values of f travel through
// LDS, copied with unit-stride loads one time point at a time -- for gf one component at
// a time -- so the tile stays at 256 nq doubles.  The four numbers of the cells of a tile are
// added in a pairwise tree in LDS and leave as one partial per tile.  `finish`: one
// workgroup adds the partials in a pairwise tree over the tile index.  No atomics: tile i is
// cells [256 i, 256 i + 256) whatever the grid, so every sum has one shape, fixed by nc.
//
// ARITHMETIC: every product and every sum rounded on its own -- contraction is SWITCHED OFF
// for this file and for p1_mesh.h (their pragmas and -ffp-contract=off in the Makefile), as
// for the load engine and the sampler, and no kernel here calls fma.
#include "p1_mesh.h"

#pragma clang fp contract(off)

struct stk_err_plan {
    int32_t d;
    int64_t nv, nc, n_free, n_tiles;
    p1_mesh_dev mesh;
    double *vol;   // [nc]
    double *grad;  // [nc][d + 1][d]
    double *work;  // [n_tiles][4] partials of a call in flight
    stk_dev_arrays dev;  // owns every device array above
};

namespace {

constexpr int BS = 256;

struct err_times {
    double w_lo[STK_ERR_MAX_K], w_hi[STK_ERR_MAX_K], c[STK_ERR_MAX_K];
};

// pairwise tree over the BS lanes of four columns in LDS; the sums end in red[x * BS]
__device__ inline void tree4(double *red, int tid)
{
    for (int s = BS / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) {
#pragma unroll
            for (int x = 0; x < 4; ++x) red[x * BS + tid] = red[x * BS + tid] + red[x * BS + tid + s];
        }
    }
    __syncthreads();
}

// LDS: BS nq doubles (the values of f or of one component of gf for one time point), and
// the 4 BS doubles of the tree
template <int D, bool GRAD>
__global__ __launch_bounds__(BS) void err_cells_kernel(int64_t nc, int64_t n_tiles, int32_t nq, int32_t n_k,
                                                       const int32_t *__restrict__ cells,
                                                       const int32_t *__restrict__ row_of, const double *__restrict__ vol,
                                                       const double *__restrict__ grad, p1_rule r, err_times tm,
                                                       const double *__restrict__ f, const double *__restrict__ gf,
                                                       const double *__restrict__ u_lo, int64_t stride_lo,
                                                       const double *__restrict__ u_hi, int64_t stride_hi,
                                                       double *__restrict__ work)
{
    extern __shared__ double lds[];
    __shared__ double red[4 * BS];
    const int tid = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t cell0 = tile * BS;
        const int here = (int)(nc - cell0 < BS ? nc - cell0 : BS);
        const bool live = tid < here;
        double lo[D + 1], hi[D + 1], g[D + 1][D], v = 0.0;
        bool free_v[D + 1];
#pragma unroll
        for (int a = 0; a <= D; ++a) {
            lo[a] = hi[a] = 0.0, free_v[a] = false;
#pragma unroll
            for (int j = 0; j < D; ++j) g[a][j] = 0.0;
        }
        if (live) {
            const int64_t t = cell0 + tid;
            v = vol[t];
#pragma unroll
            for (int a = 0; a <= D; ++a) {
                const int32_t row = row_of[cells[(D + 1) * t + a]];
                free_v[a] = row >= 0;
                if (row >= 0) {
                    lo[a] = u_lo[(int64_t)row * stride_lo];
                    hi[a] = u_hi[(int64_t)row * stride_hi];
                }
            }
            if constexpr (GRAD) {
#pragma unroll
                for (int a = 0; a <= D; ++a)
#pragma unroll
                    for (int j = 0; j < D; ++j) g[a][j] = grad[((D + 1) * t + a) * D + j];
            }
        }
        double acc[4] = {0.0, 0.0, 0.0, 0.0};  // err L2, err H1, ref L2, ref H1
        for (int k = 0; k < n_k; ++k) {
            double U[D + 1];
#pragma unroll
            for (int a = 0; a <= D; ++a) U[a] = free_v[a] ? tm.w_lo[k] * lo[a] + tm.w_hi[k] * hi[a] : 0.0;
            const double *src = f + ((int64_t)k * nc + cell0) * nq;
            __syncthreads();  // the tile's readers of the step before are done
            for (int j = tid; j < here * nq; j += BS) lds[j] = src[j];
            __syncthreads();
            double X[4] = {0.0, 0.0, 0.0, 0.0};
            if (live) {
                for (int q = 0; q < nq; ++q) {
                    const double *l = r.l + q * (D + 1);
                    double uh = l[0] * U[0] + l[1] * U[1];
#pragma unroll
                    for (int a = 2; a <= D; ++a) uh = uh + l[a] * U[a];
                    const double fq = lds[tid * nq + q];
                    const double e = fq - uh;
                    X[0] = X[0] + (e * e) * r.w[q];
                    X[2] = X[2] + (fq * fq) * r.w[q];
                }
            }
            if constexpr (GRAD) {
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    double G = U[0] * g[0][j];
#pragma unroll
                    for (int a = 1; a <= D; ++a) G = G + U[a] * g[a][j];
                    const double *srcg = gf + (((int64_t)k * D + j) * nc + cell0) * nq;
                    __syncthreads();
                    for (int i = tid; i < here * nq; i += BS) lds[i] = srcg[i];
                    __syncthreads();
                    if (live) {
                        double ej = 0.0, rj = 0.0;
                        for (int q = 0; q < nq; ++q) {
                            const double gq = lds[tid * nq + q];
                            const double e = gq - G;
                            ej = ej + (e * e) * r.w[q];
                            rj = rj + (gq * gq) * r.w[q];
                        }
                        X[1] = X[1] + ej;
                        X[3] = X[3] + rj;
                    }
                }
            }
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const double term = tm.c[k] * (X[x] * v);
                acc[x] = k ? acc[x] + term : term;
            }
        }
        __syncthreads();  // the tree of the tile before has been read
#pragma unroll
        for (int x = 0; x < 4; ++x) red[x * BS + tid] = live ? acc[x] : 0.0;
        tree4(red, tid);
        if (tid < 4) work[4 * tile + tid] = red[tid * BS];
    }
}

// one workgroup: partial i + partial i + s for s = P / 2, P / 4, ..., 1 with P the power of
// two at or above n_tiles (an absent partner adds nothing) -- a tree whose shape n_tiles
// alone fixes.  In place on the workspace down to BS partials, then in LDS.
__global__ __launch_bounds__(BS) void err_finish_kernel(int64_t n_tiles, int64_t P, double *work, double *out4)
{
    __shared__ double red[4 * BS];
    const int tid = threadIdx.x;
    for (int64_t s = P / 2; s >= BS; s >>= 1) {
        for (int64_t i = tid; i < s && i + s < n_tiles; i += BS) {
#pragma unroll
            for (int x = 0; x < 4; ++x) work[4 * i + x] = work[4 * i + x] + work[4 * (i + s) + x];
        }
        __syncthreads();
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) red[x * BS + tid] = tid < n_tiles ? work[4 * (int64_t)tid + x] : 0.0;
    tree4(red, tid);
    if (tid < 4) out4[tid] = red[tid * BS];
}

}  // namespace

extern "C" int stk_err_plan_create(int32_t d, int64_t nv, int64_t nc, const double *points, const int64_t *cells,
                                   int64_t n_free, const int64_t *free_vertices, stk_err_plan **out)
{
    const char *who = "stk_err_plan_create";
    std::vector<int32_t> row_of;
    if (int rc = p1_plan_open(who, d, nv, nc, points, cells, n_free, free_vertices, out, &row_of)) return rc;

    stk_err_plan *p = new stk_err_plan();
    p->d = d, p->nv = nv, p->nc = nc, p->n_free = n_free, p->n_tiles = (nc + BS - 1) / BS;
    int rc = p1_mesh_upload(p->dev, &p->mesh, d, nv, nc, points, cells, &row_of);
    if (!rc) rc = p1_geometry(who, p->dev, p, &p->vol);
    if (!rc && !(p->work = p->dev.alloc<double>((size_t)p->n_tiles * 4))) rc = p1_no_array(who);
    if (rc) {
        delete p;
        return rc;
    }
    *out = p;
    return 0;
}

extern "C" int stk_err_plan_destroy(stk_err_plan *plan)
{
    delete plan;
    return 0;
}

extern "C" int stk_err_points(void *stream, const stk_err_plan *plan, int32_t nq, const double *rule_points,
                              double *q_points)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan && q_points, "stk_err_points: null pointer");
    return p1_points("stk_err_points", stream, plan, nq, rule_points, q_points);
}

extern "C" int stk_err_element(void *stream, stk_err_plan *plan, int32_t nq, const double *rule_weights,
                               const double *rule_points, int32_t n_k, const double *w_lo, const double *w_hi,
                               const double *c, const double *f, const double *gf, const double *u_lo,
                               int64_t stride_lo, const double *u_hi, int64_t stride_hi, double *out4)
{
    const stk_timed timed_(STK_OP_SPACE, stream);
    STK_REQUIRE(plan && rule_weights && rule_points && w_lo && w_hi && c && f && u_lo && u_hi && out4,
                "stk_err_element: null pointer");
    STK_REQUIRE(n_k >= 1 && n_k <= STK_ERR_MAX_K, "stk_err_element: %d time points (1..%d)", n_k, STK_ERR_MAX_K);
    STK_REQUIRE(stride_lo >= 1 && stride_hi >= 1, "stk_err_element: row strides %lld and %lld (at least 1)",
                (long long)stride_lo, (long long)stride_hi);
    p1_rule r = {};
    if (int rc = p1_fill_rule("stk_err_element", plan->d, nq, rule_weights, rule_points, &r)) return rc;
    err_times tm = {};
    for (int k = 0; k < n_k; ++k) tm.w_lo[k] = w_lo[k], tm.w_hi[k] = w_hi[k], tm.c[k] = c[k];
    hipStream_t st = stk_stream(stream);
    const size_t lds = (size_t)BS * nq * sizeof(double);
    const int64_t n_tiles = plan->n_tiles;
    const dim3 grid((unsigned)(n_tiles < 256 * 16 ? n_tiles : 256 * 16));
#define STK_ERR_LAUNCH(D, GRAD)                                                                                          \
    hipLaunchKernelGGL((err_cells_kernel<D, GRAD>), grid, dim3(BS), lds, st, plan->nc, n_tiles, nq, n_k, plan->mesh.cells, \
                       plan->mesh.row_of, plan->vol, plan->grad, r, tm, f, gf, u_lo, stride_lo, u_hi, stride_hi, plan->work)
    if (plan->d == 2) {
        if (gf)
            STK_ERR_LAUNCH(2, true);
        else
            STK_ERR_LAUNCH(2, false);
    } else {
        if (gf)
            STK_ERR_LAUNCH(3, true);
        else
            STK_ERR_LAUNCH(3, false);
    }
#undef STK_ERR_LAUNCH
    STK_LAUNCH_CHECK();
    int64_t P = 1;
    while (P < n_tiles) P <<= 1;
    hipLaunchKernelGGL(err_finish_kernel, dim3(1), dim3(BS), 0, st, n_tiles, P, plan->work, out4);
    STK_LAUNCH_CHECK();
    return 0;
}
