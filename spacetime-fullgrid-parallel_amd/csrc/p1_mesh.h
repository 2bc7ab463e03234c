// The simplicial P1 mesh as the load engine (load_dev.hip), the error norms
// (err_norms.hip), the sampler (sample.hip), the time curves and the isotherms (curves.hip,
// iso.hip) and the solidification scan (solid.hip) see it: THE
// definition of the simplex geometry, of |T| and the gradients per cell, of the quadrature
// points of a cell and of the time bracket of a pair, and the host side of a plan -- the
// opening checks (p1_plan_open: the arguments, the mesh, the vertex -> slab-row map), the int32
// cells and the device arrays (p1_mesh_upload), |T| and the gradients of every cell
// (p1_geometry), all allocated from the plan's stk_dev_arrays.  Everything is file-local: a
// translation unit that includes this gets its own copy, its kernels in its own code object.
//
// ARITHMETIC: every product and every sum rounded on its own.  Contraction is SWITCHED OFF
// from here on (the pragma below); the files that include this are also compiled
// with -ffp-contract=off (Makefile), and nothing here calls fma.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "stk_common.h"

#pragma clang fp contract(off)

static_assert(STK_LOAD_MAX_NQ == STK_ERR_MAX_NQ, "stk_load_points and stk_err_points share one kernel and one rule");

namespace {

// ---- the simplex of a cell ----------------------------------------------------------------
// Edge vectors e_r = p[c[r + 1]] - p[c[0]]; cof[r] = det * grad lambda_(r + 1), the rows of
// the adjugate of the edge matrix: (e11, -e10), (-e01, e00) for a triangle, the cross
// products e1 x e2, e2 x e0, e0 x e1 for a tetrahedron; det = e00 e11 - e01 e10, or
// e0 . (e1 x e2) summed from the left.
template <int D>
struct p1_simplex {
    const double *p0;
    double cof[D][D], det;
};

template <int D>
__host__ __device__ inline p1_simplex<D> p1_simplex_of(const double *__restrict__ pts, const int32_t *__restrict__ c)
{
    p1_simplex<D> s;
    s.p0 = pts + D * (int64_t)c[0];
    double e[D][D];
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) e[r][k] = pts[D * (int64_t)c[r + 1] + k] - s.p0[k];
    if constexpr (D == 2) {
        s.cof[0][0] = e[1][1], s.cof[0][1] = -e[1][0];
        s.cof[1][0] = -e[0][1], s.cof[1][1] = e[0][0];
        s.det = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double *a = e[(r + 1) % 3], *b = e[(r + 2) % 3];
            s.cof[r][0] = a[1] * b[2] - a[2] * b[1];
            s.cof[r][1] = a[2] * b[0] - a[0] * b[2];
            s.cof[r][2] = a[0] * b[1] - a[1] * b[0];
        }
        s.det = (e[0][0] * s.cof[0][0] + e[0][1] * s.cof[0][1]) + e[0][2] * s.cof[0][2];
    }
    return s;
}

// |T|: the double of stk_p1_load_sum_2d and of source/assembly.py:_simplex_geometry
template <int D>
__host__ __device__ inline double p1_volume(const p1_simplex<D> &s)
{
    return fabs(s.det) / (D == 2 ? 2.0 : 6.0);
}

// G[a][j] = d_j lambda_a: every quotient rounded once, G[0] = ((0 - G[1]) - G[2]) [- G[3]]
template <int D>
__host__ __device__ inline void p1_gradients(const p1_simplex<D> &s, double (*G)[D])
{
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int j = 0; j < D; ++j) G[r + 1][j] = s.cof[r][j] / s.det;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        G[0][j] = (0.0 - G[1][j]) - G[2][j];
        if constexpr (D == 3) G[0][j] = G[0][j] - G[3][j];
    }
}

// barycentric coordinates of x: l_(r + 1) = ((x - p0) . cof[r]) / det, the dot product summed
// from the left; l0 = ((1 - l1) - l2) [- l3].  A vertex of the cell gets exactly (1, 0, 0).
template <int D>
__host__ __device__ inline void p1_barycentric(const p1_simplex<D> &s, const double *x, double *l)
{
    double q[D];
#pragma unroll
    for (int k = 0; k < D; ++k) q[k] = x[k] - s.p0[k];
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double dot = q[0] * s.cof[r][0] + q[1] * s.cof[r][1];
        if constexpr (D == 3) dot = dot + q[2] * s.cof[r][2];
        l[r + 1] = dot / s.det;
    }
    l[0] = (1.0 - l[1]) - l[2];
    if constexpr (D == 3) l[0] = l[0] - l[3];
}

// ---- the quadrature points of every cell --------------------------------------------------
constexpr int P1_BS = 256;

struct p1_rule {
    double w[STK_LOAD_MAX_NQ];
    double l[STK_LOAD_MAX_NQ * 4];  // l[q (d + 1) + a]
};

inline int p1_fill_rule(const char *who, int32_t d, int32_t nq, const double *w, const double *l, p1_rule *r)
{
    STK_REQUIRE(nq >= 1 && nq <= STK_LOAD_MAX_NQ, "%s: %d quadrature points (1..%d)", who, nq, STK_LOAD_MAX_NQ);
    STK_REQUIRE(l, "%s: no rule points", who);
    for (int q = 0; q < nq; ++q) {
        r->w[q] = w ? w[q] : 0.0;
        for (int a = 0; a <= d; ++a) r->l[q * (d + 1) + a] = l[q * (d + 1) + a];
    }
    return 0;
}

// one lane per (cell, q): l0 p0 + l1 p1 + ..., summed from the left
template <int D>
__global__ __launch_bounds__(P1_BS) void p1_points_kernel(int64_t total, int32_t nq, const double *__restrict__ p,
                                                          const int32_t *__restrict__ cells, p1_rule r,
                                                          double *__restrict__ out)
{
    // the rule through LDS: a lane's q is its own, and the kernel arguments are read
    // with indices the whole wavefront shares
    __shared__ double rule[STK_LOAD_MAX_NQ * (D + 1)];
    if (threadIdx.x == 0)
        for (int j = 0; j < nq * (D + 1); ++j) rule[j] = r.l[j];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * P1_BS;
    for (int64_t idx = (int64_t)blockIdx.x * P1_BS + threadIdx.x; idx < total; idx += stride) {
        const int64_t t = idx / nq;
        const int q = (int)(idx - t * nq);
        const int32_t *c = cells + (D + 1) * t;
        double l[D + 1];
#pragma unroll
        for (int a = 0; a <= D; ++a) l[a] = rule[q * (D + 1) + a];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double x = l[0] * p[D * (int64_t)c[0] + k];
#pragma unroll
            for (int a = 1; a <= D; ++a) x = x + l[a] * p[D * (int64_t)c[a] + k];
            out[k * total + idx] = x;
        }
    }
}

// ---- |T| and the gradients of every cell (the error norms, the time curves) ----------------
// |T| and grad lambda_a per cell (p1_volume, p1_gradients), but grad lambda_0 =
// -((g_1 + g_2) [+ g_3]), the expression of source/assembly.py:_simplex_geometry: it gives
// -0.0 where p1_gradients gives +0.0 (g_1 = -g_2), the only doubles in which the two differ.
// A null `vol`: |T| is not stored (the solidification scan has no use for it).
template <int D>
__global__ __launch_bounds__(P1_BS) void p1_geometry_kernel(int64_t nc, const double *__restrict__ p,
                                                          const int32_t *__restrict__ cells, double *__restrict__ vol,
                                                          double *__restrict__ grad)
{
    const int64_t stride = (int64_t)gridDim.x * P1_BS;
    for (int64_t t = (int64_t)blockIdx.x * P1_BS + threadIdx.x; t < nc; t += stride) {
        const p1_simplex<D> s = p1_simplex_of<D>(p, cells + (D + 1) * t);
        if (vol) vol[t] = p1_volume(s);
        double g[D + 1][D];  // g[a][j]
        p1_gradients(s, g);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double sum = g[1][j] + g[2][j];
            if constexpr (D == 3) sum = sum + g[3][j];
            g[0][j] = -sum;
        }
#pragma unroll
        for (int a = 0; a <= D; ++a)
#pragma unroll
            for (int j = 0; j < D; ++j) grad[((D + 1) * t + a) * D + j] = g[a][j];
    }
}

// ---- the time bracket of a pair -----------------------------------------------------------
// t_p in [0, (N - 1) h] lies in element e = min(floor(t_p / h), N - 2) with the weights
// (w0, w1) = (1 - s, s), s = t_p / h - e; c0, c1 are the columns of the nodes e, e + 1 on a
// rank whose first node is t_begin, have0 / have1 whether it holds them.
struct p1_bracket {
    double w0, w1;
    int64_t c0, c1;
    bool have0, have1;
};

__device__ inline p1_bracket p1_time_bracket(double tp, double h, int32_t N, int32_t t_begin, int32_t n_loc)
{
    p1_bracket b;
    const double x = tp / h;
    double ef = floor(x);
    if (ef > (double)(N - 2)) ef = (double)(N - 2);
    b.w1 = x - ef, b.w0 = 1.0 - b.w1;
    b.c0 = (int64_t)ef - t_begin, b.c1 = b.c0 + 1;
    b.have0 = b.c0 >= 0 && b.c0 < n_loc, b.have1 = b.c1 >= 0 && b.c1 < n_loc;
    return b;
}

// ---- the host side of a plan --------------------------------------------------------------
inline int p1_check_mesh(const char *who, int32_t d, int64_t nv, int64_t nc, const double *points, const int64_t *cells)
{
    STK_REQUIRE((d == 2 || d == 3) && nv > 0 && nc > 0 && points && cells, "%s: bad arguments", who);
    STK_REQUIRE(nv < ((int64_t)1 << 31) && (int64_t)(d + 1) * nc < ((int64_t)1 << 31), "%s: mesh too large for 32-bit tables",
                who);
    for (int64_t q = 0; q < (int64_t)(d + 1) * nc; ++q)
        STK_REQUIRE(cells[q] >= 0 && cells[q] < nv, "%s: cell %lld names vertex %lld", who, (long long)(q / (d + 1)),
                    (long long)cells[q]);
    return 0;
}

// row_of[v] = slab row of vertex v, -1 on the boundary
inline int p1_row_of(const char *who, int64_t nv, int64_t n_free, const int64_t *free_vertices, std::vector<int32_t> *row_of)
{
    row_of->assign((size_t)nv, -1);
    for (int64_t i = 0; i < n_free; ++i) {
        const int64_t v = free_vertices[i];
        STK_REQUIRE(v >= 0 && v < nv && (*row_of)[(size_t)v] < 0 && n_free < ((int64_t)1 << 31),
                    "%s: free dof %lld is vertex %lld (out of range or named twice)", who, (long long)i, (long long)v);
        (*row_of)[(size_t)v] = (int32_t)i;
    }
    return 0;
}

// what the plans of the error norms, the time curves and the solidification scan open with:
// the arguments, the mesh, and row_of from the free vertices -- all before the first HIP call
inline int p1_plan_open(const char *who, int32_t d, int64_t nv, int64_t nc, const double *points, const int64_t *cells,
                        int64_t n_free, const int64_t *free_vertices, const void *out, std::vector<int32_t> *row_of)
{
    STK_REQUIRE((d == 2 || d == 3) && nv > 0 && nc > 0 && points && cells && n_free > 0 && free_vertices && out,
                "%s: bad arguments", who);
    STK_REQUIRE(n_free < ((int64_t)1 << 31), "%s: mesh too large for 32-bit tables", who);
    if (int rc = p1_check_mesh(who, d, nv, nc, points, cells)) return rc;
    return p1_row_of(who, nv, n_free, free_vertices, row_of);
}

// a HIP call of a plan's set-up: "<who>: <what HIP says>" where it fails
inline int p1_hip(const char *who, hipError_t e)
{
    if (e != hipSuccess) stk_set_error("%s: %s", who, hipGetErrorString(e));
    return e != hipSuccess;
}

// an allocation of a plan's set-up that came back null: "<who>: <what the owner's seam said>"
inline int p1_no_array(const char *who)
{
    const std::string why = stk_last_error();
    stk_set_error("%s: %s", who, why.c_str());
    return 1;
}

// the device arrays of a checked mesh; a plan embeds one, its stk_dev_arrays owns them
struct p1_mesh_dev {
    double *points;   // [nv][d]
    int32_t *cells;   // [nc][d + 1]
    int32_t *row_of;  // [nv], or null where the plan needs none
};

inline int p1_mesh_upload(stk_dev_arrays &dev, p1_mesh_dev *m, int32_t d, int64_t nv, int64_t nc, const double *points,
                          const int64_t *cells, const std::vector<int32_t> *row_of)
{
    std::vector<int32_t> cells32((size_t)(d + 1) * nc);
    for (size_t q = 0; q < cells32.size(); ++q) cells32[q] = (int32_t)cells[q];
    m->points = dev.upload(points, (size_t)nv * d);
    m->cells = dev.upload(cells32);
    if (row_of) m->row_of = dev.upload(*row_of);
    return !m->points || !m->cells || (row_of && !m->row_of);
}

// plan->grad [nc][d + 1][d] and, where the plan wants |T|, *vol [nc] of the plan's uploaded mesh:
// allocated here from the plan's owner, filled by p1_geometry_kernel on the null stream,
// complete on return.  A template over the plan, so that only a file that calls it carries
// the kernel.
template <class Plan>
int p1_geometry(const char *who, stk_dev_arrays &dev, Plan *plan, double **vol)
{
    const int32_t d = plan->d;
    const int64_t nc = plan->nc;
    const p1_mesh_dev &m = plan->mesh;
    if (vol && !(*vol = dev.alloc<double>((size_t)nc))) return p1_no_array(who);
    if (!(plan->grad = dev.alloc<double>((size_t)(d + 1) * nc * d))) return p1_no_array(who);
    const dim3 grid(stk_flat_grid(nc, P1_BS));
    double *v = vol ? *vol : nullptr;
    if (d == 2)
        hipLaunchKernelGGL(p1_geometry_kernel<2>, grid, dim3(P1_BS), 0, 0, nc, m.points, m.cells, v, plan->grad);
    else
        hipLaunchKernelGGL(p1_geometry_kernel<3>, grid, dim3(P1_BS), 0, 0, nc, m.points, m.cells, v, plan->grad);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return p1_hip(who, e);
}

// stk_load_points and stk_err_points: q_points [d][nc][nq] on the device.  A template over the
// plan, so that only a file that calls it carries the kernel.
template <class Plan>
int p1_points(const char *who, void *stream, const Plan *plan, int32_t nq, const double *rule_points, double *q_points)
{
    p1_rule r = {};
    if (int rc = p1_fill_rule(who, plan->d, nq, nullptr, rule_points, &r)) return rc;
    const int64_t total = plan->nc * nq;
    const dim3 grid(stk_flat_grid(total, P1_BS));
    hipStream_t st = stk_stream(stream);
    const p1_mesh_dev &m = plan->mesh;
    if (plan->d == 2)
        hipLaunchKernelGGL(p1_points_kernel<2>, grid, dim3(P1_BS), 0, st, total, nq, m.points, m.cells, r, q_points);
    else
        hipLaunchKernelGGL(p1_points_kernel<3>, grid, dim3(P1_BS), 0, st, total, nq, m.points, m.cells, r, q_points);
    STK_LAUNCH_CHECK();
    return 0;
}

}  // namespace
