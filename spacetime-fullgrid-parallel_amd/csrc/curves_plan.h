// What the time curves (curves.hip) and the isotherms (iso.hip) share: the plan, and the cut
// of a cell along {u_h = theta} -- the order of the vertices and the points C_ab on the edges
// (include/stk.h "time curves").  The zone pieces of curves.hip and the level-set pieces of
// iso.hip are built from the SAME doubles: one definition, file-local like p1_mesh.h.
//
// ARITHMETIC: every product, quotient and sum rounded on its own (p1_mesh.h's pragma; the files
// that include this are compiled with -ffp-contract=off), and nothing here calls fma.
#pragma once
#include "p1_mesh.h"

#pragma clang fp contract(off)

struct stk_curves_plan {
    int32_t d;
    int64_t nv, nc, n_free, n_tiles, n_work;
    p1_mesh_dev mesh;
    double *vol;     // [nc]
    double *grad;    // [nc][d + 1][d]
    uint8_t *faces;  // [nc]: bit a = the face opposite vertex a is a boundary face
    double *work;    // [rows][batch columns][n_work] partials of a batch in flight
    int64_t work_doubles;
    stk_dev_arrays dev;  // owns every device array above
};

namespace {

// a point in registers: a vertex of the cell or a cut on one of its edges
template <int D>
struct pt {
    double x[D];
};

// how many vertices are above: U_a > theta, strictly (a NaN is not)
template <int D>
__device__ inline int cut_above(const double (&U)[D + 1], double theta)
{
    int n = 0;
#pragma unroll
    for (int a = 0; a <= D; ++a) n += U[a] > theta ? 1 : 0;
    return n;
}

// The vertices of a cell in the order q_0 .. q_d: those above in ascending a, then the others
// in ascending a, with their values W.  A stable partition, above ones first, by the adjacent
// exchanges of a bubble sort on the flag -- selects on whole records, no indexed access.
// cut(a, b) = q_a + s (q_b - q_a), s = (W_a - theta) / (W_a - W_b).
template <int D>
struct cell_cut {
    double W[D + 1], Q[D + 1][D], theta;

    __device__ inline cell_cut(const double (&U)[D + 1], const double (*P)[D], double theta_) : theta(theta_)
    {
        bool up[D + 1];
#pragma unroll
        for (int a = 0; a <= D; ++a) {
            W[a] = U[a], up[a] = U[a] > theta;
#pragma unroll
            for (int j = 0; j < D; ++j) Q[a][j] = P[a][j];
        }
#pragma unroll
        for (int pass = D; pass >= 1; --pass) {
#pragma unroll
            for (int i = 0; i < pass; ++i) {
                const bool swap = !up[i] && up[i + 1];
                const double w0 = W[i], w1 = W[i + 1];
                W[i] = swap ? w1 : w0, W[i + 1] = swap ? w0 : w1;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const double q0 = Q[i][j], q1 = Q[i + 1][j];
                    Q[i][j] = swap ? q1 : q0, Q[i + 1][j] = swap ? q0 : q1;
                }
                const bool u0 = up[i], u1 = up[i + 1];
                up[i] = swap ? u1 : u0, up[i + 1] = swap ? u0 : u1;
            }
        }
    }

    __device__ inline pt<D> vertex(int a) const
    {
        pt<D> c;
#pragma unroll
        for (int j = 0; j < D; ++j) c.x[j] = Q[a][j];
        return c;
    }

    __device__ inline pt<D> cut(int a, int b) const
    {
        const double s = (W[a] - theta) / (W[a] - W[b]);
        pt<D> c;
#pragma unroll
        for (int j = 0; j < D; ++j) c.x[j] = Q[a][j] + s * (Q[b][j] - Q[a][j]);
        return c;
    }
};

}  // namespace
