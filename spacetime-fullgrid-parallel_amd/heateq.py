#!/usr/bin/env python3
"""Serial driver: Andreev's method on tensor-product trial spaces, through the
serial LinearOperator surface of source/linop.py (counterpart of reference
heateq.py:18-158).

Same structure as the reference: X = H1_t x H1_x, Y = L2_t(order 1) x H1_x,
B = B1 + B2, K = Kinv_time kron Kinv_space, S = B^T K B + G, P block diagonal
over the wavelet levels, solved with PCG.  The matrices come from the build's own
P1 assembly (source/assembly.py) instead of NGSolve; every operator application
runs on the GPU.  The operators accept the reference's flat NumPy vectors (one
round trip over PCIe per apply) and device vectors (source/linop.py:
DeviceLinearOperator); solve() keeps the whole iteration on the device.  The
time-parallel path is heateq_mpi.py."""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from source import driver  # noqa: E402
from source.assembly import (DeviceLoadPlan, fill_test_space_slab,  # noqa: E402
                             space_load, space_matrices,
                             time_load_test_space, time_matrices,
                             time_matrices_test_space)
from source.linalg import PCG  # noqa: E402
from source.linop import (BlockDiagLinOp, CompositeLinOp,  # noqa: E402
                          DeviceLinearOperator, InvLinOp, KronLinOp,
                          device_vector, host_vector)
from source.multigrid import MeshHierarchy, MultiGrid  # noqa: E402
from source.postprocess import PostProcessing  # noqa: E402
from source.problem import problem_helper  # noqa: E402
from source.wavelets import WaveletTransformOp  # noqa: E402


class HeatEquation(PostProcessing):
    """Implementation of Andreev's method for tensor-product trial spaces
    (reference heateq.py:18-107); sampling, maps, curves and error norms of a solution:
    source/postprocess.py."""
    def __init__(self, J_space=2, J_time=None, problem='square',
                 precond='multigrid', alpha=0.3, smoothsteps=3, vcycles=2):
        if J_time is None:
            J_time = J_space
        mesh_space, bc, mesh_time, data, fn = problem_helper(problem,
                                                             J_space=J_space,
                                                             J_time=J_time)
        self._init_postprocessing(mesh_space, mesh_time, data)
        self.path = data.get('path')  # c(t) of a problem that follows one (--track_out), else None
        A_t, L_t, M_t, G_t, u0_t = time_matrices(mesh_time)
        M_Y, Minv_Y, B1_t, B2_t = time_matrices_test_space(mesh_time)
        M_x, A_x = space_matrices(mesh_space)
        self.N, self.M = A_t.shape[0], M_x.shape[0]
        self.N_Y = M_Y.shape[0]  # time dofs of the test space
        self.M_x, self.A_x = M_x, A_x
        self.time_mats = dict(A_t=A_t, L_t=L_t, M_t=M_t, G_t=G_t, u0_t=u0_t,
                              Minv_Y=Minv_Y, B1_t=B1_t, B2_t=B2_t)

        # B = B1 + B2 (heateq.py:45-54), G (:49-50, :55)
        self.B = KronLinOp(B1_t, M_x) + KronLinOp(B2_t, A_x)
        self.BT = (KronLinOp(sp.csr_matrix(B1_t.T), M_x) +
                   KronLinOp(sp.csr_matrix(B2_t.T), A_x))
        self.G = KronLinOp(G_t, M_x)

        if precond == 'multigrid':
            self.hierarchy = MeshHierarchy(mesh_space)

            def mk(mat):
                return MultiGrid(mat, self.hierarchy, smoothsteps=smoothsteps,
                                 vcycles=vcycles)
        else:
            self.hierarchy = None
            mk = InvLinOp
        # preconditioner on Y (heateq.py:57-63)
        self.K = KronLinOp(Minv_Y, mk(A_x))

        # wavelet transform (heateq.py:65-68)
        W_t = WaveletTransformOp(J_time)
        eye = sp.eye(self.M, format='csr')
        self.W = KronLinOp(W_t, eye)
        self.WT = KronLinOp(W_t.T, eye)

        # preconditioner on X (heateq.py:70-85)
        self.alpha = alpha
        self.C_j = [mk(sp.csr_matrix(2**j * M_x + alpha * A_x))
                    for j in range(J_time + 1)]
        self.CAC_j = [CompositeLinOp([self.C_j[j], A_x, self.C_j[j]])
                      for j in range(J_time + 1)]
        self.P = BlockDiagLinOp([self.CAC_j[j] for j in W_t.levels])

        # Schur complement (heateq.py:87-91)
        # (a DeviceLinearOperator: the same expression maps flat host vectors, as the
        # reference's LinearOperator does, and device vectors)
        self.S = DeviceLinearOperator(
            self.G.shape,
            matvec=lambda v: self.BT @ (self.K @ (self.B @ v)) + self.G @ v)
        self.WT_S_W = self.WT @ self.S @ self.W

        # right-hand side (heateq.py:93-106): g = sum of the separable pairs of
        # data['g'] (none for the homogeneous model problems) and of its callables
        # g(t, x, y[, z]), whose loads the device builds (the engine of heateq_mpi.py:
        # one slab of all time elements, downloaded)
        self.g_vec = np.zeros(self.K.shape[0])
        self.load_plan = slab = None
        for term in data['g']:
            if callable(term):
                if self.load_plan is None:
                    import torch
                    from source import _lib
                    self.load_plan = DeviceLoadPlan(mesh_space, row_order=getattr(M_x, 'stk_row_order', None))
                    slab = torch.zeros((self.M, self.N_Y), dtype=torch.float64, device=_lib.compute_device())
                fill_test_space_slab(self.load_plan, mesh_time, term, 0, self.N_Y // 2, slab, accumulate=True)
                continue
            g_t, g_x = term
            self.g_vec += np.kron(time_load_test_space(mesh_time, g_t),
                                  space_load(mesh_space, g_x))
        if slab is not None:
            self.g_vec += slab.t().contiguous().cpu().numpy().reshape(-1)
        self.u0_x = space_load(mesh_space, data['u0'])
        self.f = self.BT @ (self.K @ self.g_vec) + np.kron(u0_t, self.u0_x)

    def solve(self, callback=None, on_host=False, rhs=None, x0=None):
        """PCG on the wavelet-transformed system; returns (u, iterations).  The
        right-hand side goes to the device once and the solution comes back once: in
        between, every vector of the iteration is device-resident (the callback sees
        device vectors; source.linop.host_vector copies one out).  on_host=True runs
        the reference's wiring literally -- flat NumPy vectors, one round trip over
        PCIe per operator apply.  `rhs`: another right-hand side on the trial space in
        place of f -- a flat NumPy vector or a device vector (what
        ``sample_along_adjoint`` returned: S^-1 E^T r is the gradient of a point-data
        misfit).  `x0`: a start -- a flat NumPy vector or a device vector of the trial space
        (``prolong_from`` of a coarser level's solution, the solution of a nearby right-hand
        side) -- the correction form, S e = f - S x0 solved from zero, returns
        (x0 + e, iterations); the callback sees the correction's PCG.  One more apply of S;
        without x0 nothing changes."""
        from source.linop import _is_device_vector
        f = self.f if rhs is None else rhs
        if _is_device_vector(f):
            assert f.N == self.N and f.M == self.M, 'rhs= takes a vector of the trial space'
        else:
            assert np.size(f) == self.N * self.M, 'rhs= takes a vector of the trial space'
        if x0 is not None:
            return self._solve_from(x0, f, callback, on_host)
        if on_host:
            f = host_vector(f) if _is_device_vector(f) else f
            w, iters = PCG(self.WT_S_W, self.P, self.WT @ f, callback=callback)
            return self.W @ w, iters
        f = f if _is_device_vector(f) else device_vector(f, self.N)
        w, iters = PCG(self.WT_S_W, self.P, self.WT @ f, callback=callback)
        return host_vector(self.W @ w), iters

    def _solve_from(self, x0, f, callback, on_host):
        """solve() with a start: PCG on S e = f - S x0 from zero, (x0 + e, iterations)."""
        from source.linop import _is_device_vector
        if _is_device_vector(x0):
            assert x0.N == self.N and x0.M == self.M, 'x0= takes a vector of the trial space'
        else:
            assert np.size(x0) == self.N * self.M, 'x0= takes a vector of the trial space'
        if on_host:
            x0 = host_vector(x0) if _is_device_vector(x0) else np.asarray(x0, dtype=np.float64).reshape(-1)
            f = host_vector(f) if _is_device_vector(f) else f
            w, iters = PCG(self.WT_S_W, self.P, self.WT @ (f - self.S @ x0), callback=callback)
            return x0 + self.W @ w, iters
        x0 = x0 if _is_device_vector(x0) else device_vector(x0, self.N)
        f = f if _is_device_vector(f) else device_vector(f, self.N)
        w, iters = PCG(self.WT_S_W, self.P, self.WT @ (f - self.S @ x0), callback=callback)
        return host_vector(x0 + self.W @ w), iters

    def errors(self, u):
        """(algebraic error of u in the X-norm, error in Y') as the reference's
        driver reports them (heateq.py:147-153)."""
        u = device_vector(u, self.N)
        residual = device_vector(self.f, self.N) - self.S @ u
        defect = device_vector(self.g_vec, self.N_Y) - self.B @ u
        return residual.dot(self.P @ residual), defect.dot(self.K @ defect)

    def _trial_vector(self, u, who):
        """`u` -- the flat NumPy vector of the serial operators or a device vector -- as a device
        vector (the hook of source/postprocess.py)."""
        from source.linop import _is_device_vector
        if not _is_device_vector(u):
            u = device_vector(u, self.N)
        assert u.N == self.N and u.M == self.M, '%s takes vectors of the trial space' % who
        return u

    def _adjoint_target(self, out):
        """One rank, so nothing of ``sample_along_adjoint`` is collective; a NumPy `out` is
        copied to the device."""
        from source.linop import _is_device_vector, self_distribution
        if out is not None and not _is_device_vector(out):
            if np.size(out) != self.N * self.M:
                raise ValueError('out is no vector of the trial space')
            out = device_vector(out, self.N)
        return self_distribution(self.N, self.M), out


_OPTIONS = (
    ('problem', str, 'square', 'problem type (square, lshape, cube, square_forced, cube_forced,'
     ' square_nonseparable, cube_nonseparable, square_moving_source)'),
    ('J_time', int, 5, 'number of time refines'),
    ('J_space', int, 6, 'number of space refines'),
    ('precond', str, 'multigrid', 'spatial preconditioner: multigrid or direct.'),
    ('alpha', float, 0.3, 'Alpha value used in the preconditioner for X.'),
) + driver.POST_OPTIONS  # taken off the command line before the constructor sees it


def main(argv=None):
    parser = argparse.ArgumentParser(description='Solve the heat equation, serial wiring.')
    for flag, kind, default, text in _OPTIONS:
        parser.add_argument('--' + flag, type=kind, default=default, help=text)
    args, asked = driver.take_post_options(parser.parse_args(argv))
    print('Arguments: %s' % args)
    levels = [] if asked['nested'] is None else driver.nested_levels(args.J_time, args.J_space, asked['nested'].nested)
    print('\n\nCreating HeatEquation with %d time refines and %d space refines.'
          % (args.J_time, args.J_space))
    heat = HeatEquation(**vars(args))
    if asked['track'] is not None:
        driver.require_path(heat, asked['track'])
    print('Size of time mesh: %d dofs. Size of space mesh: %d dofs' % (heat.N, heat.M))
    print('Solving: ', end='')
    progress = lambda w, residual, k: print('.', end='', flush=True)  # noqa: E731
    if levels:
        u, iters, _ = driver.solve_nested(
            heat, lambda J_time, J_space: HeatEquation(**dict(vars(args), J_time=J_time, J_space=J_space)), levels,
            rhs=heat.f if asked['nested'].nested_rhs == 'restricted' else None, callback=progress)
    else:
        u, iters = heat.solve(callback=progress)
    print('Done in %d  PCG steps. X-norm algebraic error: %s. Error in Yprime: %s\n'
          % ((iters,) + heat.errors(u)))
    driver.run_post(heat, u, asked)  # this driver keeps no record: the line of the error norms is the report
    return heat, u, iters


if __name__ == '__main__':
    main()
