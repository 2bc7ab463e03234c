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
from source.problem import problem_helper  # noqa: E402
from source.wavelets import WaveletTransformOp  # noqa: E402


class HeatEquation:
    """Implementation of Andreev's method for tensor-product trial spaces
    (reference heateq.py:18-107)."""
    def __init__(self, J_space=2, J_time=None, problem='square',
                 precond='multigrid', alpha=0.3, smoothsteps=3, vcycles=2):
        if J_time is None:
            J_time = J_space
        mesh_space, bc, mesh_time, data, fn = problem_helper(problem,
                                                             J_space=J_space,
                                                             J_time=J_time)
        # what sample() builds its plan from, on first use
        self._sample_meshes, self.sample_plan = (mesh_space, mesh_time), None
        # ... and error_norms() its plan, with the problem's exact solution if it has one
        self.error_plan, self._exact = None, (data.get('exact'), data.get('exact_grad'))
        self.curves_plan = None  # built by the first time_curves()
        self.solid_plan = None  # built by the first solidification_maps()
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

    def solve(self, callback=None, on_host=False, rhs=None):
        """PCG on the wavelet-transformed system; returns (u, iterations).  The
        right-hand side goes to the device once and the solution comes back once: in
        between, every vector of the iteration is device-resident (the callback sees
        device vectors; source.linop.host_vector copies one out).  on_host=True runs
        the reference's wiring literally -- flat NumPy vectors, one round trip over
        PCIe per operator apply.  `rhs`: another right-hand side on the trial space in
        place of f -- a flat NumPy vector or a device vector (what
        ``sample_along_adjoint`` returned: S^-1 E^T r is the gradient of a point-data
        misfit)."""
        from source.linop import _is_device_vector
        f = self.f if rhs is None else rhs
        if _is_device_vector(f):
            assert f.N == self.N and f.M == self.M, 'rhs= takes a vector of the trial space'
        else:
            assert np.size(f) == self.N * self.M, 'rhs= takes a vector of the trial space'
        if on_host:
            f = host_vector(f) if _is_device_vector(f) else f
            w, iters = PCG(self.WT_S_W, self.P, self.WT @ f, callback=callback)
            return self.W @ w, iters
        f = f if _is_device_vector(f) else device_vector(f, self.N)
        w, iters = PCG(self.WT_S_W, self.P, self.WT @ f, callback=callback)
        return host_vector(self.W @ w), iters

    def errors(self, u):
        """(algebraic error of u in the X-norm, error in Y') as the reference's
        driver reports them (heateq.py:147-153)."""
        u = device_vector(u, self.N)
        residual = device_vector(self.f, self.N) - self.S @ u
        defect = device_vector(self.g_vec, self.N_Y) - self.B @ u
        return residual.dot(self.P @ residual), defect.dot(self.K @ defect)

    def sample(self, u, times, points, field='u'):
        """u_h(t_k, x_p) of a trial-space vector `u` -- the flat NumPy vector of the
        serial operators or a device vector (source.linop.device_vector) -- at `times`
        (n_k,) in [0, T] and `points` (n_p, d): an (n_k, n_p) device tensor, NaN at points
        outside the mesh.  The plan of heateq_mpi.py's sample() (source/sampling.py,
        csrc/sample.hip), built by the first call.  Test-space vectors (discontinuous in
        time) are out of scope; paired lists (t_p, x_p) are served by ``sample_along``.
        field='dt' / 'grad': the blocks of the time derivative, (n_k, n_p), and of the
        gradient, (d, n_k, n_p)."""
        from source.sampling import sample_collective
        u = self._trial_vector(u)
        return sample_collective(self.sample_plan, u, times, points, field=field)

    def _trial_vector(self, u, plan=True):
        """`u` as a device vector, and (with `plan`) the sampling plan built on first use."""
        from source.linop import _is_device_vector
        from source.sampling import SamplePlan
        if not _is_device_vector(u):
            u = device_vector(u, self.N)
        assert u.N == self.N and u.M == self.M, 'sampling takes vectors of the trial space'
        if plan and self.sample_plan is None:
            mesh_space, mesh_time = self._sample_meshes
            self.sample_plan = SamplePlan(mesh_space, mesh_time)
        return u

    def history_maps(self, u, threshold=None, points=None, fields=None):
        """The thermal history of a trial-space vector `u` -- flat NumPy vector or device
        vector -- over [0, T]: the dict of heateq_mpi.py's history_maps() (source/history.py,
        csrc/history.hip): 'peak', 't_peak', 'dose', 'max_rate', 'min_rate' and, with a
        `threshold`, 'time_above', 't_first', 't_last'; (M,) device tensors in free-dof order,
        or (n_p,) tensors plus 'inside' at `points` (n_p, d).  Test-space vectors are refused.
        Out of scope: time windows other than [0, T], several thresholds in one call, per-row
        thresholds."""
        from source.history import check_arguments, history_maps
        check_arguments(threshold, points, self._sample_meshes[0].points.shape[1], fields)  # before the upload
        return history_maps(self, self._trial_vector(u, plan=points is not None), threshold, points, fields)

    def time_curves(self, u, threshold=None):
        """What a trial-space vector `u` -- flat NumPy vector or device vector -- does over
        space at every time node: the dict of heateq_mpi.py's time_curves()
        (source/time_curves.py, csrc/curves.hip): 'heat', 'l2_sq', 'h1_sq', 'outflow', 'peak',
        'peak_row', 'peak_point' and, with a `threshold`, 'measure_above', 'moment_above',
        'centroid_above', 'box_lo', 'box_hi'; device tensors with one entry per node.
        Test-space vectors are refused.  Out of scope: time windows other than the nodes of
        [0, T], several thresholds in one call, sub-regions of the domain, values between the
        nodes."""
        from source.time_curves import check_arguments, time_curves
        check_arguments(threshold)  # before the upload
        return time_curves(self, self._trial_vector(u, plan=False), threshold)

    def solidification_maps(self, u, threshold, points=None, fields=None):
        """What a trial-space vector `u` -- flat NumPy vector or device vector -- does at the
        freezing front, per cell: the dict of heateq_mpi.py's solidification_maps()
        (source/solidification.py, csrc/solid.hip): 't_solid', 'cooling_rate', 'grad_solid',
        'G', 'front_speed', 'n_solid', 'max_grad', 't_max_grad'; device tensors per cell in the
        mesh's cell order, or per point plus 'inside' at `points` (n_p, d).  The threshold is
        required.  Test-space vectors are refused.  Out of scope: per-cell thresholds, several
        thresholds in one call, melting crossings, time windows other than [0, T]."""
        from source.solidification import check_arguments, solidification_maps
        check_arguments(threshold, points, self._sample_meshes[0].points.shape[1], fields)  # before the upload
        return solidification_maps(self, self._trial_vector(u, plan=points is not None), threshold, points, fields)

    def sample_along(self, u, times, points, fields=('u',)):
        """u_h, its time derivative and its gradient along a trajectory: at the PAIRS
        (times[p], points[p]) of a trial-space vector `u` -- flat NumPy vector or device
        vector.  The dict of heateq_mpi.py's sample_along(): 'u' (n_p,), 'dt' (n_p,),
        'grad' (d, n_p) -- those named in `fields` -- and 'inside' (n_p,), device tensors, NaN
        outside the mesh and outside [0, T]."""
        from source.sampling import sample_pairs_collective
        u = self._trial_vector(u)
        return sample_pairs_collective(self.sample_plan, u, times, points, fields)

    def sample_along_adjoint(self, weights, times, points, field='u', out=None, accumulate=False):
        """The adjoint E^T of ``sample_along``: numbers given at the pairs (times[p],
        points[p]) as a functional on the trial space (`weights` (n_p,), for field='grad'
        (d, n_p)).  Returns (vec, used) as heateq_mpi.py's sample_along_adjoint(): a DEVICE
        vector (source.linop.host_vector copies it out; ``solve(rhs=vec)`` takes it as it is)
        and a device bool tensor (n_p,), False where a pair is outside the mesh or [0, T] and
        contributes nothing.  `out`: a flat NumPy vector or a device vector to overwrite or,
        with accumulate=True, to add to (a NumPy vector is copied to the device, not changed).
        One rank, so nothing here is collective."""
        from source.linop import _is_device_vector, self_distribution
        from source.sampling import FIELDS, SamplePlan
        if field not in FIELDS:  # before a plan is built for it
            raise ValueError('field must be one of %s, not %r' % (FIELDS, field))
        if out is not None and not _is_device_vector(out):
            if np.size(out) != self.N * self.M:
                raise ValueError('out is no vector of the trial space')
            out = device_vector(out, self.N)
        if self.sample_plan is None:
            mesh_space, mesh_time = self._sample_meshes
            self.sample_plan = SamplePlan(mesh_space, mesh_time)
        plan = self.sample_plan
        return plan.adjoint_pairs(self_distribution(self.N, self.M), weights, times, plan.locate(points), field=field,
                                  out=out, accumulate=accumulate)

    def error_norms(self, u, exact=None, exact_grad=None, times=None):
        """|| u - u_h || of a trial-space vector `u` -- flat NumPy vector or device vector
        -- against `exact` (default: the problem's data['exact'] and data['exact_grad']) in
        L2(I; L2), L2(I; H^1_0) and in L2(Omega) at `times` (default [T]): the dict of
        heateq_mpi.py's error_norms() (source/error_norms.py, csrc/err_norms.hip); the plan
        is built by the first call."""
        from source.error_norms import ErrorPlan, error_norms_collective
        from source.linop import _is_device_vector
        if not _is_device_vector(u):
            u = device_vector(u, self.N)
        assert u.N == self.N and u.M == self.M, 'error_norms() takes vectors of the trial space'
        if exact is None:
            exact, default_grad = self._exact
            exact_grad = default_grad if exact_grad is None else exact_grad
        assert exact is not None, 'this problem has no exact solution: pass exact='
        if self.error_plan is None:
            mesh_space, mesh_time = self._sample_meshes
            self.error_plan = ErrorPlan(mesh_space, mesh_time)
        return error_norms_collective(self.error_plan, u, exact, exact_grad, times)


_OPTIONS = (
    ('problem', str, 'square', 'problem type (square, lshape, cube, square_forced, cube_forced,'
     ' square_nonseparable, cube_nonseparable, square_moving_source)'),
    ('J_time', int, 5, 'number of time refines'),
    ('J_space', int, 6, 'number of space refines'),
    ('precond', str, 'multigrid', 'spatial preconditioner: multigrid or direct.'),
    ('alpha', float, 0.3, 'Alpha value used in the preconditioner for X.'),
) + driver.SAMPLE_OPTIONS + driver.TRACK_OPTIONS + driver.HISTORY_OPTIONS + driver.CURVES_OPTIONS + driver.SOLID_OPTIONS  # taken off the command line before the constructor sees it


def main(argv=None):
    parser = argparse.ArgumentParser(description='Solve the heat equation, serial wiring.')
    for flag, kind, default, text in _OPTIONS:
        parser.add_argument('--' + flag, type=kind, default=default, help=text)
    args, tracking = driver.take_track_options(parser.parse_args(argv))
    args, sampling = driver.take_sample_options(args)
    args, history_maps = driver.take_history_options(args)
    args, curves = driver.take_curves_options(args)
    args, solid = driver.take_solid_options(args)
    print('Arguments: %s' % args)
    print('\n\nCreating HeatEquation with %d time refines and %d space refines.'
          % (args.J_time, args.J_space))
    heat = HeatEquation(**vars(args))
    if tracking is not None:
        driver.require_path(heat, tracking)
    print('Size of time mesh: %d dofs. Size of space mesh: %d dofs' % (heat.N, heat.M))
    print('Solving: ', end='')
    u, iters = heat.solve(callback=lambda w, residual, k: print('.', end='', flush=True))
    print('Done in %d  PCG steps. X-norm algebraic error: %s. Error in Yprime: %s\n'
          % ((iters,) + heat.errors(u)))
    if sampling is not None and sampling.sample_out:
        driver.write_samples(heat, u, sampling)
    if tracking is not None:
        driver.write_track(heat, u, tracking)
    if history_maps is not None:
        driver.write_history(heat, u, history_maps)
    if curves is not None:
        driver.write_curves(heat, u, curves)
    if solid is not None:
        driver.write_solid(heat, u, solid)
    if sampling is not None and sampling.error_norms:
        driver.report_error_norms(heat, u)  # this driver keeps no record: the line is the report
    return heat, u, iters


if __name__ == '__main__':
    main()
