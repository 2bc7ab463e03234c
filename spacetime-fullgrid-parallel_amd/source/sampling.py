"""Sampling the discrete solution: u_h(t_k, x_p) at arbitrary points and times, on the
device (csrc/sample.hip, include/stk.h "sampling the trial space").

A solution is a slab of nodal values in free-dof order; this module is what reads it:
rasters of time slices, probes at points, cuts along lines.

* ``SamplePlan(mesh)``: the mesh, the vertex -> slab-row map and a bucket grid for point
  location on the device, built once.  ``locate(points)`` finds the cell and the
  barycentric coordinates of every point; ``evaluate(vec, times, located)`` returns this
  rank's contribution to the ``(n_k, n_p)`` block of values.
* ``time_weights``: which two time nodes a time lies between, with which weights, and
  which of them a rank owns (pure NumPy).
* ``raster``: a regular grid of points over the bounding box (pure NumPy).
* ``bucket_grid``: the point-location grid as host arrays (no GPU needed).

* ``evaluate_pairs(vec, times, located, fields)``: paired lists (t_p, x_p) -- a
  trajectory, a set of tracers -- without the block they are the diagonal of, and with
  the derivatives: u_h, d/dt u_h and grad u_h per point (stk_sample_pairs).  The block
  forms of the derivatives are ``evaluate(..., field='dt' | 'grad')``.
* ``adjoint_pairs(distr, weights, times, located, field)``: the adjoint E^T of the pairs --
  numbers given at (t_p, x_p) as a functional on the trial space, the right-hand side of
  a solve that uses point data (stk_sample_pairs_adjoint): store, stable sort, sum; no
  float atomics, the same doubles whatever the launch and the number of ranks.

Scope: vectors of the TRIAL space (continuous piecewise linear in time).  Test-space
vectors (discontinuous in time) and second derivatives are not served.
"""
import ctypes

import numpy as np

from .p1_plan import MeshPlanHandle, mesh_arrays


def bucket_grid(mesh):
    """The point-location grid of a mesh, built on the host threads of libstk
    (stk_sample_grid_build): dict with bins (d,), lo (d,) = the shifted corner,
    inv_width (d,), widen, bin_ptr, bin_cells (CSR: the cells of bin
    ``(iz bins[1] + iy) bins[0] + ix`` in ascending order)."""
    from . import _lib
    pts, cells, d = mesh_arrays(mesh)
    lib, grid = _lib.lib(), ctypes.c_void_p()
    _lib.check(lib.stk_sample_grid_build(d, len(pts), len(cells), pts.ctypes.data, cells.ctypes.data,
                                         ctypes.byref(grid)))
    try:
        bins, lo, inv_w = np.zeros(3, np.int32), np.zeros(3), np.zeros(3)
        widen, entries = ctypes.c_double(), ctypes.c_int64()
        _lib.check(lib.stk_sample_grid_sizes(grid, bins.ctypes.data, lo.ctypes.data, inv_w.ctypes.data,
                                             ctypes.addressof(widen), ctypes.addressof(entries)))
        bin_ptr = np.empty(int(np.prod(bins[:d], dtype=np.int64)) + 1, np.int32)
        bin_cells = np.empty(entries.value, np.int32)
        _lib.check(lib.stk_sample_grid_copy(grid, bin_ptr.ctypes.data, bin_cells.ctypes.data))
    finally:
        lib.stk_sample_grid_free(grid)
    return {'bins': bins[:d].copy(), 'lo': lo[:d].copy(), 'inv_width': inv_w[:d].copy(), 'widen': widen.value,
            'bin_ptr': bin_ptr, 'bin_cells': bin_cells}


def time_weights(mesh_time, times, t_begin, t_end):
    """(columns (n_k, 2) int32, weights (n_k, 2)) of the times on a rank that owns the
    time nodes [t_begin, t_end): with h the element length and N the number of nodes,
    e = min(floor(t / h), N - 2), s = t / h - e, weights (1 - s, s); column a is
    e + a - t_begin where the rank owns node e + a, else -1.  Times outside [0, T]
    raise ValueError."""
    times = np.atleast_1d(np.asarray(times, dtype=np.float64))
    if times.ndim != 1:
        raise ValueError('times must be one-dimensional')
    N, h, T = mesh_time.nv, mesh_time.h, mesh_time.T
    if N < 2:
        raise ValueError('a time mesh of one node has no element')
    if not np.all((times >= 0.0) & (times <= T)):  # also refuses NaN
        raise ValueError('times outside [0, %g]' % T)
    x = times / h
    e = np.minimum(np.floor(x), N - 2).astype(np.int64)
    s = x - e
    nodes = e[:, None] + np.arange(2)[None, :]
    owned = (nodes >= t_begin) & (nodes < t_end)
    columns = np.where(owned, nodes - t_begin, -1).astype(np.int32)
    weights = np.stack([1.0 - s, s], axis=1)
    return np.ascontiguousarray(columns), np.ascontiguousarray(weights)


def raster(mesh, n):
    """The n^d points of a regular grid over the bounding box of the mesh (both ends
    included), shape (n^d, d); the first coordinate runs fastest."""
    pts = np.asarray(mesh.points, dtype=np.float64)
    d = pts.shape[1]
    axes = [np.linspace(pts[:, k].min(), pts[:, k].max(), int(n)) for k in range(d)]
    grids = np.meshgrid(*axes[::-1], indexing='ij')[::-1]
    return np.stack([g.reshape(-1) for g in grids], axis=1)


class Located:
    """Points located in a mesh: device tensors ``cell`` (n_p,) int32 (-1 = outside),
    ``lam`` (n_p, d + 1) and ``inside`` (n_p,) bool."""
    def __init__(self, cell, lam):
        self.cell, self.lam = cell, lam
        self.inside = cell >= 0
        self.n_p = cell.shape[0]


class SamplePlan:
    """The sampling engine of libstk on one mesh.  ``mesh_time``: the time mesh of the
    vectors (default: the uniform mesh of [0, 1] with the vector's number of nodes, which
    is what source/problem.py builds).  Not for two streams at once: the plan owns the
    request tables of a call in flight."""
    def __init__(self, mesh, mesh_time=None):
        from . import _lib
        self._lib = _lib
        self.mesh_time = mesh_time
        self._plan = MeshPlanHandle(mesh, lambda lib, m, out: lib.stk_sample_plan_create(*m, out),
                                    lambda lib, plan: lib.stk_sample_plan_destroy(plan))
        self.d, self.n_free = self._plan.d, self._plan.n_free

    def locate(self, points):
        """points: (n_p, d) NumPy array or device tensor (or what locate returned)."""
        import torch
        _lib = self._lib
        if isinstance(points, Located):
            return points
        if not torch.is_tensor(points):
            points = torch.from_numpy(np.array(points, dtype=np.float64, order='C'))  # a copy: torch wants it writable
        assert points.ndim == 2 and points.shape[1] == self.d, tuple(points.shape)
        x = points.to(device=_lib.compute_device(), dtype=torch.float64).t().contiguous()  # [d][n_p]
        n_p = x.shape[1]
        cell = torch.empty(n_p, dtype=torch.int32, device=x.device)
        lam = torch.empty((n_p, self.d + 1), dtype=torch.float64, device=x.device)
        if n_p:
            _lib.check(_lib.lib().stk_sample_locate(_lib.stream(), self._plan, n_p, _lib.ptr(x), _lib.ptr(cell),
                                                    _lib.ptr(lam)))
        return Located(cell, lam)

    def _time_mesh_of(self, vec):
        mesh_time = self.mesh_time
        if mesh_time is None:
            from .mesh import construct_interval
            mesh_time = construct_interval(N=vec.N - 1)
        assert mesh_time.nv == vec.N, (mesh_time.nv, vec.N)
        assert vec.M == self.n_free, (vec.M, self.n_free)
        return mesh_time

    def grad_coeffs(self, located):
        """(d, n_p, d + 1) device tensor: [j, p, a] = d_j lambda_a of the cell of point p
        (stk_sample_grad_coeffs), NaN for a point outside the mesh."""
        import torch
        _lib = self._lib
        out = torch.empty((self.d, located.n_p, self.d + 1), dtype=torch.float64, device=located.cell.device)
        if located.n_p:
            _lib.check(_lib.lib().stk_sample_grad_coeffs(_lib.stream(), self._plan, located.n_p, _lib.ptr(located.cell),
                                                         _lib.ptr(out)))
        return out

    def evaluate(self, vec, times, located, out=None, field='u'):
        """This rank's contribution to u_h(t_k, x_p) of the trial-space vector `vec`
        (KronVectorMPI), shape (n_k, n_p): the terms of the time nodes this rank owns,
        exactly 0.0 for the others, NaN at points outside the mesh.  The sum over the
        ranks is the value (HeatEquationMPI.sample all-reduces it).

        field='dt': the block of d/dt u_h, the same kernel with the weights (-1/h, 1/h)
        (the right-hand derivative at an interior node, the left-hand one at T);
        field='grad': the blocks of grad u_h, shape (d, n_k, n_p), the same kernel with
        the rows of ``grad_coeffs`` in place of the barycentric coordinates."""
        import torch
        _lib = self._lib
        if field not in FIELDS:
            raise ValueError('field must be one of %s, not %r' % (FIELDS, field))
        mesh_time = self._time_mesh_of(vec)
        columns, weights = time_weights(mesh_time, times, vec.t_begin, vec.t_end)
        n_k, n_p = len(columns), located.n_p
        if field != 'u':
            if field == 'dt':
                weights = np.ascontiguousarray(np.broadcast_to(np.array([-1.0, 1.0]) / mesh_time.h, columns.shape))
                lams = [located.lam]
            else:
                lams = list(self.grad_coeffs(located))
            shape = (len(lams), n_k, n_p)
            if out is None:
                out = torch.empty(shape, dtype=torch.float64, device=vec.buf.device)
            assert tuple(out.reshape(shape).shape) == shape and out.is_contiguous() and out.dtype == torch.float64
            if n_k and n_p:
                for j, lam in enumerate(lams):
                    _lib.check(_lib.lib().stk_sample_eval(
                        _lib.stream(), self._plan, n_p, _lib.ptr(located.cell), _lib.ptr(lam), vec.M, vec.n_loc, vec.ld,
                        _lib.ptr(vec.buf), n_k, columns.ctypes.data, weights.ctypes.data, n_p,
                        _lib.ptr(out.reshape(shape)[j])))
            return out.reshape(shape[1:]) if field == 'dt' else out
        if out is None:
            out = torch.empty((n_k, n_p), dtype=torch.float64, device=vec.buf.device)
        assert tuple(out.shape) == (n_k, n_p) and out.is_contiguous() and out.dtype == torch.float64
        if n_k and n_p:
            _lib.check(_lib.lib().stk_sample_eval(
                _lib.stream(), self._plan, n_p, _lib.ptr(located.cell), _lib.ptr(located.lam), vec.M, vec.n_loc, vec.ld,
                _lib.ptr(vec.buf), n_k, columns.ctypes.data, weights.ctypes.data, n_p, _lib.ptr(out)))
        return out

    def _pair_rows(self, vec, times, located, fields):
        """(mask, rows): the (n_rows, n_p) device tensor stk_sample_pairs fills, rows in
        the order u, dt, grad_0 .. grad_(d-1), the requested ones only."""
        import torch
        _lib = self._lib
        mask = field_mask(fields)
        mesh_time = self._time_mesh_of(vec)
        dev = vec.buf.device
        if not torch.is_tensor(times):
            times = torch.from_numpy(np.array(times, dtype=np.float64, order='C'))  # a copy: torch wants it writable
        times = times.to(device=dev, dtype=torch.float64).contiguous()
        n_p = located.n_p
        assert tuple(times.shape) == (n_p,), (tuple(times.shape), n_p)
        n_rows = (mask & 1) + (mask >> 1 & 1) + (mask >> 2 & 1) * self.d
        rows = torch.empty((n_rows, n_p), dtype=torch.float64, device=dev)
        if n_p:
            _lib.check(_lib.lib().stk_sample_pairs(
                _lib.stream(), self._plan, n_p, _lib.ptr(located.cell), _lib.ptr(located.lam), _lib.ptr(times),
                float(mesh_time.h), vec.N, vec.t_begin, vec.M, vec.n_loc, vec.ld, _lib.ptr(vec.buf), mask, n_p,
                _lib.ptr(rows)))
        return mask, rows

    def _split_rows(self, mask, rows):
        out, at = {}, 0
        if mask & 1:
            out['u'], at = rows[at], at + 1
        if mask & 2:
            out['dt'], at = rows[at], at + 1
        if mask & 4:
            out['grad'] = rows[at:at + self.d]
        return out

    def evaluate_pairs(self, vec, times, located, fields=('u',)):
        """This rank's contributions at the PAIRS (times[p], point p) -- one time per
        located point, `times` a NumPy array or device tensor of shape (n_p,) -- as a dict
        of device tensors: 'u' (n_p,), 'dt' (n_p,), 'grad' (d, n_p), those named in
        `fields`.  The terms of the time nodes this rank owns, exactly 0.0 for the others;
        NaN where the point is outside the mesh or the time is NaN or outside [0, T] (checked
        on the device: nothing here waits for it).  The sum over the ranks is the value."""
        return self._split_rows(*self._pair_rows(vec, times, located, fields))

    def adjoint_pairs(self, distr, weights, times, located, field='u', out=None, accumulate=False):
        """E^T of ``evaluate_pairs``: the numbers `weights` given at the PAIRS (times[p],
        point p) as a functional on the trial space, v -> sum_p weights[p] v_h(t_p, x_p)
        (field='u'), ... d/dt v_h (field='dt') or sum_p weights[:, p] . grad v_h (field='grad'),
        on the columns the distribution `distr` (a DofDistributionMPI) gives this rank
        (stk_sample_pairs_adjoint).  `weights`: (n_p,), for 'grad' (d, n_p); `times`: (n_p,);
        NumPy arrays or device tensors.  Returns (vec, used): the KronVectorMPI -- `out` if
        given, overwritten, or added to with accumulate=True -- and a device bool tensor
        (n_p,), False where the point is outside the mesh or the time is NaN or outside
        [0, T]: such a pair contributes nothing (decided on the device: nothing here waits).
        No float atomics: every entry is a sum of one fixed shape, the same whatever the launch
        and whatever the number of ranks -- every rank passes ALL pairs and gets its own
        columns, with no communication.  Wrong shapes or field names raise ValueError before
        anything touches the GPU.  The workspace is kept by the plan and grows with n_p."""
        weights, times = _check_adjoint_arguments(self.d, located.n_p, weights, times, field)
        if distr.M != self.n_free or distr.N < 2:
            raise ValueError('a distribution of %d x %d dofs on a plan of %d free dofs' % (distr.N, distr.M, self.n_free))
        if out is None and accumulate:
            raise ValueError('accumulate=True needs the vector to add to: out=')
        if out is not None and (out.dofs_distr.N, out.M, out.t_begin, out.t_end) != (distr.N, distr.M, distr.t_begin,
                                                                                    distr.t_end):
            raise ValueError('out is no vector of this distribution')
        import torch

        from .mpi_vector import KronVectorMPI
        _lib = self._lib
        mesh_time = self._time_mesh_of(distr)
        if out is None:
            out = KronVectorMPI(distr)
        else:
            out._invalidate()
        dev, n_p = out.buf.device, located.n_p
        as_dev = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.array(a, dtype=np.float64, order='C'))).to(
            device=dev, dtype=torch.float64).contiguous()
        weights, times = as_dev(weights), as_dev(times)
        used = torch.empty(n_p, dtype=torch.uint8, device=dev)
        size = ctypes.c_int64()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().stk_sample_pairs_adjoint_work_size(n_p, self.d, ctypes.addressof(size)))
            work = getattr(self, '_adjoint_work', None)
            if work is None or work.numel() < size.value or work.device != dev:
                self._adjoint_work = work = None  # the old one goes first
                self._adjoint_work = work = torch.empty(max(size.value, 256), dtype=torch.uint8, device=dev)
            assert _lib.ptr(work) % 256 == 0
            _lib.check(_lib.lib().stk_sample_pairs_adjoint(
                _lib.stream(), self._plan, n_p, _lib.ptr(located.cell), _lib.ptr(located.lam), _lib.ptr(times),
                float(mesh_time.h), distr.N, distr.t_begin, distr.M, out.n_loc, out.ld, _lib.ptr(out.buf), _lib.ptr(weights),
                n_p, 1 << FIELDS.index(field), int(bool(accumulate)), _lib.ptr(used), _lib.ptr(work), work.numel()))
        return out, used.bool()


FIELDS = ('u', 'dt', 'grad')


def field_mask(fields):
    """The bit mask of stk_sample_pairs (1 = u, 2 = dt, 4 = grad) of a field name or a
    sequence of names."""
    names = (fields,) if isinstance(fields, str) else tuple(fields)
    if not names or any(f not in FIELDS for f in names):
        raise ValueError('fields must name some of %s, not %r' % (FIELDS, fields))
    return sum(1 << FIELDS.index(f) for f in set(names))


def _check_adjoint_arguments(d, n_p, weights, times, field):
    """(weights, times) of ``SamplePlan.adjoint_pairs`` -- device tensors as they came,
    anything else as float64 NumPy arrays -- or ValueError: `field` one name of FIELDS,
    weights (n_p,), for 'grad' (d, n_p), times (n_p,).  Touches no GPU."""
    if not isinstance(field, str) or field not in FIELDS:
        raise ValueError('field must be one of %s, not %r' % (FIELDS, field))
    host = lambda a: a if hasattr(a, 'is_cuda') else np.asarray(a, dtype=np.float64)
    weights, times = host(weights), host(times)
    want = (d, n_p) if field == 'grad' else (n_p,)
    if tuple(weights.shape) != want:
        raise ValueError("weights of shape %s; field '%s' at %d points takes %s" % (tuple(weights.shape), field, n_p, want))
    if tuple(times.shape) != (n_p,):
        raise ValueError('times of shape %s for %d points' % (tuple(times.shape), n_p))
    return weights, times


def sample_collective(plan, vec, times, points, field='u'):
    """The full (n_k, n_p) block on every rank: the local contributions all-reduced with
    the communicator of the vector, the pattern of KronVectorMPI.dot -- every term has
    exactly one non-zero contributor, so the block is the one-rank block bit for bit
    whatever the rank count.  field='dt' / 'grad': the blocks of the derivatives
    ((n_k, n_p) / (d, n_k, n_p)), in the same way."""
    block = plan.evaluate(vec, times, plan.locate(points), field=field)
    vec.dofs_distr.comm.allreduce_tensor_(block)
    return block


def sample_pairs_collective(plan, vec, times, points, fields=('u',)):
    """The pairs (times[p], points[p]) on every rank: dict with 'u' (n_p,), 'dt' (n_p,),
    'grad' (d, n_p) -- those named in `fields` -- and 'inside' (n_p,) bool.  The local rows
    are all-reduced in one call; every term has exactly one non-zero contributor (the
    owner of its time node), so every entry is the one-rank double whatever the rank
    count."""
    located = plan.locate(points)
    mask, rows = plan._pair_rows(vec, times, located, fields)
    if rows.numel():
        vec.dofs_distr.comm.allreduce_tensor_(rows)
    out = plan._split_rows(mask, rows)
    out['inside'] = located.inside
    return out
