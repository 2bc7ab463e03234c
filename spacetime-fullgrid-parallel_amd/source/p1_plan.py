"""What the device engines on a P1 mesh share on the Python side (csrc/p1_mesh.h is the C
side).

* ``mesh_arrays``, ``MeshPlanHandle``: the mesh as libstk takes it, and the lifetime of a
  plan.  SamplePlan (sampling.py), ErrorPlan (error_norms.py), CurvesPlan (time_curves.py),
  SolidPlan (solidification.py) and DeviceLoadPlan (assembly.py) each hold one handle.
* ``threshold_value``, ``check_points_shape``, ``field_names``: the pieces the
  ``check_arguments`` of history.py, time_curves.py, solidification.py and isotherms.py are built from;
  they raise ValueError and touch no GPU.
* ``time_step``: the time mesh of a vector, the uniform one of [0, 1] by default.
* ``scan_down_the_ranks``: a scan along time whose state travels from rank to rank (the
  history maps, the solidification maps).
* ``device_address``: a device tensor or a device address, as the C ABI takes it.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib


def mesh_arrays(mesh):
    """(points (nv, d) float64, cells (nc, d + 1) int64, d), C-contiguous."""
    pts = np.ascontiguousarray(mesh.points, dtype=np.float64)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int64)
    return pts, cells, cells.shape[1] - 1


class MeshPlanHandle:
    """One plan of libstk on a mesh: made by ``create(lib, mesh_args, out)`` -- mesh_args =
    (d, nv, nc, points, cells, n_free, free_vertices) as every stk_*_plan_create starts, out
    = where the plan goes -- on the device of this process, destroyed by ``destroy(lib,
    plan)`` with this object.  Goes where the C ABI takes the plan; ``d``, ``nc``,
    ``n_free`` are the mesh's."""
    def __init__(self, mesh, create, destroy):
        from .assembly import free_dofs
        pts, cells, self.d = mesh_arrays(mesh)
        self.nc = len(cells)
        fd = np.ascontiguousarray(free_dofs(mesh), dtype=np.int64)
        self.n_free = len(fd)
        self._as_parameter_ = ctypes.c_void_p()
        self._lib, self._destroy = _lib.lib(), destroy  # kept here: __del__ may run at interpreter exit
        mesh_args = (self.d, len(pts), self.nc, pts.ctypes.data, cells.ctypes.data, self.n_free, fd.ctypes.data)
        with torch.cuda.device(_lib.compute_device()):
            _lib.check(create(self._lib, mesh_args, ctypes.byref(self._as_parameter_)))

    def __del__(self):
        if getattr(self, '_as_parameter_', None):
            self._destroy(self._lib, self._as_parameter_)
            self._as_parameter_ = None


# ---- the pieces of the check_arguments of the reductions: ValueError, no GPU ------------------
def threshold_value(threshold, needed_by=None):
    """theta of a `threshold`: a number, not NaN.  None is +inf -- or, where `needed_by` names
    a call that requires a threshold, refused."""
    if threshold is None:
        if needed_by:
            raise ValueError('%s needs a threshold' % needed_by)
        return math.inf
    try:
        theta = float(threshold)
    except (TypeError, ValueError):
        raise ValueError('threshold must be %sa number, not %r' % ('' if needed_by else 'None or ', threshold))
    if math.isnan(theta):
        raise ValueError('threshold is NaN')
    return theta


def check_points_shape(points, d):
    """`points`: None, located points (they carry no shape) or (n_p, d)."""
    if points is None or d is None or hasattr(points, 'n_p'):
        return
    shape = tuple(points.shape) if hasattr(points, 'shape') else np.asarray(points).shape
    if len(shape) != 2 or shape[1] != d:
        raise ValueError('points of shape %s; the mesh takes (n_p, %d)' % (shape, d))


def field_names(fields, known, allowed=None):
    """`fields` -- None (all of `allowed`), a name or names -- as a tuple of names of `known`
    that are in `allowed` (default: `known`; the rest needs a threshold)."""
    allowed = known if allowed is None else allowed
    if fields is None:
        return allowed
    names = (fields,) if isinstance(fields, str) else tuple(fields)
    for f in names:
        if f not in known:
            raise ValueError('fields must name some of %s, not %r' % (known, f))
        if f not in allowed:
            raise ValueError('%r needs a threshold' % f)
    return names


# ---- what the calls of the reductions share ----------------------------------------------------
def time_step(vec, mesh_time):
    """`mesh_time`, or the uniform mesh of [0, 1] with the nodes of `vec` in its place."""
    if mesh_time is None:
        from .mesh import construct_interval
        mesh_time = construct_interval(N=vec.N - 1)
    assert mesh_time.nv == vec.N, (mesh_time.nv, vec.N)
    return mesh_time


def scan_down_the_ranks(vec, state, scan):
    """A scan along time of the trial-space vector `vec` (KronVectorMPI) into `state`, a
    freshly allocated device tensor, on every rank.  COLLECTIVE and serial in the ranks by
    design: rank r > 0 receives the state from rank r - 1, ``scan(state)`` scans this rank's
    columns into it, rank r < size - 1 sends it on -- size - 1 transfers of the state.  The
    last rank's state is the result; the others zero theirs and one all-reduce gives it to all
    (one non-zero contributor per entry, the pattern of KronVectorMPI.dot; NaN and +-inf
    survive + 0.0).  Every row's operations come in one order, so the doubles are the one-rank
    doubles."""
    dd = vec.dofs_distr
    comm, rank, size = dd.comm, dd.rank, dd.size
    if rank > 0:
        comm.wait_all(comm.exchange([], [(state, rank - 1)]))
    scan(state)
    if rank < size - 1:
        comm.wait_all(comm.exchange([(state, rank + 1)], []))
        state.zero_()
    if size > 1:
        comm.allreduce_tensor_(state)
    return state


def device_address(x):
    """`x` as the C ABI takes it: the checked pointer of a device tensor, or the device address
    it already is."""
    return _lib.ptr(x) if torch.is_tensor(x) else x
