"""What the device engines on a P1 mesh share on the Python side (csrc/p1_mesh.h is the C
side): the mesh as libstk takes it, and the lifetime of a plan.  SamplePlan (sampling.py),
ErrorPlan (error_norms.py), CurvesPlan (time_curves.py), SolidPlan (solidification.py) and
DeviceLoadPlan (assembly.py) each hold one MeshPlanHandle."""
import ctypes

import numpy as np


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
        import torch

        from . import _lib
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
