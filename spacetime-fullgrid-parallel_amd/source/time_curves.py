"""Time curves: what a trial-space solution does over SPACE at every time node -- the heat
content, the squares of the L2 and H1 norms, the outflow through the boundary, the hottest
free dof and, with a threshold, the measure, first moment, centroid and bounding box of the
zone {u_h > threshold} -- from one pass over the cells on the device (csrc/curves.hip,
include/stk.h "time curves").  The complement of the history maps, which reduce along time.

The sums over the mesh have one shape, fixed by the number of cells (tiles of 256 cells in
the caller's order, a pairwise tree in a tile and over the tiles: the shape of the error
norms), so a column's numbers depend neither on the columns that share its launch, nor on
the chunking, nor on the number of ranks.

* ``CurvesPlan(mesh, mesh_time)``: the mesh, the vertex -> slab-row map, |T|, the gradients
  and the boundary-face masks on the device, built once.
* ``check_arguments(threshold)``: ValueError before anything touches the GPU.
* ``curves_eval``: the thin call of stk_curves_eval.
* ``time_curves_collective(plan, vec, theta)``: every rank its own columns, one all-reduce.

Scope: the nodes of [0, T], one threshold per call, the whole mesh, trial-space vectors.
Other time windows, several thresholds in one call, sub-regions of the mesh, values between
the nodes and test-space vectors are not served.
"""
import math

import numpy as np

from .p1_plan import MeshPlanHandle, device_address, threshold_value

SUMS = ('heat', 'l2_sq', 'h1_sq', 'outflow')
ALWAYS = SUMS + ('peak', 'peak_row', 'peak_point')
THRESHOLD_FIELDS = ('measure_above', 'moment_above', 'centroid_above', 'box_lo', 'box_hi')
FIELDS = ALWAYS + THRESHOLD_FIELDS


def rows(d):
    """{name: row or slice of rows} of the (stk_curves_rows(d), n) output: the indices of
    include/stk.h (STK_CURVES_*; the rows behind the moment as its function-like macros count them)."""
    from . import _lib as c
    m = c.STK_CURVES_MOMENT
    return {'heat': c.STK_CURVES_HEAT, 'l2_sq': c.STK_CURVES_L2, 'h1_sq': c.STK_CURVES_H1,
            'outflow': c.STK_CURVES_OUTFLOW, 'measure_above': c.STK_CURVES_MEASURE, 'moment_above': slice(m, m + d),
            'peak': m + d, 'peak_row': m + 1 + d, 'box_lo': slice(m + 2 + d, m + 2 + 2 * d),
            'box_hi': slice(m + 2 + 2 * d, m + 2 + 3 * d)}


def n_rows(d):
    return 7 + 3 * d


def check_arguments(threshold):
    """(theta, names) of a ``time_curves`` call, or ValueError; touches no GPU.  threshold:
    None (theta = +inf, the threshold fields are left out) or a number, not NaN."""
    return threshold_value(threshold), (ALWAYS if threshold is None else FIELDS)


def boundary_faces(cells):
    """(nc,) uint8: bit a set iff the face of the cell opposite its vertex a belongs to no
    other cell (stk_curves_boundary_faces; host only)."""
    from . import _lib
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    mask = np.zeros(len(cells), dtype=np.uint8)
    _lib.check(_lib.lib().stk_curves_boundary_faces(cells.shape[1] - 1, len(cells), cells.ctypes.data, mask.ctypes.data))
    return mask


class CurvesPlan:
    """The time-curves engine of libstk on one mesh.  Not for two streams at once: the plan
    owns the tile partials of a call in flight."""
    def __init__(self, mesh, mesh_time):
        from . import _lib
        from .assembly import free_dofs
        self._lib = _lib
        self.mesh_time = mesh_time
        self._plan = MeshPlanHandle(mesh, lambda lib, m, out: lib.stk_curves_plan_create(*m, out),
                                    lambda lib, plan: lib.stk_curves_plan_destroy(plan))
        self.d, self.nc, self.n_free = self._plan.d, self._plan.nc, self._plan.n_free
        # the coordinates of every slab row's vertex, for peak_point
        self.row_points = np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64)[free_dofs(mesh)])
        assert _lib.lib().stk_curves_rows(self.d) == n_rows(self.d)


def curves_eval(plan, slab, M, n_cols, row_stride, theta, out, ld_out):
    """stk_curves_eval: columns [0, n_cols) of `slab` -- a device tensor or a device address,
    rows row_stride doubles apart -- into out[q * ld_out + c], `out` a device tensor or
    address."""
    _lib = plan._lib
    _lib.check(_lib.lib().stk_curves_eval(_lib.stream(), plan._plan, int(M), int(n_cols), device_address(slab),
                                          int(row_stride), float(theta), int(ld_out), device_address(out)))
    return out


def curves_from_rows(plan, table, names):
    """The dict of a (rows, N) table: one entry per time node.  peak_point is a host-side
    lookup into the mesh points, the centroid a quotient taken here: NaN where the measure
    is 0."""
    import torch
    at = rows(plan.d)
    out = {}
    for name in names:
        if name in SUMS or name in ('peak', 'measure_above'):
            out[name] = table[at[name]]
        elif name == 'peak_row':
            out[name] = table[at[name]].to(torch.int64)
        elif name == 'peak_point':
            row = table[at['peak_row']].to(torch.int64).cpu().numpy()
            pts = np.full((len(row), plan.d), np.nan)
            found = row < plan.n_free  # (a column of nothing but NaN has no peak)
            pts[found] = plan.row_points[row[found]]
            out[name] = torch.from_numpy(pts).to(table.device)
        elif name == 'centroid_above':
            measure, moment = table[at['measure_above']], table[at['moment_above']]
            nan = torch.full((), math.nan, dtype=table.dtype, device=table.device)
            out[name] = torch.where(measure == 0.0, nan, moment / measure).t().contiguous()
        else:  # moment_above, box_lo, box_hi: (N, d)
            out[name] = table[at[name]].t().contiguous()
    return out


def time_curves_collective(plan, vec, theta):
    """The (rows, N) table of the whole trial-space vector `vec` (KronVectorMPI) on every
    rank.  COLLECTIVE: a rank evaluates the columns it owns into the columns [t_begin, t_end)
    of a zeroed table, and one all-reduce gives all of it to everyone -- one non-zero
    contributor per entry (the pattern of history_maps_collective; NaN and +-inf survive
    + 0.0), and a column's numbers do not depend on its neighbours in the launch, so the
    doubles are the one-rank doubles."""
    import torch
    assert vec.M == plan.n_free, (vec.M, plan.n_free)
    table = torch.zeros((n_rows(plan.d), vec.N), dtype=torch.float64, device=vec.buf.device)
    if vec.n_loc > 0:
        curves_eval(plan, vec.buf, vec.M, vec.n_loc, vec.ld, theta, plan._lib.ptr(table) + 8 * int(vec.t_begin), vec.N)
    dd = vec.dofs_distr
    if dd.size > 1:
        dd.comm.allreduce_tensor_(table)
    return table


def time_curves(heat, u, threshold=None):
    """What both drivers' ``time_curves`` do once `u` is a trial-space KronVectorMPI: the
    checks, the plan on first use (``heat.curves_plan``), the collective, the dict."""
    theta, names = check_arguments(threshold)
    plan = heat._lazy_plan('curves_plan', CurvesPlan)
    return curves_from_rows(plan, time_curves_collective(plan, u, theta), names)
