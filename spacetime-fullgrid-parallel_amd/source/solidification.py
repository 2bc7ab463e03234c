"""Solidification maps: what happens at the freezing front of a trial-space solution, per CELL
of the mesh -- when the cell's mean last dropped to or below a threshold, how fast it was
cooling and what the gradient of u_h was at that moment (their quotient is the speed of the
front), how often it happened, and the largest |grad u_h| the cell ever saw -- from ONE scan
over the cells' rows on the device (csrc/solid.hip, include/stk.h "solidification maps").

grad u_h is constant per cell, so the history maps (rows are dofs or points) cannot see it.
Mean and gradient of a cell are linear in time per element; the scan carries a state of
6 + 2 d doubles per cell (``n_rows(d)``), and a scan of the columns [k0, k1) followed by one
of [k1, k2) is the scan of [k0, k2) double for double, which makes the result independent of
the number of ranks and of how columns are chunked.

* ``SolidPlan(mesh, mesh_time)``: the mesh, grad lambda per cell and the tiles' row lists on
  the device, built once; the tiles are cut from the cells along a Z-curve (``cell_order``).
* ``check_arguments(threshold, points, d, fields)``: ValueError before anything touches the GPU.
* ``solid_scan``: the thin call of stk_solid_scan.
* ``solidification_collective(plan, vec, theta)``: the state travels down the ranks in the
  order of their time nodes.
* ``maps_from_state``: the dict of fields of a state; the square roots and the front speed
  are taken here, in torch.

Scope: the whole interval [0, T], one threshold for all cells per call, downward crossings,
trial-space vectors.  Per-cell thresholds, several thresholds in one call, melting
crossings, other time windows and a parallel merge of per-rank states are not served.
"""
import math

import numpy as np

from .p1_plan import (MeshPlanHandle, check_points_shape, device_address, field_names, scan_down_the_ranks,
                      threshold_value, time_step)

FIELDS = ('t_solid', 'cooling_rate', 'grad_solid', 'G', 'front_speed', 'n_solid', 'max_grad', 't_max_grad')
TILE_CELLS = 256
NO_ROW = 0xFFFF


def n_rows(d):
    return 6 + 2 * d


def rows(d):
    """{name: row or slice of rows} of the (stk_solid_rows(d), nc) state: the indices of
    include/stk.h (STK_SOLID_*)."""
    from . import _lib as c
    g = c.STK_SOLID_GRAD_SOLID
    return {'t_solid': c.STK_SOLID_T_SOLID, 'cooling_rate': c.STK_SOLID_COOLING_RATE, 'n_solid': c.STK_SOLID_N_SOLID,
            'max_grad_sq': c.STK_SOLID_MAX_GRAD_SQ, 't_max_grad': c.STK_SOLID_T_MAX_GRAD,
            'last_mean': c.STK_SOLID_LAST_MEAN, 'grad_solid': slice(g, g + d), 'last_grad': slice(g + d, g + 2 * d)}


def check_arguments(threshold, points=None, d=None, fields=None):
    """(theta, names) of a ``solidification_maps`` call, or ValueError; touches no GPU.
    threshold: a number, not NaN -- required; points: None or (n_p, d); fields: None (all) or
    names of FIELDS."""
    theta = threshold_value(threshold, needed_by='solidification_maps')
    check_points_shape(points, d)
    return theta, field_names(fields, FIELDS)


def tile_rows(cells, row_of):
    """(tile_ptr (n_tiles + 1,) int32, tile_rows int32, cell_pos (nc, d + 1) uint16): per tile
    of 256 consecutive cells the ascending list of the distinct slab rows its cells touch, and
    per cell the positions of its vertices' rows in that list, NO_ROW on the boundary
    (stk_solid_tile_rows; host only).  row_of (nv,): the slab row of a vertex, -1 on the
    boundary."""
    from . import _lib
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    row_of = np.ascontiguousarray(row_of, dtype=np.int32)
    nc, nl = cells.shape
    n_tiles = -(-nc // TILE_CELLS)
    ptr = np.zeros(n_tiles + 1, dtype=np.int32)
    listed = np.zeros(nc * nl, dtype=np.int32)
    pos = np.zeros((nc, nl), dtype=np.uint16)
    _lib.check(_lib.lib().stk_solid_tile_rows(nl - 1, len(row_of), nc, cells.ctypes.data, row_of.ctypes.data,
                                              ptr.ctypes.data, listed.ctypes.data, pos.ctypes.data))
    return ptr, listed[:ptr[-1]].copy(), pos


def cell_order(mesh):
    """(nc,) int32: the cells along the Z-curve of their centroids, ties by index -- the order
    in which a plan takes them, 256 at a time (stk_solid_cell_order; host only).  A cell's
    numbers are its own: the order changes no double, only which rows a tile shares."""
    from . import _lib
    from .p1_plan import mesh_arrays
    pts, cells, d = mesh_arrays(mesh)
    order = np.zeros(len(cells), dtype=np.int32)
    _lib.check(_lib.lib().stk_solid_cell_order(d, len(pts), len(cells), pts.ctypes.data, cells.ctypes.data, order.ctypes.data))
    return order


class SolidPlan:
    """The solidification engine of libstk on one mesh.  It owns no workspace."""
    def __init__(self, mesh, mesh_time):
        from . import _lib
        self._lib = _lib
        self.mesh_time = mesh_time
        self._plan = MeshPlanHandle(mesh, lambda lib, m, out: lib.stk_solid_plan_create(*m, out),
                                    lambda lib, plan: lib.stk_solid_plan_destroy(plan))
        self.d, self.nc, self.n_free = self._plan.d, self._plan.nc, self._plan.n_free
        assert _lib.lib().stk_solid_rows(self.d) == n_rows(self.d)


def solid_scan(plan, slab, M, n_cols, row_stride, k_first, h, theta, state, fresh):
    """stk_solid_scan: columns [0, n_cols) of `slab` -- a device tensor or a device address,
    rows row_stride doubles apart, column c the node k_first + c -- into `state`: a
    (6 + 2 d, nc) float64 device tensor, contiguous, updated in place (initialised when
    `fresh`)."""
    import torch
    _lib = plan._lib
    assert tuple(state.shape) == (n_rows(plan.d), plan.nc) and state.is_contiguous() and state.dtype == torch.float64
    _lib.check(_lib.lib().stk_solid_scan(_lib.stream(), plan._plan, int(M), int(n_cols), device_address(slab),
                                         int(row_stride), int(k_first), float(h), float(theta), int(bool(fresh)),
                                         _lib.ptr(state)))
    return state


def solidification_collective(plan, vec, theta):
    """The (6 + 2 d, nc) state of the whole trial-space vector `vec` (KronVectorMPI) on every
    rank.  COLLECTIVE and serial in the ranks by design (p1_plan.scan_down_the_ranks): every
    rank scans its own columns, fresh on the rank that owns node 0, into the state it received
    -- size - 1 transfers of 8 (6 + 2 d) nc bytes.  Every cell's operations come in one order,
    so the doubles are the one-rank doubles.  A parallel merge of per-rank states is out of
    scope."""
    import torch
    assert vec.M == plan.n_free, (vec.M, plan.n_free)
    h = float(time_step(vec, plan.mesh_time).h)
    state = torch.empty((n_rows(plan.d), plan.nc), dtype=torch.float64, device=vec.buf.device)
    return scan_down_the_ranks(vec, state, lambda state: solid_scan(
        plan, vec.buf, vec.M, vec.n_loc, vec.ld, vec.t_begin, h, theta, state, fresh=vec.t_begin == 0))


def maps_from_state(state, d, names=FIELDS):
    """The dict of the fields `names` of a (6 + 2 d, nc) state, per cell: 'G' is the square
    root of the sum of squares of grad_solid taken from the left, 'front_speed' the quotient
    cooling_rate / G (whatever IEEE gives where G == 0), 'max_grad' the square root of
    max_grad_sq, 'n_solid' int64, 'grad_solid' (nc, d)."""
    import torch
    at = rows(d)
    gs = state[at['grad_solid']]

    def G():
        q = gs[0] * gs[0] + gs[1] * gs[1]
        if d == 3:
            q = q + gs[2] * gs[2]
        return torch.sqrt(q)

    out = {}
    for name in names:
        if name in ('t_solid', 'cooling_rate', 't_max_grad'):
            out[name] = state[at[name]]
        elif name == 'grad_solid':
            out[name] = gs.t().contiguous()
        elif name == 'G':
            out[name] = G()
        elif name == 'front_speed':
            out[name] = state[at['cooling_rate']] / G()
        elif name == 'n_solid':
            out[name] = state[at['n_solid']].to(torch.int64)
        else:  # max_grad
            out[name] = torch.sqrt(state[at['max_grad_sq']])
    return out


def maps_at_points(maps, located):
    """The fields of the cell that holds each located point, plus 'inside': a gather by
    ``located.cell``; NaN outside the mesh, and -1 for 'n_solid'."""
    import torch
    inside = located.inside
    cell = located.cell.to(torch.int64).clamp(min=0)
    out = {}
    for name, value in maps.items():
        got = value.index_select(0, cell)
        outside = ~inside if got.ndim == 1 else (~inside)[:, None]
        out[name] = got.masked_fill(outside, -1 if name == 'n_solid' else math.nan)
    out['inside'] = inside
    return out


def solidification_maps(heat, u, threshold, points=None, fields=None):
    """What both drivers' ``solidification_maps`` do once `u` is a trial-space KronVectorMPI:
    the checks, the plan on first use (``heat.solid_plan``), the collective, the dict -- per
    cell in the mesh's cell order, or per point (then with 'inside')."""
    theta, names = check_arguments(threshold, points, heat._sample_meshes[0].points.shape[1], fields)
    plan = heat._lazy_plan('solid_plan', SolidPlan)
    maps = maps_from_state(solidification_collective(plan, u, theta), plan.d, names)
    if points is None:
        return maps
    return maps_at_points(maps, heat.sample_plan.locate(points))
