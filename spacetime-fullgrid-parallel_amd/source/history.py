"""Thermal history maps: how hot every point got and when, how much heat it received,
how long and between which times it was above a threshold, how fast it heated and cooled --
all from ONE scan along time on the device (csrc/history.hip, include/stk.h "history maps").

A trial-space vector is piecewise linear in time, so each of these is a reduction along a
slab row.  The scan carries a state of nine doubles per row (``STATE_ROWS``); a scan of the
columns [k0, k1) followed by one of [k1, k2) is the scan of [k0, k2) double for double, which
makes the result independent of the number of ranks and of how columns are chunked.

* ``history_scan``: the thin call of stk_history_scan.
* ``history_maps_collective(vec, threshold)``: the nodal form, one row per free dof; the
  state travels down the ranks in the order of their time nodes.
* ``history_points_collective(plan, vec, points, threshold)``: the per-point form, on the
  (n_k, n_p) blocks of ``sampling.sample_collective`` at the nodes, in column chunks.
* ``maps_from_state``: the dict of fields of a state.

Scope: the whole interval [0, T], one threshold for all rows per call.  Other time windows,
several thresholds in one call and per-row thresholds are not served.
"""
import math

import numpy as np

from .p1_plan import (check_points_shape, device_address, field_names, scan_down_the_ranks, threshold_value,
                      time_step)

FIELDS = ('peak', 't_peak', 'dose', 'time_above', 't_first', 't_last', 'max_rate', 'min_rate')
STATE_ROWS = FIELDS + ('last',)
THRESHOLD_FIELDS = ('time_above', 't_first', 't_last')
BLOCK_BYTES = 256 << 20  # the per-point form keeps a sampled block at or below this


def check_arguments(threshold, points=None, d=None, fields=None):
    """(theta, names) of a ``history_maps`` call, or ValueError; touches no GPU.  threshold:
    None (theta = +inf, the threshold fields are left out) or a number, not NaN; points: None
    or (n_p, d); fields: None (all that the threshold allows) or names of FIELDS."""
    theta = threshold_value(threshold)
    check_points_shape(points, d)
    allowed = FIELDS if threshold is not None else tuple(f for f in FIELDS if f not in THRESHOLD_FIELDS)
    return theta, field_names(fields, FIELDS, allowed)


def plan_chunks(n_nodes, n_p, block_bytes=BLOCK_BYTES):
    """[(k0, k1), ...]: the nodes 0 .. n_nodes - 1 in ascending runs whose (k1 - k0, n_p)
    block of doubles stays at or below block_bytes -- at least one column per run."""
    per = max(1, int(block_bytes) // (8 * max(int(n_p), 1)))
    return [(k, min(k + per, n_nodes)) for k in range(0, int(n_nodes), per)]


def history_scan(u, M, n_cols, strides, k_first, h, threshold, state, fresh):
    """stk_history_scan on `u` -- a device tensor or a device address -- with strides =
    (row_stride, col_stride) in doubles; `state`: (9, M) float64 device tensor, contiguous,
    updated in place (initialised when `fresh`)."""
    import torch

    from . import _lib
    assert tuple(state.shape) == (len(STATE_ROWS), M) and state.is_contiguous() and state.dtype == torch.float64
    _lib.check(_lib.lib().stk_history_scan(_lib.stream(), M, n_cols, device_address(u), strides[0], strides[1], k_first,
                                           float(h), float(threshold), int(bool(fresh)), _lib.ptr(state)))
    return state


def maps_from_state(state, names, outside=None):
    """The dict {name: (M,) tensor} of the rows `names` of a state; rows where `outside`
    (bool tensor) holds become NaN."""
    out = {}
    for f in names:
        row = state[STATE_ROWS.index(f)]
        if outside is not None:
            row = row.masked_fill(outside, math.nan)
        out[f] = row
    return out


def history_maps_collective(vec, theta, mesh_time=None):
    """The (9, M) state of the whole trial-space vector `vec` (KronVectorMPI) on every rank.
    COLLECTIVE and serial in the ranks by design (p1_plan.scan_down_the_ranks): every rank
    scans its own columns, fresh on the rank that owns node 0, into the state it received --
    size - 1 transfers of 72 M bytes.  Every row's operations come in one order, so the
    doubles are the one-rank doubles."""
    import torch
    h = float(time_step(vec, mesh_time).h)
    state = torch.empty((len(STATE_ROWS), vec.M), dtype=torch.float64, device=vec.buf.device)
    if vec.M == 0:
        return state
    return scan_down_the_ranks(vec, state, lambda state: history_scan(
        vec.buf, vec.M, vec.n_loc, (vec.ld, 1), vec.t_begin, h, theta, state, fresh=vec.t_begin == 0))


def history_points_collective(plan, vec, points, theta, block_bytes=BLOCK_BYTES):
    """((9, n_p) state, inside (n_p,) bool) of u_h at `points` ((n_p, d), or what
    plan.locate returned).  COLLECTIVE: the blocks of ``sample_collective`` at the nodes
    -- bit-identical on every rank -- in the column chunks of ``plan_chunks``, each scanned in
    the time-major form with the carried state.  Points outside the mesh hold whatever the
    scan makes of NaN: ``maps_from_state(..., outside=~inside)`` blanks them."""
    import torch

    from .sampling import sample_collective, time_weights
    mesh_time = time_step(vec, plan.mesh_time)
    h, N = float(mesh_time.h), vec.N
    located = plan.locate(points)
    n_p = located.n_p
    state = torch.empty((len(STATE_ROWS), n_p), dtype=torch.float64, device=vec.buf.device)
    if n_p == 0:
        return state, located.inside
    for k0, k1 in plan_chunks(N, n_p, block_bytes):
        times = np.array([float(k) * h for k in range(k0, k1)])
        # the doubles the kernel calls t_k must sit exactly on their nodes in the sampler
        _, w = time_weights(mesh_time, times, 0, N)
        assert np.all(((w[:, 0] == 1.0) & (w[:, 1] == 0.0)) | ((w[:, 0] == 0.0) & (w[:, 1] == 1.0))), w
        block = sample_collective(plan, vec, times, located)
        history_scan(block, n_p, k1 - k0, (1, n_p), k0, h, theta, state, fresh=k0 == 0)
        del block
    return state, located.inside


def history_maps(heat, u, threshold=None, points=None, fields=None):
    """What both drivers' ``history_maps`` do once `u` is a trial-space KronVectorMPI: the
    dict of the fields, per free dof or per point (then with 'inside')."""
    mesh_space, mesh_time = heat._sample_meshes
    theta, names = check_arguments(threshold, points, mesh_space.points.shape[1], fields)
    if points is None:
        return maps_from_state(history_maps_collective(u, theta, mesh_time), names)
    state, inside = history_points_collective(heat.sample_plan, u, points, theta)
    out = maps_from_state(state, names, outside=~inside)
    out['inside'] = inside
    return out
