"""Isotherms: the level set {u_h = threshold} of a trial-space solution at time nodes, as the
segments (d = 2) or triangles (d = 3) in which it cuts the cells -- exact for the P1 function,
the cut the time curves' zone is built from (csrc/iso.hip, include/stk.h "isotherms") -- with
the gradient and the cell of every piece, the pieces' lengths or areas, and per node the
length or area of the isotherm and the heat that crosses it.

The result has no fixed length.  The device counts the pieces per (node, tile of 256 cells),
the exclusive scan of that small int64 table says where every tile's records go, and the
device fills them in: no atomics, and record i is what it is whatever the launch shape and
the number of ranks.  The per-node sums are trees of one fixed shape (``node_tree_sums``).

* ``check_arguments(threshold, nodes, N, max_bytes)``: ValueError before anything touches the GPU.
* ``iso_count``, ``iso_fill``: the thin calls of stk_iso_count and stk_iso_fill, on a
  ``CurvesPlan`` (source/time_curves.py).
* ``piece_measure``, ``node_tree_sums``: elementwise torch on the records.
* ``isotherms_collective(plan, vec, theta, nodes, max_bytes)``: every rank its own nodes, two
  all-reduces.

Scope: time nodes, one threshold per call, the whole mesh, trial-space vectors.  Times between
the nodes, several thresholds in one call, joining the pieces into polylines, a promised
orientation, sub-regions of the mesh and test-space vectors are not served.
"""
import operator

from .p1_plan import device_address, threshold_value

TILE_CELLS = 256
MAX_BYTES = 2**30
FIELDS = ('nodes', 'times', 'offsets', 'vertices', 'grad', 'cell', 'measure', 'measure_at', 'flux_at')


def width(d):
    """Doubles per record: d vertices of d coordinates, the gradient, the cell."""
    return d * d + d + 1


def check_arguments(threshold, nodes, N, max_bytes=MAX_BYTES):
    """(theta, nodes as a list of ints, max_bytes) of an ``isotherms`` call, or ValueError;
    touches no GPU.  threshold: a number, not NaN -- required; nodes: None (all N nodes) or
    strictly ascending ints in [0, N); max_bytes: a number, not negative."""
    theta = threshold_value(threshold, needed_by='isotherms()')
    if nodes is None:
        nodes = list(range(N))
    else:
        try:
            nodes = [operator.index(k) for k in nodes]
        except TypeError:
            raise ValueError('nodes must be None or ints, not %r' % (nodes,))
        if not nodes:
            raise ValueError('nodes names no time node')
        for i, k in enumerate(nodes):
            if not 0 <= k < N:
                raise ValueError('nodes[%d] = %d is not in [0, %d)' % (i, k, N))
            if i and k <= nodes[i - 1]:
                raise ValueError('nodes must be strictly ascending: nodes[%d] = %d follows %d' % (i, k, nodes[i - 1]))
    try:
        refused = not max_bytes >= 0
    except TypeError:
        refused = True
    if refused:
        raise ValueError('max_bytes must be a number, not negative, not %r' % (max_bytes,))
    return theta, nodes, max_bytes


def iso_count(plan, slab, M, n_cols, row_stride, theta, counts):
    """stk_iso_count: the pieces per tile of the columns [0, n_cols) of `slab` -- a device
    tensor or a device address, rows row_stride doubles apart -- into counts[c * n_tiles + t]
    (int64), `counts` a device tensor or address."""
    _lib = plan._lib
    _lib.check(_lib.lib().stk_iso_count(_lib.stream(), plan._plan, int(M), int(n_cols), device_address(slab),
                                        int(row_stride), float(theta), device_address(counts)))
    return counts


def iso_fill(plan, slab, M, n_cols, row_stride, theta, counts, first, n_out, out):
    """stk_iso_fill: the records of the same columns into out[i * W ..], i = first[c * n_tiles +
    t] + the rank in the tile, where 0 <= i < n_out; device tensors or addresses."""
    _lib = plan._lib
    _lib.check(_lib.lib().stk_iso_fill(_lib.stream(), plan._plan, int(M), int(n_cols), device_address(slab),
                                       int(row_stride), float(theta), device_address(counts), device_address(first),
                                       int(n_out), device_address(out)))
    return out


def ieee_sqrt(x):
    """The correctly rounded square root of a tensor.  On the device torch's; on the host
    NumPy's, torch's vectorised CPU kernel being one ulp off for some arguments."""
    import numpy as np
    import torch
    with np.errstate(invalid='ignore'):
        return torch.sqrt(x) if x.is_cuda else torch.from_numpy(np.sqrt(x.numpy()))


def piece_measure(vertices):
    """(n,) lengths of the segments (n, 2, 2) or areas of the triangles (n, 3, 3): every
    product and sum an elementwise torch operation, the cross product as the zone's volumes
    write it."""
    d = vertices.shape[1]
    a = vertices[:, 1] - vertices[:, 0]
    if d == 2:
        return ieee_sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])
    b = vertices[:, 2] - vertices[:, 0]
    c0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    c1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    c2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return ieee_sqrt((c0 * c0 + c1 * c1) + c2 * c2) / 2.0


def node_tree_sums(values, offsets):
    """(n_k,) sums of values[offsets[k] : offsets[k + 1]], every one in the same shape: the
    node's values in record order, padded with 0.0 to the power of two P at or above the
    largest count (at least 1), reduced by x[i] + x[i + s], s = P / 2 .. 1 -- elementwise adds
    on an (n_k, P) matrix; no sum, cumsum or index_add_ on doubles.  The padding is 0.0 and
    x + 0.0 == x, so a node's sum is the tree over its own power of two whatever P is: it
    does not depend on the nodes asked for with it.  The matrix is n_k P doubles."""
    import torch
    counts = offsets[1:] - offsets[:-1]
    n_k = counts.shape[0]
    largest = int(counts.max()) if n_k else 0
    P = 1
    while P < largest:
        P *= 2
    if values.shape[0] == 0:
        return torch.zeros(n_k, dtype=values.dtype, device=values.device)
    lane = torch.arange(P, dtype=torch.int64, device=values.device)
    index = (offsets[:-1, None] + lane[None, :]).clamp(max=values.shape[0] - 1)
    zero = torch.zeros((), dtype=values.dtype, device=values.device)
    x = torch.where(lane[None, :] < counts[:, None], values[index], zero)
    s = P // 2
    while s >= 1:
        x = x[:, :s] + x[:, s:2 * s]
        s //= 2
    return x[:, 0].contiguous()


def _runs(nodes, t_begin, t_end):
    """[(j, n)]: the maximal runs nodes[j : j + n] of consecutive nodes within [t_begin, t_end)."""
    runs = []
    for j, k in enumerate(nodes):
        if not t_begin <= k < t_end:
            continue
        if runs and sum(runs[-1]) == j and nodes[j - 1] == k - 1:
            runs[-1] = (runs[-1][0], runs[-1][1] + 1)
        else:
            runs.append((j, 1))
    return runs


def isotherms_collective(plan, vec, theta, nodes, max_bytes=MAX_BYTES):
    """(records (n, W), offsets (n_k + 1,) int64) of the nodes `nodes` (ascending ints) of the
    whole trial-space vector `vec` (KronVectorMPI), on every rank: the records of node
    nodes[k] are the rows offsets[k] .. offsets[k + 1].  COLLECTIVE: a rank counts the asked
    nodes it owns, per maximal run of consecutive columns, into a zeroed (n_k, n_tiles) int64
    table, and one all-reduce gives the table to everyone (one non-zero contributor per
    entry; counts are exact in whatever dtype the communicator carries).  `first` is its
    exclusive cumsum in (node, tile) order; the total costs the one read-back.  Where the
    records would take more than max_bytes, every rank raises the same ValueError before
    anything is allocated.  Otherwise a rank fills the ranges of its nodes in a zeroed (n, W)
    table and one all-reduce gives all of it to everyone -- the pattern of
    time_curves_collective: NaN and +-inf survive + 0.0, a -0.0 may come back as +0.0 -- and a
    column's records do not depend on its neighbours in the launch, so the doubles are the
    one-rank doubles."""
    import torch
    assert vec.M == plan.n_free, (vec.M, plan.n_free)
    _lib = plan._lib
    dev = vec.buf.device
    W, n_k, n_tiles = width(plan.d), len(nodes), -(-plan.nc // TILE_CELLS)
    runs = _runs(nodes, int(vec.t_begin), int(vec.t_begin) + int(vec.n_loc))
    slab = _lib.ptr(vec.buf) if runs else None

    def column(j):
        return slab + 8 * (nodes[j] - int(vec.t_begin))

    counts = torch.zeros((n_k, n_tiles), dtype=torch.int64, device=dev)
    for j, n in runs:
        iso_count(plan, column(j), vec.M, n, vec.ld, theta, _lib.ptr(counts) + 8 * j * n_tiles)
    dd = vec.dofs_distr
    if dd.size > 1:
        dd.comm.allreduce_tensor_(counts)
    flat = counts.reshape(-1)
    first = torch.cumsum(flat, 0) - flat
    total = int((first[-1] + flat[-1]).item())
    if total * W * 8 > max_bytes:
        raise ValueError('isotherms(): %d pieces in %d nodes take %d bytes, more than max_bytes = %d: ask for fewer nodes'
                         % (total, n_k, total * W * 8, max_bytes))
    table = torch.zeros((total, W), dtype=torch.float64, device=dev)
    if total > 0:
        for j, n in runs:
            iso_fill(plan, column(j), vec.M, n, vec.ld, theta, _lib.ptr(counts) + 8 * j * n_tiles,
                     _lib.ptr(first) + 8 * j * n_tiles, total, table)
        if dd.size > 1:
            dd.comm.allreduce_tensor_(table)
    per_node = counts.sum(dim=1)  # (int64: exact)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(per_node, 0)])
    return table, offsets


def isotherms_from_records(plan, table, offsets, nodes, h):
    """The dict of a table of records: the views, the measures and the per-node tree sums."""
    import torch
    d = plan.d
    dev = table.device
    vertices = table[:, :d * d].reshape(-1, d, d)
    grad = table[:, d * d:d * d + d].contiguous()
    measure = piece_measure(vertices)
    gg = grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]
    if d == 3:
        gg = gg + grad[:, 2] * grad[:, 2]
    return {'nodes': torch.tensor(nodes, dtype=torch.int64, device=dev),
            'times': torch.tensor([float(k) * h for k in nodes], dtype=torch.float64, device=dev),
            'offsets': offsets, 'vertices': vertices.contiguous(), 'grad': grad,
            'cell': table[:, d * d + d].to(torch.int64), 'measure': measure,
            'measure_at': node_tree_sums(measure, offsets),
            'flux_at': node_tree_sums(measure * ieee_sqrt(gg), offsets)}


def isotherms(heat, u, threshold, nodes=None, max_bytes=MAX_BYTES):
    """What both drivers' ``isotherms`` do once `u` is a trial-space KronVectorMPI: the checks,
    the plan on first use (``heat.curves_plan``, shared with the time curves), the collective,
    the dict."""
    from .time_curves import CurvesPlan
    mesh_time = heat._sample_meshes[1]
    theta, nodes, max_bytes = check_arguments(threshold, nodes, mesh_time.nv, max_bytes)
    plan = heat._lazy_plan('curves_plan', CurvesPlan)
    assert plan._lib.lib().stk_iso_width(plan.d) == width(plan.d)
    table, offsets = isotherms_collective(plan, u, theta, nodes, max_bytes)
    return isotherms_from_records(plan, table, offsets, nodes, float(mesh_time.h))
