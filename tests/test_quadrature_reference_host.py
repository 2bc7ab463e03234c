"""The two quadrature engines -- the space-time load (csrc/load_dev.hip) and the error norms
(csrc/err_norms.hip), with the kernels they share in csrc/p1_mesh.h -- restated in NumPy
float64 IN THE KERNELS' OWN ORDER OF OPERATIONS, and the tests of that restatement (no GPU).
tests/test_quadrature_kernels_gpu.py compares the device with it and asserts equal doubles.

The restatement is a second derivation of the same arithmetic, vectorised over the cells: every
product and every sum below is ONE NumPy operation on float64 arrays, rounded on its own (no
dot, matmul, einsum or sum), and a Python loop runs only over q, k, a, j, the incidence rank
and the tree step.  What it pins beyond a rounding bound: a fused multiply-add anywhere (the
files are built without contraction), the order of the k sum (`acc = k ? acc + term : term`),
the order of a dof's shares (ascending (cell, local vertex)), and the shape of the two trees
(256 lanes per tile, then P = 2^ceil(log2 n_tiles) over the tiles with absent partners
skipped) -- the shape that makes a result independent of grid and rank.

`paths(...)` names, from the sizes of a call alone, every launch path the call takes: tail or
full tiles, an LDS-only finish or its in-place global steps, the second trip of each capped
grid.  The constants are read off the code: 256 lanes, 2048 workgroups per time point for the
shares, 4096 for every other grid.

Checked here: the 2-D load against libstk's host routines bit for bit (they are written
separately in csrc/mesh_refine.hip and run on host threads), the 3-D load against a longdouble
sum, the error norms against the longdouble oracle of tests/test_error_norms_host.py within its
bound B, integrals known in closed form, and the trees on integers."""
import math
import types

import numpy as np
import pytest

BS = 256           # lanes of a workgroup = cells of a tile (P1_BS, BS)
SHARES_CAP = 2048  # workgroups per time point of load_shares_kernel
GRID_CAP = 4096    # stk_flat_grid, and the grid of err_cells_kernel
FLAT = GRID_CAP * BS  # items of one trip of a flat grid: 1 048 576


# ---- meshes ----------------------------------------------------------------------------------------
def grid_mesh(nx, ny, jitter=0.3, seed=0, all_free=False):
    """A structured triangulation of [0, nx / ny] x [0, 1] by NumPy alone: (nx + 1)(ny + 1)
    points, row by row, and 2 nx ny triangles.  The diagonal of square (i, j) alternates with
    i + j, so a vertex lies in at most 8 cells; the second triangle of every square is listed
    clockwise, so det has both signs.  Interior points are moved by up to jitter / 2 of the grid
    width in either direction and rim points along their side (seeded), so no two areas are
    equal and the rectangle stays; `boundary` marks the rim --
    or nothing with all_free, which makes every vertex a free dof."""
    assert nx >= 1 and ny >= 1 and 0.0 <= jitter < 0.5
    h = 1.0 / ny
    ix, iy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))  # (ny + 1, nx + 1): row by row
    rim = (ix == 0) | (ix == nx) | (iy == 0) | (iy == ny)
    rng = np.random.RandomState(seed)
    move = jitter * h * (rng.rand(ny + 1, nx + 1, 2) - 0.5)
    move[..., 0][(ix == 0) | (ix == nx)] = 0.0  # a rim point slides along its side, a corner stays
    move[..., 1][(iy == 0) | (iy == ny)] = 0.0
    points = np.stack([ix * h, iy * h], axis=2) + move
    vid = lambda i, j: j * (nx + 1) + i
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(nx), np.arange(ny)))
    a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
    even = (i + j) % 2 == 0
    # even squares are cut along a-c, odd ones along b-d; first triangle counter-clockwise,
    # second clockwise
    first = np.where(even[:, None], np.stack([a, b, c], axis=1), np.stack([a, b, d], axis=1))
    second = np.where(even[:, None], np.stack([a, d, c], axis=1), np.stack([b, d, c], axis=1))
    cells = np.empty((2 * nx * ny, 3), dtype=np.int64)
    cells[0::2], cells[1::2] = first, second
    nv = (nx + 1) * (ny + 1)
    boundary = np.zeros(nv, dtype=bool) if all_free else rim.reshape(-1).copy()
    return types.SimpleNamespace(points=np.ascontiguousarray(points.reshape(nv, 2)), cells=cells, boundary=boundary, nv=nv)


def first_cells(mesh, n):
    """The first n cells of a mesh as a mesh of their own (the ABI does not ask the cells to
    cover anything)."""
    assert n <= len(mesh.cells)
    return types.SimpleNamespace(points=mesh.points, cells=np.ascontiguousarray(mesh.cells[:n]), boundary=mesh.boundary,
                                 nv=mesh.nv)


def free_rows(mesh):
    """(free vertices ascending, row_of (nv,) with -1 on the boundary)."""
    fd = np.flatnonzero(~np.asarray(mesh.boundary, dtype=bool))
    row_of = np.full(mesh.nv, -1, dtype=np.int64)
    row_of[fd] = np.arange(len(fd))
    return fd, row_of


# ---- the simplex geometry (p1_mesh.h) -----------------------------------------------------------------
def simplex_of(points, cells):
    """p1_simplex_of<2|3>: (e[r][k], cof[r][j], det) as lists of (nc,) arrays."""
    p, cells = np.asarray(points, dtype=np.float64), np.asarray(cells)
    d = cells.shape[1] - 1
    e = [[p[cells[:, r + 1], k] - p[cells[:, 0], k] for k in range(d)] for r in range(d)]
    if d == 2:
        cof = [[e[1][1], -e[1][0]], [-e[0][1], e[0][0]]]
        det = e[0][0] * e[1][1] - e[0][1] * e[1][0]
    else:
        cof = []
        for r in range(3):
            a, b = e[(r + 1) % 3], e[(r + 2) % 3]
            cof.append([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        det = (e[0][0] * cof[0][0] + e[0][1] * cof[0][1]) + e[0][2] * cof[0][2]
    return e, cof, det


def volume(det, d):
    """p1_volume: |det| / d!"""
    return np.abs(det) / (2.0 if d == 2 else 6.0)


def gradients(cof, det):
    """p1_gradients: G (nc, d + 1, d), every quotient rounded once, G[0] = ((0 - G[1]) - G[2]) [- G[3]]."""
    d = len(cof)
    G = np.empty((len(det), d + 1, d))
    for r in range(d):
        for j in range(d):
            G[:, r + 1, j] = cof[r][j] / det
    for j in range(d):
        g0 = (0.0 - G[:, 1, j]) - G[:, 2, j]
        if d == 3:
            g0 = g0 - G[:, 3, j]
        G[:, 0, j] = g0
    return G


def geometry_kernel(points, cells):
    """p1_geometry_kernel: (|T| (nc,), grad (nc, d + 1, d)) with grad lambda_0 = -((g_1 + g_2) [+ g_3]),
    which is -0.0 where p1_gradients gives +0.0."""
    _, cof, det = simplex_of(points, cells)
    d = len(cof)
    g = gradients(cof, det)
    for j in range(d):
        s = g[:, 1, j] + g[:, 2, j]
        if d == 3:
            s = s + g[:, 3, j]
        g[:, 0, j] = -s
    return volume(det, d), g


def quadrature_points(points, cells, ql):
    """p1_points_kernel: (d, nc, nq), l0 p0 + l1 p1 + ... summed from the left."""
    p, cells, ql = np.asarray(points, dtype=np.float64), np.asarray(cells), np.asarray(ql, dtype=np.float64)
    d = cells.shape[1] - 1
    out = np.empty((d, len(cells), len(ql)))
    for k in range(d):
        for q in range(len(ql)):
            x = ql[q, 0] * p[cells[:, 0], k]
            for a in range(1, d + 1):
                x = x + ql[q, a] * p[cells[:, a], k]
            out[k, :, q] = x
    return out


# ---- the load (load_dev.hip) ----------------------------------------------------------------------------
def load_shares(vol, qw, ql, f):
    """load_shares_kernel: (n_k, nc, d + 1), (sum_q (f_q w_q) l_qa) |T| with q ascending from 0.0."""
    f, qw, ql = np.asarray(f, dtype=np.float64), np.asarray(qw, dtype=np.float64), np.asarray(ql, dtype=np.float64)
    n_k, nc, nq = f.shape
    nl = ql.shape[1]
    out = np.empty((n_k, nc, nl))
    for k in range(n_k):
        s = [np.zeros(nc) for _ in range(nl)]
        for q in range(nq):
            fw = f[k, :, q] * qw[q]
            for a in range(nl):
                s[a] = s[a] + fw * ql[q, a]
        for a in range(nl):
            out[k, :, a] = s[a] * vol
    return out


def incidence(cells, nv, free_vertices):
    """(slot (n_free, R), present (n_free, R)): the slots (d + 1) cell + a of every free dof in
    ascending order, rank by rank; R = the largest number of cells at a vertex."""
    flat = np.asarray(cells).reshape(-1)
    by_vertex = np.argsort(flat, kind='stable')  # grouped by vertex, ascending slot inside a group
    count = np.bincount(flat, minlength=nv)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    fv = np.asarray(free_vertices)
    R = int(count[fv].max()) if len(fv) else 0
    slot = np.zeros((len(fv), R), dtype=np.int64)
    present = np.zeros((len(fv), R), dtype=bool)
    for r in range(R):
        present[:, r] = count[fv] > r
        slot[:, r] = by_vertex[np.where(present[:, r], start[fv] + r, 0)]
    return slot, present


def load_gather(shares, slot, present, coef):
    """load_gather_kernel without its store: (n_free, 2).  L_k = the shares of a dof in ascending
    slot from 0.0; t = c[k][a] L_k; acc = t at k = 0 and acc + t afterwards."""
    n_k = shares.shape[0]
    coef = np.asarray(coef, dtype=np.float64)
    acc = [None, None]
    for k in range(n_k):
        sk = shares[k].reshape(-1)
        L = np.zeros(slot.shape[0])
        for r in range(slot.shape[1]):
            L = np.where(present[:, r], L + sk[slot[:, r]], L)
        for a in range(2):
            t = coef[k, a] * L
            acc[a] = t if k == 0 else acc[a] + t
    return np.stack(acc, axis=1)


def load_pair(mesh, qw, ql, f, coef):
    """The pair of columns stk_load_columns forms for the free dofs of a mesh, (n_free, 2).  The
    row order of a plan does not enter: every row has one owner and one order of its sums."""
    _, _, det = simplex_of(mesh.points, mesh.cells)
    vol = volume(det, mesh.cells.shape[1] - 1)
    fd, _ = free_rows(mesh)
    slot, present = incidence(mesh.cells, mesh.nv, fd)
    with np.errstate(all='ignore'):  # (NaN and inf in f are data like any other)
        return load_gather(load_shares(vol, qw, ql, f), slot, present, coef)


def load_columns(mesh, qw, ql, f, coef, slab, e_local, accumulate):
    """What stk_load_columns leaves in a slab (n_free, ld): columns (2 e, 2 e + 1) are the pair,
    or old + pair with `accumulate`; everything else keeps its bits."""
    out = np.array(slab, dtype=np.float64, copy=True)
    pair = load_pair(mesh, qw, ql, f, coef)
    cols = slice(2 * e_local, 2 * e_local + 2)
    out[:, cols] = out[:, cols] + pair if accumulate else pair
    return out


# ---- the error norms (err_norms.hip) ----------------------------------------------------------------------
def tree256(a):
    """The pairwise tree over the 256 lanes: red[i] += red[i + s] for s = 128 .. 1; a (..., 256)."""
    s = BS // 2
    while s >= 1:
        a = a[..., :s] + a[..., s:2 * s]
        s //= 2
    return a[..., 0]


def tile_partials(x):
    """One partial per tile of 256 consecutive cells of x (nc,): dead lanes are 0.0."""
    n_tiles = (len(x) + BS - 1) // BS
    a = np.zeros(n_tiles * BS)
    a[:len(x)] = x
    return tree256(a.reshape(n_tiles, BS))


def finish_tree(w):
    """err_finish_kernel on the partials w (n_tiles,): partial i + partial i + s for s = P / 2,
    P / 4, ..., 1 with P the power of two at or above n_tiles; an absent partner adds nothing.
    In place while s >= 256, then the 256-lane tree with 0.0 in the absent places."""
    w = np.array(w, dtype=np.float64, copy=True)
    n = len(w)
    P = 1
    while P < n:
        P *= 2
    s = P // 2
    while s >= BS:
        m = max(min(s, n - s), 0)  # the i < s with i + s < n
        w[:m] = w[:m] + w[s:s + m]
        s //= 2
    red = np.zeros(BS)
    red[:min(n, BS)] = w[:BS]
    return tree256(red)


def err_cells(mesh, qw, ql, w_lo, w_hi, c, f, gf, lo_rows, hi_rows):
    """err_cells_kernel line for line: the four numbers of every cell, (4, nc), before the trees.
    lo_rows / hi_rows (n_free,): the slab rows of the two time nodes; boundary vertices read as 0.0."""
    cells = np.asarray(mesh.cells)
    d, nc = cells.shape[1] - 1, len(cells)
    qw, ql = np.asarray(qw, dtype=np.float64), np.asarray(ql, dtype=np.float64)
    w_lo, w_hi, c = (np.asarray(a, dtype=np.float64) for a in (w_lo, w_hi, c))
    f = np.asarray(f, dtype=np.float64)
    n_k, nq = len(c), len(qw)
    assert f.shape == (n_k, nc, nq) and (gf is None or gf.shape == (n_k, d, nc, nq))
    vol, g = geometry_kernel(mesh.points, cells)
    _, row_of = free_rows(mesh)
    row = row_of[cells]
    free_v = row >= 0
    lo = np.where(free_v, np.asarray(lo_rows, dtype=np.float64)[np.maximum(row, 0)], 0.0)
    hi = np.where(free_v, np.asarray(hi_rows, dtype=np.float64)[np.maximum(row, 0)], 0.0)
    acc = [None] * 4
    for k in range(n_k):
        U = [np.where(free_v[:, a], w_lo[k] * lo[:, a] + w_hi[k] * hi[:, a], 0.0) for a in range(d + 1)]
        X = [np.zeros(nc) for _ in range(4)]
        for q in range(nq):
            uh = ql[q, 0] * U[0] + ql[q, 1] * U[1]
            for a in range(2, d + 1):
                uh = uh + ql[q, a] * U[a]
            fq = f[k, :, q]
            e = fq - uh
            X[0] = X[0] + (e * e) * qw[q]
            X[2] = X[2] + (fq * fq) * qw[q]
        if gf is not None:
            for j in range(d):
                G = U[0] * g[:, 0, j]
                for a in range(1, d + 1):
                    G = G + U[a] * g[:, a, j]
                ej, rj = np.zeros(nc), np.zeros(nc)
                for q in range(nq):
                    gq = gf[k, j, :, q]
                    e = gq - G
                    ej = ej + (e * e) * qw[q]
                    rj = rj + (gq * gq) * qw[q]
                X[1] = X[1] + ej
                X[3] = X[3] + rj
        for x in range(4):
            term = c[k] * (X[x] * vol)
            acc[x] = term if k == 0 else acc[x] + term
    return np.stack(acc)


def err_element(mesh, qw, ql, w_lo, w_hi, c, f, gf, lo_rows, hi_rows):
    """The four doubles of stk_err_element: the cells, the tile trees, the finish tree."""
    with np.errstate(all='ignore'):
        per_cell = err_cells(mesh, qw, ql, w_lo, w_hi, c, f, gf, lo_rows, hi_rows)
        return np.array([finish_tree(tile_partials(per_cell[x])) for x in range(4)])


# ---- which paths a call takes -------------------------------------------------------------------------------
def finish_steps(n_tiles):
    """(global steps of the finish tree, whether its first step has absent partners): the steps
    s = P / 2 .. 256; only the first can miss partners (later ones have 2 s <= P / 2 < n_tiles)."""
    P = 1
    while P < n_tiles:
        P *= 2
    steps, s = 0, P // 2
    while s >= BS:
        steps, s = steps + 1, s // 2
    return steps, steps > 0 and n_tiles < P


def paths(call, d, nc, n_free, nq, n_k, with_grad=False):
    """The names of every path a call takes, from its sizes alone.  call: 'load_plan'
    (stk_load_plan_create: the volumes), 'load' (stk_load_columns: shares and gather), 'points'
    (stk_load_points / stk_err_points), 'err_plan' (stk_err_plan_create: the geometry), 'err'
    (stk_err_element: cells and finish)."""
    n_tiles = (nc + BS - 1) // BS
    tiles = (['full tile'] if nc >= BS else []) + (['tail tile'] if nc % BS else [])
    out = []
    if call == 'load_plan':
        out.append('volume<%d>' % d)
        if nc > FLAT:
            out.append('volume<%d> second trip' % d)
    elif call == 'load':
        out += ['shares<%d> %s' % (d, t) for t in tiles]
        if n_tiles > SHARES_CAP:
            out.append('shares<%d> second trip' % d)
        if nq == 16 and n_k == 16:
            out.append('shares<%d> nq = 16, n_k = 16' % d)
        out.append('gather')
        if n_free > FLAT:
            out.append('gather second trip')
    elif call == 'points':
        out.append('points<%d>' % d)
        if nc * nq > FLAT:
            out.append('points<%d> second trip' % d)
    elif call == 'err_plan':
        out.append('geometry<%d>' % d)
        if nc > FLAT:
            out.append('geometry<%d> second trip' % d)
    elif call == 'err':
        kind = 'err_cells<%d, %s>' % (d, 'grad' if with_grad else 'plain')
        out += ['%s %s' % (kind, t) for t in tiles]
        if n_tiles > GRID_CAP:
            out.append('%s second trip' % kind)
        if nq == 16 and n_k == 16 and with_grad:
            out.append('%s nq = 16, n_k = 16' % kind)
        steps, absent = finish_steps(n_tiles)
        if steps == 0:
            out.append('err_finish LDS only')
        else:
            out.append('err_finish %d global step%s, %s' % (steps, 's' if steps > 1 else '',
                                                           'absent partners' if absent else 'every partner present'))
    else:
        raise ValueError(call)
    return out


# every path the classifier knows and the GPU file has to reach
EXPECTED_PATHS = (
    ['volume<%d>' % d for d in (2, 3)] + ['volume<2> second trip']
    + ['shares<%d> %s' % (d, t) for d in (2, 3) for t in ('full tile', 'tail tile')]
    + ['shares<2> second trip'] + ['shares<%d> nq = 16, n_k = 16' % d for d in (2, 3)]
    + ['gather', 'gather second trip']
    + ['points<%d>' % d for d in (2, 3)] + ['points<2> second trip']
    + ['geometry<%d>' % d for d in (2, 3)] + ['geometry<2> second trip']
    + ['err_cells<%d, %s> %s' % (d, g, t) for d in (2, 3) for g in ('grad', 'plain') for t in ('full tile', 'tail tile')]
    + ['err_cells<2, grad> second trip'] + ['err_cells<%d, grad> nq = 16, n_k = 16' % d for d in (2, 3)]
    + ['err_finish LDS only', 'err_finish 1 global step, absent partners', 'err_finish 1 global step, every partner present',
       'err_finish 2 global steps, absent partners', 'err_finish 5 global steps, absent partners'])


# ---- what the tests share -------------------------------------------------------------------------------------
def same_bits(a, b):
    """Equal doubles: array_equal, NaN-aware, and the same sign wherever the value is no NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
        return False
    ok = ~np.isnan(a)
    return bool(np.array_equal(np.signbit(a[ok]), np.signbit(b[ok])))


def random_rule(rng, nq, d):
    """A seeded rule without symmetry: positive weights and barycentric points that sum to 1."""
    ql = rng.rand(nq, d + 1) + 0.05
    ql /= ql.sum(axis=1, keepdims=True)
    qw = rng.rand(nq) + 0.1
    return qw / qw.sum(), np.ascontiguousarray(ql)


def _longdouble_load(mesh, qw, ql, f, coef):
    """(want, magnitude, incident cells) of the pair sum_k coef[k][a] L_k in np.longdouble
    and the same sums over absolute values."""
    from source.assembly import _simplex_volumes, free_dofs
    ld = np.longdouble
    c, fd = mesh.cells, free_dofs(mesh)
    vol = _simplex_volumes(mesh).astype(ld)

    def run(f, qw, ql, coef):
        out = np.zeros((len(fd), 2), dtype=ld)
        for k in range(f.shape[0]):
            loc = np.matmul(f[k].astype(ld) * qw.astype(ld), ql.astype(ld)) * vol[:, None]
            vec = np.zeros(mesh.nv, dtype=ld)
            np.add.at(vec, c.reshape(-1), loc.reshape(-1))
            out += coef[k].astype(ld)[None, :] * vec[fd][:, None]
        return out

    incident = np.bincount(c.reshape(-1), minlength=mesh.nv)[fd]
    return run(f, qw, ql, coef), np.asarray(run(np.abs(f), np.abs(qw), np.abs(ql), np.abs(coef)), dtype=np.float64), incident


def _mesh(problem, J):
    from source.problem import problem_helper
    return problem_helper(problem, J_space=J, J_time=1)[0]


U53 = 2.0**-53
RULE_3 = (np.array([1 / 3, 1 / 3, 1 / 3]), np.array([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3]]))


def rule_2d(nq):
    """The centroid, the three-point rule of degree 2, Dunavant's 6 points, and 16 seeded points."""
    from source.assembly import _QL, _QW
    if nq == 1:
        return np.array([1.0]), np.array([[1 / 3, 1 / 3, 1 / 3]])
    if nq == 3:
        return RULE_3
    if nq == 6:
        return np.asarray(_QW, dtype=np.float64), np.asarray(_QL, dtype=np.float64)
    return random_rule(np.random.RandomState(nq), nq, 2)


# ---- 1. the 2-D load against libstk's host routines, bit for bit ----------------------------------------------
HOST_MESHES_2D = {
    'square1': lambda: _mesh('square', 1), 'square2': lambda: _mesh('square', 2), 'square4': lambda: _mesh('square', 4),
    'lshape_jitter3': lambda: _mesh('lshape_jitter', 3), 'grid187': lambda: grid_mesh(187, 187, seed=5),  # 69 938 cells
}


def _host_points_2d(mesh, ql):
    from source import _lib
    pts = np.ascontiguousarray(mesh.points, dtype=np.float64)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int64)
    ql = np.ascontiguousarray(ql)
    qx, qy = np.empty((len(cells), len(ql))), np.empty((len(cells), len(ql)))
    _lib.check(_lib.lib().stk_p1_load_points_2d(mesh.nv, len(cells), pts.ctypes.data, cells.ctypes.data, len(ql),
                                                ql.ctypes.data, qx.ctypes.data, qy.ctypes.data))
    return qx, qy


def _host_sum_2d(mesh, qw, ql, f):
    from source import _lib
    pts = np.ascontiguousarray(mesh.points, dtype=np.float64)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int64)
    qw, ql, f = np.ascontiguousarray(qw), np.ascontiguousarray(ql), np.ascontiguousarray(f)
    vec = np.empty(mesh.nv)
    _lib.check(_lib.lib().stk_p1_load_sum_2d(mesh.nv, len(cells), pts.ctypes.data, cells.ctypes.data, len(qw),
                                             qw.ctypes.data, ql.ctypes.data, f.ctypes.data, vec.ctypes.data))
    return vec


@pytest.mark.parametrize('name', sorted(HOST_MESHES_2D))
def test_load_2d_equals_the_host_routines(name):
    """stk_p1_load_points_2d and stk_p1_load_sum_2d (host threads, no GPU) give the doubles of
    the restatement: the points, and with one time point and the coefficients (1, -1) the
    load vector itself and its negative."""
    mesh = HOST_MESHES_2D[name]()
    fd, _ = free_rows(mesh)
    rng = np.random.RandomState(len(name))
    for nq in (1, 3, 6, 16):
        qw, ql = rule_2d(nq)
        qx, qy = _host_points_2d(mesh, ql)
        pts = quadrature_points(mesh.points, mesh.cells, ql)
        assert same_bits(pts[0], qx) and same_bits(pts[1], qy), (name, nq)
        f = rng.randn(1, len(mesh.cells), nq)
        want = _host_sum_2d(mesh, qw, ql, f[0])[fd]
        got = load_pair(mesh, qw, ql, f, np.array([[1.0, -1.0]]))
        assert same_bits(got[:, 0], want) and same_bits(got[:, 1], -want), (name, nq)
        assert np.all(want != 0.0)


def test_grid_mesh_is_what_it_says():
    mesh = grid_mesh(7, 5, seed=1)
    assert mesh.points.shape == (48, 2) and mesh.cells.shape == (70, 3) and mesh.nv == 48
    _, _, det = simplex_of(mesh.points, mesh.cells)
    assert (det > 0).sum() == 35 and (det < 0).sum() == 35  # both orientations
    vol = volume(det, 2)
    assert len(np.unique(vol)) == len(vol)  # no two areas equal
    assert abs(math.fsum(vol) - 7.0 / 5.0) <= 1e-14  # the cells cover the rectangle once
    assert mesh.boundary.sum() == 2 * (7 + 5) and np.bincount(mesh.cells.reshape(-1)).max() <= 8
    big = grid_mesh(64, 64)
    count = np.bincount(big.cells.reshape(-1), minlength=big.nv)
    assert count.max() == 8 and count.min() >= 1
    # every interior edge belongs to two cells: the triangulation is conforming
    edges = np.sort(np.concatenate([big.cells[:, [0, 1]], big.cells[:, [1, 2]], big.cells[:, [0, 2]]]), axis=1)
    _, times = np.unique(edges, axis=0, return_counts=True)
    assert set(times.tolist()) == {1, 2} and (times == 1).sum() == 4 * 64
    assert not grid_mesh(3, 3, all_free=True).boundary.any()
    slot, present = incidence(big.cells, big.nv, np.arange(big.nv))
    assert slot.shape[1] == 8 and np.array_equal(present.sum(axis=1), count)
    for r in range(1, 8):  # ascending slots, each naming its vertex
        both = present[:, r]
        assert np.all(slot[both, r] > slot[both, r - 1])
    assert np.array_equal(big.cells.reshape(-1)[slot[present]], np.nonzero(present)[0])


# ---- 2. the 3-D load against the longdouble sum ------------------------------------------------------------------
@pytest.mark.parametrize('J', [1, 2])
def test_load_3d_against_the_longdouble_sum(J):
    """Keast's 11 points on the cube: within (nq + n_k + incident cells + 2) 2^-53 sum |terms|,
    the bound of tests/test_spacetime_load_gpu.py for the device."""
    from source.assembly import _QL3, _QW3
    mesh = _mesh('cube', J)
    rng = np.random.RandomState(17)
    for n_k in (1, 4):
        f, coef = rng.randn(n_k, len(mesh.cells), 11), rng.randn(n_k, 2)
        want, mag, incident = _longdouble_load(mesh, _QW3, _QL3, f, coef)
        got = load_pair(mesh, _QW3, _QL3, f, coef)
        bound = (11 + n_k + incident + 2)[:, None] * U53 * mag
        err = np.asarray(np.abs(got - want), dtype=np.float64)
        print('cube %d, n_k = %d: largest share of the bound used %.3f' % (J, n_k, float(np.max(err / bound))))
        assert np.all(err <= bound)
    # the volumes are those of the assembly
    from source.assembly import _simplex_volumes
    assert same_bits(volume(simplex_of(mesh.points, mesh.cells)[2], 3), _simplex_volumes(mesh))


# ---- 3. the error norms against the longdouble oracle ------------------------------------------------------------
ERR_MESHES = {
    'square0': lambda: _mesh('square', 0), 'square1': lambda: _mesh('square', 1), 'square2': lambda: _mesh('square', 2),
    'square4': lambda: _mesh('square', 4), 'lshape_jitter3': lambda: _mesh('lshape_jitter', 3),
    'cube1': lambda: _mesh('cube', 1), 'cube2': lambda: _mesh('cube', 2),
    'first255': lambda: first_cells(_mesh('square', 4), 255), 'first256': lambda: first_cells(_mesh('square', 4), 256),
    'first257': lambda: first_cells(_mesh('square', 4), 257), 'first513': lambda: first_cells(_mesh('square', 4), 513),
}


@pytest.mark.parametrize('name', sorted(ERR_MESHES))
def test_error_norms_within_the_oracles_bound(name):
    """The eleven meshes of tests/test_error_norms_gpu.py: each of the four numbers within the
    bound B of oracle_element, with gf; without it entries 1 and 3 are 0.0."""
    from test_error_norms_host import geometry, oracle_element
    mesh = ERR_MESHES[name]()
    geo = geometry(mesh)
    d, nc = geo['d'], len(mesh.cells)
    fd, _ = free_rows(mesh)
    rng = np.random.RandomState(nc)
    worst = 0.0
    for nq, n_k in ((1, 16), (3, 1), (6, 4), (11, 4), (16, 16)):
        qw, ql = random_rule(rng, nq, d)
        lo, hi = rng.randn(len(fd)), rng.randn(len(fd))
        w_lo, w_hi, c = rng.rand(n_k), rng.rand(n_k), rng.rand(n_k) + 0.1
        f, gf = rng.randn(n_k, nc, nq), rng.randn(n_k, d, nc, nq)
        full_lo, full_hi = np.zeros(mesh.nv), np.zeros(mesh.nv)
        full_lo[fd], full_hi[fd] = lo, hi
        want, bound = oracle_element(geo, qw, ql, w_lo, w_hi, c, f, gf, full_lo, full_hi)
        got = err_element(mesh, qw, ql, w_lo, w_hi, c, f, gf, lo, hi)
        for x in range(4):
            dev = abs(np.longdouble(got[x]) - want[x])
            worst = max(worst, float(dev / bound[x]))
            assert dev <= bound[x], (name, nq, n_k, x)
        plain = err_element(mesh, qw, ql, w_lo, w_hi, c, f, None, lo, hi)
        assert plain[0] == got[0] and plain[2] == got[2] and plain[1] == 0.0 and plain[3] == 0.0
    print('%s: largest |restatement - oracle| = %.4f B' % (name, worst))


def test_geometry_is_that_of_the_time_curves_contract():
    """cell_geometry of tests/test_time_curves_host.py is a third writing of p1_geometry_kernel:
    the same doubles; p1_gradients differs from it in the sign of a zero alone."""
    from test_time_curves_host import cell_geometry
    saw_zero = False
    for mesh in (_mesh('square', 3), _mesh('lshape_jitter', 3), _mesh('cube', 2), grid_mesh(9, 8)):
        vol, g = geometry_kernel(mesh.points, mesh.cells)
        vol2, g2 = cell_geometry(mesh.points, np.asarray(mesh.cells))
        assert same_bits(vol, vol2) and same_bits(g, g2)
        _, cof, det = simplex_of(mesh.points, mesh.cells)
        plain = gradients(cof, det)
        assert np.array_equal(plain, g) and same_bits(plain[:, 1:], g[:, 1:])
        zero = g[:, 0] == 0.0
        assert np.all(np.signbit(g[:, 0][zero])) and not np.any(np.signbit(plain[:, 0][zero]))
        saw_zero = saw_zero or bool(zero.any())
    assert saw_zero


# ---- 4. integrals known in closed form ------------------------------------------------------------------------------
def test_exact_integrals():
    """f = 1: the load vectors sum to the area (weights and barycentric coordinates sum to 1).
    A linear f is integrated exactly by the rule of degree 2: int_T f phi_a =
    |T| (f(p_a) + sum_b f(p_b)) / 12, within 32 roundings of the sum of the absolute terms.
    A P1 function against itself: error entries 0 and 1 are 0.0, exactly (integer data on a
    grid whose arithmetic is exact)."""
    mesh = grid_mesh(12, 9, seed=3, all_free=True)
    nc = len(mesh.cells)
    vol = volume(simplex_of(mesh.points, mesh.cells)[2], 2)
    area = math.fsum(vol)
    for nq in (1, 3, 6):
        qw, ql = rule_2d(nq)
        pair = load_pair(mesh, qw, ql, np.ones((1, nc, nq)), np.array([[1.0, 0.0]]))
        assert abs(math.fsum(pair[:, 0]) - area) <= 64 * U53 * area and abs(area - 12.0 / 9.0) <= 1e-14
        assert not pair[:, 1].any()
    qw, ql = RULE_3
    lin = lambda x, y: 0.5 + 2.0 * x - 3.0 * y
    pts = quadrature_points(mesh.points, mesh.cells, ql)
    pair = load_pair(mesh, qw, ql, lin(pts[0], pts[1])[None], np.array([[1.0, 1.0]]))
    fv = lin(mesh.points[:, 0], mesh.points[:, 1])[mesh.cells]  # (nc, 3)
    local = vol[:, None] * (fv + fv.sum(axis=1, keepdims=True)) / 12.0
    want = np.bincount(mesh.cells.reshape(-1), weights=local.reshape(-1), minlength=mesh.nv)
    mag = np.bincount(mesh.cells.reshape(-1), weights=np.abs(local).reshape(-1), minlength=mesh.nv)
    assert np.all(np.abs(pair[:, 0] - want) <= 32 * U53 * mag) and same_bits(pair[:, 0], pair[:, 1])
    # a P1 function against itself, linear in time: integers on an unjittered grid of width 1/8,
    # barycentric points that are dyadic -- every operation is exact, so the error is 0.0
    mesh = grid_mesh(8, 8, jitter=0.0, all_free=True)
    nc = len(mesh.cells)
    ql = np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]])
    qw = np.array([0.25, 0.5, 0.25])
    u = lambda t, x, y: (1.0 + 2.0 * t) * (3.0 + 8.0 * x - 16.0 * y)
    s = np.array([0.25, 0.75])
    pts = quadrature_points(mesh.points, mesh.cells, ql)
    f = np.stack([u(t, pts[0], pts[1]) for t in s])
    gf = np.stack([np.stack([np.full((nc, 3), (1.0 + 2.0 * t) * 8.0), np.full((nc, 3), (1.0 + 2.0 * t) * -16.0)]) for t in s])
    lo, hi = u(0.0, mesh.points[:, 0], mesh.points[:, 1]), u(1.0, mesh.points[:, 0], mesh.points[:, 1])
    got = err_element(mesh, qw, ql, 1.0 - s, s, np.array([0.5, 0.5]), f, gf, lo, hi)
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] > 0.0 and got[3] > 0.0
    # || grad u ||^2 over the unit square, by the rule in time: exact
    assert got[3] == 0.5 * (1.5**2 + 2.5**2) * (64.0 + 256.0)


# ---- 5. the trees and the classifier -----------------------------------------------------------------------------------
@pytest.mark.parametrize('n_tiles', [1, 2, 255, 256, 257, 511, 512, 513, 4096, 4097])
def test_finish_tree_on_integers_is_the_plain_sum(n_tiles):
    rng = np.random.RandomState(n_tiles)
    w = rng.randint(-1000, 1000, size=n_tiles).astype(np.float64)
    assert finish_tree(w) == float(int(w.astype(np.int64).sum()))
    # ... and with the tile trees in front: nc cells, the last tile a tail of 7
    nc = (n_tiles - 1) * BS + 7
    x = rng.randint(-1000, 1000, size=nc).astype(np.float64)
    assert finish_tree(tile_partials(x)) == float(int(x.astype(np.int64).sum()))
    # every partial is read exactly once: a single 1.0 anywhere gives 1.0
    for i in {0, n_tiles // 2, n_tiles - 1}:
        one = np.zeros(n_tiles)
        one[i] = 1.0
        assert finish_tree(one) == 1.0
    # the contract of the time curves has the same shape
    from test_time_curves_host import tile_tree
    y = rng.randn(nc)
    assert finish_tree(tile_partials(y)) == tile_tree(y)


def test_trees_have_the_shape_the_kernels_have():
    """On data whose sums round, the order shows: a literal walk over the steps of tree4 and of
    err_finish_kernel, lane by lane in Python, against the vectorised restatement."""
    rng = np.random.RandomState(2)
    red = rng.randn(BS)
    walk = red.copy()
    s = BS // 2
    while s >= 1:
        for i in range(s):
            walk[i] = walk[i] + walk[i + s]
        s //= 2
    assert tree256(red) == walk[0] and walk[0] != math.fsum(red)
    for n in (257, 300, 513, 1025):
        w = rng.randn(n)
        work = w.copy()
        P = 1 << (n - 1).bit_length()
        s = P // 2
        while s >= BS:
            for i in range(s):
                if i + s < n:
                    work[i] = work[i] + work[i + s]
            s //= 2
        lanes = np.array([work[t] if t < n else 0.0 for t in range(BS)])
        assert finish_tree(w) == tree256(lanes), n


def test_the_classifier_at_every_threshold():
    has = lambda call, word, **kw: any(word in p for p in paths(call, **dict(dict(d=2, nc=1000, n_free=10, nq=1, n_k=1), **kw)))
    for nc, tail, full in ((255, True, False), (256, False, True), (257, True, True)):
        assert has('load', 'tail tile', nc=nc) == tail and has('load', 'full tile', nc=nc) == full
        assert has('err', 'tail tile', nc=nc) == tail and has('err', 'full tile', nc=nc) == full
    # shares: 2048 tiles per trip
    cap = SHARES_CAP * BS
    assert [has('load', 'shares<2> second trip', nc=n) for n in (cap - 1, cap, cap + 1)] == [False, False, True]
    # the flat grids: 4096 workgroups of 256
    assert FLAT == 1048576
    for call, word, key in (('load', 'gather second trip', 'n_free'), ('load_plan', 'volume<2> second trip', 'nc'),
                            ('err_plan', 'geometry<2> second trip', 'nc'), ('points', 'points<2> second trip', 'nc')):
        assert [has(call, word, **{key: n}) for n in (FLAT - 1, FLAT, FLAT + 1)] == [False, False, True], call
    assert has('points', 'second trip', nc=65536, nq=16) is False and has('points', 'second trip', nc=65537, nq=16) is True
    # err_cells: 4096 tiles per trip
    assert [has('err', 'err_cells<2, plain> second trip', nc=n) for n in (FLAT - 1, FLAT, FLAT + 1)] == [False, False, True]
    assert has('err', 'err_cells<3, grad> full tile', d=3, with_grad=True)
    # the finish: LDS only up to 256 tiles
    assert [finish_steps(n) for n in (1, 255, 256)] == [(0, False)] * 3
    assert [finish_steps(n) for n in (257, 258, 511, 512)] == [(1, True), (1, True), (1, True), (1, False)]
    assert [finish_steps(n) for n in (513, 1023, 1024, 1025)] == [(2, True), (2, True), (2, False), (3, True)]
    assert finish_steps(4096) == (4, False) and finish_steps(4097) == (5, True) and finish_steps(4107) == (5, True)
    assert has('err', 'err_finish LDS only', nc=65536) and has('err', '1 global step, absent', nc=65537)
    assert has('err', '1 global step, absent', nc=65793) and has('err', '1 global step, every partner present', nc=131072)
    assert has('err', '2 global steps, absent', nc=131073) and has('err', '5 global steps, absent', nc=1051250)
    assert has('load', 'nq = 16, n_k = 16', nq=16, n_k=16) and not has('load', 'nq = 16', nq=16, n_k=4)
    # every name the classifier can give at the sizes of the GPU file is in the ledger's list
    for call in ('load_plan', 'load', 'points', 'err_plan', 'err'):
        for d in (2, 3):
            for nc, n_free in ((8, 1), (513, 200), (65793, 300), (131073, 300))[:4 if d == 2 else 2]:
                for grad in (False, True):
                    for p in paths(call, d, nc, n_free, 16, 16, grad):
                        assert p in EXPECTED_PATHS, p
    with pytest.raises(ValueError):
        paths('nothing', 2, 1, 1, 1, 1)
