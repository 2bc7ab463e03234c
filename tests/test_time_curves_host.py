"""The contract of the time curves (include/stk.h "time curves", source/time_curves.py) as a
plain NumPy loop -- the oracle of tests/test_time_curves_gpu.py, which compares the device
against it with array_equal -- checked here against dense NumPy and math.fsum that know
nothing of its trees; the host routine stk_curves_boundary_faces against a NumPy face count;
and the argument checks of the public call that need no device.

The independent checks use the absolute tolerance 1e-12 max(1, |Omega|): at most 3072
non-negative terms, each with a relative error of a few tens of 2^-53, in a pairwise tree
give about 50 * 2^-53 ~ 1e-14 of the sum; the cut cells add an absolute 2^-53 diam(Omega)
along the front; that leaves two orders of margin.  The data is scaled so that every
quantity compared is of the size of |Omega| or below, as the derivation assumes (nodal values
of size 0.05 on meshes down to h = 1/32: the H1 square, the largest of them, is then at most
10, and 50 * 2^-53 of it 6e-14).  Every test prints its gaps."""
import math
import types

import numpy as np
import pytest

from source.assembly import free_dofs, space_matrices
from source.problem import problem_helper
from source.time_curves import ALWAYS, FIELDS, THRESHOLD_FIELDS, boundary_faces, check_arguments, n_rows, rows
from test_history_host import same

BS = 256
HEAT, L2, H1, OUTFLOW, MEASURE, MOMENT = range(6)


def _mesh(problem, J):
    return problem_helper(problem, J_space=J, J_time=1)[0]


def first_cells(mesh, n):
    """The first n cells of a mesh as a mesh of their own (the ABI does not ask the cells to
    cover anything); the faces the cut exposes ARE boundary faces of it."""
    assert n <= len(mesh.cells)
    return types.SimpleNamespace(points=mesh.points, cells=np.ascontiguousarray(mesh.cells[:n]),
                                 boundary=mesh.boundary, nv=mesh.nv)


HOST_MESHES = {
    'square2': lambda: _mesh('square', 2), 'square3': lambda: _mesh('square', 3), 'square4': lambda: _mesh('square', 4),
    'lshape_jitter3': lambda: _mesh('lshape_jitter', 3), 'cube1': lambda: _mesh('cube', 1), 'cube2': lambda: _mesh('cube', 2),
}


def row_map(mesh):
    """row_of (nv,): the slab row of a vertex, -1 on the boundary."""
    fd = np.asarray(free_dofs(mesh), dtype=np.int64)
    row_of = np.full(mesh.nv, -1, dtype=np.int64)
    row_of[fd] = np.arange(len(fd))
    return row_of


# ---- the contract ---------------------------------------------------------------------------------
def numpy_boundary_faces(cells):
    """(nc,) uint8 by counting faces: bit a set iff the face opposite vertex a is in one cell."""
    cells = np.asarray(cells, dtype=np.int64)
    nc, nl = cells.shape
    count = {}
    for t in range(nc):
        for a in range(nl):
            key = tuple(sorted(np.delete(cells[t], a)))
            count[key] = count.get(key, 0) + 1
    mask = np.zeros(nc, dtype=np.uint8)
    for t in range(nc):
        for a in range(nl):
            if count[tuple(sorted(np.delete(cells[t], a)))] == 1:
                mask[t] |= 1 << a
    return mask


def cell_geometry(points, cells):
    """(|T| (nc,), grad lambda [nc][d + 1][d]): the doubles of csrc/p1_mesh.h, every operation
    one NumPy operation."""
    p, d = np.asarray(points, dtype=np.float64), cells.shape[1] - 1
    p0 = p[cells[:, 0]]
    e = [p[cells[:, r + 1]] - p0 for r in range(d)]
    if d == 2:
        cof = [[e[1][:, 1], -e[1][:, 0]], [-e[0][:, 1], e[0][:, 0]]]
        det = e[0][:, 0] * e[1][:, 1] - e[0][:, 1] * e[1][:, 0]
    else:
        cof = []
        for r in range(3):
            a, b = e[(r + 1) % 3], e[(r + 2) % 3]
            cof.append([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                        a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]])
        det = (e[0][:, 0] * cof[0][0] + e[0][:, 1] * cof[0][1]) + e[0][:, 2] * cof[0][2]
    vol = np.abs(det) / (2.0 if d == 2 else 6.0)
    grad = np.empty((len(cells), d + 1, d))
    with np.errstate(all='ignore'):
        for r in range(d):
            for j in range(d):
                grad[:, r + 1, j] = cof[r][j] / det
    for j in range(d):
        s = grad[:, 1, j] + grad[:, 2, j]
        if d == 3:
            s = s + grad[:, 3, j]
        grad[:, 0, j] = -s
    return vol, grad


def tile_tree(x):
    """The one sum shape of the contract for x (nc,): tiles of 256 in order, absent cells 0.0,
    x[j] + x[j + s] for s = 128 .. 1 in a tile; over the tiles partial i + partial i + s for
    s = P / 2 .. 1, P the power of two at or above the number of tiles, an absent partner adds
    nothing -- from 256 partials down with zeros in the absent places, as the device's LDS."""
    x = np.asarray(x, dtype=np.float64)
    nt = (len(x) + BS - 1) // BS
    a = np.zeros(nt * BS)
    a[:len(x)] = x
    a = a.reshape(nt, BS)
    s = BS // 2
    while s >= 1:
        a = a[:, :s] + a[:, s:2 * s]
        s //= 2
    w = a[:, 0].copy()
    P = 1
    while P < nt:
        P *= 2
    s = P // 2
    while s >= BS:
        k = max(min(s, nt - s), 0)
        w[:k] = w[:k] + w[s:s + k]
        s //= 2
    r = np.zeros(BS)
    r[:min(nt, BS)] = w[:BS]
    s = BS // 2
    while s >= 1:
        r = r[:s] + r[s:2 * s]
        s //= 2
    return r[0]


def _sub_volume(x0, x1, x2, x3=None):
    e0, e1 = x1 - x0, x2 - x0
    if x3 is None:
        return np.abs(e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]) / 2.0
    e2 = x3 - x0
    c0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    c1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    c2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.abs((e0[:, 0] * c0 + e0[:, 1] * c1) + e0[:, 2] * c2) / 6.0


def zone_of_cells(U, P, vol, theta):
    """(measure (nc,), moment (nc, d), lo (nc, d), hi (nc, d), n_above (nc,)) of the cells with
    nodal values U (nc, d + 1) and vertices P (nc, d + 1, d): the pieces of include/stk.h."""
    nc, nl = U.shape
    d = nl - 1
    measure, moment = np.zeros(nc), np.zeros((nc, d))
    lo, hi = np.full((nc, d), np.inf), np.full((nc, d), -np.inf)
    up = U > theta
    n = up.sum(axis=1)

    def widen(sel, pts):
        for x in pts:
            lo[sel] = np.where(x < lo[sel], x, lo[sel])
            hi[sel] = np.where(x > hi[sel], x, hi[sel])

    def piece(sel, xs):
        m = _sub_volume(*xs)
        measure[sel] = measure[sel] + m
        for j in range(d):
            s = (xs[0][:, j] + xs[1][:, j]) + xs[2][:, j]
            if d == 3:
                s = s + xs[3][:, j]
            moment[sel, j] = moment[sel, j] + (m * s) / float(d + 1)

    full = n == nl
    if full.any():
        measure[full] = vol[full]
        for j in range(d):
            s = P[full, 0, j] + P[full, 1, j]
            for a in range(2, nl):
                s = s + P[full, a, j]
            moment[full, j] = (vol[full] * s) / float(d + 1)
        widen(full, [P[full, a] for a in range(nl)])
    order = np.argsort(~up, axis=1, kind='stable')  # above ones first, each group ascending
    W = np.take_along_axis(U, order, axis=1)
    Q = P[np.arange(nc)[:, None], order]
    for k in range(1, nl):
        sel = n == k
        if not sel.any():
            continue
        w, q = W[sel], Q[sel]

        def cut(a, b):
            with np.errstate(all='ignore'):
                s = (w[:, a] - theta) / (w[:, a] - w[:, b])
                return q[:, a] + s[:, None] * (q[:, b] - q[:, a])

        if d == 2 and k == 1:
            xs = [q[:, 0], cut(0, 1), cut(0, 2)]
            pieces = [xs]
        elif d == 2:
            xs = [q[:, 0], q[:, 1], cut(1, 2), cut(0, 2)]
            pieces = [[xs[0], xs[1], xs[2]], [xs[0], xs[2], xs[3]]]
        elif k == 1:
            xs = [q[:, 0], cut(0, 1), cut(0, 2), cut(0, 3)]
            pieces = [xs]
        else:
            if k == 2:
                xs = [q[:, 0], cut(0, 2), cut(0, 3), q[:, 1], cut(1, 2), cut(1, 3)]
            else:
                xs = [q[:, 0], q[:, 1], q[:, 2], cut(0, 3), cut(1, 3), cut(2, 3)]
            pieces = [xs[0:4], xs[1:5], xs[2:6]]
        with np.errstate(all='ignore'):
            widen(sel, xs)
            for one in pieces:
                piece(sel, one)
    return measure, moment, lo, hi, n


def numpy_time_curves(points, cells, row_of, U, theta, faces=None):
    """The contract: the (7 + 3 d, n) table of the columns of U (M, n), the slab rows of the
    vertices with row_of >= 0 (row_of=None: U holds ALL vertices, none carries the Dirichlet
    zero).  One column at a time, vectorised over the cells; every operation is one NumPy
    operation on doubles, rounded on its own, and every sum over the mesh is tile_tree."""
    points, cells = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    U = np.asarray(U, dtype=np.float64)
    M, n_cols = U.shape
    nc, d = len(cells), cells.shape[1] - 1
    row_of = np.arange(len(points)) if row_of is None else np.asarray(row_of)
    vol, g = cell_geometry(points, cells)
    faces = numpy_boundary_faces(cells) if faces is None else faces
    P = points[cells]
    r = row_of[cells]
    at = rows(d)
    out = np.empty((n_rows(d), n_cols))
    for c in range(n_cols):
        col = U[:, c]
        Uc = np.where(r >= 0, col[np.maximum(r, 0)], 0.0)
        with np.errstate(all='ignore'):
            S, Q2 = Uc[:, 0] + Uc[:, 1], Uc[:, 0] * Uc[:, 0] + Uc[:, 1] * Uc[:, 1]
            for a in range(2, d + 1):
                S, Q2 = S + Uc[:, a], Q2 + Uc[:, a] * Uc[:, a]
            heat = (vol * S) / float(d + 1)
            l2 = (vol * (S * S + Q2)) / float((d + 1) * (d + 2))
            G = []
            for j in range(d):
                Gj = Uc[:, 0] * g[:, 0, j]
                for a in range(1, d + 1):
                    Gj = Gj + Uc[:, a] * g[:, a, j]
                G.append(Gj)
            GG = G[0] * G[0] + G[1] * G[1]
            if d == 3:
                GG = GG + G[2] * G[2]
            h1 = vol * GG
            flow = np.zeros(nc)
            for a in range(d + 1):
                dot = G[0] * g[:, a, 0] + G[1] * g[:, a, 1]
                if d == 3:
                    dot = dot + G[2] * g[:, a, 2]
                flow = np.where((faces >> a) & 1 == 1, flow + dot, flow)
            outflow = (float(d) * vol) * flow
            measure, moment, lo, hi, _ = zone_of_cells(Uc, P, vol, np.float64(theta))
            out[at['heat'], c], out[at['l2_sq'], c] = tile_tree(heat), tile_tree(l2)
            out[at['h1_sq'], c], out[at['outflow'], c] = tile_tree(h1), tile_tree(outflow)
            out[at['measure_above'], c] = tile_tree(measure)
            for j in range(d):
                out[at['moment_above'].start + j, c] = tile_tree(moment[:, j])
        valid = ~np.isnan(col)
        if valid.any():
            peak = col[valid].max()
            row = int(np.nonzero(valid & (col == peak))[0][0])
        else:
            peak, row = -np.inf, M
        out[at['peak'], c], out[at['peak_row'], c] = peak, float(row)
        blo, bhi = lo.min(axis=0), hi.max(axis=0)  # (no NaN gets in: x < lo is false for one)
        out[at['box_lo'], c] = np.where(blo == np.inf, np.nan, blo)
        out[at['box_hi'], c] = np.where(bhi == -np.inf, np.nan, bhi)
    return out


def planted_values(rng, M, n, theta):
    """randn columns (M, n) with the planted cases, by column c % 4: 1 -- integers around the
    rounded threshold (vertices exactly AT an integer theta, and ties for the peak); 2 -- the
    largest value 7.5 at every third row (ties for the peak); 3 -- values close around theta
    (many cut cells of every kind)."""
    v = rng.randn(M, n)
    for c in range(n):
        if c % 4 == 1:
            v[:, c] = np.round(theta) + rng.randint(-1, 2, size=M)
        elif c % 4 == 2:
            v[:, c] = np.where(np.arange(M) % 3 == 1, 7.5, v[:, c].clip(max=7.0))
        elif c % 4 == 3:
            v[:, c] = theta + 0.25 * v[:, c]
    return v


def dict_from_table(table, d, row_points, threshold):
    """The dict of the public call from the contract's table: what source.time_curves.
    curves_from_rows does with torch."""
    at = rows(d)
    out = {k: table[at[k]] for k in ('heat', 'l2_sq', 'h1_sq', 'outflow', 'peak')}
    out['peak_row'] = table[at['peak_row']].astype(np.int64)
    found = out['peak_row'] < len(row_points)  # (a column of nothing but NaN has no peak: row M, no point)
    out['peak_point'] = np.full((len(found), d), np.nan)
    out['peak_point'][found] = row_points[out['peak_row'][found]]
    if threshold is not None:
        measure, moment = table[at['measure_above']], table[at['moment_above']]
        out['measure_above'] = measure
        out['moment_above'] = moment.T
        with np.errstate(all='ignore'):
            out['centroid_above'] = np.where(measure == 0.0, np.nan, moment / measure).T
        out['box_lo'], out['box_hi'] = table[at['box_lo']].T, table[at['box_hi']].T
    return out


# ---- the contract against dense NumPy and math.fsum ---------------------------------------------------
def _tolerance(vol):
    return 1e-12 * max(1.0, math.fsum(vol))


def _cells_U(mesh, U):
    r = row_map(mesh)[mesh.cells]
    return np.where(r >= 0, U[np.maximum(r, 0)], 0.0)


@pytest.mark.parametrize('name', sorted(HOST_MESHES))
def test_sums_match_direct_formulas(name):
    mesh = HOST_MESHES[name]()
    cells, p = np.asarray(mesh.cells), np.asarray(mesh.points, dtype=np.float64)
    d, M = cells.shape[1] - 1, len(free_dofs(mesh))
    U = 0.05 * np.random.RandomState(11).randn(M, 2)
    got = numpy_time_curves(p, cells, row_map(mesh), U, np.inf)
    E = p[cells[:, 1:]] - p[cells[:, :1]]
    vol = np.abs(np.linalg.det(E)) / math.factorial(d)
    X = np.linalg.inv(E)  # column a = grad lambda_(a + 1)
    grad = np.concatenate([-X.sum(axis=2)[:, None, :], np.swapaxes(X, 1, 2)], axis=1)
    tol = _tolerance(vol)
    Mx, Ax = space_matrices(mesh)
    # boundary faces by counting, normals geometrically
    faces = {}
    for t in range(len(cells)):
        for a in range(d + 1):
            faces.setdefault(tuple(sorted(np.delete(cells[t], a))), []).append((t, a))
    for c in range(2):
        Uc = _cells_U(mesh, U[:, c])
        heat = math.fsum(vol * Uc.sum(axis=1) / (d + 1))
        l2 = math.fsum(vol / ((d + 1) * (d + 2)) * (Uc.sum(axis=1)**2 + (Uc**2).sum(axis=1)))
        G = np.einsum('ta,taj->tj', Uc, grad)
        h1 = math.fsum(vol * (G**2).sum(axis=1))
        outflow = []
        for key, owners in faces.items():
            if len(owners) != 1:
                continue
            t, a = owners[0]
            f = p[list(key)]
            if d == 2:
                edge = f[1] - f[0]
                normal = np.array([edge[1], -edge[0]])  # the edge rotated: its length is |F|
            else:
                normal = 0.5 * np.cross(f[1] - f[0], f[2] - f[0])
            if normal @ (p[cells[t, a]] - f[0]) > 0:  # away from the opposite vertex
                normal = -normal
            outflow.append(-(G[t] @ normal))
        outflow = math.fsum(outflow)
        gaps = {'heat': got[HEAT, c] - heat, 'l2_sq': got[L2, c] - l2, 'h1_sq': got[H1, c] - h1,
                'outflow': got[OUTFLOW, c] - outflow, 'h1_sq (U^T A U)': got[H1, c] - U[:, c] @ (Ax @ U[:, c]),
                'l2_sq (U^T M U)': got[L2, c] - U[:, c] @ (Mx @ U[:, c])}
        print(name, c, {k: '%.2e' % v for k, v in gaps.items()}, 'sizes %.2e %.2e %.2e %.2e' % tuple(got[:4, c]), 'tol %.1e' % tol)
        for key, gap in gaps.items():
            assert abs(gap) <= tol, (name, c, key, gap, tol)
        assert got[H1, c] > 0.0 and got[L2, c] > 0.0


@pytest.mark.parametrize('name,J', [('square', 2), ('square', 3), ('square', 4), ('cube', 1), ('cube', 2)])
def test_zone_of_a_linear_function_is_analytic(name, J):
    """u = x_0 on ALL vertices of the unit square / cube: {u > theta} = {x_0 > theta} has the
    measure 1 - theta and the centroid ((1 + theta) / 2, 1 / 2 [, 1 / 2]), the box [theta, 1] x
    [0, 1]^(d - 1)."""
    mesh = _mesh(name, J)
    p, cells = np.asarray(mesh.points, dtype=np.float64), np.asarray(mesh.cells)
    d = p.shape[1]
    assert np.array_equal(p.min(axis=0), np.zeros(d)) and np.array_equal(p.max(axis=0), np.ones(d))
    at = rows(d)
    faces = numpy_boundary_faces(cells)
    for theta in (0.3, 0.5, 1.0 / 3.0, 0.0625, 0.77):
        table = numpy_time_curves(p, cells, None, p[:, :1], theta, faces=faces)[:, 0]
        measure = table[at['measure_above']]
        centroid = table[at['moment_above']] / measure
        want = np.array([0.5 * (1.0 + theta)] + [0.5] * (d - 1))
        print(name, J, theta, 'measure gap %.2e, centroid gap %.2e' % (measure - (1.0 - theta), np.abs(centroid - want).max()))
        assert abs(measure - (1.0 - theta)) <= 1e-12
        assert np.abs(centroid - want).max() <= 1e-12
        assert np.abs(table[at['box_lo']] - np.array([theta] + [0.0] * (d - 1))).max() <= 1e-15
        assert np.array_equal(table[at['box_hi']], np.ones(d))


@pytest.mark.parametrize('name', sorted(HOST_MESHES))
def test_infinite_thresholds_and_the_complement(name):
    mesh = HOST_MESHES[name]()
    cells, p = np.asarray(mesh.cells), np.asarray(mesh.points, dtype=np.float64)
    d, M, row_of = cells.shape[1] - 1, len(free_dofs(mesh)), row_map(mesh)
    at = rows(d)
    faces = numpy_boundary_faces(cells)
    U = np.random.RandomState(12).randn(M, 2)
    vol, _ = cell_geometry(p, cells)
    low = numpy_time_curves(p, cells, row_of, U, -np.inf, faces=faces)
    high = numpy_time_curves(p, cells, row_of, U, np.inf, faces=faces)
    assert np.all(low[at['measure_above']] == tile_tree(vol))  # every cell whole: exactly the tree of |T|
    assert np.all(high[at['measure_above']] == 0.0) and np.all(high[at['moment_above']] == 0.0)
    assert np.isnan(high[at['box_lo']]).all() and np.isnan(high[at['box_hi']]).all()
    assert np.array_equal(low[at['box_lo']][:, 0], p[cells].reshape(-1, d).min(axis=0))
    assert np.array_equal(low[at['box_hi']][:, 0], p[cells].reshape(-1, d).max(axis=0))
    for q in (at['heat'], at['l2_sq'], at['h1_sq'], at['outflow'], at['peak'], at['peak_row']):
        assert same(low[q], high[q])
    # no vertex sits at theta (randn data; the boundary's 0.0 is not 0.3 either)
    theta, tol = 0.3, _tolerance(vol)
    above = numpy_time_curves(p, cells, row_of, U, theta, faces=faces)[at['measure_above']]
    below = numpy_time_curves(p, cells, row_of, -U, -theta, faces=faces)[at['measure_above']]
    print(name, 'above + below - |Omega| = %s, tol %.1e' % (above + below - math.fsum(vol), tol))
    assert np.all(above > 0.0) and np.all(below > 0.0)
    assert np.abs(above + below - math.fsum(vol)).max() <= tol


@pytest.mark.parametrize('name', ['square3', 'cube2'])
def test_planted_cases(name):
    mesh = HOST_MESHES[name]()
    cells, p = np.asarray(mesh.cells), np.asarray(mesh.points, dtype=np.float64)
    d, M, row_of = cells.shape[1] - 1, len(free_dofs(mesh)), row_map(mesh)
    at = rows(d)
    vol, _ = cell_geometry(p, cells)
    # a cell with all its vertices on the boundary: every term of it is 0 but |T| under -inf
    assert (row_of[cells] < 0).all(axis=1).any()
    seen = set()
    for theta in (0.3, 1.0):
        U = planted_values(np.random.RandomState(13), M, 8, theta)
        table = numpy_time_curves(p, cells, row_of, U, theta)
        for c in range(U.shape[1]):
            Uc = _cells_U(mesh, U[:, c])
            seen.update(np.unique((Uc > theta).sum(axis=1)).tolist())
            if theta == 1.0 and c % 4 == 1:
                assert np.count_nonzero(U[:, c] == theta) > M // 6  # vertices exactly AT theta
                # ... are not above: the zone is that of a threshold a little higher
                higher = numpy_time_curves(p, cells, row_of, U[:, c:c + 1], np.nextafter(theta, 2.0))
                assert abs(higher[at['measure_above'], 0] - table[at['measure_above'], c]) <= 1e-12
            # ties: the lowest row that has the peak
            assert table[at['peak'], c] == U[:, c].max() and table[at['peak_row'], c] == np.argmax(U[:, c])
            if c % 4 in (1, 2):
                assert np.count_nonzero(U[:, c] == U[:, c].max()) > 1
            assert 0.0 <= table[at['measure_above'], c] <= math.fsum(vol) + 1e-12
    assert seen == set(range(d + 2)), seen  # cells with 0, 1, .., d + 1 vertices above
    # NaN and inf in u: whatever comes, nothing raises, and the peak skips NaN
    U = np.random.RandomState(14).randn(M, 3)
    U[5, 0], U[7, 1], U[:, 2] = np.nan, np.inf, np.nan
    table = numpy_time_curves(p, cells, row_of, U, 0.3)
    assert table[at['peak'], 0] == np.nanmax(U[:, 0]) and table[at['peak'], 1] == np.inf and table[at['peak_row'], 1] == 7
    assert table[at['peak'], 2] == -np.inf and table[at['peak_row'], 2] == M


def test_dict_of_a_column_without_a_peak():
    """A column of nothing but NaN: peak_row = M, and the dict's peak_point is NaN there."""
    mesh = HOST_MESHES['square2']()
    p, row_of = np.asarray(mesh.points, dtype=np.float64), row_map(mesh)
    M = len(free_dofs(mesh))
    U = np.random.RandomState(17).randn(M, 3)
    U[:, 1] = np.nan
    table = numpy_time_curves(p, np.asarray(mesh.cells), row_of, U, 0.3)
    got = dict_from_table(table, 2, p[free_dofs(mesh)], 0.3)
    assert got['peak_row'].tolist() == [int(np.argmax(U[:, 0])), M, int(np.argmax(U[:, 2]))]
    assert np.isnan(got['peak_point'][1]).all() and got['peak'][1] == -np.inf
    assert np.array_equal(got['peak_point'][[0, 2]], p[free_dofs(mesh)][got['peak_row'][[0, 2]]])


def test_tile_tree_is_a_sum():
    rng = np.random.RandomState(15)
    for n in (1, 255, 256, 257, 513, 3072, 256 * 257 + 3, 256 * 600):
        x = rng.rand(n)
        assert abs(tile_tree(x) - math.fsum(x)) <= 1e-13 * n
    assert tile_tree(np.ones(1000)) == 1000.0


# ---- the host routine of the library ------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HOST_MESHES) + ['first255', 'first257'])
def test_boundary_faces_routine_against_the_face_count(name):
    mesh = first_cells(_mesh('square', 4), int(name[5:])) if name.startswith('first') else HOST_MESHES[name]()
    cells = np.asarray(mesh.cells, dtype=np.int64)
    got, want = boundary_faces(cells), numpy_boundary_faces(cells)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    d = cells.shape[1] - 1
    if name.startswith('first'):
        whole = numpy_boundary_faces(np.asarray(_mesh('square', 4).cells))[:len(cells)]
        assert np.all(want & whole == whole) and np.any(want != whole)  # the cut exposes more faces
    else:
        # a boundary face has all its vertices on the boundary
        bnd = np.asarray(mesh.boundary, dtype=bool)
        for t, a in zip(*np.nonzero((want[:, None] >> np.arange(d + 1)) & 1)):
            assert bnd[np.delete(cells[t], a)].all()
    # a permutation of the cells permutes the masks; one of a cell's vertices permutes its bits
    perm = np.random.RandomState(16).permutation(len(cells))
    assert np.array_equal(boundary_faces(cells[perm]), want[perm])
    rolled = np.ascontiguousarray(np.roll(cells, 1, axis=1))
    assert np.array_equal(boundary_faces(rolled), ((want << 1) | (want >> d)) & ((1 << (d + 1)) - 1))


def test_boundary_faces_routine_refuses():
    from source import _lib
    lib = _lib.lib()
    cells = np.array([[0, 1, 2]], dtype=np.int64)
    mask = np.full(1, 77, dtype=np.uint8)
    for args, text in (((4, 1, cells.ctypes.data, mask.ctypes.data), 'd = 4'),
                       ((2, 0, cells.ctypes.data, mask.ctypes.data), 'nc = 0'),
                       ((2, 1, None, mask.ctypes.data), 'cells is null'),
                       ((2, 1, cells.ctypes.data, None), 'mask is null'),
                       ((2, 1, np.array([[0, -1, 2]], dtype=np.int64).ctypes.data, mask.ctypes.data), 'vertex -1')):
        assert lib.stk_curves_boundary_faces(*args) != 0 and text in lib.stk_last_error().decode(), text
    assert mask[0] == 77
    assert lib.stk_curves_boundary_faces(2, 1, cells.ctypes.data, mask.ctypes.data) == 0 and mask[0] == 7
    assert lib.stk_curves_rows(2) == 13 == n_rows(2) and lib.stk_curves_rows(3) == 16 == n_rows(3)
    assert lib.stk_curves_rows(4) == 0


# ---- argument checks that need no device ------------------------------------------------------------------
def test_check_arguments():
    assert check_arguments(None) == (np.inf, ALWAYS)
    assert check_arguments(0.5) == (0.5, FIELDS) and check_arguments(1) == (1.0, FIELDS)
    assert check_arguments(-np.inf) == (-np.inf, FIELDS) and check_arguments(np.inf) == (np.inf, FIELDS)
    assert FIELDS == ALWAYS + THRESHOLD_FIELDS and len(FIELDS) == 12
    with pytest.raises(ValueError, match='threshold is NaN'):
        check_arguments(float('nan'))
    with pytest.raises(ValueError, match='None or a number'):
        check_arguments('hot')
    with pytest.raises(ValueError, match='None or a number'):
        check_arguments([0.1, 0.2])  # one threshold per call


def test_the_public_call_checks_before_it_touches_anything():
    """source.time_curves.time_curves is the body of both drivers' time_curves(); with a
    heat of nothing it can only get as far as the checks."""
    from source.time_curves import time_curves
    with pytest.raises(ValueError, match='threshold is NaN'):
        time_curves(types.SimpleNamespace(), None, threshold=float('nan'))
