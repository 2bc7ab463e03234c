"""Sampling the trial space, the parts that need no GPU: the NumPy brute-force oracle the
GPU tests compare against (and its agreement with the written-out cross-product form the
kernels use), time_weights, raster, the bucket grid of libstk's host code through ctypes
and from a plain C program.

Tolerance of every VALUE comparison here and in tests/test_sampling_gpu.py:
1e-12 max|U|.  A value is a convex combination of 2 (d + 1) nodal values with
well-conditioned barycentric coordinates, so two correct evaluations differ by a few
units of rounding, 1e-16 max|U| (measured between the two NumPy forms below:
<= 3.7e-15 max|U|, the larger figures where np.linalg.inv meets the jittered cells); an
indexing mistake is O(1) on random nodal values."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO

VALUE_TOL = 1e-12
INSIDE = -1e-12
MESHES = [('square', 1), ('square', 3), ('lshape', 2), ('lshape_jitter', 3), ('cube', 1), ('cube', 2)]


@functools.lru_cache(maxsize=None)
def mesh_of(problem, J):
    from source.problem import problem_helper
    return problem_helper(problem, J_space=J, J_time=1)[0]


def edges_of(mesh):
    c = mesh.cells
    k = c.shape[1]
    e = np.concatenate([c[:, [a, b]] for a in range(k) for b in range(a + 1, k)])
    return np.unique(np.sort(e, axis=1), axis=0)


@functools.lru_cache(maxsize=None)
def point_sets(problem, J):
    """The point sets of the tests: 1000 seeded points in the bounding box stretched by
    10 % on every side, all vertices, all centroids, all edge midpoints."""
    mesh = mesh_of(problem, J)
    pts = mesh.points
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    rs = np.random.RandomState(11)
    sets = {'random': lo - 0.1 * (hi - lo) + 1.2 * (hi - lo) * rs.rand(1000, pts.shape[1]),
            'vertices': pts.copy(),
            'centroids': pts[mesh.cells].mean(axis=1),
            'midpoints': pts[edges_of(mesh)].mean(axis=1)}
    for v in sets.values():
        v.setflags(write=False)
    return sets


# ---- the oracle ------------------------------------------------------------------------
def _best(lam_of_chunk, n_p, d, chunk=256):
    cell, lam, low = np.empty(n_p, np.int64), np.empty((n_p, d + 1)), np.empty(n_p)
    for a in range(0, n_p, chunk):
        l = lam_of_chunk(slice(a, min(a + chunk, n_p)))  # (n, nc, d + 1)
        m = l.min(axis=2)
        best = np.argmax(m, axis=1)  # the first of equal maxima: the lowest index
        rows = np.arange(len(best))
        cell[a:a + chunk], lam[a:a + chunk], low[a:a + chunk] = best, l[rows, best], m[rows, best]
    return cell, lam, low


def numpy_locate(mesh, points):
    """(cell, lam, smallest coordinate) of every point: barycentric coordinates in EVERY
    cell from np.linalg.inv of the (d + 1) x (d + 1) vertex matrices, the cell with the
    largest minimum, the lowest index on ties."""
    pts, cells = mesh.points, mesh.cells
    d = pts.shape[1]
    A = np.ones((len(cells), d + 1, d + 1))
    A[:, 1:, :] = pts[cells].transpose(0, 2, 1)
    Ainv = np.linalg.inv(A)
    rhs = np.concatenate([np.ones((len(points), 1)), points], axis=1)
    return _best(lambda s: np.einsum('cij,nj->nci', Ainv, rhs[s]), len(points), d)


def cross_locate(mesh, points):
    """The same by the written-out signed-area / cofactor expressions of include/stk.h."""
    pts, cells = mesh.points, mesh.cells
    d = pts.shape[1]
    p0 = pts[cells[:, 0]]
    e = [pts[cells[:, r + 1]] - p0 for r in range(d)]

    def lam_of(s):
        q = points[s][:, None, :] - p0[None, :, :]  # (n, nc, d)
        if d == 2:
            det = e[0][:, 0] * e[1][:, 1] - e[0][:, 1] * e[1][:, 0]
            l1 = (q[..., 0] * e[1][:, 1] - q[..., 1] * e[1][:, 0]) / det
            l2 = (e[0][:, 0] * q[..., 1] - e[0][:, 1] * q[..., 0]) / det
            return np.stack([(1.0 - l1) - l2, l1, l2], axis=2)
        n = [np.cross(e[(r + 1) % 3], e[(r + 2) % 3]) for r in range(3)]
        det = (e[0][:, 0] * n[0][:, 0] + e[0][:, 1] * n[0][:, 1]) + e[0][:, 2] * n[0][:, 2]
        l = [((q[..., 0] * n[r][:, 0] + q[..., 1] * n[r][:, 1]) + q[..., 2] * n[r][:, 2]) / det for r in range(3)]
        return np.stack([((1.0 - l[0]) - l[1]) - l[2]] + l, axis=2)

    return _best(lam_of, len(points), d)


def time_rule(mesh_time, times):
    """e = min(floor(t / h), N - 2), s = t / h - e."""
    x = np.asarray(times, dtype=np.float64) / mesh_time.h
    e = np.minimum(np.floor(x), mesh_time.nv - 2).astype(np.int64)
    return e, x - e


def numpy_sample(mesh, U, times, points, located=None, mesh_time=None):
    """u_h(t_k, x_p) of the nodal values U (N, M) (time-major, free dofs in ascending
    vertex order), shape (n_k, n_p), NaN where a point is outside (its best smallest
    coordinate < -1e-12).  `located`: what numpy_locate (or cross_locate) returned for
    these points, to share it between tests."""
    from source.assembly import free_dofs
    from source.mesh import construct_interval
    U = np.asarray(U, dtype=np.float64)
    mesh_time = construct_interval(N=U.shape[0] - 1) if mesh_time is None else mesh_time
    cell, lam, low = numpy_locate(mesh, points) if located is None else located
    full = np.zeros((U.shape[0], mesh.nv))  # boundary vertices: 0
    full[:, free_dofs(mesh)] = U
    at_nodes = np.einsum('tpa,pa->tp', full[:, mesh.cells[cell]], lam)  # (N, n_p)
    e, s = time_rule(mesh_time, times)
    out = (1.0 - s)[:, None] * at_nodes[e] + s[:, None] * at_nodes[e + 1]
    out[:, low < INSIDE] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def oracle_located(problem, J, which):
    return numpy_locate(mesh_of(problem, J), point_sets(problem, J)[which])


@pytest.mark.parametrize('problem,J', [('square', 3), ('lshape', 2), ('lshape_jitter', 3)])
def test_oracle_agrees_with_the_cross_product_form(problem, J):
    from source.assembly import free_dofs
    mesh, sets = mesh_of(problem, J), point_sets(problem, J)
    rs = np.random.RandomState(5)
    N = 9
    U = rs.randn(N, len(free_dofs(mesh)))
    times = rs.rand(7)
    worst = 0.0
    for which, points in sets.items():
        a = numpy_sample(mesh, U, times, points, located=oracle_located(problem, J, which))
        b = numpy_sample(mesh, U, times, points, located=cross_locate(mesh, points))
        assert np.array_equal(np.isnan(a), np.isnan(b)), which
        if which != 'random':
            assert not np.isnan(a).any(), which
        ok = ~np.isnan(a)
        worst = max(worst, np.max(np.abs(a[ok] - b[ok])) / np.max(np.abs(U)))
    print('oracle against the cross-product form on %s J=%d: %.2e max|U|' % (problem, J, worst))
    assert worst <= VALUE_TOL


def test_oracle_reproduces_linear_functions():
    """A function linear in t and x is in the trial space: sampled exactly (the oracle is
    what every device test leans on)."""
    from source.assembly import free_dofs
    from source.mesh import construct_interval
    mesh = mesh_of('lshape_jitter', 3)
    mt = construct_interval(N=8)
    fd = free_dofs(mesh)
    f = lambda t, x: (1.0 + 2.0 * t) * (0.5 + x[..., 0] - 3.0 * x[..., 1])
    # boundary values are taken as 0 by the trial space: sample well inside, where every
    # vertex of the cell is free
    points = mesh.points[mesh.cells].mean(axis=1)
    points = points[np.all(~mesh.boundary[mesh.cells], axis=1)]
    U = f(mt.nodes[:, None], mesh.points[fd][None, :, :])
    times = np.random.RandomState(3).rand(6)
    # bilinear in (t, x): exact in x at every node, and linear in t between the nodes
    got = numpy_sample(mesh, U, times, points, mesh_time=mt)
    assert np.max(np.abs(got - f(times[:, None], points[None, :, :]))) <= 1e-13


# ---- time_weights and raster -----------------------------------------------------------
def test_time_weights():
    from source.mesh import construct_interval
    from source.sampling import time_weights
    mt = construct_interval(N=8, T=1)
    N = mt.nv
    rs = np.random.RandomState(2)
    times = np.concatenate([mt.nodes, [0.0, mt.T], 0.5 * (mt.nodes[1:] + mt.nodes[:-1]), rs.rand(40) * mt.T])
    cols, w = time_weights(mt, times, 0, N)
    assert cols.dtype == np.int32 and cols.shape == w.shape == (len(times), 2)
    assert np.all(w[:, 0] + w[:, 1] == 1.0) and np.all(w >= 0.0)
    e, s = time_rule(mt, times)
    assert np.array_equal(cols[:, 0], e) and np.array_equal(cols[:, 1], e + 1) and np.array_equal(w[:, 1], s)
    # node times: s == 0 -- except T, which is the end of the last element
    assert np.all(w[:N - 1, 1] == 0.0) and np.array_equal(cols[:N - 1, 0], np.arange(N - 1))
    assert tuple(cols[N - 1]) == (N - 2, N - 1) and tuple(w[N - 1]) == (0.0, 1.0)
    assert np.allclose(w[:, 0] * mt.nodes[cols[:, 0]] + w[:, 1] * mt.nodes[cols[:, 1]], times, rtol=0, atol=1e-15)
    for bad in ([-1e-9], [mt.T + 1e-9], [0.5, float('nan')], [float('inf')]):
        with pytest.raises(ValueError):
            time_weights(mt, bad, 0, N)


class _FakeComm:
    def __init__(self, rank, size):
        self.rank, self.size = rank, size

    def Get_rank(self):
        return self.rank

    def Get_size(self):
        return self.size


@pytest.mark.parametrize('N,size', [(5, 1), (5, 2), (5, 3), (5, 5), (9, 8)])
def test_every_term_has_exactly_one_owner(N, size):
    from source.mesh import construct_interval
    from source.mpi_vector import DofDistributionMPI
    from source.sampling import time_weights
    mt = construct_interval(N=N - 1)
    times = np.concatenate([mt.nodes, 0.5 * (mt.nodes[1:] + mt.nodes[:-1]), np.random.RandomState(N).rand(20)])
    e, s = time_rule(mt, times)
    owners = np.zeros((len(times), 2), dtype=np.int64)
    for rank in range(size):
        dd = DofDistributionMPI(_FakeComm(rank, size), N, 3)
        cols, w = time_weights(mt, times, dd.t_begin, dd.t_end)
        owned = cols >= 0
        owners += owned
        nodes = np.stack([e, e + 1], axis=1)
        assert np.array_equal(cols[owned], (nodes - dd.t_begin)[owned])
        assert np.all((cols < dd.t_end - dd.t_begin))
        assert np.array_equal(w[:, 1], s)  # the weights do not depend on the rank
    assert np.all(owners == 1)


def test_raster():
    from source.sampling import raster
    for problem, J, n in (('lshape', 2, 5), ('cube', 1, 3)):
        mesh = mesh_of(problem, J)
        r = raster(mesh, n)
        d = mesh.points.shape[1]
        assert r.shape == (n ** d, d)
        assert np.array_equal(r.min(axis=0), mesh.points.min(axis=0)) and np.array_equal(r.max(axis=0), mesh.points.max(axis=0))
        assert len(np.unique(r, axis=0)) == n ** d
        assert np.all(np.diff(r[:n, 0]) > 0) and np.all(r[:n, 1:] == r[0, 1:])  # first coordinate fastest


# ---- the bucket grid, host code of libstk through ctypes -------------------------------
def bin_index(grid, x):
    """Per-axis bins of coordinates x (..., d): the expression of include/stk.h."""
    t = np.floor((x - grid['lo']) * grid['inv_width'])
    return np.clip(t, 0, grid['bins'] - 1).astype(np.int64)


def check_grid(mesh, grid):
    pts, cells = mesh.points, mesh.cells
    nc, d = len(cells), pts.shape[1]
    bins, ptr, lst = grid['bins'], grid['bin_ptr'], grid['bin_cells']
    extent = (pts.max(axis=0) - pts.min(axis=0)).max()
    assert grid['widen'] == 1e-12 * extent
    assert np.all(bins == max(1, int(np.floor(nc ** (1.0 / d) + 0.5))))
    assert ptr[0] == 0 and ptr[-1] == len(lst) and np.all(np.diff(ptr) >= 0) and len(ptr) == np.prod(bins) + 1
    assert lst.min() >= 0 and lst.max() < nc
    flat = lambda b: sum(b[..., k] * int(np.prod(bins[:k])) for k in range(d))
    # ascending lists
    owner = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    same = owner[1:] == owner[:-1]
    assert np.all(lst[1:][same] > lst[:-1][same])
    member = set(zip(owner.tolist(), lst.tolist()))
    # every cell in the bin of its centroid and of each of its vertices
    corners = pts[cells]  # (nc, d + 1, d)
    for where in [corners.mean(axis=1)] + [corners[:, a] for a in range(d + 1)]:
        b = flat(bin_index(grid, where))
        assert all((int(bb), c) in member for c, bb in enumerate(b))
    # every listed cell's widened box touches its bin: per axis the bin's interval
    # [lo + i / inv_width, lo + (i + 1) / inv_width] meets [min - widen, max + widen]
    # (one unit of rounding of the bin edges allowed for)
    idx = np.stack([(owner // int(np.prod(bins[:k]))) % bins[k] for k in range(d)], axis=1)
    blo = grid['lo'] + idx / grid['inv_width']
    bhi = grid['lo'] + (idx + 1) / grid['inv_width']
    clo = corners.min(axis=1)[lst] - grid['widen']
    chi = corners.max(axis=1)[lst] + grid['widen']
    slack = 4 * np.finfo(float).eps * extent
    assert np.all(clo <= bhi + slack) and np.all(chi >= blo - slack)
    # ... and the lists are exactly the bins between the two corners' bins
    lo_b, hi_b = bin_index(grid, corners.min(axis=1) - grid['widen']), bin_index(grid, corners.max(axis=1) + grid['widen'])
    assert len(lst) == int(np.prod(hi_b - lo_b + 1, axis=1).sum())
    assert np.all(idx >= lo_b[lst]) and np.all(idx <= hi_b[lst])


@pytest.mark.parametrize('problem,J', MESHES)
def test_bucket_grid(problem, J):
    from source.sampling import bucket_grid
    mesh = mesh_of(problem, J)
    check_grid(mesh, bucket_grid(mesh))


def test_bucket_grid_does_not_depend_on_the_host_threads(monkeypatch):
    """Above 16 384 cells the grid is built on several threads, each owning a slab of
    bins: the same lists as on one."""
    from source.sampling import bucket_grid
    mesh = mesh_of('lshape_jitter', 5)
    assert len(mesh.cells) > 16384
    monkeypatch.setenv('STK_HOST_THREADS', '1')
    one = bucket_grid(mesh)
    monkeypatch.setenv('STK_HOST_THREADS', '7')
    many = bucket_grid(mesh)
    for key in one:
        assert np.array_equal(one[key], many[key]), key
    check_grid(mesh, many)


def test_bucket_grid_refuses_bad_meshes():
    import ctypes

    from source import _lib
    pts = np.array([[0., 0.], [1., 0.], [0., 1.]])
    grid = ctypes.c_void_p()
    for cells in (np.array([[0, 1, 3]], dtype=np.int64), np.array([[0, -1, 2]], dtype=np.int64)):
        assert _lib.lib().stk_sample_grid_build(2, 3, 1, pts.ctypes.data, cells.ctypes.data, ctypes.byref(grid)) != 0
    cells = np.array([[0, 1, 2]], dtype=np.int64)
    flat = np.zeros((3, 2))
    assert _lib.lib().stk_sample_grid_build(2, 3, 1, flat.ctypes.data, cells.ctypes.data, ctypes.byref(grid)) != 0
    assert b'extent' in _lib.lib().stk_last_error()


# ---- a host without Python ---------------------------------------------------------------
@pytest.mark.parametrize('side', [1, 4, 37])
def test_c_host_builds_the_grid(tmp_path, side):
    """tests/c_host/sample_host.c: stk_sample_grid_* from plain C on a sheared grid of
    2 side^2 triangles, the properties above checked inside the program; compiled and run
    the way tests/test_c_host.py handles setup_host.c.  No GPU is touched."""
    from test_c_host import _build
    exe = _build(str(tmp_path / 'sample_host'), os.path.join(REPO, 'tests', 'c_host', 'sample_host.c'))
    res = subprocess.run([exe, str(side)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'sample_host ok' in res.stdout, res.stdout + res.stderr
    assert '%d triangles' % (2 * side * side) in res.stdout


def test_library_and_package_agree():
    assert os.path.exists(os.path.join(PKG, 'csrc', 'sample.hip'))
    from source import _lib
    assert all(hasattr(_lib.lib(), name) for name in _lib.EXPORTED_SYMBOLS if name.startswith('stk_sample_'))
