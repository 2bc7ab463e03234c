"""Sampling along trajectories, the parts that need no GPU: the NumPy oracle
``numpy_sample_along`` the GPU tests compare against (u_h, its time derivative and its
gradient at paired (t_p, x_p)), its agreement with the written-out cross-product form of
the gradients of the barycentric coordinates (include/stk.h "sampling the trial space"),
the path of square_moving_source, and the .npz the drivers' --track_out writes.

Tolerances, here and in tests/test_sample_along_gpu.py, with h the time step and max|G| the
largest gradient coefficient of the oracle on the mesh:
    u     1e-12 max|U|            (tests/test_sampling_host.py says why)
    dt    1e-12 max|U| / h        (a difference of two such values over h)
    grad  1e-12 max|U| max|G|     (a combination of 2 (d + 1) nodal values with coefficients
                                   of size max|G|)
Measured on the CPU between the two NumPy forms below on the six meshes: coefficients
<= 1.1e-15 max|G|, gradients of random nodal values <= 5.6e-16 max|U| max|G| (the largest on
lshape_jitter J = 3, exactly 0 on the uniform meshes); an indexing or sign error is O(1)."""
import argparse
import functools

import numpy as np
import pytest

from test_sampling_host import INSIDE, MESHES, VALUE_TOL, mesh_of, numpy_locate, oracle_located, point_sets, time_rule

DERIV_TOL = 1e-12


# ---- the oracle ------------------------------------------------------------------------
def _vertex_inverses(mesh):
    pts, cells = mesh.points, mesh.cells
    d = pts.shape[1]
    A = np.ones((len(cells), d + 1, d + 1))
    A[:, 1:, :] = pts[cells].transpose(0, 2, 1)
    return np.linalg.inv(A)


@functools.lru_cache(maxsize=None)
def _inverses_of(problem, J):
    return _vertex_inverses(mesh_of(problem, J))


def inv_grad_coeffs(mesh, Ainv=None):
    """(nc, d + 1, d): the gradient of lambda_a is row a, columns 1: of the inverse of the
    (d + 1) x (d + 1) vertex matrix (lambda = Ainv (1, x))."""
    Ainv = _vertex_inverses(mesh) if Ainv is None else Ainv
    return Ainv[:, :, 1:]


def cross_grad_coeffs(mesh):
    """The same by the written-out expressions of include/stk.h."""
    pts, cells = mesh.points, mesh.cells
    d = pts.shape[1]
    p0 = pts[cells[:, 0]]
    e = [pts[cells[:, r + 1]] - p0 for r in range(d)]
    G = np.empty((len(cells), d + 1, d))
    if d == 2:
        det = e[0][:, 0] * e[1][:, 1] - e[0][:, 1] * e[1][:, 0]
        G[:, 1, 0], G[:, 1, 1] = e[1][:, 1] / det, (-e[1][:, 0]) / det
        G[:, 2, 0], G[:, 2, 1] = (-e[0][:, 1]) / det, e[0][:, 0] / det
        G[:, 0] = (0.0 - G[:, 1]) - G[:, 2]
    else:
        n = [np.cross(e[(r + 1) % 3], e[(r + 2) % 3]) for r in range(3)]
        det = (e[0][:, 0] * n[0][:, 0] + e[0][:, 1] * n[0][:, 1]) + e[0][:, 2] * n[0][:, 2]
        for r in range(3):
            G[:, r + 1] = n[r] / det[:, None]
        G[:, 0] = ((0.0 - G[:, 1]) - G[:, 2]) - G[:, 3]
    return G


def numpy_sample_along(mesh, U, times, points, cell=None, mesh_time=None, Ainv=None, coeffs=None):
    """u_h, d/dt u_h and grad u_h of the nodal values U (N, M) (time-major, free dofs in
    ascending vertex order) at the pairs (times[p], points[p]): dict with u (n_p,), dt (n_p,),
    grad (d, n_p), inside (n_p,) and max_G, everything from np.linalg.inv of the vertex
    matrices.  `cell`: the cell of every point (-1: outside) where the caller has located
    them -- the gradient is discontinuous across cells, so a point on a shared edge must be
    differentiated in the cell the code under test chose; default: numpy_locate's, outside
    where its best smallest coordinate is < -1e-12.  The time derivative is the element's
    (right-hand at an interior node, left-hand at T).  `coeffs`: other gradient
    coefficients (nc, d + 1, d) than the inverse's."""
    from source.assembly import free_dofs
    from source.mesh import construct_interval
    U = np.asarray(U, dtype=np.float64)
    points, times = np.asarray(points, dtype=np.float64), np.asarray(times, dtype=np.float64)
    mesh_time = construct_interval(N=U.shape[0] - 1) if mesh_time is None else mesh_time
    Ainv = _vertex_inverses(mesh) if Ainv is None else Ainv
    if cell is None:
        cell, _, low = numpy_locate(mesh, points)
        cell = np.where(low >= INSIDE, cell, -1)
    cell = np.asarray(cell, dtype=np.int64)
    inside = cell >= 0
    c = np.where(inside, cell, 0)
    n_p, d = len(points), points.shape[1]
    lam = np.einsum('pij,pj->pi', Ainv[c], np.concatenate([np.ones((n_p, 1)), points], axis=1))
    G = (inv_grad_coeffs(mesh, Ainv) if coeffs is None else coeffs)
    full = np.zeros((U.shape[0], mesh.nv))  # boundary vertices: 0
    full[:, free_dofs(mesh)] = U
    e, s = time_rule(mesh_time, times)
    verts = mesh.cells[c]  # (n_p, d + 1)
    V0, V1 = full[e[:, None], verts], full[(e + 1)[:, None], verts]
    S0, S1 = np.einsum('pa,pa->p', V0, lam), np.einsum('pa,pa->p', V1, lam)
    out = {'u': (1.0 - s) * S0 + s * S1, 'dt': (S1 - S0) / mesh_time.h,
           'grad': (1.0 - s) * np.einsum('pa,paj->jp', V0, G[c]) + s * np.einsum('pa,paj->jp', V1, G[c])}
    for v in out.values():
        v[..., ~inside] = np.nan
    out.update(inside=inside, max_G=float(np.max(np.abs(G))))
    return out


# ---- the oracle against the cross-product form -------------------------------------------
@pytest.mark.parametrize('problem,J', MESHES)
def test_oracle_agrees_with_the_cross_product_form(problem, J):
    from source.assembly import free_dofs
    mesh, sets = mesh_of(problem, J), point_sets(problem, J)
    a, b = inv_grad_coeffs(mesh, _inverses_of(problem, J)), cross_grad_coeffs(mesh)
    max_G = np.max(np.abs(a))
    coeff = np.max(np.abs(a - b)) / max_G
    # the coefficients of a cell sum to zero: the coordinates sum to one
    assert np.max(np.abs(b.sum(axis=1))) <= 1e-14 * max_G
    rs = np.random.RandomState(5)
    N = 9
    U = rs.randn(N, len(free_dofs(mesh)))
    worst = 0.0
    for which in ('random', 'centroids'):
        points = sets[which]
        cell, _, low = oracle_located(problem, J, which)
        cell = np.where(low >= INSIDE, cell, -1)
        times = rs.rand(len(points))
        one = numpy_sample_along(mesh, U, times, points, cell=cell, Ainv=_inverses_of(problem, J))
        two = numpy_sample_along(mesh, U, times, points, cell=cell, Ainv=_inverses_of(problem, J), coeffs=b)
        assert np.array_equal(np.isnan(one['grad']), np.isnan(two['grad']))
        ok = one['inside']
        assert ok.any() and np.array_equal(np.isnan(one['grad'][0]), ~ok)
        worst = max(worst, np.max(np.abs(one['grad'][:, ok] - two['grad'][:, ok])) / (np.max(np.abs(U)) * max_G))
    print('%s J=%d: coefficients differ by %.2e max|G|, gradients by %.2e max|U| max|G|' % (problem, J, coeff, worst))
    assert coeff <= DERIV_TOL and worst <= DERIV_TOL


def test_oracle_u_is_the_diagonal_of_the_block_oracle():
    from source.assembly import free_dofs
    from test_sampling_host import numpy_sample
    problem, J = 'lshape_jitter', 3
    mesh, points = mesh_of(problem, J), point_sets(problem, J)['random'][:200]
    rs = np.random.RandomState(6)
    U = rs.randn(9, len(free_dofs(mesh)))
    times = np.concatenate([[0.0, 1.0, 0.5, 0.125], rs.rand(196)])
    located = tuple(a[:200] for a in oracle_located(problem, J, 'random'))
    block = numpy_sample(mesh, U, times, points, located=located)
    got = numpy_sample_along(mesh, U, times, points)
    assert np.array_equal(np.isnan(got['u']), np.isnan(np.diagonal(block)))
    ok = got['inside']
    assert 0 < ok.sum() < 200
    assert np.max(np.abs(got['u'][ok] - np.diagonal(block)[ok])) <= VALUE_TOL * np.max(np.abs(U))


def test_oracle_reproduces_linear_functions():
    """a + b . x + c t is in the trial space where no vertex of the cell is on the boundary:
    the oracle returns b and c, also at the nodes and at T."""
    from source.assembly import free_dofs
    from source.mesh import construct_interval
    for problem, J in (('lshape_jitter', 3), ('cube', 2)):
        mesh = mesh_of(problem, J)
        d = mesh.points.shape[1]
        mt = construct_interval(N=8)
        b, c = np.array([1.0, -3.0, 0.7])[:d], 2.5
        f = lambda t, x: 0.5 + x @ b + c * t
        interior = np.all(~mesh.boundary[mesh.cells], axis=1)
        points = mesh.points[mesh.cells].mean(axis=1)[interior]
        cell = np.flatnonzero(interior)
        assert len(points) > 0
        U = f(mt.nodes[:, None], mesh.points[free_dofs(mesh)][None, :, :])
        times = np.resize(np.concatenate([mt.nodes, np.random.RandomState(3).rand(6)]), len(points))
        got = numpy_sample_along(mesh, U, times, points, cell=cell, mesh_time=mt)
        assert np.max(np.abs(got['u'] - f(times, points))) <= 1e-13
        assert np.max(np.abs(got['dt'] - c)) <= 1e-12 * np.max(np.abs(U)) / mt.h
        assert np.max(np.abs(got['grad'] - b[:, None])) <= 1e-12 * np.max(np.abs(U)) * got['max_G']


# ---- fields -------------------------------------------------------------------------------
def test_field_mask():
    from source.sampling import FIELDS, field_mask
    assert FIELDS == ('u', 'dt', 'grad')
    assert field_mask('u') == 1 and field_mask(('dt',)) == 2 and field_mask(['grad']) == 4
    assert field_mask(('grad', 'u')) == 5 and field_mask(('u', 'dt', 'grad', 'u')) == 7
    for bad in ((), ('v',), 'laplace', ('u', 'hessian')):
        with pytest.raises(ValueError):
            field_mask(bad)


# ---- the path of the moving source ---------------------------------------------------------
def test_moving_source_has_a_path():
    import torch
    from source.problem import problem_helper
    data = problem_helper('square_moving_source', J_space=2, J_time=2)[3]
    path = data['path']
    t = np.linspace(0.0, 1.0, 9)
    c = path(t)
    assert c.shape == (9, 2) and c.dtype == np.float64
    assert np.array_equal(c[:, 0], 0.5 + 0.25 * np.cos(2.0 * np.pi * t))
    assert np.array_equal(c[:, 1], 0.5 + 0.25 * np.sin(2.0 * np.pi * t))
    assert np.allclose(np.hypot(c[:, 0] - 0.5, c[:, 1] - 0.5), 0.25, rtol=0, atol=1e-15)
    # it is the centre of the source: g is 1 there and smaller everywhere else
    g = data['g'][0]
    assert np.array_equal(g(t, c[:, 0], c[:, 1]), np.ones(9))
    assert np.all(g(t, c[:, 0] + 0.01, c[:, 1]) < 1.0)
    ct = path(torch.from_numpy(t))
    assert tuple(ct.shape) == (9, 2) and np.allclose(ct.numpy(), c, rtol=0, atol=1e-15)
    for other in ('square', 'square_forced', 'cube_nonseparable'):
        assert 'path' not in problem_helper(other, J_space=1, J_time=1)[3]


# ---- --track_out on a stubbed sample_along ---------------------------------------------------
class _StubHeat:
    def __init__(self, path):
        import torch
        from source.mesh import construct_interval
        self.path, self._sample_meshes, self.calls, self.torch = path, (None, construct_interval(N=4)), [], torch

    def sample_along(self, u, times, points, fields=('u',)):
        t = self.torch
        self.calls.append((u, np.array(times), np.array(points), tuple(fields)))
        K = len(times)
        return {'u': t.arange(K, dtype=t.float64), 'dt': -t.arange(K, dtype=t.float64),
                'grad': t.arange(2 * K, dtype=t.float64).reshape(2, K), 'inside': t.arange(K) != 1}


def test_track_options_and_the_file(tmp_path):
    from source import driver
    from source.problem import problem_helper
    assert [flag for flag, _, _, _ in driver.TRACK_OPTIONS] == ['track_out', 'track_points']
    assert not {f for f, _, _, _ in driver.TRACK_OPTIONS} & {f for f, _, _, _ in driver.SAMPLE_OPTIONS}
    assert dict((f, d) for f, _, d, _ in driver.TRACK_OPTIONS) == {'track_out': None, 'track_points': 1025}
    args, tracking = driver.take_options(argparse.Namespace(J_time=2, track_out=None, track_points=1025), driver.TRACK_OPTIONS,
                                         ('track_out',))
    assert tracking is None and vars(args) == {'J_time': 2}
    out = str(tmp_path / 'track.npz')
    args, tracking = driver.take_options(argparse.Namespace(J_time=2, track_out=out, track_points=7), driver.TRACK_OPTIONS,
                                         ('track_out',))
    assert vars(args) == {'J_time': 2} and tracking.track_out == out and tracking.track_points == 7

    path = problem_helper('square_moving_source', J_space=1, J_time=1)[3]['path']
    heat = _StubHeat(path)
    driver.write_track(heat, 'the solution', tracking)
    (u, times, points, fields), = heat.calls
    assert u == 'the solution' and set(fields) == {'u', 'dt', 'grad'}
    assert np.array_equal(times, np.linspace(0.0, 1.0, 7)) and np.array_equal(points, path(times))
    data = np.load(out)
    assert sorted(data.files) == ['dt', 'grad', 'inside', 'points', 'times', 'u']
    assert data['times'].shape == (7,) and data['points'].shape == (7, 2) and data['inside'].shape == (7,)
    assert data['u'].shape == (7,) and data['dt'].shape == (7,) and data['grad'].shape == (2, 7)
    assert data['inside'].dtype == bool and np.array_equal(data['inside'], np.arange(7) != 1)
    assert np.array_equal(data['times'], times) and np.array_equal(data['points'], points)
    assert np.array_equal(data['u'], np.arange(7.0)) and np.array_equal(data['dt'], -np.arange(7.0))
    assert np.array_equal(data['grad'], np.arange(14.0).reshape(2, 7))
    # another rank computes with the others and writes nothing
    other = str(tmp_path / 'other.npz')
    driver.write_track(heat, 'the solution', argparse.Namespace(track_out=other, track_points=3), rank=1)
    assert len(heat.calls) == 2 and not (tmp_path / 'other.npz').exists()
    # a problem without a path says so
    with pytest.raises(SystemExit) as err:
        driver.write_track(_StubHeat(None), 'the solution', tracking)
    assert 'no path' in str(err.value)


def test_library_declares_the_pair_calls():
    from source import _lib
    assert {'stk_sample_pairs', 'stk_sample_grad_coeffs'} <= set(_lib.EXPORTED_SYMBOLS)
    assert all(hasattr(_lib.lib(), name) for name in ('stk_sample_pairs', 'stk_sample_grad_coeffs'))
