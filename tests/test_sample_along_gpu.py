"""Sampling along trajectories on the device (stk_sample_pairs, stk_sample_grad_coeffs;
source/sampling.py evaluate_pairs, evaluate(field=...); sample_along of both solvers)
against the NumPy oracle of tests/test_sample_along_host.py: values, the diagonal of the
block bit for bit, a rank's view of a split slab, independence of the rank count,
reproduction of linear functions, convergence to the exact solution and the drivers.

Tolerances (tests/test_sample_along_host.py says why): u 1e-12 max|U|, dt 1e-12 max|U| / h,
grad 1e-12 max|U| max|G|."""
import functools
import threading

import numpy as np
import pytest
import torch

from test_sample_along_host import DERIV_TOL, _inverses_of, numpy_sample_along
from test_sampling_gpu import BAND, _slab, _times, all_points, plan_of
from test_sampling_host import INSIDE, MESHES, VALUE_TOL, _FakeComm, mesh_of, point_sets

pytestmark = pytest.mark.gpu

ALL = ('u', 'dt', 'grad')
TOLS = {'u': VALUE_TOL, 'dt': DERIV_TOL, 'grad': DERIV_TOL}


def _scales(U, h, max_G):
    m = np.max(np.abs(U))
    return {'u': m, 'dt': m / h, 'grad': m * max_G}


def _host(fields):
    return {k: v.cpu().numpy() for k, v in fields.items()}


def _slab_of(U):
    """The vector of the nodal values U (N, M), the padding column of its slab NaN."""
    from source.linop import self_distribution
    from source.mpi_vector import KronVectorMPI
    N, M = U.shape
    buf = torch.full((M, N + (N & 1)), float('nan'), dtype=torch.float64, device='cuda')
    buf[:, :N] = torch.from_numpy(np.ascontiguousarray(U.T)).cuda()
    return KronVectorMPI.around(self_distribution(N, M), buf)


def _cycled_times(N, n_p):
    """0, T, every node, the midpoints, random ones, again and again."""
    return np.resize(_times(N, 2 * N + 131), n_p)


# ---- 1. values against the oracle ------------------------------------------------------------
@pytest.mark.parametrize('N', [2, 5, 9, 65])
@pytest.mark.parametrize('problem,J', MESHES)
def test_values_against_the_oracle(problem, J, N):
    mesh, plan = mesh_of(problem, J), plan_of(problem, J)
    d = mesh.points.shape[1]
    points, located_o = all_points(problem, J)
    n_p = len(points)
    loc = plan.locate(points)
    cell, inside = loc.cell.cpu().numpy(), loc.inside.cpu().numpy()
    inside_o, clear = located_o[2] >= INSIDE, np.abs(located_o[2]) >= BAND
    assert np.array_equal(inside[clear], inside_o[clear]) and 0 < inside.sum() < n_p
    vec, U = _slab(plan.n_free, N, seed=N + J)
    h = 1.0 / (N - 1)
    times = _cycled_times(N, n_p)
    assert {0.0, 1.0, 0.5 * h} <= set(times.tolist())
    Ainv = _inverses_of(problem, J)
    # the oracle differentiates in the cell the device chose (a point on an edge has two)
    want = numpy_sample_along(mesh, U, times, points, cell=cell, Ainv=Ainv)
    scales = _scales(U, h, want['max_G'])
    got = _host(plan.evaluate_pairs(vec, times, loc, fields=ALL))
    assert sorted(got) == ['dt', 'grad', 'u']
    worst = {}
    for f in ALL:
        assert got[f].shape == ((d, n_p) if f == 'grad' else (n_p,))
        # NaN exactly where the point is outside
        assert np.isnan(got[f][..., ~inside]).all() and not np.isnan(got[f][..., inside]).any()
        worst[f] = np.max(np.abs(got[f][..., inside] - want[f][..., inside])) / scales[f]
    # u against the oracle's own location too
    own = numpy_sample_along(mesh, U, times, points, Ainv=Ainv)
    both = inside & own['inside']
    worst['u (own cells)'] = np.max(np.abs(got['u'][both] - own['u'][both])) / scales['u']
    # every subset of the fields is those rows; times as a device tensor
    t_dev = torch.from_numpy(times.copy()).cuda()
    for fields in (('u',), ('dt',), ('grad',), ('u', 'grad'), ('grad', 'dt')):
        part = _host(plan.evaluate_pairs(vec, t_dev, loc, fields=fields))
        assert sorted(part) == sorted(fields)
        for f in fields:
            assert np.array_equal(part[f], got[f], equal_nan=True), (fields, f)
    # the block forms of the derivatives, on the same scales
    times_k = _times(N, 7)
    blocks = {'dt': plan.evaluate(vec, times_k, loc, field='dt').cpu().numpy(),
              'grad': plan.evaluate(vec, times_k, loc, field='grad').cpu().numpy()}
    assert blocks['dt'].shape == (7, n_p) and blocks['grad'].shape == (d, 7, n_p)
    for k, t in enumerate(times_k):
        row = numpy_sample_along(mesh, U, np.full(n_p, t), points, cell=cell, Ainv=Ainv)
        for f, g in (('dt', blocks['dt'][k]), ('grad', blocks['grad'][:, k])):
            assert np.isnan(g[..., ~inside]).all() and not np.isnan(g[..., inside]).any()
            key = 'block ' + f
            worst[key] = max(worst.get(key, 0.0), np.max(np.abs(g[..., inside] - row[f][..., inside])) / scales[f])
    print('%s J=%d N=%d: largest scaled differences %s' % (
        problem, J, N, ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))
    for key, value in worst.items():
        assert value <= TOLS[key.split()[-1] if key.startswith('block') else key.split()[0]], (key, value)


def test_times_outside_the_interval_give_nan():
    """NaN, a negative time and one beyond T: NaN in every field, decided on the device."""
    problem, J, N = 'square', 3, 9
    plan = plan_of(problem, J)
    points = point_sets(problem, J)['centroids'][:8]
    vec, U = _slab(plan.n_free, N, seed=2)
    times = np.array([0.0, float('nan'), -1e-9, 1.0, 1.0 + 1e-9, float('inf'), 0.3, -0.0])
    bad = np.array([False, True, True, False, True, True, False, False])
    got = _host(plan.evaluate_pairs(vec, times, plan.locate(points), fields=ALL))
    for f in ALL:
        assert np.array_equal(np.isnan(got[f]).reshape(-1, 8).any(axis=0), bad), f
        assert np.array_equal(np.isnan(got[f]).reshape(-1, 8).all(axis=0), bad), f
    with pytest.raises(ValueError):
        plan.evaluate_pairs(vec, times, plan.locate(points), fields=('laplace',))


# ---- 2. pairs are the diagonal of the block, bit for bit ---------------------------------------
@pytest.mark.parametrize('steps', [4, 8, 64])
@pytest.mark.parametrize('problem,J', [('lshape_jitter', 3), ('cube', 1)])
def test_pairs_are_the_diagonal_of_the_block(problem, J, steps):
    """N - 1 a power of two: t / h is exact, host and device weights are the same doubles."""
    N = steps + 1
    plan = plan_of(problem, J)
    vec, U = _slab(plan.n_free, N, seed=steps)
    for n_p in (1, 63, 64, 65, 255, 256, 257):
        points = point_sets(problem, J)['random'][:n_p]
        times = np.roll(_cycled_times(N, 300), n_p)[:n_p]
        loc = plan.locate(points)
        pairs = _host(plan.evaluate_pairs(vec, times, loc, fields=ALL))
        block_u = plan.evaluate(vec, times, loc).cpu().numpy()
        block_dt = plan.evaluate(vec, times, loc, field='dt').cpu().numpy()
        block_grad = plan.evaluate(vec, times, loc, field='grad').cpu().numpy()
        assert block_u.shape == block_dt.shape == block_grad.shape[1:] == (n_p, n_p)
        assert np.array_equal(pairs['u'], np.diagonal(block_u), equal_nan=True), n_p
        assert np.array_equal(pairs['dt'], np.diagonal(block_dt), equal_nan=True), n_p
        assert np.array_equal(pairs['grad'], np.diagonal(block_grad, axis1=1, axis2=2), equal_nan=True), n_p
        inside = loc.inside.cpu().numpy()
        assert np.array_equal(np.isnan(pairs['u']), ~inside)
        if n_p >= 63:
            assert 0 < inside.sum() < n_p and np.abs(pairs['grad'][:, inside]).max() > 0.1


# ---- 3. a rank's view -----------------------------------------------------------------------------
def test_a_ranks_view_and_absent_columns():
    """A split slab: columns that are "not on this rank" contribute exactly 0.0, are not read
    (the padding column is NaN) and the parts sum to the whole, bit for bit."""
    from source.mpi_vector import DofDistributionMPI, KronVectorMPI
    problem, J = 'lshape_jitter', 3
    plan = plan_of(problem, J)
    points = point_sets(problem, J)['random'][:300]
    loc = plan.locate(points)
    inside = loc.inside.cpu().numpy()
    assert 0 < inside.sum() < 300
    seen = set()
    for N, ranks in ((9, 3), (5, 5)):
        vec, U = _slab(plan.n_free, N, seed=1)
        times = _cycled_times(N, 300)
        whole = _host(plan.evaluate_pairs(vec, times, loc, fields=ALL))
        e = np.minimum(np.floor(times * (N - 1)), N - 2).astype(int)
        total = {f: np.zeros_like(whole[f]) for f in ALL}
        for rank in range(ranks):
            dd = DofDistributionMPI(_FakeComm(rank, ranks), N, plan.n_free)
            n_loc = dd.t_end - dd.t_begin
            buf = torch.full((plan.n_free, n_loc + (n_loc & 1)), float('nan'), dtype=torch.float64, device='cuda')
            buf[:, :n_loc] = vec.buf[:, dd.t_begin:dd.t_end]
            part = _host(plan.evaluate_pairs(KronVectorMPI.around(dd, buf), times, loc, fields=ALL))
            c0 = e - dd.t_begin
            if n_loc == 1:
                seen.add('a slab of one column')
            if np.any(c0 == n_loc - 1):
                seen.add('c0 on the last local column')
            if np.any(c0 == -1):
                seen.add('c0 = -1 with c1 = 0')
            for parity in (0, 1):
                if np.any((c0 >= 0) & (c0 + 1 < n_loc) & (c0 % 2 == parity)):
                    seen.add('both columns present, c0 %s' % ('even', 'odd')[parity])
            absent = (c0 + 1 < 0) | (c0 >= n_loc)
            for f in ALL:
                assert np.isnan(part[f][..., ~inside]).all() and not np.isnan(part[f][..., inside]).any()
                assert np.all(part[f][..., inside & absent] == 0.0)  # neither node on this rank
                total[f] += part[f]
        for f in ALL:
            assert np.array_equal(total[f][..., inside], whole[f][..., inside]), (N, f)
            assert np.isnan(total[f][..., ~inside]).all()
    assert seen == {'a slab of one column', 'c0 on the last local column', 'c0 = -1 with c1 = 0',
                    'both columns present, c0 even', 'both columns present, c0 odd'}, seen


def test_no_points_and_an_odd_leading_dimension():
    """n_p = 0 returns empty tensors; a slab whose rows are an odd number of doubles apart
    (only through the C ABI) takes the 8-byte loads everywhere and gives the same doubles."""
    from source import _lib
    for problem, J in (('lshape_jitter', 3), ('cube', 1)):
        plan = plan_of(problem, J)
        d, N = plan.d, 9
        vec, U = _slab(plan.n_free, N, seed=4)
        none = plan.evaluate_pairs(vec, np.zeros(0), plan.locate(np.zeros((0, d))), fields=ALL)
        assert tuple(none['u'].shape) == tuple(none['dt'].shape) == (0,) and tuple(none['grad'].shape) == (d, 0)
        assert tuple(plan.evaluate(vec, [0.5], plan.locate(np.zeros((0, d))), field='grad').shape) == (d, 1, 0)
        points = point_sets(problem, J)['random'][:257]
        times = _cycled_times(N, 257)
        loc = plan.locate(points)
        want = plan.evaluate_pairs(vec, times, loc, fields=ALL)
        tight = vec.buf[:, :N].contiguous()  # ld = 9
        t_dev = torch.from_numpy(times.copy()).cuda()
        rows = torch.empty((2 + d, 257), dtype=torch.float64, device='cuda')
        _lib.check(_lib.lib().stk_sample_pairs(_lib.stream(), plan._plan, 257, _lib.ptr(loc.cell), _lib.ptr(loc.lam),
                                               _lib.ptr(t_dev), 1.0 / (N - 1), N, 0, plan.n_free, N, N, _lib.ptr(tight), 7,
                                               257, _lib.ptr(rows)))
        rows = rows.cpu().numpy()
        assert np.array_equal(rows[0], want['u'].cpu().numpy(), equal_nan=True)
        assert np.array_equal(rows[1], want['dt'].cpu().numpy(), equal_nan=True)
        assert np.array_equal(rows[2:], want['grad'].cpu().numpy(), equal_nan=True)
        # what the library refuses
        for fields, ld in ((0, N), (8, N), (7, N - 1)):
            assert _lib.lib().stk_sample_pairs(_lib.stream(), plan._plan, 257, _lib.ptr(loc.cell), _lib.ptr(loc.lam),
                                               _lib.ptr(t_dev), 1.0 / (N - 1), N, 0, plan.n_free, N, ld, _lib.ptr(tight),
                                               fields, 257, _lib.ptr(torch.empty_like(want['u']))) != 0
        # stk_sample_grad_coeffs: the oracle's coefficients, NaN outside
        G = plan.grad_coeffs(loc).cpu().numpy()
        cell, inside = loc.cell.cpu().numpy(), loc.inside.cpu().numpy()
        assert G.shape == (d, 257, d + 1) and np.isnan(G[:, ~inside]).all()
        oracle = _inverses_of(problem, J)[:, :, 1:][cell[inside]]  # (n, d + 1, d)
        assert np.max(np.abs(G[:, inside] - oracle.transpose(2, 0, 1))) <= DERIV_TOL * np.max(np.abs(oracle))


@pytest.mark.parametrize('problem,J', [('square', 1), ('square', 2), ('lshape', 1), ('cube', 1)])
def test_grad_coeffs_are_the_gradients_of_the_assembly(problem, J):
    """At the centroid of every cell, stk_sample_grad_coeffs gives the doubles of
    assembly._simplex_geometry -- what the error norms and the stiffness matrix use -- and
    not merely close ones.  (array_equal does not tell -0.0 from +0.0: grad lambda_0 is
    ((0 - g_1) - g_2) [- g_3] here and -((g_1 + g_2) [+ g_3]) there.)"""
    from source.assembly import _simplex_geometry
    mesh, plan = mesh_of(problem, J), plan_of(problem, J)
    loc = plan.locate(point_sets(problem, J)['centroids'])
    assert np.array_equal(loc.cell.cpu().numpy(), np.arange(len(mesh.cells)))
    G = plan.grad_coeffs(loc).cpu().numpy()  # [j, cell, a]
    want = _simplex_geometry(mesh)[1]  # [cell, a, j]
    assert G.shape == want.transpose(2, 0, 1).shape and np.isfinite(want).all()
    assert np.array_equal(G, want.transpose(2, 0, 1))


# ---- 4. rank independence ----------------------------------------------------------------------------
_lock = threading.Lock()  # plan construction reads process-wide tuning keys


def _along_run(comm, J_time):
    import heateq_mpi as hm
    from source import driver
    from source.mpi_vector import KronVectorMPI
    with _lock:
        h = hm.HeatEquationMPI(J_space=3, J_time=J_time, problem='square_forced', comm=comm)
    assert h.sample_plan is None
    u = driver.seeded_vector(h, KronVectorMPI)  # the same global vector on every rank count
    nodes = np.arange(h.N) / (h.N - 1.0)
    times = np.resize(np.concatenate([nodes, 0.5 * (nodes[1:] + nodes[:-1]), np.random.RandomState(4).rand(9)]), 200)
    points = -0.02 + 1.04 * np.random.RandomState(8).rand(200, 2)
    out = _host(h.sample_along(u, times, points, fields=ALL))
    assert h.sample_plan is not None
    out['block dt'] = h.sample(u, times[:7], points, field='dt').cpu().numpy()
    out['block grad'] = h.sample(u, times[:7], points, field='grad').cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def _one_rank_along(J_time):
    from source.comm import Comm
    return _along_run(Comm(distributed=False), J_time)


@pytest.mark.parametrize('J_time,ranks', [(2, 2), (2, 3), (2, 5), (3, 8)])
def test_sample_along_does_not_depend_on_the_number_of_ranks(J_time, ranks):
    """Every node and every midpoint is a sample time: every rank boundary, and every
    element that straddles two ranks."""
    from thread_comm import run_ranks
    got = run_ranks(ranks, lambda comm: _along_run(comm, J_time))
    one = _one_rank_along(J_time)
    inside = one['inside']
    assert sorted(one) == ['block dt', 'block grad', 'dt', 'grad', 'inside', 'u']
    assert 0 < (~inside).sum() < 50 and inside.dtype == bool
    assert one['u'].shape == one['dt'].shape == (200,) and one['grad'].shape == (2, 200)
    assert one['block dt'].shape == (7, 200) and one['block grad'].shape == (2, 7, 200)
    for key in ('u', 'dt', 'grad', 'block dt', 'block grad'):
        assert np.array_equal(np.isnan(one[key]).reshape(-1, 200).any(axis=0), ~inside), key
        assert np.nanmax(np.abs(one[key])) > 0.1
    for rank in range(ranks):
        for key, value in one.items():
            assert np.array_equal(got[rank][key], value, equal_nan=True), (rank, key)


# ---- 5. linear reproduction ---------------------------------------------------------------------------
@pytest.mark.parametrize('problem,J', [('lshape_jitter', 3), ('square', 3), ('cube', 2)])
def test_linear_functions_are_reproduced(problem, J):
    """Nodal values of a + b . x + c t, sampled in cells without a boundary vertex: grad = b
    and dt = c.  A wrong orientation or sign of a gradient coefficient is O(1) here."""
    from source.assembly import free_dofs
    mesh, plan = mesh_of(problem, J), plan_of(problem, J)
    d, N = mesh.points.shape[1], 9
    h = 1.0 / (N - 1)
    b, c = np.array([1.0, -3.0, 0.7])[:d], 2.5
    f = lambda t, x: 0.5 + x @ b + c * t
    interior = np.all(~mesh.boundary[mesh.cells], axis=1)
    corners = mesh.points[mesh.cells[interior]]  # (n, d + 1, d)
    assert len(corners) > 0
    w = np.random.RandomState(9).dirichlet(np.ones(d + 1), size=len(corners))
    points = np.concatenate([corners.mean(axis=1), np.einsum('na,nak->nk', w, corners)])
    times = _cycled_times(N, len(points))
    U = f((np.arange(N) * h)[:, None], mesh.points[free_dofs(mesh)][None, :, :])
    got = _host(plan.evaluate_pairs(_slab_of(U), times, plan.locate(points), fields=ALL))
    max_G = np.max(np.abs(_inverses_of(problem, J)[:, :, 1:]))
    scales = _scales(U, h, max_G)
    errs = {'u': np.max(np.abs(got['u'] - f(times, points))), 'dt': np.max(np.abs(got['dt'] - c)),
            'grad': np.max(np.abs(got['grad'] - b[:, None]))}
    print('%s J=%d: %s' % (problem, J, ', '.join('%s %.2e' % (k, errs[k] / scales[k]) for k in ALL)))
    for k in ALL:
        assert errs[k] <= TOLS[k] * scales[k], (k, errs[k] / scales[k])


# ---- 6. end to end -----------------------------------------------------------------------------------------
# SciPy solve (tests/test_forcing_host.py::scipy_error's system) sampled with numpy_sample_along
CPU_ERRORS = {'u': {3: 2.682e-2, 4: 7.481e-3}, 'dt': {3: 1.028e-1, 4: 3.599e-2}, 'grad': {3: 9.499e-1, 4: 5.483e-1}}


@functools.lru_cache(maxsize=None)
def _along_errors(J):
    import heateq_mpi as hm
    from source.comm import Comm
    from source.problem import problem_helper
    h = hm.HeatEquationMPI(J_space=J, J_time=J, problem='square_forced', comm=Comm(distributed=False))
    u, _ = h.solve()
    rs = np.random.RandomState(7)
    q = rs.rand(500, 2)
    t = rs.rand(500)
    got = _host(h.sample_along(u, t, q, fields=ALL))
    assert got['inside'].all() and got['u'].shape == (500,) and got['grad'].shape == (2, 500)
    data = problem_helper('square_forced', J_space=J, J_time=J)[3]
    x, y = q[:, 0], q[:, 1]
    u_t = -np.exp(-t) * np.sin(np.pi * x) * np.sin(np.pi * y) + np.sin(2.0 * np.pi * x) * np.sin(np.pi * y)
    grad = np.stack([np.asarray(g) for g in data['exact_grad'](t, x, y)])
    return {'u': float(np.max(np.abs(got['u'] - data['exact'](t, x, y)))),
            'dt': float(np.max(np.abs(got['dt'] - u_t))),
            'grad': float(np.max(np.abs(got['grad'] - grad)))}


def test_sampled_fields_converge_to_the_exact_ones():
    """max over the 500 random (t_i, q_i) of tests/test_sampling_gpu.py of |u_h - u|,
    |d/dt u_h - u_t| and |grad u_h - grad u| (largest component) at J_time = J_space = 3
    and 4, without the 500 x 500 block.  On the CPU (SciPy restatement sampled with
    numpy_sample_along): u 2.682e-2 and 7.481e-3 (ratio 3.585), d/dt 1.028e-1 and 3.599e-2
    (ratio 2.857), grad 9.499e-1 and 5.483e-1 (ratio 1.732: first order, as P1 gradients
    are).  The device figures are asserted within 1 % of them and the ratios within 0.3: the PCG stopping rule shows in the fifth digit, a sampling error is larger."""
    e3, e4 = _along_errors(3), _along_errors(4)
    for f in ALL:
        ratio, cpu_ratio = e3[f] / e4[f], CPU_ERRORS[f][3] / CPU_ERRORS[f][4]
        print('%s: max error at 500 random pairs: J=3 %.4e, J=4 %.4e, ratio %.3f (CPU %.4e, %.4e, %.3f)'
              % (f, e3[f], e4[f], ratio, CPU_ERRORS[f][3], CPU_ERRORS[f][4], cpu_ratio))
    for f in ALL:
        assert abs(e3[f] - CPU_ERRORS[f][3]) <= 0.01 * CPU_ERRORS[f][3], f
        assert abs(e4[f] - CPU_ERRORS[f][4]) <= 0.01 * CPU_ERRORS[f][4], f
        assert abs(e3[f] / e4[f] - CPU_ERRORS[f][3] / CPU_ERRORS[f][4]) <= 0.3, f


# ---- 7. the drivers -------------------------------------------------------------------------------------------
def test_drivers_follow_the_moving_source(tmp_path, capsys, monkeypatch):
    import heateq
    import heateq_mpi as hm
    from source.mpi_kron import LinearOperatorMPI
    monkeypatch.setattr(LinearOperatorMPI, 'sync_timing', LinearOperatorMPI.sync_timing)  # main() sets it
    common = ['--J_time', '3', '--J_space', '3', '--problem', 'square_moving_source']
    for name, main in (('mpi', hm.main), ('serial', heateq.main)):
        out = str(tmp_path / (name + '.npz'))
        res = main(common + ['--track_out', out, '--track_points', '33'])
        heat, u = res[0], res[1]
        data = np.load(out)
        assert sorted(data.files) == ['dt', 'grad', 'inside', 'points', 'times', 'u']
        assert np.array_equal(data['times'], np.linspace(0.0, 1.0, 33))
        assert np.array_equal(data['points'], heat.path(data['times'])) and data['points'].shape == (33, 2)
        assert data['inside'].dtype == bool and data['inside'].shape == (33,) and data['inside'].all()
        assert data['u'].shape == data['dt'].shape == (33,) and data['grad'].shape == (2, 33)
        direct = _host(heat.sample_along(u, data['times'], data['points'], fields=ALL))
        for f in ALL:
            assert np.array_equal(data[f], direct[f]) and not np.isnan(data[f]).any(), f
        assert data['u'].max() > 0.0  # the source heats what lies under it
        assert 'track_' not in capsys.readouterr().out  # what the drivers print is what it was
        # the default is 1025 points; without the option nothing is sampled
        res = main(common)
        assert res[0].sample_plan is None
    # a problem without a path
    with pytest.raises(SystemExit) as err:
        heateq.main(['--J_time', '2', '--J_space', '2', '--problem', 'square_forced', '--track_out',
                     str(tmp_path / 'none.npz')])
    assert 'no path' in str(err.value) and not (tmp_path / 'none.npz').exists()
