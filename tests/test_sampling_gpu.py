"""Sampling the trial space on the device (csrc/sample.hip, source/sampling.py) against
the NumPy brute-force oracle of tests/test_sampling_host.py: point location, the
evaluation kernel, reproduction of the slab, independence of the rank count, the
convergence of sampled values to the exact solution, and the drivers.

Every value comparison: 1e-12 max|U| (test_sampling_host.py says why)."""
import functools
import threading

import numpy as np
import pytest
import torch

from test_sampling_host import (INSIDE, MESHES, VALUE_TOL, mesh_of, numpy_sample, oracle_located, point_sets)

pytestmark = pytest.mark.gpu

BAND = 1e-9  # random points this close to an edge of the mesh may be decided either way


@functools.lru_cache(maxsize=None)
def plan_of(problem, J):
    from source.sampling import SamplePlan
    return SamplePlan(mesh_of(problem, J))


def all_points(problem, J):
    sets = point_sets(problem, J)
    names = ['random', 'vertices', 'centroids', 'midpoints']
    points = np.concatenate([sets[k] for k in names])
    located = [oracle_located(problem, J, k) for k in names]
    return points, tuple(np.concatenate([l[i] for l in located]) for i in range(3))


# ---- 1. locate ---------------------------------------------------------------------------
@pytest.mark.parametrize('problem,J', MESHES)
def test_locate(problem, J):
    mesh, plan, sets = mesh_of(problem, J), plan_of(problem, J), point_sets(problem, J)
    pts, cells = mesh.points, mesh.cells
    d = pts.shape[1]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    extent = (hi - lo).max()

    def check_lam(points, cell, lam, inside):
        assert np.max(np.abs(lam[inside].sum(axis=1) - 1.0)) <= 1e-14
        back = np.einsum('pa,pak->pk', lam[inside], pts[cells[cell[inside]]])
        assert np.max(np.abs(back - points[inside])) <= 1e-13 * extent

    # random points, whole and in prefixes around the wavefront size
    cell_o, lam_o, low_o = oracle_located(problem, J, 'random')
    clear = np.abs(low_o) >= BAND
    assert (~clear).sum() <= 10  # at most 1 % in the band
    for n in (1, 63, 64, 65, 1000):
        loc = plan.locate(sets['random'][:n])
        cell, lam, inside = loc.cell.cpu().numpy(), loc.lam.cpu().numpy(), loc.inside.cpu().numpy()
        assert cell.shape == (n,) and lam.shape == (n, d + 1) and cell.dtype == np.int32
        ok = clear[:n]
        assert np.array_equal(inside[ok], low_o[:n][ok] >= INSIDE)
        want = np.where(low_o[:n] >= INSIDE, cell_o[:n], -1)
        assert np.array_equal(cell[ok], want[ok])
        assert np.array_equal(inside, cell >= 0)
        if inside.any():
            check_lam(sets['random'][:n], cell, lam, inside)
        beyond = np.any((sets['random'][:n] < lo - BAND) | (sets['random'][:n] > hi + BAND), axis=1)
        assert not inside[beyond].any()
    print('%s J=%d: %d of 1000 random points inside, %d in the band' % (problem, J, inside.sum(), (~clear).sum()))
    assert 0 < inside.sum() < 1000

    for which in ('vertices', 'centroids', 'midpoints'):
        loc = plan.locate(torch.from_numpy(np.array(sets[which])).cuda())  # a device tensor this time
        cell, lam, inside = loc.cell.cpu().numpy(), loc.lam.cpu().numpy(), loc.inside.cpu().numpy()
        assert inside.all(), (which, int((~inside).sum()))
        check_lam(sets[which], cell, lam, inside)
        assert lam.min() >= INSIDE
    # a centroid's cell is its own
    assert np.array_equal(plan.locate(sets['centroids']).cell.cpu().numpy(), np.arange(len(cells)))
    if problem.startswith('lshape'):
        notch = plan.locate(np.array([[0.5, -0.5]]))
        assert not notch.inside.any() and int(notch.cell[0]) == -1
    assert plan.locate(np.zeros((0, d))).cell.shape == (0,)


# ---- 2. evaluate -------------------------------------------------------------------------
def _slab(M, N, seed):
    """(vector whose slab's padding column is NaN, its nodal values (N, M))"""
    from source.linop import self_distribution
    from source.mpi_vector import KronVectorMPI
    U = np.random.RandomState(seed).randn(N, M)
    ld = N + (N & 1)
    buf = torch.full((M, ld), float('nan'), dtype=torch.float64, device='cuda')
    buf[:, :N] = torch.from_numpy(np.ascontiguousarray(U.T)).cuda()
    return KronVectorMPI.around(self_distribution(N, M), buf), U


def _times(N, n_k):
    """0, T, every node, the element midpoints, then seeded random times: the first n_k."""
    nodes = np.arange(N) / (N - 1.0)
    pool = np.concatenate([[0.0, 1.0], nodes, 0.5 * (nodes[1:] + nodes[:-1]), np.random.RandomState(N).rand(130)])
    return pool[:n_k]


@pytest.mark.parametrize('N', [5, 9, 65, 129, 200])
@pytest.mark.parametrize('problem,J', MESHES)
def test_evaluate(problem, J, N):
    mesh, plan = mesh_of(problem, J), plan_of(problem, J)
    points, located_o = all_points(problem, J)
    inside_o = located_o[2] >= INSIDE
    clear = np.abs(located_o[2]) >= BAND
    loc = plan.locate(points)
    assert np.array_equal(loc.inside.cpu().numpy()[clear], inside_o[clear])
    vec, U = _slab(plan.n_free, N, seed=N + J)
    tol = VALUE_TOL * np.max(np.abs(U))
    worst = 0.0
    for n_k in (1, 2, 7, 65, 130, 2 * N + 1):  # the last: 0, T, every node and every midpoint
        times = _times(N, n_k)
        got = plan.evaluate(vec, times, loc).cpu().numpy()
        want = numpy_sample(mesh, U, times, points, located=located_o)
        assert got.shape == (n_k, len(points))
        inside = loc.inside.cpu().numpy()
        assert np.isnan(got[:, ~inside]).all() and not np.isnan(got[:, inside]).any()
        both = inside & inside_o
        err = np.max(np.abs(got[:, both] - want[:, both]))
        worst = max(worst, err)
        assert err <= tol, (n_k, err / np.max(np.abs(U)))
    print('%s J=%d N=%d: largest difference %.2e max|U|' % (problem, J, N, worst / np.max(np.abs(U))))


@pytest.mark.parametrize('n_p', [1, 63, 64, 65])
def test_evaluate_short_tiles_and_absent_columns(n_p):
    """Fewer points than a tile, one more than a tile; and a rank's view: columns that are
    "not on this rank" contribute exactly 0.0 and the parts of a split sum to the whole."""
    from source.mpi_vector import DofDistributionMPI, KronVectorMPI
    from test_sampling_host import _FakeComm
    problem, J, N = 'lshape_jitter', 3, 9
    mesh, plan = mesh_of(problem, J), plan_of(problem, J)
    points = point_sets(problem, J)['random'][:n_p]
    located_o = tuple(a[:n_p] for a in oracle_located(problem, J, 'random'))
    vec, U = _slab(plan.n_free, N, seed=1)
    times = _times(N, 30)
    loc = plan.locate(points)
    whole = plan.evaluate(vec, times, loc).cpu().numpy()
    want = numpy_sample(mesh, U, times, points, located=located_o)
    inside = loc.inside.cpu().numpy()
    assert np.array_equal(inside, located_o[2] >= INSIDE)
    assert np.isnan(whole[:, ~inside]).all()
    if inside.any():
        assert np.max(np.abs(whole[:, inside] - want[:, inside])) <= VALUE_TOL * np.max(np.abs(U))
    total = np.zeros_like(whole)
    for rank in range(3):
        dd = DofDistributionMPI(_FakeComm(rank, 3), N, plan.n_free)
        n_loc = dd.t_end - dd.t_begin
        buf = torch.full((plan.n_free, n_loc + (n_loc & 1)), float('nan'), dtype=torch.float64, device='cuda')
        buf[:, :n_loc] = vec.buf[:, dd.t_begin:dd.t_end]
        total += plan.evaluate(KronVectorMPI.around(dd, buf), times, loc).cpu().numpy()
    assert np.array_equal(total[:, inside], whole[:, inside]) and np.isnan(total[:, ~inside]).all()


# ---- 3. reproduction -----------------------------------------------------------------------
@pytest.mark.parametrize('problem,J', [('lshape_jitter', 3), ('cube', 1), ('square', 3)])
def test_free_vertices_at_the_nodes_give_the_slab(problem, J):
    from source.assembly import free_dofs
    mesh, plan = mesh_of(problem, J), plan_of(problem, J)
    N = 9
    vec, U = _slab(plan.n_free, N, seed=3)
    nodes = np.arange(N) / (N - 1.0)
    tol = VALUE_TOL * np.max(np.abs(U))
    fd = free_dofs(mesh)
    got = plan.evaluate(vec, nodes, plan.locate(mesh.points[fd])).cpu().numpy()
    assert np.max(np.abs(got - U)) <= tol
    on_boundary = plan.evaluate(vec, nodes, plan.locate(mesh.points[mesh.boundary])).cpu().numpy()
    assert on_boundary.shape[1] > 0 and np.max(np.abs(on_boundary)) <= tol


# ---- 4. rank independence -------------------------------------------------------------------
_lock = threading.Lock()  # plan construction reads process-wide tuning keys


def _sample_run(comm, J_time):
    import heateq_mpi as hm
    from source import driver
    from source.mpi_vector import KronVectorMPI
    with _lock:
        h = hm.HeatEquationMPI(J_space=3, J_time=J_time, problem='square_forced', comm=comm)
    assert h.sample_plan is None
    u = driver.seeded_vector(h, KronVectorMPI)  # the same global vector on every rank count
    nodes = np.arange(h.N) / (h.N - 1.0)
    times = np.concatenate([nodes, 0.5 * (nodes[1:] + nodes[:-1]), np.random.RandomState(4).rand(9)])
    points = np.random.RandomState(8).rand(200, 2)
    out = h.sample(u, times, points).cpu().numpy()
    assert h.sample_plan is not None
    return out


@functools.lru_cache(maxsize=None)
def _one_rank_sample(J_time):
    from source.comm import Comm
    return _sample_run(Comm(distributed=False), J_time)


@pytest.mark.parametrize('J_time,ranks', [(2, 2), (2, 3), (2, 5), (3, 8)])
def test_sample_does_not_depend_on_the_number_of_ranks(J_time, ranks):
    """Every node is a sample time, so every rank boundary is one, and so is the midpoint
    of every element, those that straddle two ranks included."""
    from thread_comm import run_ranks
    got = run_ranks(ranks, lambda comm: _sample_run(comm, J_time))
    one = _one_rank_sample(J_time)
    assert not np.isnan(one).any() and np.abs(one).max() > 0.1
    for rank in range(ranks):
        assert np.array_equal(got[rank], one), (rank, np.max(np.abs(got[rank] - one)))


# ---- 5. end to end ----------------------------------------------------------------------------
CPU_ERRORS = {3: 2.682e-2, 4: 7.481e-3}  # SciPy solve sampled with the NumPy oracle


@functools.lru_cache(maxsize=None)
def _sampled_error(J):
    import heateq_mpi as hm
    from source.comm import Comm
    from source.problem import problem_helper
    h = hm.HeatEquationMPI(J_space=J, J_time=J, problem='square_forced', comm=Comm(distributed=False))
    u, _ = h.solve()
    rs = np.random.RandomState(7)
    q = rs.rand(500, 2)
    t = rs.rand(500)
    block = h.sample(u, t, q).cpu().numpy()
    assert block.shape == (500, 500)
    exact = problem_helper('square_forced', J_space=J, J_time=J)[3]['exact']
    return float(np.max(np.abs(np.diagonal(block) - exact(t, q[:, 0], q[:, 1]))))


def test_sampled_solution_converges_to_the_exact_one():
    """max over 500 random (t_i, q_i) of |u_h - u|, the diagonal of the 500 x 500 block, at
    J_time = J_space = 3 and 4.  On the CPU (SciPy restatement of
    tests/test_forcing_host.py::scipy_error sampled with the NumPy oracle): 2.682e-2 and
    7.481e-3, ratio 3.585."""
    e3, e4 = _sampled_error(3), _sampled_error(4)
    print('max error at 500 random points and times: J=3 %.4e, J=4 %.4e, ratio %.3f' % (e3, e4, e3 / e4))
    assert e4 <= 8.0e-3
    assert 3.3 <= e3 / e4 <= 3.9
    assert abs(e3 - CPU_ERRORS[3]) <= 0.01 * CPU_ERRORS[3]
    assert abs(e4 - CPU_ERRORS[4]) <= 0.01 * CPU_ERRORS[4]


# ---- 6. the serial driver ----------------------------------------------------------------------
def test_serial_driver_samples_host_and_device_vectors():
    import heateq
    import heateq_mpi as hm
    from source.comm import Comm
    from source.linop import device_vector
    from source.mpi_vector import KronVectorMPI
    serial = heateq.HeatEquation(J_space=2, J_time=2, problem='square_forced')
    mpi = hm.HeatEquationMPI(J_space=2, J_time=2, problem='square_forced', comm=Comm(distributed=False))
    assert serial.sample_plan is None and (serial.N, serial.M) == (mpi.N, mpi.M)
    X = np.random.RandomState(6).randn(serial.N, serial.M)
    rs = np.random.RandomState(9)
    points, times = -0.05 + 1.1 * rs.rand(300, 2), np.concatenate([[0.0, 1.0], rs.rand(11)])
    want = mpi.sample(KronVectorMPI(mpi.dofs_distr, X), times, points).cpu().numpy()
    tol = VALUE_TOL * np.max(np.abs(X))
    outside = np.isnan(want).all(axis=0)
    assert 0 < outside.sum() < 300 and not np.isnan(want[:, ~outside]).any()
    for u in (X.reshape(-1), device_vector(X.reshape(-1), serial.N)):
        got = serial.sample(u, times, points).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.max(np.abs(got[:, ~outside] - want[:, ~outside])) <= tol
    assert serial.sample_plan is not None


# ---- 7. the drivers -----------------------------------------------------------------------------
def test_drivers_write_the_samples(tmp_path, capsys, monkeypatch):
    import heateq
    import heateq_mpi as hm
    from source.mpi_kron import LinearOperatorMPI
    from source.sampling import raster
    monkeypatch.setattr(LinearOperatorMPI, 'sync_timing', LinearOperatorMPI.sync_timing)  # main() sets it
    common = ['--J_time', '2', '--J_space', '2', '--problem', 'square_forced']
    for name, main in (('mpi', hm.main), ('serial', heateq.main)):
        out = str(tmp_path / (name + '.npz'))
        res = main(common + ['--sample_out', out, '--sample_raster', '17', '--sample_times', '3'])
        heat, u = res[0], res[1]
        data = np.load(out)
        assert sorted(data.files) == ['inside', 'points', 'times', 'values']
        assert data['times'].shape == (3,) and np.array_equal(data['times'], [0.0, 0.5, 1.0])
        assert data['points'].shape == (289, 2) and data['inside'].shape == (289,) and data['values'].shape == (3, 289)
        assert data['inside'].all() and data['inside'].dtype == bool
        assert np.array_equal(data['points'], raster(mesh_of('square', 2), 17))
        direct = heat.sample(u, data['times'], data['points']).cpu().numpy()
        assert np.array_equal(data['values'], direct)
        # the initial condition sin(pi x) sin(pi y) on the first slice, to the mesh's accuracy
        x, y = data['points'][:, 0], data['points'][:, 1]
        assert np.max(np.abs(data['values'][0] - np.sin(np.pi * x) * np.sin(np.pi * y))) < 0.1
        text = capsys.readouterr().out
        assert 'sample_' not in text  # what the drivers print is what it was
        # without the option: no plan
        res = main(common)
        assert res[0].sample_plan is None
        assert 'sample_' not in capsys.readouterr().out
