"""The solidification maps on the device (csrc/solid.hip, source/solidification.py) against
the NumPy contract of tests/test_solidification_host.py -- array_equal, NaN-aware, on the whole
state: at every tile edge and column count, every launch form, the infinite thresholds, NaN
and inf in the slab, the refusals, the public call of both drivers, its independence of the
number of ranks, the torch composition the timing tool compares with, and the drivers'
--solid_out."""
import functools
import importlib.util
import os
import threading

import numpy as np
import pytest
import torch

from test_history_host import same
from test_solidification_host import (N_MAX, THETA, cell_tables, dyadic_values, jitter_tolerances, numpy_solid_scan)
from test_time_curves_host import _mesh, first_cells

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COLS = (1, 2, 3, 9, 64, 65, 130)
INF = float('inf')
H = 0.01  # no power of two: the cooling rate takes a real division
SENTINEL = 123.25

MESHES = {
    'square2': lambda: _mesh('square', 2),
    'square4': lambda: _mesh('square', 4),  # 2048 cells: eight tiles
    'lshape_jitter3': lambda: _mesh('lshape_jitter', 3),
    'cube1': lambda: _mesh('cube', 1),  # one free dof
    'cube2': lambda: _mesh('cube', 2),
    'first1': lambda: first_cells(_mesh('square', 4), 1),
    'first255': lambda: first_cells(_mesh('square', 4), 255),  # tail lanes
    'first256': lambda: first_cells(_mesh('square', 4), 256),  # exactly one tile
    'first257': lambda: first_cells(_mesh('square', 4), 257),  # a second tile of one cell
    'first513': lambda: first_cells(_mesh('square', 4), 513),  # two full tiles and a third of one cell
}


class _Case:
    """A mesh with its plan and, per kind of data, the slab values (M, 130) and the contract's
    state after 1 .. 130 of their columns -- computed once (one pass with the carried state,
    which the host file shows to give the one-shot doubles), shared by the tests, never changed."""
    def __init__(self, name):
        from source.solidification import SolidPlan
        self.mesh = MESHES[name]()
        self.plan = SolidPlan(self.mesh, None)
        self.grad, self.cell_rows = cell_tables(self.mesh)
        self.d, self.M, self.nc = self.plan.d, self.plan.n_free, self.plan.nc
        self._kept = {}

    def contract(self, U, theta, k_first=0, state=None, h=H):
        return numpy_solid_scan(self.grad, self.cell_rows, U, k_first, h, theta, state=state)

    def reference(self, kind):
        if kind not in self._kept:
            if kind == 'randn':
                U = np.random.RandomState(2000 + self.nc).randn(self.M, N_MAX)
            else:
                U = dyadic_values(self.mesh)
            states, s, done = {}, None, 0
            for n in N_COLS:
                s = self.contract(U[:, done:n], THETA, k_first=done, state=s)
                s.setflags(write=False)
                states[n], done = s, n
            U.setflags(write=False)
            self._kept[kind] = (U, states)
        return self._kept[kind]


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


def _dev(a):
    from source import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(_lib.compute_device())


def _slab(v, ld=None):
    """(M, ld) device slab of the rows v (M, n), the padding NaN; ld: even and > n by default."""
    M, n = v.shape
    buf = np.full((M, (n | 1) + 1 if ld is None else ld), np.nan)
    buf[:, :n] = v
    return _dev(buf)


def _fresh_state(case):
    from source import _lib
    return torch.full((2 * case.d + 6, case.nc), SENTINEL, dtype=torch.float64, device=_lib.compute_device())


def _scan(case, slab, n, theta, first=0, k_first=None, state=None, h=H):
    """The state after the columns [first, first + n) of a slab: fresh without `state`, else
    carried (and updated in place)."""
    from source.solidification import solid_scan
    fresh = state is None
    if fresh:
        state = _fresh_state(case)
    solid_scan(case.plan, slab.data_ptr() + 8 * first, case.M, n, slab.shape[1], first if k_first is None else k_first, h,
               theta, state, fresh)
    return state


def _np(t):
    return t.cpu().numpy()


class _tile:
    """stk_solid_tile(cols, lds_kib) for the block."""
    def __init__(self, cols, kib):
        self.form = (cols, kib)

    def __enter__(self):
        from source import _lib
        _lib.check(_lib.lib().stk_solid_tile(*self.form))

    def __exit__(self, *exc):
        from source import _lib
        _lib.check(_lib.lib().stk_solid_tile(0, 0))


# ---- 1. the device is the contract ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(MESHES))
def test_device_is_the_contract(name):
    """randn and the dyadic data with theta = 0.3; 1 .. 130 columns of a slab whose padding is NaN."""
    case = _case(name)
    for kind in ('randn', 'dyadic'):
        U, states = case.reference(kind)
        for n in N_COLS:
            slab = _slab(U[:, :n])
            assert slab.shape[1] % 2 == 0 and bool(torch.isnan(slab[:, n:]).all())
            got = _np(_scan(case, slab, n, THETA))
            want = states[n]
            for q in range(len(want)):
                assert same(got[q], want[q]), (name, kind, n, q, got[q], want[q])
            assert not np.isnan(got[2:6]).any()  # no padding column came in, no sentinel stayed
        full = states[N_MAX][2]
        if name in ('square4', 'cube2', 'lshape_jitter3'):
            assert (full >= 2).any() and ((full == 0).any() or kind == 'randn')


@pytest.mark.parametrize('name', ['first257', 'cube2'])
def test_nan_and_inf_in_the_slab_give_what_the_contract_gives(name):
    case = _case(name)
    U = np.random.RandomState(21).randn(case.M, 7)
    U[3 % case.M, 0], U[5 % case.M, 1], U[7 % case.M, 2], U[:, 4] = np.nan, np.inf, -np.inf, np.nan
    U[2 % case.M, 5] = np.inf
    for theta in (0.3, -INF, INF):
        got = _np(_scan(case, _slab(U), 7, theta))
        assert same(got, case.contract(U, theta)), (name, theta)


@pytest.mark.parametrize('name', ['square2', 'first513', 'cube2'])
def test_infinite_thresholds(name):
    case = _case(name)
    U, _ = case.reference('randn')
    n = 9
    slab = _slab(U[:, :n])
    for theta in (INF, -INF):
        got = _np(_scan(case, slab, n, theta))
        assert same(got, case.contract(U[:, :n], theta)), (name, theta)
        assert np.all(got[2] == 0.0) and np.isnan(got[0]).all() and np.isnan(got[1]).all() and np.isnan(got[6:6 + case.d]).all()


# ---- 2. every launch form gives the same doubles ---------------------------------------------------------------
@pytest.mark.parametrize('name', ['first513', 'cube2', 'square4', 'lshape_jitter3'])
def test_every_launch_form_gives_the_one_shot_doubles(name):
    case = _case(name)
    U, states = case.reference('randn')
    for n in (9, 65):
        slab = _slab(U[:, :n])
        whole = _np(_scan(case, slab, n, THETA))
        assert same(whole, states[n])
        # chunks of one column, odd ones, one beside and one above n, the largest accepted
        for cols in (1, 2, 3, 5, 7, 8, 10, 33, 64, 66, 127, 128):
            with _tile(cols, 0):
                assert same(_np(_scan(case, slab, n, THETA)), whole), (n, cols)
        # LDS budgets: 1 KiB forces chunks of one column, 64 is the maximum
        for kib in (1, 2, 7, 64):
            with _tile(0, kib):
                assert same(_np(_scan(case, slab, n, THETA)), whole), (n, kib)
    # the scan cut at every column boundary, the state carried, the second call from base + 8 s
    n = 9
    slab = _slab(U[:, :n])
    for s in range(1, n):
        state = _scan(case, slab, s, THETA)
        assert same(_np(state), case.contract(U[:, :s], THETA)), s
        _scan(case, slab, n - s, THETA, first=s, state=state)
        assert same(_np(state), states[n]), s
    # n_cols == 0 without fresh leaves the state as it is
    before = _np(state).copy()
    _scan(case, slab, 0, THETA, first=n, state=state)
    assert same(_np(state), before)
    # a slab pointer offset by 8 bytes (the scan starts at node 1), row strides odd and even
    for ld in (n, n + 1, n + 2, n + 5):
        other = _slab(U[:, :n], ld=ld)
        assert (other.data_ptr() + 8) % 16 == 8
        got = _np(_scan(case, other, n - 1, THETA, first=1))
        assert same(got, case.contract(U[:, 1:n], THETA, k_first=1)), ld
        assert same(_np(_scan(case, other, n, THETA)), states[n]), ld


@pytest.mark.parametrize('name', ['first513', 'cube2', 'lshape_jitter3'])
def test_the_order_of_the_cells_changes_no_double(name):
    """A plan that cuts its tiles from the cells as given (stk_solid_order(1)) beside the
    default, the cells along a Z-curve: the same state, in the mesh's cell order."""
    from source import _lib
    from source.solidification import SolidPlan, solid_scan
    case = _case(name)
    U, states = case.reference('dyadic')
    _lib.check(_lib.lib().stk_solid_order(1))
    try:
        plan = SolidPlan(case.mesh, None)
    finally:
        _lib.check(_lib.lib().stk_solid_order(0))
    for n in (1, 9, 65):
        slab = _slab(U[:, :n])
        state = _fresh_state(case)
        solid_scan(plan, slab, case.M, n, slab.shape[1], 0, H, THETA, state, True)
        assert same(_np(state), states[n]), n
        assert same(_np(_scan(case, slab, n, THETA)), states[n]), n


def test_tile_setting_refuses_and_changes_nothing():
    from source import _lib
    lib = _lib.lib()
    case = _case('first513')
    U, states = case.reference('randn')
    slab = _slab(U[:, :9])
    for cols, kib, text in ((-1, 0, 'cols'), (129, 0, 'cols'), (0, -1, 'lds_kib'), (0, 65, 'lds_kib')):
        assert lib.stk_solid_tile(cols, kib) != 0 and text in lib.stk_last_error().decode(), (cols, kib)
    assert same(_np(_scan(case, slab, 9, THETA)), states[9])
    assert lib.stk_solid_tile(0, 0) == 0


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_the_state():
    from source import _lib
    lib = _lib.lib()
    case = _case('square2')
    U, states = case.reference('randn')
    n = 9
    slab = _slab(U[:, :n])
    state = _fresh_state(case)
    good = dict(plan=case.plan._plan, M=case.M, n_cols=n, slab=slab.data_ptr(), row_stride=slab.shape[1], k_first=0, h=H,
                threshold=THETA, fresh=1, state=state.data_ptr())
    order = ('plan', 'M', 'n_cols', 'slab', 'row_stride', 'k_first', 'h', 'threshold', 'fresh', 'state')
    cases = [(' plan is null', dict(plan=None)), (' slab is null', dict(slab=None)), (' state is null', dict(state=None)),
             (' M = %d' % (case.M + 1), dict(M=case.M + 1)), (' M = 0', dict(M=0)), (' n_cols = -3', dict(n_cols=-3)),
             (' fresh with n_cols = 0', dict(n_cols=0)), (' k_first = -1', dict(k_first=-1)), (' h = 0', dict(h=0.0)),
             (' h = -0.5', dict(h=-0.5)), (' h = inf', dict(h=INF)), (' h = nan', dict(h=float('nan'))),
             (' threshold is NaN', dict(threshold=float('nan'))), (' row_stride = %d' % (n - 1), dict(row_stride=n - 1))]
    for text, change in cases:
        a = dict(good, **change)
        rc = lib.stk_solid_scan(_lib.stream(), *[a[k] for k in order])
        said = lib.stk_last_error().decode()
        assert rc != 0 and 'stk_solid_scan' in said and text in said, (text, rc, said)
        with pytest.raises(_lib.StkError):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((state == SENTINEL).all())
    assert lib.stk_solid_scan(_lib.stream(), *[dict(good, n_cols=0, fresh=0)[k] for k in order]) == 0
    torch.cuda.synchronize()
    assert bool((state == SENTINEL).all())
    for theta in (INF, -INF, THETA):
        assert lib.stk_solid_scan(_lib.stream(), *[dict(good, threshold=theta)[k] for k in order]) == 0
    assert same(_np(state), states[n])


# ---- 4. the public call -------------------------------------------------------------------------------------------
def _solver(problem, J_space, J_time, comm=None, **kw):
    import heateq_mpi as hm
    from source.comm import Comm
    return hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem=problem,
                              comm=Comm(distributed=False) if comm is None else comm, **kw)


def _numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _node_values(N, M, seed):
    """(N, M): every row of the slab is a random walk of steps in [-0.25, 0.25] from a start in
    [0, 1]: the cells cross 0.5 a few times."""
    rng = np.random.RandomState(seed)
    return (rng.rand(1, M) + np.cumsum(0.5 * rng.rand(N, M) - 0.25, axis=0))


def _table_of(heat, X, theta):
    """The contract's state of the node values X (N, M) on the solver's meshes."""
    mesh, mesh_time = heat._sample_meshes
    grad, cell_rows = cell_tables(mesh)
    return numpy_solid_scan(grad, cell_rows, np.ascontiguousarray(X.T), 0, float(mesh_time.h), theta)


def _derived(table, d):
    """The public dict from a state by the torch expressions of the issue, on the device."""
    t = _dev(table)
    gs = t[6:6 + d]
    q = gs[0] * gs[0] + gs[1] * gs[1]
    if d == 3:
        q = q + gs[2] * gs[2]
    G = torch.sqrt(q)
    return _numpy({'t_solid': t[0], 'cooling_rate': t[1], 'grad_solid': gs.t().contiguous(), 'G': G,
                   'front_speed': t[1] / G, 'n_solid': t[2].to(torch.int64), 'max_grad': torch.sqrt(t[3]), 't_max_grad': t[4]})


def _check_dict(heat, got, X, theta):
    from source.solidification import FIELDS
    mesh = heat._sample_meshes[0]
    d, nc = np.asarray(mesh.points).shape[1], len(mesh.cells)
    want = _derived(_table_of(heat, X, theta), d)
    assert sorted(got) == sorted(want) == sorted(FIELDS)
    for key, value in want.items():
        assert got[key].shape == value.shape == ((nc, d) if key == 'grad_solid' else (nc,)), key
        assert got[key].dtype == value.dtype and same(got[key], value), key
    assert got['n_solid'].dtype == np.int64
    crossed = got['n_solid'] >= 1
    assert crossed.any() and same(np.isnan(got['t_solid']), ~crossed) and same(np.isnan(got['G']), ~crossed)
    assert np.all(got['cooling_rate'][crossed] > 0.0) and np.all(got['max_grad'] >= 0.0)
    return want


@pytest.mark.parametrize('problem,J', [('square_moving_source', 3), ('cube_forced', 2)])
def test_public_call_of_both_drivers(problem, J):
    import heateq
    from source.linop import device_vector
    from source.mpi_vector import KronVectorMPI
    from source.sampling import raster
    heat = _solver(problem, J, 3)
    X = _node_values(heat.N, heat.M, 31)
    u = KronVectorMPI(heat.dofs_distr, X)
    assert heat.solid_plan is None  # nothing is built without the call
    with pytest.raises(ValueError, match='NaN'):
        heat.solidification_maps(u, float('nan'))
    with pytest.raises(ValueError, match='needs a threshold'):
        heat.solidification_maps(u, None)
    with pytest.raises(ValueError, match='fields must name'):
        heat.solidification_maps(u, 0.5, fields=('peak',))
    with pytest.raises(AssertionError, match='trial space'):
        heat.solidification_maps(heat.g, 0.5)
    assert heat.solid_plan is None
    want = _check_dict(heat, _numpy(heat.solidification_maps(u, 0.5)), X, 0.5)
    plan = heat.solid_plan
    assert plan is not None and heat.sample_plan is None and heat.curves_plan is None
    some = _numpy(heat.solidification_maps(u, 0.5, fields=('front_speed', 'n_solid')))
    assert sorted(some) == ['front_speed', 'n_solid'] and same(some['front_speed'], want['front_speed'])
    assert heat.solid_plan is plan

    # the points form: the fields of the cell that holds each point, NaN / -1 outside
    mesh = heat._sample_meshes[0]
    d = np.asarray(mesh.points).shape[1]
    pts = np.concatenate([raster(mesh, 6) * 0.96 + 0.013, np.full((2, d), 7.5), np.full((1, d), -0.25)])
    at_points = _numpy(heat.solidification_maps(u, 0.5, points=pts))
    located = heat.sample_plan.locate(pts)
    cell, inside = located.cell.cpu().numpy().astype(np.int64), located.inside.cpu().numpy()
    assert same(at_points.pop('inside'), inside) and inside[:-3].all() and not inside[-3:].any()
    assert sorted(at_points) == sorted(want)
    for key, value in want.items():
        assert same(at_points[key][inside], value[cell[inside]]), key
        outside = at_points[key][~inside]
        assert (outside == -1).all() if key == 'n_solid' else np.isnan(outside).all(), key
        assert at_points[key].dtype == value.dtype and at_points[key].shape[1:] == value.shape[1:]
    again = _numpy(heat.solidification_maps(u, 0.5, points=located))  # what locate returned
    assert all(same(again[key], at_points[key]) for key in at_points)
    with pytest.raises(ValueError, match='points of shape'):
        heat.solidification_maps(u, 0.5, points=np.zeros((4, d + 1)))

    # after a solve: the threshold at half the largest value
    solved, _ = heat.solve()
    Xs = solved.X_loc.cpu().numpy()
    theta = 0.5 * float(Xs.max())
    got = _numpy(heat.solidification_maps(solved, theta))
    want = _derived(_table_of(heat, Xs, theta), d)
    for key, value in want.items():
        assert same(got[key], value), key
    assert np.isfinite(got['max_grad']).all() and got['max_grad'].max() > 0.0

    serial = heateq.HeatEquation(J_space=J, J_time=3, problem=problem, precond='direct')
    assert (serial.N, serial.M) == (heat.N, heat.M) and serial.solid_plan is None
    with pytest.raises(ValueError, match='NaN'):
        serial.solidification_maps(X.reshape(-1), float('nan'))
    with pytest.raises(ValueError, match='needs a threshold'):
        serial.solidification_maps(X.reshape(-1), None)
    with pytest.raises(AssertionError, match='trial space'):
        serial.solidification_maps(device_vector(np.zeros(serial.N_Y * serial.M), serial.N_Y), 0.5)
    assert serial.solid_plan is None
    flat = _numpy(serial.solidification_maps(X.reshape(-1), 0.5))
    on_device = _numpy(serial.solidification_maps(device_vector(X.reshape(-1), serial.N), 0.5))
    _check_dict(serial, flat, X, 0.5)
    _check_dict(serial, on_device, X, 0.5)
    assert serial.solid_plan is not None and serial.sample_plan is None
    serial_points = _numpy(serial.solidification_maps(X.reshape(-1), 0.5, points=pts))
    assert all(same(serial_points[key], value) for key, value in at_points.items()) and same(serial_points['inside'], inside)


# ---- 5. rank independence ---------------------------------------------------------------------------------------
_lock = threading.Lock()  # plan construction reads process-wide tuning keys


def _rank_run(comm, J_time):
    from source import driver
    from source.mpi_vector import KronVectorMPI
    from source.solidification import solidification_collective
    with _lock:
        heat = _solver('square_moving_source', 3, J_time, comm=comm)
    u = driver.seeded_vector(heat, KronVectorMPI)  # the same global vector on every rank count
    maps = _numpy(heat.solidification_maps(u, 0.5))
    return _np(solidification_collective(heat.solid_plan, u, 0.5)), maps


@functools.lru_cache(maxsize=None)
def _one_rank(J_time):
    return _rank_run(None, J_time)


@pytest.mark.parametrize('J_time,ranks', [(3, 2), (3, 3), (3, 8), (2, 5)])
def test_solidification_maps_do_not_depend_on_the_number_of_ranks(J_time, ranks):
    """The state and every tensor of the dict, on every rank: array_equal to the one-rank
    ones.  (2, 5): five nodes on five ranks -- every scan is a single column."""
    from thread_comm import run_ranks
    got = run_ranks(ranks, lambda comm: _rank_run(comm, J_time))
    state, maps = _one_rank(J_time)
    assert (state[2] >= 1).any() and len(maps) == 8
    for rank in range(ranks):
        assert same(got[rank][0], state), rank
        assert sorted(got[rank][1]) == sorted(maps)
        for key, value in maps.items():
            assert same(got[rank][1][key], value), (rank, key)


# ---- 6. the torch composition of the timing tool -------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location('solidification_time', os.path.join(REPO, 'tools', 'solidification_time.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.mark.parametrize('name', ['square4', 'cube2'])
def test_the_timed_composition_computes_what_the_kernel_computes(name):
    """On the dyadic data every mean, gradient and square is exact, so the crossings, their
    times, the rates and the node of the largest gradient are EQUAL; the gradients within the
    tolerance the host file derives, because torch may contract."""
    case = _case(name)
    U, states = case.reference('dyadic')
    n = 65
    slab = _slab(U[:, :n])
    got = _np(_scan(case, slab, n, THETA))
    assert same(got, states[n])
    comp = _tool().Composition(case.mesh, slab)
    _, tol_grad, tol_Q = jitter_tolerances(case.grad)
    for chunk in (8, 1, 65, 7):
        ref = _numpy(comp.fields(slab[:, :n], H, THETA, chunk=chunk))
        for key, row in (('n_solid', 2), ('t_solid', 0), ('cooling_rate', 1), ('t_max_grad', 4)):
            assert same(ref[key], got[row]), (name, chunk, key)
        gap = np.nanmax(np.abs(ref['grad_solid'] - got[6:6 + case.d]))
        gap_q = np.abs(ref['max_grad_sq'] - got[3]).max()
        print('%s chunk %d: grad_solid %.3e (tolerance %.1e), max_grad_sq %.3e (tolerance %.1e)' %
              (name, chunk, gap, tol_grad, gap_q, tol_Q))
        assert gap <= tol_grad and gap_q <= tol_Q
        assert same(np.isnan(ref['grad_solid']), np.isnan(got[6:6 + case.d]))


# ---- 7. the drivers ----------------------------------------------------------------------------------------------------
def test_drivers_write_solid_out(tmp_path, monkeypatch, capsys):
    import heateq
    import heateq_mpi as hm
    from source.mpi_kron import LinearOperatorMPI
    from source.solidification import FIELDS
    monkeypatch.setattr(LinearOperatorMPI, 'sync_timing', LinearOperatorMPI.sync_timing)  # main() sets it
    common = ['--J_time', '2', '--J_space', '2', '--problem', 'square_moving_source']
    for name, main in (('mpi', hm.main), ('serial', heateq.main)):
        out = str(tmp_path / (name + '.npz'))
        res = main(common + ['--solid_out', out, '--solid_threshold', '0.01'])
        heat, u = res[0], res[1]
        data = np.load(out)
        assert sorted(data.files) == sorted(('centroids', 'threshold') + FIELDS)
        mesh = heat._sample_meshes[0]
        p, cells = np.asarray(mesh.points, dtype=np.float64), np.asarray(mesh.cells, dtype=np.int64)
        assert np.array_equal(data['centroids'], p[cells].mean(axis=1)) and float(data['threshold']) == 0.01
        direct = _numpy(heat.solidification_maps(u, 0.01))
        for key in FIELDS:
            assert same(data[key], direct[key]), (name, key)
        assert data['t_solid'].shape == (len(cells),) and data['grad_solid'].shape == (len(cells), 2)
        assert data['max_grad'].max() > 0.0
        assert 'solid_' not in capsys.readouterr().out  # what the drivers print is what it was
        # --solid_out without --solid_threshold is an argument error, before anything is built
        missing = str(tmp_path / (name + '_missing.npz'))
        with pytest.raises(SystemExit, match='--solid_threshold'):
            main(common + ['--solid_out', missing])
        # without the option nothing is written and nothing is built
        before = sorted(os.listdir(tmp_path))
        assert os.path.basename(missing) not in before
        res = main(common)
        assert res[0].solid_plan is None and sorted(os.listdir(tmp_path)) == before
