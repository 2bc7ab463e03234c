"""The history scan on the device (csrc/history.hip, source/history.py) against the NumPy
contract of tests/test_history_host.py -- array_equal, NaN-aware, on all nine state rows:
the slab form at every tile edge, every path into the kernel, the infinite thresholds, the
refusals, the public call of both drivers, its independence of the number of ranks, the torch
composition the timing tool compares with, and the drivers' --history_out."""
import functools
import importlib.util
import os
import threading

import numpy as np
import pytest
import torch

from test_history_host import (ABOVE, DOSE, LAST, MAX_RATE, MIN_RATE, PEAK, T_FIRST, T_LAST, T_PEAK,
                               numpy_history_scan, planted_rows, same)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THETA = 0.3


def _dev(a):
    from source import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(_lib.compute_device())


def _slab(v):
    """(M, ld) device slab of the rows v (M, n), ld = n + (n & 1), the padding column NaN."""
    M, n = v.shape
    buf = np.full((M, n + (n & 1)), np.nan)
    buf[:, :n] = v
    return _dev(buf)


def _state(M, fill=None):
    from source import _lib
    s = torch.empty((9, M), dtype=torch.float64, device=_lib.compute_device())
    return s.fill_(np.nan if fill is None else fill)


def _scan(u, M, n, strides, k_first, h, theta, state, fresh):
    from source.history import history_scan
    return history_scan(u, M, n, strides, k_first, h, theta, state, fresh)


class _tile:
    """The slab kernel's tile for the block: rows per workgroup, LDS in KiB (stk_history_tile)."""
    def __init__(self, rows, kib):
        self.shape = (rows, kib)

    def __enter__(self):
        from source import _lib
        _lib.check(_lib.lib().stk_history_tile(*self.shape))

    def __exit__(self, *exc):
        from source import _lib
        _lib.check(_lib.lib().stk_history_tile(0, 0))


# ---- 1. the slab form against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize('n_cols', [1, 2, 3, 5, 9, 64, 65, 130])
@pytest.mark.parametrize('M', [1, 63, 64, 65, 255, 256, 257, 1000])
def test_slab_form_is_the_contract(M, n_cols):
    """theta = 0.3 on randn data with the planted rows; and theta = 1.0, an integer, where the
    planted row of integers has nodes exactly AT the threshold."""
    for theta in (THETA, 1.0):
        rng = np.random.RandomState(1000 * n_cols + M)
        v = planted_rows(rng, M, n_cols, theta)
        h = 1.0 / max(n_cols - 1, 1)
        buf = _slab(v)
        assert buf.shape[1] == n_cols + (n_cols & 1) and (n_cols % 2 == 0 or bool(torch.isnan(buf[:, -1]).all()))
        got = _scan(buf, M, n_cols, (buf.shape[1], 1), 0, h, theta, _state(M), True).cpu().numpy()
        want = numpy_history_scan(v, 0, h, theta)
        for row in range(9):
            assert same(got[row], want[row]), (theta, row, got[row], want[row])
        assert not np.isnan(got[[PEAK, T_PEAK, DOSE, ABOVE, LAST]]).any()  # no padding column came in
        # row 0 sits AT the threshold: never above
        assert got[ABOVE, 0] == 0.0 and np.isnan(got[T_FIRST, 0]) and np.isnan(got[T_LAST, 0])
        if M > 2 and theta == 1.0:
            assert np.count_nonzero(v[2] == theta) >= n_cols // 3


@pytest.mark.parametrize('rows,kib', [(64, 40), (128, 40), (256, 40), (512, 40), (256, 16), (512, 64), (512, 1), (64, 1)])
@pytest.mark.parametrize('M,n_cols', [(257, 9), (1000, 65), (130, 130), (700, 200)])
def test_every_tile_shape_gives_the_same_doubles(rows, kib, M, n_cols):
    """64 .. 512 rows per workgroup and 1 .. 64 KiB of LDS: the columns in one chunk or several,
    the last one shorter, down to chunks of one column (1 KiB)."""
    v = planted_rows(np.random.RandomState(M + n_cols), M, n_cols, THETA)
    buf, h = _slab(v), 0.01
    with _tile(rows, kib):
        got = _scan(buf, M, n_cols, (buf.shape[1], 1), 3, h, THETA, _state(M), True).cpu().numpy()
    assert same(got, numpy_history_scan(v, 3, h, THETA))


def test_tile_setter_refuses_other_shapes():
    from source import _lib
    lib = _lib.lib()
    for rows, kib, name in ((100, 40, 'rows'), (-64, 0, 'rows'), (1024, 0, 'rows'), (256, 65, 'lds_kib'), (256, -1, 'lds_kib')):
        assert lib.stk_history_tile(rows, kib) != 0 and name in lib.stk_last_error().decode(), (rows, kib)
    assert lib.stk_history_tile(0, 0) == 0


# ---- 2. the same doubles from every path into the kernel -------------------------------------------------
def test_every_path_gives_the_one_shot_doubles():
    M, n, h = 300, 9, 0.125
    v = planted_rows(np.random.RandomState(2), M, n, THETA)
    buf = _slab(v)
    ld = buf.shape[1]
    whole = _scan(buf, M, n, (ld, 1), 0, h, THETA, _state(M), True).clone()
    assert same(whole.cpu().numpy(), numpy_history_scan(v, 0, h, THETA))
    # two calls split at every column: the second from base + 8 skip (odd and even skip)
    for skip in range(1, n):
        state = _scan(buf, M, skip, (ld, 1), 0, h, THETA, _state(M), True)
        _scan(buf.data_ptr() + 8 * skip, M, n - skip, (ld, 1), skip, h, THETA, state, False)
        assert torch.equal(torch.nan_to_num(state, nan=-7.0), torch.nan_to_num(whole, nan=-7.0)), skip
        assert same(state.cpu().numpy(), whole.cpu().numpy()), skip
    # the time-major form on the transposed copy, whole and in chunks of 1, 2 and 4 columns
    block = _dev(np.ascontiguousarray(v.T))
    state = _scan(block, M, n, (1, M), 0, h, THETA, _state(M), True)
    assert same(state.cpu().numpy(), whole.cpu().numpy())
    for width in (1, 2, 4):
        state = _state(M)
        for k0 in range(0, n, width):
            k1 = min(k0 + width, n)
            _scan(block.data_ptr() + 8 * k0 * M, M, k1 - k0, (1, M), k0, h, THETA, state, k0 == 0)
        assert same(state.cpu().numpy(), whole.cpu().numpy()), width
    # a time-major block with rows further apart than M
    wide = _dev(np.concatenate([v.T, np.full((n, 5), np.nan)], axis=1))
    state = _scan(wide, M, n, (1, M + 5), 0, h, THETA, _state(M), True)
    assert same(state.cpu().numpy(), whole.cpu().numpy())


# ---- 3. the infinite thresholds --------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['slab', 'time-major'])
def test_infinite_thresholds(form):
    M, n, h = 200, 9, 0.125
    v = np.random.RandomState(3).randn(M, n)
    u, strides = (_slab(v), (10, 1)) if form == 'slab' else (_dev(np.ascontiguousarray(v.T)), (1, M))
    low = _scan(u, M, n, strides, 0, h, -np.inf, _state(M), True).cpu().numpy()
    high = _scan(u, M, n, strides, 0, h, np.inf, _state(M), True).cpu().numpy()
    assert np.all(low[ABOVE] == 1.0) and np.all(low[T_FIRST] == 0.0) and np.all(low[T_LAST] == 1.0)
    assert np.all(high[ABOVE] == 0.0) and np.isnan(high[T_FIRST]).all() and np.isnan(high[T_LAST]).all()
    for row in (PEAK, T_PEAK, DOSE, MAX_RATE, MIN_RATE, LAST):
        assert same(low[row], high[row])
    assert same(low, numpy_history_scan(v, 0, h, -np.inf)) and same(high, numpy_history_scan(v, 0, h, np.inf))


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_the_state():
    from source import _lib
    lib = _lib.lib()
    M, n, h = 70, 9, 0.125
    v = np.random.RandomState(4).randn(M, n)
    buf = _slab(v)
    ld = buf.shape[1]
    state = _state(M, 123.25)
    u, s, st = buf.data_ptr(), state.data_ptr(), _lib.stream()
    nan, inf = float('nan'), float('inf')
    good = dict(M=M, n_cols=n, u=u, row_stride=ld, col_stride=1, k_first=0, h=h, threshold=THETA, fresh=1, state=s)
    cases = [
        (' u is null', dict(u=None)), (' state is null', dict(state=None)), (' M = -1', dict(M=-1)),
        (' n_cols = -1', dict(n_cols=-1)), (' fresh with n_cols = 0', dict(n_cols=0, fresh=1)),
        (' k_first = -1', dict(k_first=-1)),
        (' h = ', dict(h=0.0)), (' h = ', dict(h=-0.125)), (' h = ', dict(h=nan)), (' h = ', dict(h=inf)),
        (' threshold is NaN', dict(threshold=nan)),
        (' row_stride = 2, col_stride = 2', dict(row_stride=2, col_stride=2)),
        (' row_stride = %d, col_stride = 1' % (n - 1), dict(row_stride=n - 1, col_stride=1)),
        (' row_stride = 1, col_stride = %d' % (M - 1), dict(row_stride=1, col_stride=M - 1)),
        (' row_stride = 0,', dict(row_stride=0, col_stride=1)), (' col_stride = 0', dict(row_stride=ld, col_stride=0)),
        (' row_stride = -%d' % ld, dict(row_stride=-ld, col_stride=1)),
    ]
    order = ('M', 'n_cols', 'u', 'row_stride', 'col_stride', 'k_first', 'h', 'threshold', 'fresh', 'state')
    for name, change in cases:
        a = dict(good, **change)
        rc = lib.stk_history_scan(st, *[a[k] for k in order])
        text = lib.stk_last_error().decode()
        assert rc != 0 and 'stk_history_scan' in text and name in text, (name, change, rc, text)
        with pytest.raises(_lib.StkError):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((state == 123.25).all())
    # the no-op leaves it too; then the good call goes through, +-inf thresholds included
    assert lib.stk_history_scan(st, *[dict(good, n_cols=0, fresh=0)[k] for k in order]) == 0
    torch.cuda.synchronize()
    assert bool((state == 123.25).all())
    for theta in (inf, -inf, THETA):
        assert lib.stk_history_scan(st, *[dict(good, threshold=theta)[k] for k in order]) == 0
    assert same(state.cpu().numpy(), numpy_history_scan(v, 0, h, THETA))
    kept = state.clone()
    assert lib.stk_history_scan(st, *[dict(good, n_cols=0, fresh=0, k_first=n)[k] for k in order]) == 0
    assert torch.equal(torch.nan_to_num(state, nan=-7.0), torch.nan_to_num(kept, nan=-7.0))


# ---- 5. the public call -------------------------------------------------------------------------------------------
def _solver(J_space, J_time, comm=None, **kw):
    import heateq_mpi as hm
    from source.comm import Comm
    return hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem='square_moving_source',
                              comm=Comm(distributed=False) if comm is None else comm, **kw)


def _free_vertices(heat):
    from source.assembly import free_dofs
    mesh = heat._sample_meshes[0]
    return np.ascontiguousarray(np.asarray(mesh.points, dtype=np.float64)[free_dofs(mesh)])


def _numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


THRESHOLD_KEYS = ['t_first', 't_last', 'time_above']
OTHER_KEYS = ['dose', 'max_rate', 'min_rate', 'peak', 't_peak']


def test_public_call_on_a_seeded_vector():
    from source import driver
    from source.history import FIELDS, STATE_ROWS
    from source.mpi_vector import KronVectorMPI
    heat = _solver(3, 3)
    u = driver.seeded_vector(heat, KronVectorMPI)
    X = u.X_loc.cpu().numpy()  # (N, M)
    theta, h = float(np.median(X)), float(heat._sample_meshes[1].h)
    want = numpy_history_scan(X.T, 0, h, theta)
    nodal = _numpy(heat.history_maps(u, theta))
    assert heat.sample_plan is None  # the nodal form needs no plan
    assert sorted(nodal) == sorted(FIELDS)
    for key, value in nodal.items():
        assert value.shape == (heat.M,) and same(value, want[STATE_ROWS.index(key)]), key
    assert nodal['time_above'].max() > 0.0
    # at the free vertices the per-point form samples the slab back
    points = np.concatenate([_free_vertices(heat), [[2.0, 2.0]]])
    at = _numpy(heat.history_maps(u, theta, points=points))
    assert sorted(at) == sorted(FIELDS + ('inside',))
    assert at['inside'].dtype == bool and at['inside'][:-1].all() and not at['inside'][-1]
    for key in FIELDS:
        assert at[key].shape == (heat.M + 1,) and same(at[key][:-1], nodal[key]), key
        assert np.isnan(at[key][-1]), key
    # without a threshold: exactly the three threshold keys are gone, nothing else moves
    for points_, full in ((None, nodal), (points, at)):
        plain = _numpy(heat.history_maps(u, points=points_))
        assert sorted(plain) == sorted(k for k in full if k not in THRESHOLD_KEYS)
        for key, value in plain.items():
            assert same(value, full[key]), key
    only = heat.history_maps(u, theta, fields=('dose', 't_last'))
    assert sorted(only) == ['dose', 't_last'] and same(only['dose'].cpu().numpy(), nodal['dose'])
    # the checks come before the GPU; a test-space vector is refused
    with pytest.raises(ValueError, match='NaN'):
        heat.history_maps(u, float('nan'))
    with pytest.raises(ValueError, match='points of shape'):
        heat.history_maps(u, theta, points=np.zeros((3, 3)))
    with pytest.raises(ValueError, match='needs a threshold'):
        heat.history_maps(u, fields=('t_first',))
    with pytest.raises(AssertionError, match='trial space'):
        heat.history_maps(heat.g, theta)


def test_serial_class_takes_flat_and_device_vectors():
    import heateq
    from source.history import FIELDS
    from source.linop import device_vector
    heat = heateq.HeatEquation(J_space=3, J_time=3, problem='square_moving_source', precond='direct')
    X = np.random.RandomState(5).rand(heat.N, heat.M)
    theta, h = float(np.median(X)), float(heat._sample_meshes[1].h)
    flat = _numpy(heat.history_maps(X.reshape(-1), theta))
    assert heat.sample_plan is None
    on_device = _numpy(heat.history_maps(device_vector(X.reshape(-1), heat.N), theta))
    want = numpy_history_scan(X.T, 0, h, theta)
    assert sorted(flat) == sorted(on_device) == sorted(FIELDS)
    for row, key in enumerate(FIELDS):
        assert same(flat[key], want[row]) and same(on_device[key], want[row]), key
    points = _free_vertices(heat)
    at = _numpy(heat.history_maps(X.reshape(-1), theta, points=points))
    assert at['inside'].all() and all(same(at[key], flat[key]) for key in FIELDS)
    with pytest.raises(ValueError, match='NaN'):
        heat.history_maps(X.reshape(-1), float('nan'))
    with pytest.raises(AssertionError, match='trial space'):
        heat.history_maps(device_vector(np.zeros(heat.N_Y * heat.M), heat.N_Y), theta)


def test_after_a_solve_of_the_moving_source():
    from source.sampling import raster
    heat = _solver(3, 3, precond='direct')
    u, _ = heat.solve()
    mesh_space, mesh_time = heat._sample_meshes
    h, T, N = float(mesh_time.h), float(mesh_time.T), heat.N
    pts = raster(mesh_space, 23)
    block = heat.sample(u, np.array([float(k) * h for k in range(N)]), pts)
    assert not bool(torch.isnan(block).any())
    theta = 0.5 * float(block.max())
    got = heat.history_maps(u, theta, points=pts)
    assert bool(got['inside'].all())
    assert torch.equal(got['peak'], block.max(dim=0).values)
    dose = torch.trapezoid(block, dx=h, dim=0)
    gap = float((got['dose'] - dose).abs().max())
    print('dose against torch.trapezoid: %.3e of max|dose| %.3e' % (gap, float(dose.abs().max())))
    assert gap <= 1e-12 * float(dose.abs().max())
    above = got['time_above']
    assert bool(((above >= 0.0) & (above <= T)).all()) and float(above.max()) > 0.0
    first, last = got['t_first'], got['t_last']
    both = ~torch.isnan(first) & ~torch.isnan(last)
    assert bool(both.any()) and bool((first[both] <= last[both]).all())
    assert torch.equal(torch.isnan(first), torch.isnan(last))
    assert bool((above[~both] == 0.0).all())


# ---- 6. rank independence ---------------------------------------------------------------------------------------
_lock = threading.Lock()  # plan construction reads process-wide tuning keys


def _rank_run(comm, J_time):
    from source import driver
    from source.mpi_vector import KronVectorMPI
    with _lock:
        heat = _solver(4, J_time, comm=comm)
    u = driver.seeded_vector(heat, KronVectorMPI)  # the same global vector on every rank count
    theta = 0.5
    nodal = _numpy(heat.history_maps(u, theta))
    points = np.concatenate([_free_vertices(heat), [[0.3, 0.7], [-1.0, 0.5]]])
    at = _numpy(heat.history_maps(u, theta, points=points))
    return nodal, at


@functools.lru_cache(maxsize=None)
def _one_rank(J_time):
    return _rank_run(None, J_time)


@pytest.mark.parametrize('J_time,ranks', [(3, 2), (3, 3), (3, 8), (2, 5)])
def test_history_maps_do_not_depend_on_the_number_of_ranks(J_time, ranks):
    """Both forms, every key, every rank: array_equal to the one-rank dict.  (2, 5): five
    nodes on five ranks -- every scan is a single column with a carried state."""
    from thread_comm import run_ranks
    got = run_ranks(ranks, lambda comm: _rank_run(comm, J_time))
    one = _one_rank(J_time)
    assert one[0]['time_above'].max() > 0.0 and np.isnan(one[1]['peak'][-1]) and not one[1]['inside'][-1]
    for rank in range(ranks):
        for form in (0, 1):
            assert sorted(got[rank][form]) == sorted(one[form])
            for key, value in one[form].items():
                assert same(got[rank][form][key], value), (rank, form, key)


# ---- 7. the torch composition of the timing tool -------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location('history_time', os.path.join(REPO, 'tools', 'history_time.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_timed_composition_computes_what_the_kernel_computes():
    M, n, h = 1000, 65, 1.0 / 64
    v = np.random.RandomState(7).randn(M, n)
    buf = _slab(v)
    state = _scan(buf, M, n, (buf.shape[1], 1), 0, h, THETA, _state(M), True)
    ref = _tool().torch_composition(buf[:, :n], h, THETA)
    for key, row in (('peak', PEAK), ('max_rate', MAX_RATE), ('min_rate', MIN_RATE)):
        assert torch.equal(ref[key], state[row]), key
    for key, row in (('dose', DOSE), ('time_above', ABOVE)):
        gap, size = float((ref[key] - state[row]).abs().max()), float(state[row].abs().max())
        print('%s: kernel against composition %.3e of %.3e' % (key, gap, size))
        assert gap <= 1e-12 * size, key


# ---- 8. the drivers ----------------------------------------------------------------------------------------------------
def test_drivers_write_history_out(tmp_path, monkeypatch, capsys):
    import heateq
    import heateq_mpi as hm
    from source.mpi_kron import LinearOperatorMPI
    from source.sampling import raster
    monkeypatch.setattr(LinearOperatorMPI, 'sync_timing', LinearOperatorMPI.sync_timing)  # main() sets it
    common = ['--J_time', '2', '--J_space', '2', '--problem', 'square_moving_source']
    for name, main in (('mpi', hm.main), ('serial', heateq.main)):
        out = str(tmp_path / (name + '.npz'))
        res = main(common + ['--history_out', out, '--history_threshold', '0.01', '--history_raster', '17'])
        heat, u = res[0], res[1]
        data = np.load(out)
        assert sorted(data.files) == sorted(['points', 'inside'] + THRESHOLD_KEYS + OTHER_KEYS)
        points = raster(heat._sample_meshes[0], 17)
        assert data['points'].shape == (289, 2) and np.array_equal(data['points'], points)
        assert data['inside'].dtype == bool and data['inside'].shape == (289,) and data['inside'].all()
        direct = _numpy(heat.history_maps(u, 0.01, points=points))
        for key in THRESHOLD_KEYS + OTHER_KEYS:
            assert data[key].shape == (289,) and same(data[key], direct[key]), (name, key)
        assert 'history_' not in capsys.readouterr().out  # what the drivers print is what it was
        # without a threshold the three threshold arrays are not written
        plain = str(tmp_path / (name + '_plain.npz'))
        main(common + ['--history_out', plain, '--history_raster', '5'])
        assert sorted(np.load(plain).files) == sorted(['points', 'inside'] + OTHER_KEYS)
        # without the option nothing is written and nothing is built
        before = sorted(os.listdir(tmp_path))
        res = main(common)
        assert res[0].sample_plan is None and sorted(os.listdir(tmp_path)) == before
