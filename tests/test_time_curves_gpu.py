"""The time curves on the device (csrc/curves.hip, source/time_curves.py) against the NumPy
contract of tests/test_time_curves_host.py -- array_equal, NaN-aware, on every row: at every
tile edge and column count, every launch form, the infinite thresholds, the refusals, the
public call of both drivers, its independence of the number of ranks, the torch composition
the timing tool compares with, and the drivers' --curves_out."""
import functools
import importlib.util
import os
import threading
import types

import numpy as np
import pytest
import torch

from test_history_host import same
from test_time_curves_host import (_mesh, _tolerance, cell_geometry, dict_from_table, first_cells, numpy_boundary_faces,
                                   numpy_time_curves, planted_values, row_map)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COLS = (1, 2, 3, 8, 9, 17, 65)
INF = float('inf')

MESHES = {
    'square0': lambda: _mesh('square', 0),  # 8 cells, one free dof
    'square1': lambda: _mesh('square', 1),
    'square2': lambda: _mesh('square', 2),
    'square4': lambda: _mesh('square', 4),  # 2048 cells: eight tiles
    'lshape_jitter3': lambda: _mesh('lshape_jitter', 3),
    'cube1': lambda: _mesh('cube', 1),
    'cube2': lambda: _mesh('cube', 2),
    'first255': lambda: first_cells(_mesh('square', 4), 255),  # tail lanes
    'first256': lambda: first_cells(_mesh('square', 4), 256),  # exactly one tile
    'first257': lambda: first_cells(_mesh('square', 4), 257),  # a second tile of one cell
    'first513': lambda: first_cells(_mesh('square', 4), 513),  # two full tiles and a third of one cell
}


class _Case:
    """A mesh with its plan and, per threshold, the planted slab values (M, 65) and the
    contract's table of them -- computed once, shared by the tests, never changed."""
    def __init__(self, name):
        from source.time_curves import CurvesPlan
        self.mesh = MESHES[name]()
        self.plan = CurvesPlan(self.mesh, None)
        self.points = np.asarray(self.mesh.points, dtype=np.float64)
        self.cells = np.asarray(self.mesh.cells, dtype=np.int64)
        self.row_of, self.faces = row_map(self.mesh), numpy_boundary_faces(self.cells)
        self.d, self.M = self.plan.d, self.plan.n_free
        self._kept = {}

    def contract(self, U, theta):
        return numpy_time_curves(self.points, self.cells, self.row_of, U, theta, faces=self.faces)

    def reference(self, theta):
        if theta not in self._kept:
            U = planted_values(np.random.RandomState(1000 + len(self.cells)), self.M, max(N_COLS), theta if np.isfinite(theta) else 0.3)
            want = self.contract(U, theta)
            U.setflags(write=False), want.setflags(write=False)
            self._kept[theta] = (U, want)
        return self._kept[theta]


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


def _dev(a):
    from source import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(_lib.compute_device())


def _slab(v):
    """(M, ld) device slab of the rows v (M, n) with an even ld > n, the padding NaN."""
    M, n = v.shape
    buf = np.full((M, (n | 1) + 1), np.nan)
    buf[:, :n] = v
    return _dev(buf)


def _eval(case, slab, n, theta, out=None, first=0, ld_out=None):
    """The table (rows, n) of the columns [first, first + n) of a slab."""
    from source.time_curves import curves_eval, n_rows
    R = n_rows(case.d)
    ld_out = n + 3 if ld_out is None else ld_out
    if out is None:
        out = torch.full((R, ld_out), -7.0, dtype=torch.float64, device=slab.device)
    curves_eval(case.plan, slab.data_ptr() + 8 * first, case.M, n, slab.shape[1], theta, out, ld_out)
    assert bool((out[:, n:] == -7.0).all())  # nothing beyond the columns asked for
    return out[:, :n].cpu().numpy()


class _setting:
    """stk_curves_tile / stk_curves_batch for the block."""
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from source import _lib
        _lib.check(getattr(_lib.lib(), self.name)(self.value))

    def __exit__(self, *exc):
        from source import _lib
        _lib.check(getattr(_lib.lib(), self.name)(0))


# ---- 1. the device is the contract ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(MESHES))
def test_device_is_the_contract(name):
    """theta = 0.3 on the planted data, theta = 1.0 where the planted integer columns have
    vertices exactly AT it, and both infinities; 1 .. 65 columns of a slab whose padding is NaN."""
    case = _case(name)
    at = _rows(case.d)
    for theta in (0.3, 1.0, INF, -INF):
        U, want = case.reference(theta)
        for n in N_COLS:
            slab = _slab(U[:, :n])
            assert slab.shape[1] % 2 == 0 and bool(torch.isnan(slab[:, n:]).all())
            got = _eval(case, slab, n, theta)
            for q in range(len(want)):
                assert same(got[q], want[q, :n]), (name, theta, n, q, got[q], want[q, :n])
            sums = got[:at['peak_row'] + 1]
            assert not np.isnan(sums).any()  # no padding column came in
            if theta == INF:
                assert np.all(got[at['measure_above']] == 0.0) and np.isnan(got[at['box_lo']]).all()
            else:
                empty = got[at['measure_above']] == 0.0
                assert np.array_equal(np.isnan(got[at['box_lo']]).any(axis=0), np.isnan(got[at['box_hi']]).any(axis=0))
                assert not np.isnan(got[at['box_lo']][:, ~empty]).any()
            if theta == -INF:
                vol, _ = cell_geometry(case.points, case.cells)
                assert not np.isnan(got).any() and abs(got[at['measure_above'], 0] - vol.sum()) <= _tolerance(vol)


def _rows(d):
    from source.time_curves import rows
    return rows(d)


@pytest.mark.parametrize('name', ['first257', 'cube2'])
def test_nan_and_inf_in_the_slab_give_what_the_contract_gives(name):
    case = _case(name)
    U = np.random.RandomState(21).randn(case.M, 5)
    U[3 % case.M, 0], U[5 % case.M, 1], U[7 % case.M, 2], U[:, 3] = np.nan, np.inf, -np.inf, np.nan
    for theta in (0.3, -INF):
        got = _eval(case, _slab(U), 5, theta)
        assert same(got, case.contract(U, theta)), (name, theta)


def _faces_by_sorting(cells):
    """numpy_boundary_faces without its loop over the cells: the face keys of all cells sorted and
    counted at once."""
    nc, nl = cells.shape
    keys = np.concatenate([np.sort(np.delete(cells, a, axis=1), axis=1) for a in range(nl)])
    _, inverse, count = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    alone = (count[inverse.reshape(-1)] == 1).reshape(nl, nc)
    mask = np.zeros(nc, dtype=np.uint8)
    for a in range(nl):
        mask |= alone[a].astype(np.uint8) << a
    return mask


# more than 256 tiles: the finish kernel adds in place in global memory before it goes to LDS
PAST_256_TILES = {
    # 258 cell tiles (one step, two partners) beside 1021 row tiles for the peak and the box (two steps)
    'square8 first 65793': lambda: first_cells(_mesh('square', 8), 65793),
    # 512 cell tiles: one step with every partner present
    'square7': lambda: _mesh('square', 7),
    # 2048 cell tiles: three steps, every partner present
    'square8': lambda: _mesh('square', 8),
    # 3 cell tiles beside 4088 row tiles: the sums stay in LDS, the peak and the box take four steps
    'square9 first 513': lambda: first_cells(_mesh('square', 9), 513),
}


@pytest.mark.parametrize('name', sorted(PAST_256_TILES))
def test_finish_kernel_past_256_tiles(name):
    """The global stage of curves_finish_kernel, with its four kinds of join and n_tiles differing
    from n_work, against the contract: 1 and 3 columns, theta = 0.3 and +inf.  A peak planted in
    tile 0 and again, with the same value, in a tile at or above 256 comes back with the lower
    row -- the tie rule of the join across a global step; in the third column the two equal peaks
    lie in the tiles 10 and 300.
    The contract's Python loop over the cells for the boundary faces would take minutes on the
    whole of square 8; the faces are counted by sorting instead (_faces_by_sorting, checked
    against that loop on the first 513 cells of every case)."""
    from source.time_curves import CurvesPlan
    mesh = PAST_256_TILES[name]()
    plan = CurvesPlan(mesh, None)
    points, cells = np.asarray(mesh.points, dtype=np.float64), np.asarray(mesh.cells, dtype=np.int64)
    case = types.SimpleNamespace(plan=plan, d=plan.d, M=plan.n_free)
    M, at = case.M, _rows(plan.d)
    n_tiles, row_tiles = -(-len(cells) // 256), -(-M // 256)
    assert max(n_tiles, row_tiles) > 256
    faces = _faces_by_sorting(cells)
    assert np.array_equal(_faces_by_sorting(cells[:513]), numpy_boundary_faces(cells[:513]))
    row_of = row_map(mesh)
    again_0, again_2 = min(256 * 299 + 7, M - 2), min(256 * 300 + 1, M - 1)  # (square 7 has 255 row tiles)
    for theta in (0.3, INF):
        U = planted_values(np.random.RandomState(len(cells)), M, 3, 0.3)
        U[5, 0] = U[again_0, 0] = 9.5
        U[256 * 10 + 3, 2] = U[again_2, 2] = 9.5
        want = numpy_time_curves(points, cells, row_of, U, theta, faces=faces)
        assert want[at['peak_row'], 0] == 5.0 and want[at['peak_row'], 2] == 256.0 * 10 + 3
        assert want[at['peak'], 0] == 9.5 and want[at['peak'], 2] == 9.5
        for n in (1, 3):
            got = _eval(case, _slab(U[:, :n]), n, theta)
            for q in range(len(want)):
                assert same(got[q], want[q, :n]), (name, theta, n, q, got[q], want[q, :n])
            assert not np.isnan(got[:at['peak_row'] + 1]).any()  # no padding column came in
            assert got[at['peak_row'], 0] == 5.0


# ---- 2. every launch form gives the same doubles ---------------------------------------------------------------
@pytest.mark.parametrize('name', ['first513', 'cube2', 'square4'])
def test_every_launch_form_gives_the_one_shot_doubles(name):
    from source import _lib
    from source.time_curves import n_rows
    case = _case(name)
    U, want = case.reference(0.3)
    n = 17
    slab = _slab(U[:, :n])
    whole = _eval(case, slab, n, 0.3)
    assert same(whole, want[:, :n])
    # EVERY accepted column chunk, 1 .. 32: most do not divide 17, those above it take all at once
    for cols in range(1, 33):
        with _setting('stk_curves_tile', cols):
            assert same(_eval(case, slab, n, 0.3), whole), cols
    # column batches smaller than n_cols: 1, 2, 5 columns of partials, and a cap below one column
    per_column = 8 * n_rows(case.d) * max(-(-len(case.cells) // 256), -(-case.M // 256))
    for cap in (8, per_column, 2 * per_column, 5 * per_column + 8):
        with _setting('stk_curves_batch', cap):
            assert same(_eval(case, slab, n, 0.3), whole), cap
            with _setting('stk_curves_tile', 2):
                assert same(_eval(case, slab, n, 0.3), whole), cap
    # column ranges [0, s) + [s, n) for every s, the second from base + 8 s (odd and even s)
    m = 9
    for s in range(1, m):
        out = torch.full((n_rows(case.d), m + 3), -7.0, dtype=torch.float64, device=slab.device)
        _eval(case, slab, s, 0.3, out=out, ld_out=m + 3)
        from source.time_curves import curves_eval
        curves_eval(case.plan, slab.data_ptr() + 8 * s, case.M, m - s, slab.shape[1], 0.3, out.data_ptr() + 8 * s, m + 3)
        assert same(out[:, :m].cpu().numpy(), whole[:, :m]), s
        assert bool((out[:, m:] == -7.0).all())
    lib = _lib.lib()
    for fn, bad, text in ((lib.stk_curves_tile, -1, 'cols'), (lib.stk_curves_tile, 33, 'cols'),
                          (lib.stk_curves_batch, -1, 'bytes'), (lib.stk_curves_batch, (8 << 20) + 1, 'bytes')):
        assert fn(bad) != 0 and text in lib.stk_last_error().decode(), (bad, text)
    assert lib.stk_curves_tile(0) == 0 and lib.stk_curves_batch(0) == 0
    assert same(_eval(case, slab, n, 0.3), whole)  # a refused value changed nothing


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_out():
    from source import _lib
    from source.time_curves import n_rows
    lib = _lib.lib()
    case = _case('square2')
    U, want = case.reference(0.3)
    n = 9
    slab = _slab(U[:, :n])
    out = torch.full((n_rows(case.d), n), 123.25, dtype=torch.float64, device=slab.device)
    good = dict(plan=case.plan._plan, M=case.M, n_cols=n, slab=slab.data_ptr(), row_stride=slab.shape[1], threshold=0.3,
                ld_out=n, out=out.data_ptr())
    order = ('plan', 'M', 'n_cols', 'slab', 'row_stride', 'threshold', 'ld_out', 'out')
    cases = [(' plan is null', dict(plan=None)), (' slab is null', dict(slab=None)), (' out is null', dict(out=None)),
             (' n_cols = 0', dict(n_cols=0)), (' n_cols = -3', dict(n_cols=-3)),
             (' M = %d' % (case.M + 1), dict(M=case.M + 1)), (' M = 0', dict(M=0)),
             (' threshold is NaN', dict(threshold=float('nan'))), (' ld_out = %d' % (n - 1), dict(ld_out=n - 1)),
             (' row_stride = %d' % (n - 1), dict(row_stride=n - 1))]
    for text, change in cases:
        a = dict(good, **change)
        rc = lib.stk_curves_eval(_lib.stream(), *[a[k] for k in order])
        said = lib.stk_last_error().decode()
        assert rc != 0 and 'stk_curves_eval' in said and text in said, (text, rc, said)
        with pytest.raises(_lib.StkError):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((out == 123.25).all())
    for theta in (INF, -INF, 0.3):
        assert lib.stk_curves_eval(_lib.stream(), *[dict(good, threshold=theta)[k] for k in order]) == 0
    assert same(out.cpu().numpy(), want[:, :n])


# ---- 4. the public call -------------------------------------------------------------------------------------------
def _solver(problem, J_space, J_time, comm=None, **kw):
    import heateq_mpi as hm
    from source.comm import Comm
    return hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem=problem,
                              comm=Comm(distributed=False) if comm is None else comm, **kw)


def _numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _node_values(N, M, seed):
    """(N, M): uniform numbers, every third node not positive (an empty zone there)."""
    X = np.random.RandomState(seed).rand(N, M)
    X[::3] *= -1.0
    return X


def _check_dict(heat, got, X, threshold):
    from source.assembly import free_dofs
    from source.time_curves import ALWAYS, FIELDS
    mesh = heat._sample_meshes[0]
    p, cells = np.asarray(mesh.points, dtype=np.float64), np.asarray(mesh.cells, dtype=np.int64)
    d, N = p.shape[1], X.shape[0]
    theta = INF if threshold is None else threshold
    table = numpy_time_curves(p, cells, row_map(mesh), X.T, theta)
    want = dict_from_table(table, d, p[free_dofs(mesh)], threshold)
    assert sorted(got) == sorted(want) == sorted(ALWAYS if threshold is None else FIELDS)
    for key, value in want.items():
        assert got[key].shape == value.shape and same(got[key], value), key
        assert got[key].shape == ((N, d) if key in ('peak_point', 'moment_above', 'centroid_above', 'box_lo', 'box_hi') else (N,))
    assert got['peak_row'].dtype == np.int64
    assert same(got['peak'], X.max(axis=1)) and same(got['peak_row'], X.argmax(axis=1))
    assert same(got['peak_point'], p[free_dofs(mesh)][X.argmax(axis=1)])
    if threshold is not None:
        empty = got['measure_above'] == 0.0
        assert empty.any() and not empty.all()
        assert np.array_equal(np.isnan(got['centroid_above']), np.repeat(empty[:, None], d, axis=1))
        assert np.array_equal(np.isnan(got['box_lo']), np.repeat(empty[:, None], d, axis=1))
        inside = ~empty
        assert np.all(got['centroid_above'][inside] >= got['box_lo'][inside] - 1e-12)
        assert np.all(got['centroid_above'][inside] <= got['box_hi'][inside] + 1e-12)


@pytest.mark.parametrize('problem,J', [('square_moving_source', 3), ('cube_forced', 2)])
def test_public_call_of_both_drivers(problem, J):
    import heateq
    from source.linop import device_vector
    from source.mpi_vector import KronVectorMPI
    heat = _solver(problem, J, 3)
    X = _node_values(heat.N, heat.M, 31)
    u = KronVectorMPI(heat.dofs_distr, X)
    assert heat.curves_plan is None  # nothing is built without the call
    with pytest.raises(ValueError, match='NaN'):
        heat.time_curves(u, float('nan'))
    with pytest.raises(AssertionError, match='trial space'):
        heat.time_curves(heat.g, 0.25)
    assert heat.curves_plan is None
    _check_dict(heat, _numpy(heat.time_curves(u, 0.25)), X, 0.25)
    plan = heat.curves_plan
    assert plan is not None
    _check_dict(heat, _numpy(heat.time_curves(u)), X, None)
    assert heat.curves_plan is plan and heat.sample_plan is None and heat.error_plan is None

    serial = heateq.HeatEquation(J_space=J, J_time=3, problem=problem, precond='direct')
    assert (serial.N, serial.M) == (heat.N, heat.M) and serial.curves_plan is None
    with pytest.raises(ValueError, match='NaN'):
        serial.time_curves(X.reshape(-1), float('nan'))
    with pytest.raises(AssertionError, match='trial space'):
        serial.time_curves(device_vector(np.zeros(serial.N_Y * serial.M), serial.N_Y), 0.25)
    assert serial.curves_plan is None
    flat = _numpy(serial.time_curves(X.reshape(-1), 0.25))
    on_device = _numpy(serial.time_curves(device_vector(X.reshape(-1), serial.N), 0.25))
    _check_dict(serial, flat, X, 0.25)
    _check_dict(serial, on_device, X, 0.25)
    _check_dict(serial, _numpy(serial.time_curves(X.reshape(-1))), X, None)
    assert serial.sample_plan is None


def test_a_node_of_nothing_but_nan_has_no_peak_point():
    """peak_row = M and peak = -inf there, and the lookup of the public dict fills peak_point
    with NaN instead of indexing the mesh points with M; the other nodes keep theirs."""
    from source.assembly import free_dofs
    from source.mpi_vector import KronVectorMPI
    heat = _solver('square_moving_source', 3, 3)
    X = _node_values(heat.N, heat.M, 32)
    X[4] = np.nan
    got = _numpy(heat.time_curves(KronVectorMPI(heat.dofs_distr, X), 0.25))
    mesh = heat._sample_meshes[0]
    p = np.asarray(mesh.points, dtype=np.float64)
    table = numpy_time_curves(p, np.asarray(mesh.cells, dtype=np.int64), row_map(mesh), X.T, 0.25)
    want = dict_from_table(table, 2, p[free_dofs(mesh)], 0.25)
    assert sorted(got) == sorted(want)
    for key, value in want.items():
        assert got[key].shape == value.shape and same(got[key], value), key
    assert got['peak_row'][4] == heat.M and got['peak'][4] == -INF
    assert np.array_equal(np.isnan(got['peak_point']).all(axis=1), np.arange(heat.N) == 4)
    assert not np.isnan(np.delete(got['peak_point'], 4, axis=0)).any()


# ---- 5. rank independence ---------------------------------------------------------------------------------------
_lock = threading.Lock()  # plan construction reads process-wide tuning keys


def _rank_run(comm, J_time):
    from source import driver
    from source.mpi_vector import KronVectorMPI
    with _lock:
        heat = _solver('square_moving_source', 3, J_time, comm=comm)
    u = driver.seeded_vector(heat, KronVectorMPI)  # the same global vector on every rank count
    return _numpy(heat.time_curves(u, 0.5)), _numpy(heat.time_curves(u))


@functools.lru_cache(maxsize=None)
def _one_rank(J_time):
    return _rank_run(None, J_time)


@pytest.mark.parametrize('J_time,ranks', [(3, 2), (3, 3), (3, 8), (2, 5)])
def test_time_curves_do_not_depend_on_the_number_of_ranks(J_time, ranks):
    """Every tensor, every rank: array_equal to the one-rank dict.  (2, 5): five nodes on five
    ranks -- every call is a single column."""
    from thread_comm import run_ranks
    got = run_ranks(ranks, lambda comm: _rank_run(comm, J_time))
    one = _one_rank(J_time)
    assert one[0]['measure_above'].min() > 0.0 and len(one[0]) == 12 and len(one[1]) == 7
    for rank in range(ranks):
        for form in (0, 1):
            assert sorted(got[rank][form]) == sorted(one[form])
            for key, value in one[form].items():
                assert same(got[rank][form][key], value), (rank, form, key)


# ---- 6. the torch composition of the timing tool -------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location('time_curves_time', os.path.join(REPO, 'tools', 'time_curves_time.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.mark.parametrize('name', ['square4', 'cube2'])
def test_the_timed_composition_computes_what_the_kernel_computes(name):
    case = _case(name)
    at = _rows(case.d)
    n = 9
    U = 0.05 * np.random.RandomState(41).randn(case.M, n)  # every sum O(1): the host file's tolerance
    U[:, 4] = np.where(np.arange(case.M) % 5 == 2, 0.5, U[:, 4])  # ties for the peak
    slab = _slab(U)
    got = _eval(case, slab, n, INF)
    tool = _tool()
    comp = tool.Composition(case.mesh, slab)
    sums, extrema = _numpy(comp.sums(slab[:, :n])), _numpy(tool.Composition.extrema(slab[:, :n]))
    vol, _ = cell_geometry(case.points, case.cells)
    tol = _tolerance(vol)
    for key, value in sums.items():
        gap = np.abs(value - got[at[key]]).max()
        print('%s %s: kernel against composition %.3e of %.3e (tolerance %.1e)' % (name, key, gap, np.abs(value).max(), tol))
        assert gap <= tol, key
    assert np.array_equal(extrema['peak'], got[at['peak']]) and np.array_equal(extrema['peak_row'], got[at['peak_row']])
    assert got[at['peak_row'], 4] == 2.0


# ---- 7. the drivers ----------------------------------------------------------------------------------------------------
def test_drivers_write_curves_out(tmp_path, monkeypatch, capsys):
    import heateq
    import heateq_mpi as hm
    from source.mpi_kron import LinearOperatorMPI
    from source.time_curves import ALWAYS, FIELDS
    monkeypatch.setattr(LinearOperatorMPI, 'sync_timing', LinearOperatorMPI.sync_timing)  # main() sets it
    common = ['--J_time', '2', '--J_space', '2', '--problem', 'square_moving_source']
    for name, main in (('mpi', hm.main), ('serial', heateq.main)):
        out = str(tmp_path / (name + '.npz'))
        res = main(common + ['--curves_out', out, '--curves_threshold', '0.01'])
        heat, u = res[0], res[1]
        data = np.load(out)
        assert sorted(data.files) == sorted(('times',) + FIELDS)
        h = float(heat._sample_meshes[1].h)
        assert np.array_equal(data['times'], np.array([k * h for k in range(heat.N)]))
        direct = _numpy(heat.time_curves(u, 0.01))
        for key in FIELDS:
            assert same(data[key], direct[key]), (name, key)
        assert data['heat'].shape == (heat.N,) and data['box_hi'].shape == (heat.N, 2) and data['heat'].max() > 0.0
        assert 'curves_' not in capsys.readouterr().out  # what the drivers print is what it was
        plain = str(tmp_path / (name + '_plain.npz'))
        main(common + ['--curves_out', plain])
        assert sorted(np.load(plain).files) == sorted(('times',) + ALWAYS)
        # without the option nothing is written and nothing is built
        before = sorted(os.listdir(tmp_path))
        res = main(common)
        assert res[0].curves_plan is None and sorted(os.listdir(tmp_path)) == before
