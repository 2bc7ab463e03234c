"""The isotherms on the device (csrc/iso.hip, source/isotherms.py) against the NumPy contract
of tests/test_isotherms_host.py -- array_equal, NaN-aware, the counts table and every record:
at every tile edge and column count, every launch form, with tables that do not belong
together, NaN and inf in the slab, the refusals, the public call of both drivers, its
independence of the number of ranks, the torch composition the timing tool compares with, and
the drivers' --iso_out."""
import functools
import importlib.util
import os
import threading

import numpy as np
import pytest
import torch

from test_history_host import same
from test_isotherms_host import MESHES, N_PLANTED, numpy_dict, numpy_isotherms, planted
from test_time_curves_host import row_map

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COLS = (1, 2, 3, 8, 9, 17, 65)
INF = float('inf')
SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def _plan(name):
    from source.time_curves import CurvesPlan
    return CurvesPlan(planted(name).mesh, None)


def _dev(a):
    from source import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(_lib.compute_device())


def _slab(v):
    """(M, ld) device slab of the rows v (M, n) with an even ld > n, the padding NaN."""
    M, n = v.shape
    buf = np.full((M, (n | 1) + 1), np.nan)
    buf[:, :n] = v
    return _dev(buf)


def _first(counts):
    flat = counts.reshape(-1)
    return (torch.cumsum(flat, 0) - flat).reshape(counts.shape)


def _count(name, slab, n, theta, first=0):
    """The counts table (n, n_tiles) of the columns [first, first + n) of a slab; nothing is
    written beyond it."""
    from source.isotherms import iso_count
    case = planted(name)
    counts = torch.full((n + 1, case.n_tiles), -5, dtype=torch.int64, device=slab.device)
    iso_count(_plan(name), slab.data_ptr() + 8 * first, case.M, n, slab.shape[1], theta, counts)
    assert bool((counts[n] == -5).all())
    return counts[:n]


def _fill(name, slab, n, theta, counts, first_table=None, first=0, n_out=None, room=3):
    """The table of records (n_out + room, W) the fill leaves, sentinel where it wrote nothing."""
    from source.isotherms import iso_fill
    case = planted(name)
    total = int(counts.sum())
    n_out = total if n_out is None else n_out
    first_table = _first(counts) if first_table is None else first_table
    out = torch.full((n_out + room, case.W), SENTINEL, dtype=torch.float64, device=slab.device)
    iso_fill(_plan(name), slab.data_ptr() + 8 * first, case.M, n, slab.shape[1], theta, counts.contiguous(),
             first_table.contiguous(), n_out, out)
    return out.cpu().numpy()


def _records(name, slab, n, theta, first=0):
    """(counts, records) of the columns [first, first + n): the two calls and the scan between."""
    counts = _count(name, slab, n, theta, first)
    out = _fill(name, slab, n, theta, counts, first=first)
    total = int(counts.sum())
    assert np.all(out[total:] == SENTINEL)  # rows beyond the total keep the sentinel
    return counts.cpu().numpy(), out[:total]


class _chunk:
    """stk_iso_tile for the block."""
    def __init__(self, cols):
        self.cols = cols

    def __enter__(self):
        from source import _lib
        _lib.check(_lib.lib().stk_iso_tile(self.cols))

    def __exit__(self, *exc):
        from source import _lib
        _lib.check(_lib.lib().stk_iso_tile(0))


# ---- 1. the device is the contract ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(MESHES))
def test_device_is_the_contract(name):
    """theta = 0.3 on the planted data, theta = 1.0 where the planted integer columns have
    vertices exactly AT it, and both infinities; 1 .. 65 columns of a slab whose padding is NaN."""
    case = planted(name)
    for theta in (0.3, 1.0, INF, -INF):
        U, want_counts, want = case.reference(theta)
        per_column = np.concatenate([[0], np.cumsum(want_counts.sum(axis=1))])
        for n in N_COLS:
            slab = _slab(U[:, :n])
            assert slab.shape[1] % 2 == 0 and bool(torch.isnan(slab[:, n:]).all())
            counts, got = _records(name, slab, n, theta)
            assert counts.dtype == np.int64 and np.array_equal(counts, want_counts[:n]), (name, theta, n)
            assert got.shape == (per_column[n], case.W) and same(got, want[:per_column[n]]), (name, theta, n)
            assert not np.isnan(got).any()  # no padding column came in
            if not np.isfinite(theta):
                assert not counts.any() and len(got) == 0


@pytest.mark.parametrize('name', ['first257', 'cube2'])
def test_nan_and_inf_in_the_slab_give_what_the_contract_gives(name):
    case = planted(name)
    U = np.random.RandomState(21).randn(case.M, 5)
    U[3 % case.M, 0], U[5 % case.M, 1], U[7 % case.M, 2], U[:, 3] = np.nan, np.inf, -np.inf, np.nan
    for theta in (0.3, -0.2, -INF):
        want_counts, want = case.contract(U, theta)
        counts, got = _records(name, _slab(U), 5, theta)
        assert np.array_equal(counts, want_counts) and same(got, want), (name, theta)
        if theta == 0.3:
            assert not want_counts[3].any()  # a NaN is not above, nor is the boundary's 0.0: no piece
        elif theta == -0.2:
            assert want_counts[3].any()  # the boundary's 0.0 is above: cut cells whose cuts are NaN
        else:
            assert not want_counts.any()
        if np.isfinite(theta):
            assert np.isnan(want).any() and np.isinf(want).any()  # coordinates from a NaN or inf: what IEEE gives


# ---- 2. every launch form gives the same doubles ---------------------------------------------------------------
@pytest.mark.parametrize('name', ['first513', 'cube2', 'square4'])
def test_every_launch_form_gives_the_one_shot_doubles(name):
    case = planted(name)
    U, want_counts, want = case.reference(0.3)
    n = 17
    slab = _slab(U[:, :n])
    counts, whole = _records(name, slab, n, 0.3)
    total = len(whole)
    assert np.array_equal(counts, want_counts[:n]) and same(whole, want[:total]) and total > 0
    for cols in (1, 3, 8, 32):
        with _chunk(cols):
            c, r = _records(name, slab, n, 0.3)
            assert np.array_equal(c, counts) and same(r, whole), cols
    # a pointer offset by one column (8-byte alignment), and column ranges [a, b): the slice of the whole
    start = np.concatenate([[0], np.cumsum(counts.sum(axis=1))])
    for a, b in ((1, n), (0, 5), (5, 6), (4, 13), (16, 17)):
        c, r = _records(name, slab, b - a, 0.3, first=a)
        assert np.array_equal(c, counts[a:b]) and same(r, whole[start[a]:start[b]]), (a, b)
    # ... and filled into the places of the whole table, range by range
    from source.isotherms import iso_fill
    dev_counts = _dev(counts)
    first = _first(dev_counts)
    out = torch.full((total + 3, case.W), SENTINEL, dtype=torch.float64, device=slab.device)
    for a, b in ((9, 17), (0, 4), (4, 9)):
        iso_fill(_plan(name), slab.data_ptr() + 8 * a, case.M, b - a, slab.shape[1], 0.3, dev_counts[a:b].contiguous(),
                 first[a:b].contiguous(), total, out)
    out = out.cpu().numpy()
    assert same(out[:total], whole) and np.all(out[total:] == SENTINEL)


# ---- 3. tables that do not belong together ------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['first513', 'cube2'])
def test_fill_never_writes_beyond_what_the_tables_say(name):
    case = planted(name)
    U, _, _ = case.reference(0.3)
    n = 9
    slab = _slab(U[:, :n])
    counts = _count(name, slab, n, 0.3)
    whole = _fill(name, slab, n, 0.3, counts, room=0)
    total = len(whole)
    # n_out below the total: exactly the prefix, also where n_out falls inside a tile's run
    inside = int(counts.reshape(-1)[:case.n_tiles + 1].sum()) - 1
    for n_out in (0, 1, inside, total - 1):
        out = _fill(name, slab, n, 0.3, counts, n_out=n_out)
        assert same(out[:n_out], whole[:n_out]) and np.all(out[n_out:] == SENTINEL), n_out
    # a counts table zeroed for some tiles leaves their ranges untouched
    first = _first(counts)
    gated = counts.clone()
    gated[2] = 0
    gated[:, case.n_tiles - 1] = 0
    out = _fill(name, slab, n, 0.3, gated, first_table=first, n_out=total)
    kept = np.ones(total, dtype=bool)
    host_counts, host_first = counts.cpu().numpy(), first.cpu().numpy()
    for c, t in zip(*np.nonzero(gated.cpu().numpy() == 0)):
        kept[host_first[c, t]:host_first[c, t] + host_counts[c, t]] = False
    assert kept.any() and not kept.all()
    assert same(out[:total][kept], whole[kept]) and np.all(out[:total][~kept] == SENTINEL)
    # places before the table or far beyond it: nothing is written, nothing faults
    for shift in (-(total + 5), total + 5, 2**62):
        out = _fill(name, slab, n, 0.3, counts, first_table=first + shift)
        assert np.all(out == SENTINEL), shift
    # shifted by three: the records that still fit, three places on
    out = _fill(name, slab, n, 0.3, counts, first_table=first + 3)
    assert np.all(out[:3] == SENTINEL) and same(out[3:total], whole[:total - 3])


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_the_outputs():
    from source import _lib
    lib = _lib.lib()
    name = 'square2'
    case = planted(name)
    U, want_counts, want = case.reference(0.3)
    n = 9
    slab = _slab(U[:, :n])
    good_counts = _count(name, slab, n, 0.3).contiguous()
    first = _first(good_counts).contiguous()
    total = int(good_counts.sum())
    counts = torch.full((n, case.n_tiles), -5, dtype=torch.int64, device=slab.device)
    out = torch.full((total, case.W), 123.25, dtype=torch.float64, device=slab.device)
    good = dict(plan=_plan(name)._plan, M=case.M, n_cols=n, slab=slab.data_ptr(), row_stride=slab.shape[1], threshold=0.3,
                counts=counts.data_ptr(), first=first.data_ptr(), n_out=total, out=out.data_ptr())
    count_order = ('plan', 'M', 'n_cols', 'slab', 'row_stride', 'threshold', 'counts')
    fill_order = count_order + ('first', 'n_out', 'out')
    shared = [(' plan is null', dict(plan=None)), (' slab is null', dict(slab=None)), (' counts is null', dict(counts=None)),
              (' n_cols = 0', dict(n_cols=0)), (' n_cols = -3', dict(n_cols=-3)),
              (' M = %d' % (case.M + 1), dict(M=case.M + 1)), (' M = 0', dict(M=0)),
              (' threshold is NaN', dict(threshold=float('nan'))), (' row_stride = %d' % (n - 1), dict(row_stride=n - 1))]
    only_fill = [(' first is null', dict(first=None)), (' out is null', dict(out=None)), (' n_out = -1', dict(n_out=-1))]
    for who, fn, order, cases in (('stk_iso_count', lib.stk_iso_count, count_order, shared),
                                  ('stk_iso_fill', lib.stk_iso_fill, fill_order, shared + only_fill)):
        for text, change in cases:
            a = dict(good, counts=good_counts.data_ptr() if who == 'stk_iso_fill' else counts.data_ptr())
            a.update(change)
            rc = fn(_lib.stream(), *[a[k] for k in order])
            said = lib.stk_last_error().decode()
            assert rc != 0 and said.startswith(who + ':') and text in said, (who, text, rc, said)
            with pytest.raises(_lib.StkError):
                _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((counts == -5).all()) and bool((out == 123.25).all())
    assert lib.stk_iso_count(_lib.stream(), *[good[k] for k in count_order]) == 0
    assert lib.stk_iso_fill(_lib.stream(), *[good[k] for k in fill_order]) == 0
    assert np.array_equal(counts.cpu().numpy(), want_counts[:n]) and same(out.cpu().numpy(), want[:total])
    for bad in (-1, 33):
        assert lib.stk_iso_tile(bad) != 0 and 'cols' in lib.stk_last_error().decode()
    assert lib.stk_iso_tile(0) == 0


# ---- 5. the public call -------------------------------------------------------------------------------------------
def _solver(problem, J_space, J_time, comm=None, **kw):
    import heateq_mpi as hm
    from source.comm import Comm
    return hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem=problem,
                              comm=Comm(distributed=False) if comm is None else comm, **kw)


def _numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _node_values(N, M, seed):
    """(N, M): uniform numbers, every third node not positive (no piece there)."""
    X = np.random.RandomState(seed).rand(N, M)
    X[::3] *= -1.0
    return X


KEYS = ('nodes', 'times', 'offsets', 'vertices', 'grad', 'cell', 'measure', 'measure_at', 'flux_at')


def _contract_dict(heat, X, theta, nodes):
    mesh, mesh_time = heat._sample_meshes
    p, cells = np.asarray(mesh.points, dtype=np.float64), np.asarray(mesh.cells, dtype=np.int64)
    counts, records = numpy_isotherms(p, cells, row_map(mesh), X[nodes].T, theta)
    return numpy_dict(records, counts, p.shape[1], nodes, float(mesh_time.h))


def _check_dict(heat, got, X, theta, nodes=None):
    nodes = list(range(X.shape[0])) if nodes is None else nodes
    want = _contract_dict(heat, X, theta, nodes)
    d, n_k, n = heat._sample_meshes[0].points.shape[1], len(nodes), len(want['cell'])
    assert sorted(got) == sorted(want) == sorted(KEYS)
    shapes = {'nodes': (n_k,), 'times': (n_k,), 'offsets': (n_k + 1,), 'vertices': (n, d, d), 'grad': (n, d), 'cell': (n,),
              'measure': (n,), 'measure_at': (n_k,), 'flux_at': (n_k,)}
    for key, value in want.items():
        assert got[key].shape == shapes[key] == value.shape and got[key].dtype == value.dtype, key
        assert same(got[key], value), key
    return want


@pytest.mark.parametrize('problem,J', [('square_moving_source', 3), ('cube_forced', 2)])
def test_public_call_of_both_drivers(problem, J):
    import heateq
    from source.linop import device_vector
    from source.mpi_vector import KronVectorMPI
    heat = _solver(problem, J, 3)
    X = _node_values(heat.N, heat.M, 31)
    N = heat.N
    u = KronVectorMPI(heat.dofs_distr, X)
    assert heat.curves_plan is None  # nothing is built without the call
    with pytest.raises(ValueError, match='NaN'):
        heat.isotherms(u, float('nan'))
    with pytest.raises(ValueError, match='needs a threshold'):
        heat.isotherms(u, None)
    with pytest.raises(ValueError, match='strictly ascending'):
        heat.isotherms(u, 0.25, nodes=[2, 2])
    with pytest.raises(AssertionError, match='trial space'):
        heat.isotherms(heat.g, 0.25)
    assert heat.curves_plan is None
    full = _numpy(heat.isotherms(u, 0.25))
    want = _check_dict(heat, full, X, 0.25)
    plan = heat.curves_plan
    assert plan is not None and heat.sample_plan is None and heat.solid_plan is None
    per_node = np.diff(want['offsets'])
    assert np.all(per_node[::3] == 0) and np.all(np.delete(per_node, np.arange(0, N, 3)) > 0)  # empty nodes between full ones
    assert np.all(want['measure_at'][::3] == 0.0) and want['measure_at'].max() > 0.0 and want['flux_at'].max() > 0.0
    # the time curves share the plan and see the same cut: every vertex within the node's box
    curves = _numpy(heat.time_curves(u, 0.25))
    assert heat.curves_plan is plan
    node_of = np.repeat(np.arange(N), per_node)
    for r in range(full['vertices'].shape[1]):
        assert np.all(full['vertices'][:, r] >= curves['box_lo'][node_of])
        assert np.all(full['vertices'][:, r] <= curves['box_hi'][node_of])
    # some nodes: the slices of the full result
    nodes = [0, 3, 4, N - 1]
    some = _numpy(heat.isotherms(u, 0.25, nodes=nodes))
    _check_dict(heat, some, X, 0.25, nodes)
    off = full['offsets']
    pick = np.concatenate([np.arange(off[k], off[k + 1]) for k in nodes]).astype(np.int64)
    for key in ('vertices', 'grad', 'cell', 'measure'):
        assert same(some[key], full[key][pick]), key
    for key in ('times', 'measure_at', 'flux_at'):
        assert same(some[key], full[key][nodes]), key
    assert same(some['nodes'], nodes) and same(np.diff(some['offsets']), per_node[nodes])
    # more than max_bytes: the error names the count, before anything is allocated
    n, W = len(want['cell']), plan.d * plan.d + plan.d + 1
    with pytest.raises(ValueError, match=r'isotherms\(\): %d pieces' % n):
        heat.isotherms(u, 0.25, max_bytes=8 * W * n - 1)
    assert same(_numpy(heat.isotherms(u, 0.25, max_bytes=8 * W * n))['vertices'], full['vertices'])
    # no piece at all
    none = _numpy(heat.isotherms(u, 2.0, nodes=[1, 2]))
    _check_dict(heat, none, X, 2.0, [1, 2])
    assert none['vertices'].shape == (0, plan.d, plan.d) and same(none['offsets'], [0, 0, 0]) and same(none['measure_at'], [0.0, 0.0])
    _check_dict(heat, _numpy(heat.isotherms(u, INF, max_bytes=0)), X, INF)

    serial = heateq.HeatEquation(J_space=J, J_time=3, problem=problem, precond='direct')
    assert (serial.N, serial.M) == (heat.N, heat.M) and serial.curves_plan is None
    with pytest.raises(ValueError, match='NaN'):
        serial.isotherms(X.reshape(-1), float('nan'))
    with pytest.raises(AssertionError, match='trial space'):
        serial.isotherms(device_vector(np.zeros(serial.N_Y * serial.M), serial.N_Y), 0.25)
    assert serial.curves_plan is None
    flat = _numpy(serial.isotherms(X.reshape(-1), 0.25))
    on_device = _numpy(serial.isotherms(device_vector(X.reshape(-1), serial.N), 0.25, nodes=nodes))
    for key in KEYS:
        assert same(flat[key], full[key]) and same(on_device[key], some[key]), key
    assert serial.sample_plan is None and serial.curves_plan is not None


# ---- 6. rank independence ---------------------------------------------------------------------------------------
_lock = threading.Lock()  # plan construction reads process-wide tuning keys


def _rank_run(comm, J_time):
    from source import driver
    from source.mpi_vector import KronVectorMPI
    with _lock:
        heat = _solver('square_moving_source', 3, J_time, comm=comm)
    u = driver.seeded_vector(heat, KronVectorMPI)  # the same global vector on every rank count
    return _numpy(heat.isotherms(u, 0.5)), _numpy(heat.isotherms(u, 0.5, nodes=[0, 2, 3, heat.N - 1]))


@functools.lru_cache(maxsize=None)
def _one_rank(J_time):
    return _rank_run(None, J_time)


@pytest.mark.parametrize('J_time,ranks', [(3, 2), (3, 3), (3, 8), (2, 5)])
def test_isotherms_do_not_depend_on_the_number_of_ranks(J_time, ranks):
    """Every tensor, every rank: array_equal to the one-rank dict.  (2, 5): five nodes on five
    ranks -- every call is a single column."""
    from thread_comm import run_ranks
    got = run_ranks(ranks, lambda comm: _rank_run(comm, J_time))
    one = _one_rank(J_time)
    assert np.diff(one[0]['offsets']).min() > 0 and len(one[0]) == len(KEYS) and one[0]['measure_at'].min() > 0.0
    assert len(one[1]['cell']) > 0
    for rank in range(ranks):
        for form in (0, 1):
            assert sorted(got[rank][form]) == sorted(one[form])
            for key, value in one[form].items():
                assert got[rank][form][key].dtype == value.dtype and same(got[rank][form][key], value), (rank, form, key)


# ---- 7. the torch composition of the timing tool -------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location('isotherms_time', os.path.join(REPO, 'tools', 'isotherms_time.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.mark.parametrize('name', ['square2', 'cube1'])
def test_the_timed_composition_gives_the_kernels_records(name):
    case = planted(name)
    tool = _tool()
    for theta in (0.3, 1.0):
        U, want_counts, want = case.reference(theta)
        n = 17
        slab = _slab(U[:, :n])
        counts, got = _records(name, slab, n, theta)
        comp = tool.Composition(case.mesh, slab)
        c, r = comp.records(slab[:, :n], theta)
        assert np.array_equal(c.cpu().numpy(), counts) and len(got) > 0
        assert same(r.cpu().numpy(), got), (name, theta)
    c, r = comp.records(slab[:, :n], INF)
    assert not bool(c.any()) and tuple(r.shape) == (0, case.W)


# ---- 8. the drivers ----------------------------------------------------------------------------------------------------
def test_drivers_write_iso_out(tmp_path, monkeypatch, capsys):
    import heateq
    import heateq_mpi as hm
    from source.mpi_kron import LinearOperatorMPI
    monkeypatch.setattr(LinearOperatorMPI, 'sync_timing', LinearOperatorMPI.sync_timing)  # main() sets it
    common = ['--J_time', '2', '--J_space', '2', '--problem', 'square_moving_source']
    for name, main in (('mpi', hm.main), ('serial', heateq.main)):
        # without the option nothing is written and nothing is built
        res = main(common)
        assert res[0].curves_plan is None and os.listdir(tmp_path) == []
        theta = 0.5 * float(res[0].time_curves(res[1])['peak'].max())  # half the solution's maximum
        assert theta > 0.0
        capsys.readouterr()
        out = str(tmp_path / (name + '.npz'))
        res = main(common + ['--iso_out', out, '--iso_threshold', repr(theta)])
        heat, u = res[0], res[1]
        data = np.load(out)
        assert sorted(data.files) == sorted(KEYS + ('threshold',)) and float(data['threshold']) == theta
        direct = _numpy(heat.isotherms(u, theta))
        for key in KEYS:
            assert same(data[key], direct[key]), (name, key)
        h = float(heat._sample_meshes[1].h)
        assert np.array_equal(data['times'], np.array([k * h for k in range(heat.N)]))
        assert data['vertices'].shape[1:] == (2, 2) and len(data['cell']) > 0 and data['measure_at'].max() > 0.0
        assert 'iso_' not in capsys.readouterr().out  # what the drivers print is what it was
        every = str(tmp_path / (name + '_every.npz'))
        main(common + ['--iso_out', every, '--iso_threshold', repr(theta), '--iso_every', '2'])
        thinned = np.load(every)
        nodes = list(range(0, heat.N, 2))
        assert thinned['nodes'].tolist() == nodes
        assert same(thinned['measure_at'], direct['measure_at'][nodes]) and same(thinned['flux_at'], direct['flux_at'][nodes])
        # without its threshold the run ends before anything is built
        before = sorted(os.listdir(tmp_path))
        with pytest.raises(SystemExit, match='--iso_out needs --iso_threshold'):
            main(common + ['--iso_out', str(tmp_path / 'never.npz')])
        with pytest.raises(SystemExit, match='--iso_every'):
            main(common + ['--iso_out', str(tmp_path / 'never.npz'), '--iso_threshold', '0.01', '--iso_every', '0'])
        assert sorted(os.listdir(tmp_path)) == before
        for made in before:
            os.remove(str(tmp_path / made))
    assert N_PLANTED == max(N_COLS)
