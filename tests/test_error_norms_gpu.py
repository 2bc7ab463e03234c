"""Error norms on the device (csrc/err_norms.hip, source/error_norms.py) against the
np.longdouble oracle of tests/test_error_norms_host.py and its first-order rounding bound
B (n = nq + n_k + ceil(log2 nc) + 8): the element kernel on random data at every shape where it takes another path, the
doubles that must be EQUAL (strides, boundary cells, quadrature points), the refusals, the
public call, its independence of the number of ranks, and the solvers end to end.

Measured on the MI355X (the tests print their figures): see the docstrings.  The whole file
takes 12 s there."""
import ctypes
import functools
import math
import threading
import types

import numpy as np
import pytest
import torch

from test_error_norms_host import (PINNED, UNIT, geometry, nodal_values, numpy_error_norms, oracle_element)

pytestmark = pytest.mark.gpu


def _mesh(problem, J):
    from source.problem import problem_helper
    return problem_helper(problem, J_space=J, J_time=1)[0]


def _first_cells(mesh, n):
    """The first n cells of a mesh as a mesh of their own (the ABI does not ask the cells to
    cover anything)."""
    assert n <= len(mesh.cells)
    return types.SimpleNamespace(points=mesh.points, cells=np.ascontiguousarray(mesh.cells[:n]),
                                 boundary=mesh.boundary, nv=mesh.nv)


MESHES = {
    'square0': lambda: _mesh('square', 0),  # 8 cells, one free dof
    'square1': lambda: _mesh('square', 1),
    'square2': lambda: _mesh('square', 2),
    'square4': lambda: _mesh('square', 4),  # 2048 cells: eight tiles
    'lshape_jitter3': lambda: _mesh('lshape_jitter', 3),
    'cube1': lambda: _mesh('cube', 1),
    'cube2': lambda: _mesh('cube', 2),
    'first255': lambda: _first_cells(_mesh('square', 4), 255),  # tail lanes
    'first256': lambda: _first_cells(_mesh('square', 4), 256),  # exactly one tile
    'first257': lambda: _first_cells(_mesh('square', 4), 257),  # a second tile of one cell
    'first513': lambda: _first_cells(_mesh('square', 4), 513),  # two full tiles and a third of one cell
}


def _plan(mesh):
    from source.error_norms import ErrorPlan
    return ErrorPlan(mesh, None)


def _dev(a):
    from source import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(_lib.compute_device())


def _full(mesh, values):
    from source.assembly import free_dofs
    out = np.zeros(mesh.nv)
    out[free_dofs(mesh)] = values
    return out


def _random_rule(rng, nq, d):
    ql = rng.rand(nq, d + 1) + 0.05
    ql /= ql.sum(axis=1, keepdims=True)
    qw = rng.rand(nq) + 0.1
    return qw / qw.sum(), np.ascontiguousarray(ql)


# ---- 1. the element kernel against the oracle ------------------------------------------------------
@pytest.mark.parametrize('name', sorted(MESHES))
def test_element_kernel_against_the_oracle(name):
    """Random nodal values, random f and gf (the difference is O(1) everywhere), random
    rules of nq = 1, 3, 6, 11, 16 points and n_k = 1, 4, 16 time points, all fifteen pairs,
    with and without the gradient (on the meshes above 600 cells five pairs that name every
    value run both ways and the other ten without gf: the oracle's longdouble sums over gf are
    what takes time there): |device - oracle| <= B for each of the four numbers, B the bound
    of oracle_element with n = nq + n_k + ceil(log2 nc) + 8.  Without gf entries 1 and 3 are
    exactly 0.0.  The looser worst-case figure of oracle_element(refined=True) is printed
    beside it, never asserted.
    Measured on the MI355X, the largest |device - oracle| over all cases of a mesh:
    between 0.042 B (square4) and 0.118 B (square1); of the refined figure 0.035 to 0.085 --
    a bound counts every rounding at its worst, the sums see them at random."""
    mesh = MESHES[name]()
    plan, geo = _plan(mesh), geometry(mesh)
    d, nc, M = plan.d, plan.nc, plan.n_free
    rng = np.random.RandomState(len(name) * 1000 + nc)
    worst = worst_refined = 0.0
    pairs = [(nq, n_k) for nq in (1, 3, 6, 11, 16) for n_k in (1, 4, 16)]
    both_ways = pairs if nc <= 600 else [(1, 16), (3, 1), (6, 4), (11, 4), (16, 16)]
    for nq, n_k in pairs:
        qw, ql = _random_rule(rng, nq, d)
        lo, hi = rng.randn(M), rng.randn(M)
        w_lo, w_hi, c = rng.rand(n_k), rng.rand(n_k), rng.rand(n_k) + 0.1
        f = rng.randn(n_k, nc, nq)
        gf = rng.randn(n_k, d, nc, nq) if (nq, n_k) in both_ways else None
        lo_d, hi_d, f_d = _dev(lo), _dev(hi), _dev(f)
        gf_d = None if gf is None else _dev(gf)
        # (entries 0 and 2 do not depend on gf: one oracle serves both calls)
        args = (geo, qw, ql, w_lo, w_hi, c, f, gf, _full(mesh, lo), _full(mesh, hi))
        want, bound = oracle_element(*args)
        loose = oracle_element(*args, refined=True)[1]
        for with_grad in (True, False) if gf is not None else (False,):
            out = torch.full((4,), -7.0, dtype=torch.float64, device=f_d.device)
            plan.element(f_d, gf_d if with_grad else None, w_lo, w_hi, c, lo_d.data_ptr(), 1, hi_d.data_ptr(), 1,
                         out, qw=qw, ql=ql)
            got = out.cpu().numpy()
            for x in (0, 1, 2, 3) if with_grad else (0, 2):
                dev = abs(np.longdouble(got[x]) - want[x])
                worst, worst_refined = max(worst, float(dev / bound[x])), max(worst_refined, float(dev / loose[x]))
                assert dev <= bound[x], (name, nq, n_k, with_grad, x, got[x], float(want[x]), float(bound[x]))
                assert got[x] > 0.0
            if not with_grad:
                assert got[1] == 0.0 and got[3] == 0.0
    print('%s: nc = %d, largest |device - oracle| = %.4f B (%.4f of the refined worst-case figure)'
          % (name, nc, worst, worst_refined))


# ---- 2. equal doubles ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['square4', 'cube2'])
def test_slab_columns_and_contiguous_rows_give_the_same_doubles(name):
    """The two time nodes as columns e, e + 1 of a slab (row stride ld; e even and odd; an
    odd number of local columns, the padding column full of NaN) and as contiguous copies
    (stride 1, what a ghost row is): array_equal, and mixed."""
    mesh = MESHES[name]()
    plan = _plan(mesh)
    d, nc, M = plan.d, plan.nc, plan.n_free
    rng = np.random.RandomState(17)
    n_loc = 5
    ld = n_loc + 1
    slab = np.full((M, ld), np.nan)
    slab[:, :n_loc] = rng.randn(M, n_loc)
    slab_d = _dev(slab)
    s = np.array([0.1, 0.4, 0.6, 0.9])
    c = np.array([0.2, 0.3, 0.3, 0.2])
    f_d, gf_d = _dev(rng.randn(4, nc, len(plan.qw))), _dev(rng.randn(4, d, nc, len(plan.qw)))

    def run(lo, stride_lo, hi, stride_hi):
        out = torch.zeros(4, dtype=torch.float64, device=slab_d.device)
        plan.element(f_d, gf_d, 1.0 - s, s, c, lo, stride_lo, hi, stride_hi, out)
        return out.cpu().numpy()

    for e in (0, 1, 2, 3):
        lo_c, hi_c = slab_d[:, e].contiguous(), slab_d[:, e + 1].contiguous()
        strided = run(slab_d.data_ptr() + 8 * e, ld, slab_d.data_ptr() + 8 * (e + 1), ld)
        assert not np.isnan(strided).any() and np.all(strided > 0.0)
        assert np.array_equal(strided, run(lo_c.data_ptr(), 1, hi_c.data_ptr(), 1)), e
        assert np.array_equal(strided, run(lo_c.data_ptr(), 1, slab_d.data_ptr() + 8 * (e + 1), ld)), e


def test_a_boundary_only_cell_contributes_the_norm_of_f():
    """A cell whose vertices are all boundary vertices reads no row: err = ref =
    sum_k c_k (R_k |T|), R_k = sum_q (f_q^2) w_q, in exactly these doubles (and the same for
    the gradient, summed over j)."""
    mesh = _mesh('square', 2)
    cell = mesh.cells[5]
    boundary = mesh.boundary.copy()
    boundary[cell] = True
    assert (~boundary).sum() > 0
    one = types.SimpleNamespace(points=mesh.points, cells=np.ascontiguousarray(mesh.cells[5:6]), boundary=boundary,
                                nv=mesh.nv)
    plan = _plan(one)
    rng = np.random.RandomState(3)
    n_k, nq, d = 4, len(plan.qw), 2
    f, gf = rng.randn(n_k, 1, nq), rng.randn(n_k, d, 1, nq)
    c, s = rng.rand(n_k) + 0.1, rng.rand(n_k)
    rows = _dev(rng.randn(plan.n_free))
    out = torch.zeros(4, dtype=torch.float64, device=rows.device)
    plan.element(_dev(f), _dev(gf), 1.0 - s, s, c, rows.data_ptr(), 1, rows.data_ptr(), 1, out)
    got = out.cpu().numpy()
    p = mesh.points[cell]
    e = p[1:] - p[0]
    vol = abs(e[0, 0] * e[1, 1] - e[0, 1] * e[1, 0]) / 2.0

    def weighted(values):  # sum_q (v_q^2) w_q from 0.0
        total = 0.0
        for q in range(nq):
            total = total + (values[q] * values[q]) * plan.qw[q]
        return total

    want_l2 = want_h1 = None
    for k in range(n_k):
        term = c[k] * (weighted(f[k, 0]) * vol)
        want_l2 = term if k == 0 else want_l2 + term
        grad_sum = 0.0
        for j in range(d):
            grad_sum = grad_sum + weighted(gf[k, j, 0])
        term = c[k] * (grad_sum * vol)
        want_h1 = term if k == 0 else want_h1 + term
    assert got[0] == got[2] == want_l2, (got, want_l2)
    assert got[1] == got[3] == want_h1, (got, want_h1)


@pytest.mark.parametrize('name', ['square4', 'lshape_jitter3', 'cube2'])
def test_points_are_those_of_the_load_engine(name):
    from source.assembly import DeviceLoadPlan
    mesh = MESHES[name]()
    plan, load = _plan(mesh), DeviceLoadPlan(mesh)
    assert torch.equal(plan.points(), load.points())
    ql = _random_rule(np.random.RandomState(1), 16, plan.d)[1]
    assert torch.equal(plan.points(ql), load.points(ql))
    assert tuple(plan.points().shape) == (plan.d, plan.nc, len(plan.qw))


# ---- 3. refusals -------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_out4_stays():
    from source import _lib
    lib = _lib.lib()
    mesh = _mesh('square', 2)
    plan = _plan(mesh)
    nq, n_k = len(plan.qw), 4
    rng = np.random.RandomState(0)
    f, gf = _dev(rng.randn(n_k, plan.nc, nq)), _dev(rng.randn(n_k, 2, plan.nc, nq))
    rows = _dev(rng.randn(plan.n_free))
    w = np.ascontiguousarray(rng.rand(16))
    big_w, big_l = np.ones(17) / 17.0, np.full((17, 3), 1.0 / 3.0)
    out = torch.full((4,), 123.25, dtype=torch.float64, device=rows.device)
    good = dict(plan=plan._plan, nq=nq, qw=plan.qw.ctypes.data, ql=plan.ql.ctypes.data, n_k=n_k, w_lo=w.ctypes.data,
                w_hi=w.ctypes.data, c=w.ctypes.data, f=f.data_ptr(), gf=gf.data_ptr(), u_lo=rows.data_ptr(), stride_lo=1,
                u_hi=rows.data_ptr(), stride_hi=1, out=out.data_ptr())

    def call(**change):
        a = dict(good, **change)
        return lib.stk_err_element(_lib.stream(), a['plan'], a['nq'], a['qw'], a['ql'], a['n_k'], a['w_lo'], a['w_hi'],
                                   a['c'], a['f'], a['gf'], a['u_lo'], a['stride_lo'], a['u_hi'], a['stride_hi'], a['out'])

    cases = [(dict([(name, None)]), b'null pointer') for name in ('plan', 'qw', 'w_lo', 'w_hi', 'c', 'f', 'u_lo', 'u_hi')]
    cases += [(dict(ql=None), b'null pointer'), (dict(out=None), b'null pointer')]
    cases += [(dict(n_k=0), b'time points'), (dict(n_k=17), b'time points')]
    cases += [(dict(nq=0), b'quadrature points'),
              (dict(nq=17, qw=big_w.ctypes.data, ql=big_l.ctypes.data), b'quadrature points')]
    cases += [(dict(stride_lo=0), b'strides'), (dict(stride_hi=0), b'strides'), (dict(stride_hi=-3), b'strides')]
    for change, word in cases:
        assert call(**change) != 0, change
        assert word in lib.stk_last_error(), (change, lib.stk_last_error())
        torch.cuda.synchronize()
        assert torch.all(out == 123.25), change
    # ... and the good call goes through (gf may be null)
    assert call() == 0 and call(gf=None) == 0
    torch.cuda.synchronize()
    assert out[0].item() > 0.0 and out[1].item() == 0.0
    # the plan's own checks, those of the load and the sample plans
    pts = np.ascontiguousarray(mesh.points)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int64)
    from source.assembly import free_dofs
    fd = np.ascontiguousarray(free_dofs(mesh), dtype=np.int64)
    made = ctypes.c_void_p()

    def create(d=2, cells=cells, fd=fd):
        return lib.stk_err_plan_create(d, mesh.nv, len(cells), pts.ctypes.data, cells.ctypes.data, len(fd), fd.ctypes.data,
                                       ctypes.byref(made))

    bad_cells = cells.copy()
    bad_cells[-1, 2] = mesh.nv
    for kw, word in ((dict(d=4), b'bad arguments'), (dict(cells=bad_cells), b'names vertex'),
                     (dict(fd=np.array([mesh.nv], dtype=np.int64)), b'free dof'),
                     (dict(fd=np.array([fd[0], fd[0]], dtype=np.int64)), b'named twice')):
        assert create(**kw) != 0, kw
        assert word in lib.stk_last_error(), (kw, lib.stk_last_error())
        assert not made.value
    assert lib.stk_err_plan_destroy(None) == 0
    assert lib.stk_err_points(_lib.stream(), plan._plan, 3, None, rows.data_ptr()) != 0


# ---- 4. the public call ---------------------------------------------------------------------------------------
def _solver(problem, J_space, J_time, comm=None, **kw):
    import heateq_mpi as hm
    from source.comm import Comm
    return hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem=problem,
                              comm=Comm(distributed=False) if comm is None else comm, **kw)


def _device_evaluate(fn, t, x):
    """exact / exact_grad as error_norms evaluates them: with torch on the device."""
    tt = _dev(np.asarray(t, dtype=np.float64)).reshape(-1, 1, 1)
    out = fn(tt, *[_dev(c) for c in x])
    if isinstance(out, (tuple, list)):
        return tuple(torch.as_tensor(o).cpu().numpy() for o in out)
    return torch.as_tensor(out).cpu().numpy()


def _oracle_of(h, U, exact, exact_grad, times):
    """The oracle from the doubles the device starts from: its quadrature points and its
    values of exact."""
    mesh, mesh_time = h._sample_meshes
    return numpy_error_norms(mesh, mesh_time, U, exact, exact_grad, times=times,
                             points=h.error_plan.points().cpu().numpy(), evaluate=_device_evaluate)


def _assert_within_bound(got, want, what=''):
    """Every entry of the dict against the oracle, within B (+ 4 u of the value where a
    square root and its square lie between)."""
    N1 = want['per_element'].shape[0]
    dev = np.abs(got['per_element'].astype(np.longdouble) - want['per_element'])
    grad = got['l2_h1'] is not None
    cols = (0, 1, 2, 3) if grad else (0, 2)
    worst = 0.0
    for x in cols:
        worst = max(worst, float(np.max(dev[:, x] / want['bound_per_element'][:, x])))
    assert worst <= 1.0, (what, 'per_element', worst)
    keys = [('l2_l2', 0), ('exact_l2_l2', 2)] + ([('l2_h1', 1), ('exact_l2_h1', 3)] if grad else [])
    for key, x in keys:
        sq = np.longdouble(got[key])**2
        room = want['bound'][x] + 4 * UNIT * want['sq'][x]
        ratio = float(abs(sq - want['sq'][x]) / room)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, key, got[key], float(want['sq'][x]), float(room))
    at = np.abs(got['l2_at'].astype(np.longdouble)**2 - want['sq_at']) / (want['bound_at'] + 4 * UNIT * want['sq_at'])
    assert got['l2_at'].shape == want['sq_at'].shape and np.all(at <= 1.0), (what, 'l2_at', at)
    assert got['per_element'].shape == (N1, 4)
    return max(worst, float(at.max()))


def test_error_norms_of_the_interpolant_against_the_oracle():
    """I_h(exact) on square_forced, J = 3: the interpolation error in all norms, at
    times 0 (exactly the nodal values: the spatial interpolation error of u0), T / 3 (inside an
    element) and T, each within B of the oracle.  Measured: largest deviation 0.064 B."""
    from source.mpi_vector import KronVectorMPI
    h = _solver('square_forced', 3, 3)
    assert h.error_plan is None
    mesh, mesh_time = h._sample_meshes
    exact, grad = h._exact
    U = nodal_values(mesh, mesh_time, exact)
    u = KronVectorMPI(h.dofs_distr, U)
    times = [0.0, mesh_time.T / 3.0, mesh_time.T]
    got = h.error_norms(u, times=times)
    assert h.error_plan is not None
    assert sorted(got) == ['exact_l2_h1', 'exact_l2_l2', 'l2_at', 'l2_h1', 'l2_l2', 'per_element']
    worst = _assert_within_bound(got, _oracle_of(h, U, exact, grad, times))
    print('interpolant: l2_l2 %.6e l2_h1 %.6e l2_at %s; largest deviation %.4f B'
          % (got['l2_l2'], got['l2_h1'], got['l2_at'], worst))
    assert 1e-3 < got['l2_l2'] < 1e-2 and 0.1 < got['l2_h1'] < 1.0  # O(h^2) and O(h) at h = 1/8
    # without a gradient: no H1 entries, the same L2 ones
    plain = h.error_norms(u, exact=exact, times=times)
    assert plain['l2_h1'] is None and plain['exact_l2_h1'] is None
    assert plain['l2_l2'] == got['l2_l2'] and np.array_equal(plain['l2_at'], got['l2_at'])
    assert np.array_equal(plain['per_element'][:, [0, 2]], got['per_element'][:, [0, 2]])
    assert not plain['per_element'][:, [1, 3]].any()


def test_error_against_zero_is_the_energy_of_the_vector():
    """exact = 0 t: || u_h ||^2 = u^T (M_t kron M_x) u and || grad u_h ||^2 =
    u^T (M_t kron A_x) u -- both rules are exact for these polynomials -- within 1e-12
    relative, the tolerance of the sampling tests for quantities of this kind.
    Measured: 1.1e-16 and 1.4e-15."""
    from source import driver
    from source.assembly import time_matrices
    from source.mpi_vector import KronVectorMPI
    h = _solver('square_forced', 3, 3)
    u = driver.seeded_vector(h, KronVectorMPI)
    U = u.X_loc.cpu().numpy()
    zero = lambda t, *x: 0.0 * t
    got = h.error_norms(u, exact=zero, exact_grad=lambda t, *x: (0.0 * t, 0.0 * t))
    M_t = time_matrices(h._sample_meshes[1])[2]
    V = M_t @ U  # (N, M)
    mass = float(np.sum(V * (h.M_x @ U.T).T))
    energy = float(np.sum(V * (h.A_x @ U.T).T))
    devs = (abs(got['l2_l2']**2 / mass - 1.0), abs(got['l2_h1']**2 / energy - 1.0))
    print('against u^T (M_t kron M_x) u: %.2e, against u^T (M_t kron A_x) u: %.2e' % devs)
    assert max(devs) <= 1e-12
    assert got['exact_l2_l2'] == 0.0 and got['exact_l2_h1'] == 0.0
    # at the final time: the spatial mass norm of the last time row
    last = float(U[-1] @ (h.M_x @ U[-1]))
    assert abs(got['l2_at'][0]**2 / last - 1.0) <= 1e-12


def test_nothing_is_built_without_the_call():
    h = _solver('square_forced', 2, 2)
    assert h.error_plan is None and h.sample_plan is None
    h.solve()
    assert h.error_plan is None


# ---- 5. rank independence ---------------------------------------------------------------------------------------
_lock = threading.Lock()  # plan construction reads process-wide tuning keys


def _rank_run(comm, J_time):
    from source import driver
    from source.mpi_vector import KronVectorMPI
    with _lock:
        h = _solver('square_nonseparable', 4, J_time, comm=comm)
    assert h.error_plan is None
    u = driver.seeded_vector(h, KronVectorMPI)  # the same global vector on every rank count
    T = h._sample_meshes[1].T
    out = h.error_norms(u, times=[0.0, T / 3.0, 0.5 * T, T])
    assert h.error_plan is not None
    return out


@functools.lru_cache(maxsize=None)
def _one_rank(J_time):
    return _rank_run(None, J_time)


@pytest.mark.parametrize('J_time,ranks', [(3, 2), (3, 3), (3, 8), (2, 5)])
def test_error_norms_do_not_depend_on_the_number_of_ranks(J_time, ranks):
    """Every entry of the dict, per_element included, array_equal to the one-rank run.
    (2, 5): five nodes on five ranks -- the first integrates nothing, every other one
    element whose lower node is its ghost row."""
    from thread_comm import run_ranks
    got = run_ranks(ranks, lambda comm: _rank_run(comm, J_time))
    one = _one_rank(J_time)
    assert one['l2_l2'] > 0.1 and one['l2_h1'] > 1.0 and np.all(one['per_element'] > 0.0)
    for rank in range(ranks):
        assert sorted(got[rank]) == sorted(one)
        for key, value in one.items():
            assert np.array_equal(np.asarray(got[rank][key]), np.asarray(value)), (rank, key, got[rank][key], value)


# ---- 6. end to end -------------------------------------------------------------------------------------------------
# |device / SciPy restatement - 1| over the three pinned norms at J = 3, 4, measured on the MI355X:
# with solve() converged as SciPy's CG is (eps = 1e-9) ...
PINNED_GAP = 9.9e-9  # the larger of 3.5e-9 (square_forced) and 9.9e-9 (square_nonseparable)
# ... and with solve() at its default stopping rule (r.Pr < 1e-12)
DEFAULT_SOLVE_GAP = {'square_forced': 5.501e-7, 'square_nonseparable': 1.754e-5}


@functools.lru_cache(maxsize=None)
def _solved(problem, J):
    """(norms of solve()'s solution, its deviation from the oracle in B, norms of
    solve(eps=1e-9)'s solution)."""
    h = _solver(problem, J, J, precond='direct')
    u, _ = h.solve()
    got = h.error_norms(u)
    exact, grad = h._exact
    worst = _assert_within_bound(got, _oracle_of(h, u.X_loc.cpu().numpy(), exact, grad, None), (problem, J))
    u, _ = h.solve(eps=1e-9, kmax=80)
    converged = h.error_norms(u)
    worst = max(worst, _assert_within_bound(converged, _oracle_of(h, u.X_loc.cpu().numpy(), exact, grad, None),
                                            (problem, J, 'converged')))
    return got, worst, converged


def _gaps(problem, J, n):
    got = (n['l2_l2'], n['l2_h1'], n['l2_at'][0])
    return [abs(g / w - 1.0) for g, w in zip(got, PINNED[(problem, J)])]


@pytest.mark.parametrize('problem', ['square_forced', 'square_nonseparable'])
def test_device_solution_converges_in_the_error_norms(problem):
    """precond='direct' at J_time = J_space = 3, 4: the device's norms within B of the oracle
    applied to the downloaded solution and the ratios of the host test (L2 in [3.5, 4.5], H1
    in [1.8, 2.2]; measured 3.970 and 1.993 on square_forced, 3.983 and 1.997 on
    square_nonseparable).

    Against the SciPy restatement's pinned figures (tests/test_error_norms_host.py: PINNED).
    The two solves stop at different algebraic tolerances: SciPy's CG at 1e-12 of the
    residual, solve() by default at r.Pr < 1e-12, an algebraic error of 1e-6 in the energy
    norm, which the norms of u - u_h see against a discretisation error of 4e-4 .. 1e-2.
    * solve(eps=1e-9), converged as SciPy's is: the gap is PINNED_GAP (3.5e-9 and 9.9e-9);
      allowed 100 x that, never more than 1e-6.
    * solve() as it stands: 5.5e-7 on square_forced and 1.75e-5 on square_nonseparable (L2 at
      T, J = 4) -- the DEFAULT stopping rule cannot meet a cap of 1e-6 there, and it is the
      solver's rule, not the norms, that sets this figure.  It is pinned per problem
      (DEFAULT_SOLVE_GAP) and held to twice its measured value, so that a change of what
      solve() returns, or of the norms on it, shows."""
    (n3, w3, c3), (n4, w4, c4) = _solved(problem, 3), _solved(problem, 4)
    for J, n in ((3, n3), (4, n4)):
        print('%s J = %d: l2_l2 %.10e l2_h1 %.10e l2_at(T) %.10e' % (problem, J, n['l2_l2'], n['l2_h1'], n['l2_at'][0]))
    as_solved = max(_gaps(problem, 3, n3) + _gaps(problem, 4, n4))
    gaps = _gaps(problem, 3, c3) + _gaps(problem, 4, c4)
    print('%s: ratios L2 %.3f, H1 %.3f; against the oracle at most %.4f B, %.4f B; against the pinned figures: '
          'solve() %.3e, solve(eps=1e-9) %.3e'
          % (problem, n3['l2_l2'] / n4['l2_l2'], n3['l2_h1'] / n4['l2_h1'], w3, w4, as_solved, max(gaps)))
    assert 3.5 <= n3['l2_l2'] / n4['l2_l2'] <= 4.5
    assert 1.8 <= n3['l2_h1'] / n4['l2_h1'] <= 2.2
    assert 3.5 <= c3['l2_l2'] / c4['l2_l2'] <= 4.5
    assert 1.8 <= c3['l2_h1'] / c4['l2_h1'] <= 2.2
    assert max(gaps) <= min(100 * PINNED_GAP, 1e-6), gaps
    assert as_solved <= 2.0 * DEFAULT_SOLVE_GAP[problem], as_solved


# ---- 7. the drivers --------------------------------------------------------------------------------------------------
def test_drivers_report_the_error_norms(capsys, monkeypatch):
    import heateq
    import heateq_mpi as hm
    from source.mpi_kron import LinearOperatorMPI
    monkeypatch.setattr(LinearOperatorMPI, 'sync_timing', LinearOperatorMPI.sync_timing)  # main() sets it
    common = ['--J_time', '2', '--J_space', '2']
    for name, main in (('mpi', hm.main), ('serial', heateq.main)):
        res = main(common + ['--problem', 'square_forced', '--error_norms', '1'])
        text = capsys.readouterr().out
        lines = [line for line in text.splitlines() if line.startswith('Error norms:')]
        assert len(lines) == 1 and 'L2(H1)' in lines[0] and 'relative' in lines[0], text
        assert 'error_norms=' not in text  # the option is taken off before the arguments are printed
        heat, u = res[0], res[1]
        assert heat.error_plan is not None
        again = heat.error_norms(u)
        assert ('%.6e' % again['l2_l2']) in lines[0] and ('%.6e' % again['l2_h1']) in lines[0]
        # without an exact solution: said, and nothing built
        res = main(common + ['--problem', 'square', '--error_norms', '1'])
        text = capsys.readouterr().out
        assert 'no exact solution' in text and res[0].error_plan is None
        # without the option: no plan, no line
        res = main(common + ['--problem', 'square_forced'])
        assert res[0].error_plan is None and 'Error norms' not in capsys.readouterr().out
