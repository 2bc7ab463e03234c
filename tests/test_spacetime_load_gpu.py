"""Non-separable source terms on the device (needs an MI355X): the load engine of libstk
(csrc/load_dev.hip) against the host routines it repeats bit for bit, whole slabs built
from a callable against the NumPy restatement, parity with the separable path,
independence of the number of ranks, convergence to the exact solution, the moving-source
demo, and no cost for problems without a callable."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from conftest import relerr
from test_quadrature_reference_host import _longdouble_load
from test_spacetime_load_host import numpy_load, sum_of_pairs

pytestmark = pytest.mark.gpu

U = 2.0**-53

# barycentric rules on the triangle: centroid, the three-point rule of degree 2, Dunavant 6
RULES_2D = {
    1: (np.array([1.0]), np.array([[1 / 3, 1 / 3, 1 / 3]])),
    3: (np.array([1 / 3, 1 / 3, 1 / 3]), np.array([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3]])),
}


def _mesh(problem, J_space):
    from source.problem import problem_helper
    return problem_helper(problem, J_space=J_space, J_time=1)[0]


def _rule_2d(nq):
    from source.assembly import _QL, _QW
    if nq == 16:  # STK_LOAD_MAX_NQ points: seeded, weights and coordinates sum to 1, no symmetry
        rng = np.random.RandomState(16)
        w, l = rng.rand(16), rng.rand(16, 3)
        return w / w.sum(), l / l.sum(axis=1)[:, None]
    return (_QW, _QL) if nq == 6 else RULES_2D[nq]


def _host_points_2d(mesh, ql):
    from source import _lib
    pts = np.ascontiguousarray(mesh.points, dtype=np.float64)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int64)
    ql = np.ascontiguousarray(ql)
    qx, qy = np.empty((len(cells), len(ql))), np.empty((len(cells), len(ql)))
    _lib.check(_lib.lib().stk_p1_load_points_2d(mesh.nv, len(cells), pts.ctypes.data, cells.ctypes.data, len(ql),
                                                ql.ctypes.data, qx.ctypes.data, qy.ctypes.data))
    return qx, qy


def _host_sum_2d(mesh, qw, ql, f):
    """stk_p1_load_sum_2d on the free dofs."""
    from source import _lib
    from source.assembly import free_dofs
    pts = np.ascontiguousarray(mesh.points, dtype=np.float64)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int64)
    qw, ql, f = np.ascontiguousarray(qw), np.ascontiguousarray(ql), np.ascontiguousarray(f)
    vec = np.empty(mesh.nv)
    _lib.check(_lib.lib().stk_p1_load_sum_2d(mesh.nv, len(cells), pts.ctypes.data, cells.ctypes.data, len(qw),
                                             qw.ctypes.data, ql.ctypes.data, f.ctypes.data, vec.ctypes.data))
    return vec[free_dofs(mesh)]


# ---- 1. the points kernel ----------------------------------------------------------------------
@pytest.mark.parametrize('problem,J_space', [('square', 1), ('square', 2), ('square', 4), ('lshape', 3),
                                             ('lshape_jitter', 3)])
def test_points_kernel_equals_the_host_routine(problem, J_space):
    """stk_load_points against stk_p1_load_points_2d, the same doubles, for the three
    rules and one of 16 points, the most the engine takes; 512 triangles on the square at J_space = 4 are two workgroups of cells."""
    from source.assembly import DeviceLoadPlan
    mesh = _mesh(problem, J_space)
    plan = DeviceLoadPlan(mesh)
    for nq in (1, 3, 6, 16):
        _, ql = _rule_2d(nq)
        got = plan.points(ql).cpu().numpy()
        qx, qy = _host_points_2d(mesh, ql)
        assert got.shape == (2, len(mesh.cells), nq)
        assert np.array_equal(got[0], qx) and np.array_equal(got[1], qy), (problem, J_space, nq)
    assert plan.points() is plan.points()  # the mesh's own rule: computed once


@pytest.mark.parametrize('J_space', [1, 2])
def test_points_kernel_on_tetrahedra(J_space):
    """Against np.matmul(ql, p[c]), whose order of the four products belongs to the BLAS:
    three additions of terms below the largest coordinate, 4 * 2^-53 of it."""
    from source.assembly import _QL3, DeviceLoadPlan
    mesh = _mesh('cube', J_space)
    got = DeviceLoadPlan(mesh).points().cpu().numpy()
    want = np.matmul(_QL3, mesh.points[mesh.cells])  # (nc, nq, 3)
    assert got.shape == (3, len(mesh.cells), 11)
    dev = np.max(np.abs(got - np.moveaxis(want, 2, 0)))
    print('largest difference %.2e of the bound' % (dev / (4 * U * np.max(np.abs(want)))))
    assert dev <= 4 * U * np.max(np.abs(want))


# ---- 2. the columns kernel, arithmetic alone -----------------------------------------------------
@pytest.mark.parametrize('problem,J_space', [('square', 1), ('square', 2), ('square', 4), ('lshape_jitter', 3)])
def test_columns_kernel_equals_the_host_sums(problem, J_space):
    """Random f (signs mixed) and random coefficients: the pair of columns is
    c[0][a] L_0 + c[1][a] L_1 + ... added left to right, L_k = stk_p1_load_sum_2d of f[k],
    in the SAME doubles; with the accumulate switch, the old value plus that sum.  Slabs
    of 1, 2, 3, 8 elements and one more pair as padding; the pair written is the first,
    the last or one in between; everything else keeps its bits.  A row order (here a
    random permutation) changes nothing.  square at J_space = 1 has ONE free dof; on
    the jittered L-shape no two areas are equal."""
    from source.assembly import DeviceLoadPlan, free_dofs
    mesh = _mesh(problem, J_space)
    M, nc = len(free_dofs(mesh)), len(mesh.cells)
    rng = np.random.RandomState(31 + J_space)
    plans = {'ascending': DeviceLoadPlan(mesh), 'permuted': DeviceLoadPlan(mesh, row_order=rng.permutation(M))}
    for nq in (1, 3, 6, 16):
        qw, ql = _rule_2d(nq)
        for n_k in (1, 4):
            f = rng.randn(n_k, nc, nq)
            coef = rng.randn(n_k, 2)
            L = [_host_sum_2d(mesh, qw, ql, f[k]) for k in range(n_k)]
            want = coef[0][None, :] * L[0][:, None]
            for k in range(1, n_k):
                want = want + coef[k][None, :] * L[k][:, None]
            f_dev = torch.from_numpy(f).cuda()
            for n_el in (1, 2, 3, 8):
                ld = 2 * n_el + 2
                for e in sorted({0, n_el // 2, n_el - 1}):
                    for accumulate in (False, True):
                        old = rng.randn(M, ld)
                        expect = old.copy()
                        expect[:, 2 * e:2 * e + 2] = old[:, 2 * e:2 * e + 2] + want if accumulate else want
                        for name, plan in plans.items():
                            buf = torch.from_numpy(old).cuda()
                            plan.columns(f_dev, coef, buf, e, accumulate=accumulate, qw=qw, ql=ql)
                            assert np.array_equal(buf.cpu().numpy(), expect), (problem, nq, n_k, n_el, e, accumulate, name)


@pytest.mark.parametrize('J_space', [1, 2])
def test_columns_kernel_on_tetrahedra(J_space):
    """Keast's 11 points on the cube, against an np.longdouble restatement: an entry is
    nq products and sums per share, one product with |T|, the sum over its incident
    cells, n_k products and sums with the coefficients -- (nq + n_k + incident cells + 2)
    roundings of partial sums that the sum of the absolute values bounds."""
    from source.assembly import _QL3, _QW3, DeviceLoadPlan, free_dofs
    mesh = _mesh('cube', J_space)
    M, nc = len(free_dofs(mesh)), len(mesh.cells)
    rng = np.random.RandomState(17)
    plan = DeviceLoadPlan(mesh)
    worst = 0.0
    for n_k in (1, 4):
        f, coef = rng.randn(n_k, nc, 11), rng.randn(n_k, 2)
        want, mag, incident = _longdouble_load(mesh, _QW3, _QL3, f, coef)
        bound = (11 + n_k + incident + 2)[:, None] * U * mag
        buf = torch.zeros((M, 4), dtype=torch.float64, device='cuda')
        plan.columns(torch.from_numpy(f).cuda(), coef, buf, 1)
        got = buf.cpu().numpy()
        assert not np.any(got[:, :2])
        err = np.asarray(np.abs(got[:, 2:] - want), dtype=np.float64)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), float(np.max(err / bound))
    print('largest share of the bound used: %.3f' % worst)


# ---- 3. whole slabs from a callable ----------------------------------------------------------------
# largest |device - host| / (2^-53 sum |terms|) over the entries of g, measured on the MI355X:
# torch's exp, sin and cos on the device against NumPy's (and on the cube NumPy's own order
# of the sums)
CALLABLE_DEV = {'square_nonseparable': 3.97, 'cube_nonseparable': 6.16}


@pytest.mark.parametrize('problem,J', [('square_nonseparable', 3), ('cube_nonseparable', 2)])
def test_slab_from_a_callable_against_the_numpy_restatement(problem, J):
    """h.g of the driver against numpy_load with the NumPy form of the callable (on the
    square through the host threads of libstk: the arithmetic is then bit-equal by the
    tests above, and the difference is that of the elementary functions).  Entry by
    entry under c 2^-53 sum |terms|, the restatement run on |g|; c = 8 x the measured
    CALLABLE_DEV, never more than 64.  The serial driver's g_vec is the one-rank slab."""
    import heateq as hs
    import heateq_mpi as hm
    from source.problem import problem_helper
    h = hm.HeatEquationMPI(J_space=J, J_time=J, problem=problem)
    assert h.load_plan is not None
    got = h.g.X_loc.cpu().numpy()
    mesh_space, _, mesh_time, data, _ = problem_helper(problem, J_space=J, J_time=J)
    g = data['g'][0]
    triangles = mesh_space.cells.shape[1] == 3  # these take the host threads of libstk, tetrahedra NumPy
    want = numpy_load(mesh_space, mesh_time, g, numpy_path=not triangles)
    mag = numpy_load(mesh_space, mesh_time, lambda *a: np.abs(g(*a)), numpy_path=not triangles)
    assert got.shape == want.shape and np.all(mag > 0)
    ratio = float(np.max(np.abs(got - want) / (U * mag)))
    print('%s: largest |device - host| = %.3f x 2^-53 sum |terms|' % (problem, ratio))
    assert ratio <= min(8 * CALLABLE_DEV[problem], 64.0)
    serial = hs.HeatEquation(J_space=J, J_time=J, problem=problem)
    assert serial.load_plan is not None
    assert np.array_equal(serial.g_vec, got.reshape(-1))


# ---- 4. the separable data as a callable -------------------------------------------------------------
def test_separable_data_as_a_callable_gives_the_pair_path(monkeypatch):
    """square_forced with its two pairs folded into one callable: g within 1e-14 of the
    largest entry of the pair path's (the same rules; rounding alone), f within F_BOUND."""
    import heateq_mpi as hm
    from source.problem import problem_helper
    from test_forcing_gpu import F_BOUND
    pairs = hm.HeatEquationMPI(J_space=3, J_time=3, problem='square_forced')
    assert pairs.load_plan is None

    def as_callable(problem, J_space, J_time=None):
        mesh_space, bc, mesh_time, data, name = problem_helper(problem, J_space=J_space, J_time=J_time)
        return mesh_space, bc, mesh_time, dict(data, g=[sum_of_pairs_on_any_arrays(data['g'])]), name

    monkeypatch.setattr(hm, 'problem_helper', as_callable)
    one = hm.HeatEquationMPI(J_space=3, J_time=3, problem='square_forced')
    assert one.load_plan is not None
    g0, g1 = pairs.g.X_loc.cpu().numpy(), one.g.X_loc.cpu().numpy()
    dev = np.max(np.abs(g1 - g0)) / np.max(np.abs(g0))
    f_dev = relerr(one.f.X_loc.cpu().numpy(), pairs.f.X_loc.cpu().numpy())
    print('g: %.2e of the largest entry; f: %.2e relative' % (dev, f_dev))
    assert dev <= 1e-14
    assert f_dev <= F_BOUND


def sum_of_pairs_on_any_arrays(pairs):
    """sum_of_pairs for torch tensors as well: the factors of square_forced are NumPy
    functions (np.exp, np.sin), evaluated here on the host and sent back -- test
    plumbing for data that was never meant to be a callable."""
    inner = sum_of_pairs(pairs)

    def g(t, *x):
        if not torch.is_tensor(t):
            return inner(t, *x)
        return torch.from_numpy(inner(t.cpu().numpy(), *(c.cpu().numpy() for c in x))).to(t.device)

    return g


def test_mixed_lists_accumulate_into_one_slab(monkeypatch):
    """A pair followed by a callable and a callable followed by a pair: the slab is the
    sum of both terms in either order (stk_outer and the accumulate switch of
    stk_load_columns share it), within rounding of the sum of the two slabs built alone."""
    import heateq_mpi as hm
    from source.problem import problem_helper
    base = problem_helper('square_forced', J_space=3, J_time=2)
    pair, other = base[3]['g'][0], sum_of_pairs_on_any_arrays([base[3]['g'][1]])
    slabs = {}
    for name, terms in (('pair', [pair]), ('callable', [other]), ('pair first', [pair, other]),
                        ('callable first', [other, pair])):
        monkeypatch.setattr(hm, 'problem_helper', lambda problem, J_space, J_time=None, terms=terms: (
            base[0], base[1], base[2], dict(base[3], g=terms), base[4]))
        slabs[name] = hm.HeatEquationMPI(J_space=3, J_time=2, problem='square_forced').g.X_loc.cpu().numpy()
    total = slabs['pair'] + slabs['callable']
    for name in ('pair first', 'callable first'):
        assert np.max(np.abs(slabs[name] - total)) <= 4 * U * np.max(np.abs(total)), name


# ---- 5. rank independence ---------------------------------------------------------------------------
_one_rank = {}


def _one_rank_run(J_time):
    from source.comm import Comm
    from test_forcing_gpu import _forced_run
    if J_time not in _one_rank:
        _one_rank[J_time] = _forced_run(Comm(distributed=False), J_time, 4, problem='square_nonseparable')
    return _one_rank[J_time]


@pytest.mark.parametrize('J_time,ranks', [(3, 2), (3, 3), (3, 8), (2, 5)])
def test_callable_forcing_does_not_depend_on_the_number_of_ranks(J_time, ranks):
    """square_nonseparable at J_space = 4 on thread ranks: g, g.g, f, the iterate with its
    iteration count and history and both error numbers EQUAL the one-rank run -- every
    rank builds its held elements, the copied first one included, with the instructions
    the one rank uses.  J_time = 2 on 5 ranks: the last rank owns a node and no element."""
    from test_forcing_gpu import _assert_equal_runs, _forced_run
    from thread_comm import run_ranks
    got = run_ranks(ranks, lambda comm: _forced_run(comm, J_time, 4, problem='square_nonseparable'))[0]
    one = _one_rank_run(J_time)
    assert one['iters'] > 3 and one['gg'] > 0
    _assert_equal_runs(got, one)


# ---- 6. against the exact solution --------------------------------------------------------------------
def _device_error(J):
    import heateq_mpi as hm
    from source.assembly import free_dofs, time_matrices_test_space
    from source.problem import problem_helper
    h = hm.HeatEquationMPI(J_space=J, J_time=J, problem='square_nonseparable', precond='direct')
    u, iters = h.solve()
    est = h.errors(u)[1]
    u = u.X_loc.cpu().numpy().reshape(-1)
    mesh_space, _, mesh_time, data, _ = problem_helper('square_nonseparable', J_space=J, J_time=J)
    pts = mesh_space.points[free_dofs(mesh_space)]
    t = mesh_time.h * np.arange(h.N)
    exact = data['exact'](t[:, None], pts[None, :, 0], pts[None, :, 1]).reshape(-1)
    MM = sp.kron(h.M_t, h.M_x)
    e = u - exact
    # the Y' estimator on the host from the device's u and g: exact K by splu
    _, Minv_Y, B1_t, B2_t = time_matrices_test_space(mesh_time)
    g = h.g.X_loc.cpu().numpy().reshape(-1)
    defect = g - (sp.kron(B1_t, h.M_x) + sp.kron(B2_t, h.A_x)) @ u
    lu = spla.splu(sp.csc_matrix(h.A_x))
    Z = Minv_Y @ defect.reshape(Minv_Y.shape[0], h.M)
    est_host = defect @ lu.solve(np.ascontiguousarray(Z.T)).T.reshape(-1)
    return np.sqrt(e @ (MM @ e)) / np.sqrt(exact @ (MM @ exact)), est, est_host


ESTIMATOR_DEV = 1.8e-11  # measured on the MI355X: the larger of the two figures in the test below (1.8e-12, 1.8e-11)


def test_device_solution_of_the_nonseparable_problem_converges():
    """precond='direct' on the device: the ratio and the bound of the SciPy restatement
    (tests/test_spacetime_load_host.py: 5.99e-3 at J = 3, 1.50e-3 at J = 4).  The device's
    Y' estimator against SciPy's from the same u and g, recorded as ESTIMATOR_DEV as in
    tests/test_forcing_gpu.py; allowed 100 x that, and never more than 1e-8."""
    (e3, est3, host3), (e4, est4, host4) = _device_error(3), _device_error(4)
    print('relative M_t kron M_x error: J=3 %.4e, J=4 %.4e, ratio %.3f' % (e3, e4, e3 / e4))
    devs = [abs(est3 / host3 - 1.0), abs(est4 / host4 - 1.0)]
    print('Yprime estimator, device against host: %.3e (J=3), %.3e (J=4)' % tuple(devs))
    assert 3.5 <= e3 / e4 <= 4.5
    assert e4 <= 1.9e-3
    assert max(devs) <= min(100 * ESTIMATOR_DEV, 1e-8), devs


# ---- 7. the demo ------------------------------------------------------------------------------------------
def test_moving_source_solves_and_its_estimator_falls():
    """square_moving_source, no exact solution: the Y' estimator at J = 4 is below half
    its value at J = 3 (a SciPy restatement gives 7.77e-6, 2.21e-6, 8.31e-7 at J = 3, 4, 5)."""
    import heateq_mpi as hm
    est = {}
    for J in (3, 4):
        h = hm.HeatEquationMPI(J_space=J, J_time=J, problem='square_moving_source')
        assert h.load_plan is not None and not torch.any(h.rhs.buf)  # u0 = 0
        u, iters = h.solve()
        alg, est[J] = h.errors(u)
        print('J = %d: %d iterations, algebraic error %.3e, Yprime estimator %.3e' % (J, iters, alg, est[J]))
        assert iters > 3 and np.isfinite(est[J]) and est[J] > 0
    assert est[4] < 0.5 * est[3]


# ---- 8. no cost elsewhere ---------------------------------------------------------------------------------
def test_no_load_plan_without_a_callable():
    import heateq as hs
    import heateq_mpi as hm
    for problem in ('square', 'square_forced'):
        assert hm.HeatEquationMPI(J_space=3, J_time=3, problem=problem).load_plan is None
    assert hs.HeatEquation(J_space=3, J_time=3, problem='square_forced').load_plan is None


# ---- 9. what the engine refuses ------------------------------------------------------------------------------
def test_columns_refuses_a_misaligned_pair_and_too_many_time_points():
    from source import _lib
    from source.assembly import DeviceLoadPlan, free_dofs
    mesh = _mesh('square', 2)
    plan = DeviceLoadPlan(mesh, max_k=2)
    M, nc = len(free_dofs(mesh)), len(mesh.cells)
    qw, ql = _rule_2d(6)
    buf = torch.zeros((M, 4), dtype=torch.float64, device='cuda')
    f = torch.zeros((3, nc, 6), dtype=torch.float64, device='cuda')
    with pytest.raises(_lib.StkError, match='time points'):
        plan.columns(f, np.zeros((3, 2)), buf, 0)
    lib, coef = _lib.lib(), np.zeros((2, 2))
    args = lambda ld, ptr: (_lib.stream(), plan._plan, 6, qw.ctypes.data, ql.ctypes.data, 2, _lib.ptr(f),
                            coef.ctypes.data, 0, ld, ptr)
    assert lib.stk_load_columns(*args(4, _lib.ptr(buf) + 8)) != 0 and b'aligned' in lib.stk_last_error()
    assert lib.stk_load_columns(*args(3, _lib.ptr(buf))) != 0 and b'aligned' in lib.stk_last_error()
    big = (ctypes.c_double * (3 * 17))()
    assert lib.stk_load_points(_lib.stream(), plan._plan, 17, big, _lib.ptr(buf)) != 0
    assert b'quadrature points' in lib.stk_last_error()
    torch.cuda.synchronize()
    assert not torch.any(buf)
