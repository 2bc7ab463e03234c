"""Non-separable source terms, host side (no GPU): the formulas of the manufactured
problems against finite differences of their exact solutions, a NumPy restatement of the
general space-time load (one space_load per time quadrature point) that converges to the
exact solution at second order and reproduces the separable path, and the argument checks
of the device engine that need no device."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from source.assembly import (free_dofs, space_load, space_matrices, time_load_test_space, time_matrices,
                             time_matrices_test_space, time_rule_test_space)
from source.problem import problem_helper

NONSEPARABLE = [('square_nonseparable', 2), ('cube_nonseparable', 3)]


def numpy_load(mesh_space, mesh_time, fn, numpy_path=True, elements=None):
    """The general load of the test space, restated: for every time element e and Gauss
    point t_k = h (e + s_k) one spatial load vector L_k of fn(t_k, .) (space_load), and
    the element's pair sum_k coef[k][a] L_k with k ascending, the first product starting
    the sum.  Time-major (2 n_elements, M), rows 2e + a.  numpy_path=False takes the host
    threads of libstk on triangulations (the sums the device engine reproduces bit for
    bit)."""
    s, coef = time_rule_test_space(mesh_time)
    elements = range(mesh_time.nv - 1) if elements is None else elements
    rows = []
    for e in elements:
        pair = None
        for k, t in enumerate(mesh_time.h * (e + s)):
            L = space_load(mesh_space, lambda *x: fn(t, *x), numpy_path=numpy_path)
            term = coef[k][:, None] * L[None, :]
            pair = term if pair is None else pair + term
        rows.append(pair)
    return np.concatenate(rows)


def sum_of_pairs(pairs):
    """The separable pairs of a problem as ONE callable g(t, x, y[, z])."""
    return lambda t, *x: sum(g_t(t) * g_x(*x) for g_t, g_x in pairs)


# ---- 1. the formulas -----------------------------------------------------------------------
@pytest.mark.parametrize('problem,d', NONSEPARABLE)
def test_g_is_the_heat_operator_of_the_exact_solution(problem, d):
    """g = u_t - laplace u of data['exact'] by central differences with h = 1e-4 at 1000
    seeded interior points: truncation h^2 / 6 |u'''| + h^2 / 12 sum |u''''| ~ 1e-6 and
    rounding 4 d 2^-53 |u| / h^2 ~ 1e-7, against 1e-5 of the largest |g|.  The test prints
    its figures; at THIS file's points (RandomState(2024), 0.05 + 0.9 rand), on the CPU
    with NumPy: largest difference 1.84e-7 where the largest |g| is 16.1 on the square,
    2.85e-7 and 24.6 on the cube.  Both figures depend on the points drawn (the issue
    quotes 2.0e-7 and 15.3 for the square from a draw of its own); the bound does not."""
    data = problem_helper(problem, J_space=1, J_time=1)[3]
    u, g = data['exact'], data['g'][0]
    rng = np.random.RandomState(2024)
    t = 0.05 + 0.9 * rng.rand(1000)
    x = [0.05 + 0.9 * rng.rand(1000) for _ in range(d)]
    h = 1e-4
    ut = (u(t + h, *x) - u(t - h, *x)) / (2 * h)
    lap = 0.0
    for k in range(d):
        lo, hi = list(x), list(x)
        lo[k], hi[k] = x[k] - h, x[k] + h
        lap = lap + (u(t, *hi) - 2.0 * u(t, *x) + u(t, *lo)) / h**2
    want, got = ut - lap, g(t, *x)
    err = np.max(np.abs(got - want))
    print('%s: largest |g| %.3f, difference %.2e' % (problem, np.max(np.abs(got)), err))
    assert err <= 1e-5 * np.max(np.abs(got))
    # u(0) is the problem's u0
    assert np.array_equal(u(0.0, *x), data['u0'](*x))


# ---- 2. the new problems exist, and their functions take both array types -------------------
@pytest.mark.parametrize('problem,d', NONSEPARABLE + [('square_moving_source', 2)])
def test_new_problems_return_callables_for_numpy_and_torch(problem, d):
    """problem_helper returns (it asserted on these names before); data['g'] is a list
    of one callable that broadcasts (n_k, 1, 1) against (cells, points), on NumPy arrays and
    on torch tensors alike -- the same function within a few roundings of its terms."""
    import torch
    mesh_space, _, mesh_time, data, name = problem_helper(problem, J_space=2, J_time=3)
    assert name == problem and mesh_time.nv == 9 and mesh_space.cells.shape[1] == d + 1
    assert len(data['g']) == 1 and callable(data['g'][0])
    g = data['g'][0]
    rng = np.random.RandomState(5)
    t, x = rng.rand(4, 1, 1), [rng.rand(7, 6) for _ in range(d)]
    on_numpy = g(t, *x)
    on_torch = g(torch.from_numpy(t), *[torch.from_numpy(c) for c in x])
    assert isinstance(on_numpy, np.ndarray) and on_numpy.shape == (4, 7, 6) and on_numpy.dtype == np.float64
    assert torch.is_tensor(on_torch) and on_torch.dtype == torch.float64 and tuple(on_torch.shape) == (4, 7, 6)
    scale = 64.0 if 'nonseparable' in problem else 1.0  # the terms of g: up to (d pi^2 + 2 pi) |s E|
    assert np.max(np.abs(on_torch.numpy() - on_numpy)) <= 16 * 2.0**-53 * scale
    # a scalar time, as the NumPy restatement passes it
    assert np.allclose(g(float(t[1, 0, 0]), *x), on_numpy[1], rtol=1e-14, atol=1e-15)
    if problem == 'square_moving_source':
        # the centre of the source is on the circle: g = 1 there, and u0 = 0
        assert g(0.25, np.array([0.5]), np.array([0.75]))[0] == pytest.approx(1.0, abs=1e-15)
        assert not np.any(data['u0'](*x)) and 'exact' not in data


# ---- 3. the restatement reproduces the separable path ---------------------------------------
@pytest.mark.parametrize('problem,J', [('square_forced', 3), ('cube_forced', 2)])
def test_restatement_agrees_with_the_separable_path(problem, J):
    """The separable g of a forced problem fed as one callable: the same quadrature rules
    in time and space, so only rounding separates the two -- 1e-14 of the largest entry
    (measured 2.7e-16 on the square, 3.6e-16 on the cube)."""
    mesh_space, _, mesh_time, data, _ = problem_helper(problem, J_space=J, J_time=J)
    pairs = sum(np.kron(time_load_test_space(mesh_time, g_t), space_load(mesh_space, g_x, numpy_path=True))
                for g_t, g_x in data['g'])
    got = numpy_load(mesh_space, mesh_time, sum_of_pairs(data['g'])).reshape(-1)
    dev = np.max(np.abs(got - pairs)) / np.max(np.abs(pairs))
    print('%s J = %d: %.2e of the largest entry' % (problem, J, dev))
    assert dev <= 1e-14
    if mesh_space.cells.shape[1] == 3:
        # ... and through the host threads of libstk, the sums the device engine repeats
        lib = numpy_load(mesh_space, mesh_time, sum_of_pairs(data['g']), numpy_path=False).reshape(-1)
        assert np.max(np.abs(lib - pairs)) / np.max(np.abs(pairs)) <= 1e-14


# ---- 4. SciPy restatement against the exact solution -----------------------------------------
def scipy_error(problem, J):
    """Relative (M_t kron M_x) error of the discrete solution at J_time = J_space = J
    against the nodal values of the exact solution, as tests/test_forcing_host.py:
    scipy_error, with g from numpy_load."""
    mesh_space, _, mesh_time, data, _ = problem_helper(problem, J_space=J, J_time=J)
    A_t, L_t, M_t, G_t, u0_t = time_matrices(mesh_time)
    M_Y, Minv_Y, B1_t, B2_t = time_matrices_test_space(mesh_time)
    M_x, A_x = space_matrices(mesh_space, scipy_path=True)
    g = numpy_load(mesh_space, mesh_time, data['g'][0]).reshape(-1)
    u0_x = space_load(mesh_space, data['u0'], numpy_path=True)
    N, M, NY = G_t.shape[0], M_x.shape[0], Minv_Y.shape[0]
    B = sp.kron(B1_t, M_x) + sp.kron(B2_t, A_x)
    G = sp.kron(G_t, M_x)
    lu = spla.splu(sp.csc_matrix(A_x))

    def K(y):
        Z = Minv_Y @ y.reshape(NY, M)
        return lu.solve(np.ascontiguousarray(Z.T)).T.reshape(-1)

    S = spla.LinearOperator((N * M, N * M), matvec=lambda v: B.T @ K(B @ v) + G @ v, dtype=np.float64)
    f = B.T @ K(g) + np.kron(u0_t, u0_x)
    Pre = spla.LinearOperator((N * M, N * M), dtype=np.float64,
                              matvec=lambda v: lu.solve(np.ascontiguousarray(v.reshape(N, M).T)).T.reshape(-1))
    u, info = spla.cg(S, f, rtol=1e-12, atol=0.0, M=Pre, maxiter=20000)
    assert info == 0, info
    pts = mesh_space.points[free_dofs(mesh_space)]
    t = mesh_time.h * np.arange(N)
    exact = data['exact'](t[:, None], *(pts[None, :, k] for k in range(pts.shape[1]))).reshape(-1)
    MM = sp.kron(M_t, M_x)
    e = u - exact
    return np.sqrt(e @ (MM @ e)) / np.sqrt(exact @ (MM @ exact))


def test_scipy_restatement_of_the_nonseparable_problem_converges():
    """Measured on the CPU: 2.32e-2 at J = 2, 5.99e-3 at J = 3, 1.50e-3 at J = 4: second
    order, ratio 3.99 from J = 3 to 4; the bound on J = 4 is the measured value and a
    quarter.  A wrong sign or scale of any term of g stalls the error at the size of
    that term."""
    e3, e4 = scipy_error('square_nonseparable', 3), scipy_error('square_nonseparable', 4)
    print('relative M_t kron M_x error: J=3 %.4e, J=4 %.4e, ratio %.3f' % (e3, e4, e3 / e4))
    assert 3.5 <= e3 / e4 <= 4.5
    assert e4 <= 1.9e-3


# ---- 5. the device engine refuses what it cannot do, before it touches a device ---------------
def test_load_plan_arguments_are_checked_on_the_host():
    from source import _lib
    lib = _lib.lib()
    mesh = problem_helper('square', J_space=2)[0]
    assert len(free_dofs(mesh)) > 1
    pts = np.ascontiguousarray(mesh.points)
    cells = np.ascontiguousarray(mesh.cells, dtype=np.int64)
    fd = np.ascontiguousarray(free_dofs(mesh), dtype=np.int64)
    plan = ctypes.c_void_p()

    def create(d=2, nv=mesh.nv, cells=cells, fd=fd, order=None, max_k=4):
        return lib.stk_load_plan_create(d, nv, len(cells), pts.ctypes.data, cells.ctypes.data, len(fd),
                                        fd.ctypes.data, None if order is None else order.ctypes.data, max_k,
                                        ctypes.byref(plan))

    bad_cells = cells.copy()
    bad_cells[-1, 2] = mesh.nv
    for kw, word in ((dict(d=4), b'bad arguments'), (dict(max_k=0), b'time points'),
                     (dict(max_k=17), b'time points'), (dict(cells=bad_cells), b'names vertex'),
                     (dict(fd=np.array([mesh.nv], dtype=np.int64)), b'free dof'),
                     (dict(order=np.zeros(len(fd), dtype=np.int32)), b'permutation')):
        assert create(**kw) != 0, kw
        assert word in lib.stk_last_error(), (kw, lib.stk_last_error())
        assert not plan.value
    assert lib.stk_load_plan_destroy(None) == 0
