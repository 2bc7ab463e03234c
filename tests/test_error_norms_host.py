"""Error norms against an exact solution, host side (no GPU): the gradients of the
manufactured problems against finite differences, the exact solutions on host tensors,
which rank integrates which time element, and a NumPy oracle of the device computation in
np.longdouble -- with the first-order rounding bound the device is held to in
tests/test_error_norms_gpu.py -- checked on functions of the discrete space, against a
rule of degree 13, and on the SciPy restatements of two problems, whose L2(L2), L2(H1) and
final-time errors are pinned here."""
import ctypes
import functools
import math

import numpy as np
import pytest

from source.assembly import free_dofs, simplex_rule
from source.error_norms import element_owner, time_rule
from source.problem import problem_helper

MANUFACTURED = [('square_forced', 2), ('cube_forced', 3), ('square_nonseparable', 2), ('cube_nonseparable', 3)]
LD = np.longdouble
UNIT = 2.0**-53


# ---- the oracle --------------------------------------------------------------------------------
def geometry(mesh):
    """cells, |T| and grad lambda_a [nc][d + 1][d] in np.longdouble: the inverse of the edge
    matrix from np.linalg.inv, refined by one Newton step X + X (I - E X) in longdouble (the
    double inverse is good to cond(E) 2^-53, the step squares that).  Also, for the refined
    figure of oracle_element only, what the DEVICE's
    expressions (include/stk.h "space-time error norms") may lose, to first order in
    u = 2^-53, from the running bounds of their operations: an edge component p_r - p_0 one
    rounding; a difference of two products a b - c d of such components 5 u (|a b| + |c d|)
    (two roundings per product from its factors and its own, one for the difference); in 3-D
    det = sum e_i C_i: sum |e_i| err(C_i) + 4 u sum |e_i C_i|; a quotient
    err(num) / |det| + |num| err(det) / det^2 + u |num / det|; grad lambda_0: the sum of its
    terms' errors + (d - 1) u sum |terms|.  `vol_count` = err(det) / (u |det|) + 1 roundings
    of |T|; `grad_err` = the absolute error of every gradient entry."""
    p = np.asarray(mesh.points, dtype=np.float64)
    cells = np.asarray(mesh.cells, dtype=np.int64)
    d = cells.shape[1] - 1
    E64 = p[cells[:, 1:]] - p[cells[:, :1]]  # rows = edges
    X0 = np.linalg.inv(E64).astype(LD)
    E = p.astype(LD)[cells[:, 1:]] - p.astype(LD)[cells[:, :1]]
    X = X0 + X0 @ (np.eye(d, dtype=LD) - E @ X0)  # column a = grad lambda_{a + 1}
    grad = np.empty((len(cells), d + 1, d), dtype=LD)
    grad[:, 1:] = np.swapaxes(X, 1, 2)
    grad[:, 0] = -grad[:, 1:].sum(axis=1)
    aE = np.abs(E)
    if d == 2:
        det = E[:, 0, 0] * E[:, 1, 1] - E[:, 0, 1] * E[:, 1, 0]
        err_det = 5 * UNIT * (aE[:, 0, 0] * aE[:, 1, 1] + aE[:, 0, 1] * aE[:, 1, 0])
        num_abs = np.abs(grad[:, 1:] * det[:, None, None])
        err_num = UNIT * num_abs  # the numerators are single edge components
    else:
        cross = lambda a, b: np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                       a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
        det = (E[:, 0] * cross(E[:, 1], E[:, 2])).sum(axis=1)
        # numerator of grad lambda_{a + 1}[j] = (e_b x e_c)[j], (b, c) the cyclic successors of a:
        # |b c| + |c b| of its two products
        cof_abs = np.empty((len(cells), 3, 3), dtype=LD)
        for r in range(3):
            u, v = aE[:, (r + 1) % 3], aE[:, (r + 2) % 3]
            for j in range(3):
                cof_abs[:, r, j] = u[:, (j + 1) % 3] * v[:, (j + 2) % 3] + u[:, (j + 2) % 3] * v[:, (j + 1) % 3]
        err_num = 5 * UNIT * cof_abs
        err_det = (aE[:, 0] * err_num[:, 0]).sum(axis=1) + 4 * UNIT * (aE[:, 0] * cof_abs[:, 0]).sum(axis=1)
        num_abs = np.abs(grad[:, 1:] * det[:, None, None])
    adet = np.abs(det)
    grad_err = np.empty_like(grad)
    grad_err[:, 1:] = (err_num / adet[:, None, None] + num_abs * (err_det / adet**2)[:, None, None]
                       + UNIT * np.abs(grad[:, 1:]))
    grad_err[:, 0] = grad_err[:, 1:].sum(axis=1) + (d - 1) * UNIT * np.abs(grad[:, 1:]).sum(axis=1)
    vol = adet / math.factorial(d)
    return {'d': d, 'cells': cells, 'vol': vol, 'grad': grad, 'grad_err': grad_err,
            'vol_count': err_det / (UNIT * adet) + 1.0, 'points': p}


def oracle_element(geo, qw, ql, w_lo, w_hi, c, f, gf, lo, hi, refined=False):
    """What stk_err_element documents, in np.longdouble from the same doubles: f
    (n_k, nc, nq), gf (n_k, d, nc, nq) or None, lo / hi (nv,) nodal values of the two time
    nodes on ALL vertices (0 on the boundary).  Returns (values (4,), bounds (4,)).

    THE BOUND B the device is held to, to first order in u = 2^-53:
        B_L2  = u sum_{cells, k, q} c_k w_q |T| [n e_q^2 + 2 |e_q| (d + 4) (|f_q| + sum_a |l_qa| |U_a|)],
        n     = nq + n_k + ceil(log2 nc) + 8,
        B_H1  = the same with e_qj = gf_qj - G_j and |gf_qj| + sum_a |U_a| |grad l_a[j]|, summed over j,
        B_ref = n u sum |terms|.
    A term e_q^2 w_q |T| c_k passes the square, three products, at most nq - 1 + n_k - 1
    additions of its cell and at most ceil(log2 nc) + 1 of the two trees (absent lanes add exact
    zeros), and |T| carries its own few roundings: n covers them.  e_q = f_q - uh_q carries the
    rounding of the difference and d + 3 of uh_q (3 in U_a, a product, d additions).

    refined=True returns instead a LOOSER bound, never asserted, only printed beside B by the
    GPU tests -- what a worst-case analysis that trusts nothing adds: Ub_a = |w_lo lo_a| +
    |w_hi hi_a| in place of |U_a| (lo and hi of opposite sign cancel in U_a, its roundings
    do not), geometry()'s running count of the roundings of |T| added to n, one more addition
    in n for the sum over j, and 2 |e_qj| sum_a Ub_a err(grad l_a[j]) for the device's
    gradients."""
    d, cells = geo['d'], geo['cells']
    nc = len(cells)
    qw, ql = np.asarray(qw, dtype=LD), np.asarray(ql, dtype=LD)
    w_lo, w_hi, c = (np.asarray(a, dtype=LD) for a in (w_lo, w_hi, c))
    n_k, nq = len(c), len(qw)
    f = np.asarray(f, dtype=LD).reshape(n_k, nc, nq)
    lo_c, hi_c = np.asarray(lo, dtype=LD)[cells], np.asarray(hi, dtype=LD)[cells]  # (nc, d + 1)
    U = w_lo[:, None, None] * lo_c[None] + w_hi[:, None, None] * hi_c[None]  # (n_k, nc, d + 1)
    if refined:
        Ub = np.abs(w_lo)[:, None, None] * np.abs(lo_c)[None] + np.abs(w_hi)[:, None, None] * np.abs(hi_c)[None]
    else:
        Ub = np.abs(U)
    uh = np.einsum('qa,kca->kcq', ql, U)
    uh_abs = np.einsum('qa,kca->kcq', np.abs(ql), Ub)
    n = np.full(nc, nq + n_k + math.ceil(math.log2(max(nc, 2))) + 8, dtype=LD)  # per cell
    if refined:
        n = n + geo['vol_count']
    weight = np.abs(c)[:, None, None] * np.abs(qw)[None, None, :] * geo['vol'][None, :, None]  # (n_k, nc, nq)
    signed = c[:, None, None] * qw[None, None, :] * geo['vol'][None, :, None]
    e = f - uh
    vals, bounds = np.zeros(4, dtype=LD), np.zeros(4, dtype=LD)
    vals[0] = (signed * e * e).sum()
    vals[2] = (signed * f * f).sum()
    bounds[0] = UNIT * (weight * (n[None, :, None] * e * e + 2 * np.abs(e) * (d + 4) * (np.abs(f) + uh_abs))).sum()
    bounds[2] = UNIT * (weight * n[None, :, None] * f * f).sum()
    if gf is not None:
        gf = np.asarray(gf, dtype=LD).reshape(n_k, d, nc, nq)
        G = np.einsum('kca,caj->kjc', U, geo['grad'])  # (n_k, d, nc)
        G_abs = np.einsum('kca,caj->kjc', Ub, np.abs(geo['grad']))
        eg = gf - G[..., None]
        wj, sj, nj = weight[:, None], signed[:, None], (n + 1 if refined else n)[None, None, :, None]
        vals[1] = (sj * eg * eg).sum()
        vals[3] = (sj * gf * gf).sum()
        inner = UNIT * (nj * eg * eg + 2 * np.abs(eg) * (d + 4) * (np.abs(gf) + G_abs[..., None]))
        if refined:
            inner = inner + 2 * np.abs(eg) * np.einsum('kca,caj->kjc', Ub, geo['grad_err'])[..., None]
        bounds[1] = (wj * inner).sum()
        bounds[3] = UNIT * (wj * nj * gf * gf).sum()
    return vals, bounds


def quadrature_points(geo, ql):
    """(d, nc, nq) in float64: l_q0 p0 + l_q1 p1 + ..., summed from the left."""
    p, cells = geo['points'], geo['cells']
    ql = np.asarray(ql, dtype=np.float64)
    out = np.empty((geo['d'], len(cells), len(ql)))
    for k in range(geo['d']):
        x = ql[None, :, 0] * p[cells[:, 0], k][:, None]
        for a in range(1, geo['d'] + 1):
            x = x + ql[None, :, a] * p[cells[:, a], k][:, None]
        out[k] = x
    return out


def numpy_error_norms(mesh, mesh_time, U, exact, exact_grad=None, times=None, rule=None, nq_time=4, points=None,
                      evaluate=None):
    """The dict of source.error_norms.error_norms_collective from U (N, M) nodal values on
    the free dofs, in np.longdouble, with the same rules (`rule` = (weights, barycentric
    points) and `nq_time` replace them); squares under 'sq' = (4,), 'sq_at', and their
    first-order device bounds under 'bound', 'bound_at', 'bound_per_element'.  `points`
    (d, nc, nq) replaces the quadrature points and `evaluate(fn, t, points)` the NumPy
    evaluation of exact / exact_grad (the GPU tests pass the device's, so that the oracle
    starts from the same doubles)."""
    geo = geometry(mesh)
    d = geo['d']
    qw, ql = simplex_rule(mesh) if rule is None else rule
    pts = quadrature_points(geo, ql) if points is None else np.asarray(points)
    if evaluate is None:
        evaluate = lambda fn, t, x: fn(np.asarray(t).reshape(-1, 1, 1), *x)
    N, h, T = mesh_time.nv, mesh_time.h, mesh_time.T
    U = np.asarray(U, dtype=np.float64).reshape(N, -1)
    full = np.zeros((N, mesh.nv))
    full[:, free_dofs(mesh)] = U
    shape = lambda n_k: (n_k,) + pts.shape[1:]
    s, c = time_rule(mesh_time, nq_time)
    per, per_b = np.zeros((N - 1, 4), dtype=LD), np.zeros((N - 1, 4), dtype=LD)
    for e in range(N - 1):
        t = h * (e + s)
        f = np.broadcast_to(evaluate(exact, t, pts), shape(len(t)))
        gf = None
        if exact_grad is not None:
            gf = np.stack([np.broadcast_to(g, shape(len(t))) for g in evaluate(exact_grad, t, pts)], axis=1)
        per[e], per_b[e] = oracle_element(geo, qw, ql, 1.0 - s, s, c, f, gf, full[e], full[e + 1])
    times = np.atleast_1d(np.asarray([T] if times is None else times, dtype=np.float64))
    sq_at, b_at = np.zeros(len(times), dtype=LD), np.zeros(len(times), dtype=LD)
    for i, t in enumerate(times):
        x = t / h
        e = int(min(np.floor(x), N - 2))
        sv = x - e
        f = np.broadcast_to(evaluate(exact, times[i:i + 1], pts), shape(1))
        v, b = oracle_element(geo, qw, ql, [1.0 - sv], [sv], [1.0], f, None, full[e], full[e + 1])
        sq_at[i], b_at[i] = v[0], b[0]
    sq = per.sum(axis=0)
    # the host adds N - 1 doubles in ascending e: (N - 2) u sum |terms| more
    bound = per_b.sum(axis=0) + (N - 2) * UNIT * np.abs(per).sum(axis=0)
    root = lambda v: float(np.sqrt(v))
    grad = exact_grad is not None
    return {'l2_l2': root(sq[0]), 'l2_h1': root(sq[1]) if grad else None, 'exact_l2_l2': root(sq[2]),
            'exact_l2_h1': root(sq[3]) if grad else None, 'l2_at': np.sqrt(sq_at).astype(np.float64),
            'per_element': per, 'sq': sq, 'sq_at': sq_at, 'bound': bound, 'bound_at': b_at,
            'bound_per_element': per_b}


def conical_rule(n=7):
    """Stroud's conical product rule on the triangle, n x n points, exact to degree 2 n - 1
    (13 for n = 7): Gauss-Legendre along one side, Gauss-Jacobi (1, 0) towards the apex.
    Weights sum to 1; barycentric points (n^2, 3)."""
    from scipy.special import roots_jacobi
    xa, wa = roots_jacobi(n, 1.0, 0.0)
    xb, wb = np.polynomial.legendre.leggauss(n)
    u, v = 0.5 * (xa + 1.0), 0.5 * (xb + 1.0)  # u: weight (1 - u)
    l1 = np.repeat(u, n)
    l2 = np.outer(1.0 - u, v).reshape(-1)
    w = np.outer(wa / 4.0, wb / 2.0).reshape(-1) * 2.0  # area of the reference triangle = 1/2
    return w, np.stack([1.0 - l1 - l2, l1, l2], axis=1)


def nodal_values(mesh, mesh_time, fn):
    pts = mesh.points[free_dofs(mesh)]
    t = mesh_time.h * np.arange(mesh_time.nv)
    return fn(t[:, None], *(pts[None, :, k] for k in range(pts.shape[1])))


# ---- 1. the formulas ---------------------------------------------------------------------------
@pytest.mark.parametrize('problem,d', MANUFACTURED)
def test_exact_grad_is_the_gradient_of_exact(problem, d):
    """Central differences of data['exact'] with h = 1e-4 at 1000 seeded points, as
    test_g_is_the_heat_operator_of_the_exact_solution checks g: truncation
    h^2 / 6 |u'''| <= 1e-8 / 6 (2 pi)^3 ~ 4e-7 and rounding 2^-53 |u| / h ~ 1e-12, against
    1e-6 of the largest component.  Measured: 1.1e-7 .. 4.1e-7 relative to it."""
    data = problem_helper(problem, J_space=1, J_time=1)[3]
    u, grad = data['exact'], data['exact_grad']
    rng = np.random.RandomState(2024)
    t = 0.05 + 0.9 * rng.rand(1000)
    x = [0.05 + 0.9 * rng.rand(1000) for _ in range(d)]
    got = grad(t, *x)
    assert len(got) == d
    h = 1e-4
    for k in range(d):
        lo, hi = list(x), list(x)
        lo[k], hi[k] = x[k] - h, x[k] + h
        want = (u(t, *hi) - u(t, *lo)) / (2 * h)
        err, scale = np.max(np.abs(got[k] - want)), np.max(np.abs(want))
        print('%s d/dx%d: largest %.3f, difference %.2e' % (problem, k, scale, err))
        assert got[k].shape == (1000,) and err <= 1e-6 * scale
    # broadcasts like exact, on torch tensors too
    import torch
    tt, xx = rng.rand(4, 1, 1), [rng.rand(7, 6) for _ in range(d)]
    on_numpy = grad(tt, *xx)
    on_torch = grad(torch.from_numpy(tt), *[torch.from_numpy(c) for c in xx])
    for a, b in zip(on_numpy, on_torch):
        assert a.shape == (4, 7, 6) and torch.is_tensor(b) and b.dtype == torch.float64
        assert np.max(np.abs(b.numpy() - a)) <= 16 * UNIT * 8.0  # a few roundings of terms up to 2 pi


@pytest.mark.parametrize('problem,d', [('square_forced', 2), ('cube_forced', 3)])
def test_forced_exact_takes_torch_tensors_and_keeps_its_numpy_doubles(problem, d):
    import torch
    data = problem_helper(problem, J_space=1, J_time=1)[3]
    rng = np.random.RandomState(5)
    t, x = rng.rand(4, 1, 1), [rng.rand(70, 6) for _ in range(d)]
    first = {2: lambda x, y: np.sin(np.pi * x) * np.sin(np.pi * y),
             3: lambda x, y, z: np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)}[d]
    second = {2: lambda x, y: np.sin(2 * np.pi * x) * np.sin(np.pi * y),
              3: lambda x, y, z: np.sin(2 * np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)}[d]
    on_numpy = data['exact'](t, *x)
    assert np.array_equal(on_numpy, np.exp(-t) * first(*x) + t * second(*x))  # the doubles it gave before
    on_torch = data['exact'](torch.from_numpy(t), *[torch.from_numpy(c) for c in x])
    assert torch.is_tensor(on_torch) and on_torch.dtype == torch.float64 and tuple(on_torch.shape) == (4, 70, 6)
    assert np.array_equal(on_torch.numpy(), on_numpy)
    assert np.array_equal(data['exact'](0.25, *x), (np.exp(-0.25) * first(*x) + 0.25 * second(*x)))


# ---- 2. who integrates which element -------------------------------------------------------------
def test_every_element_has_exactly_one_integrating_rank():
    from source import _lib
    lib = _lib.lib()
    for N in range(2, 18):
        for size in range(1, min(8, N) + 1):  # size = N: more ranks than the N - 1 elements
            count = np.zeros(N - 1, dtype=int)
            for rank in range(size):
                tb, te = ctypes.c_int32(), ctypes.c_int32()
                assert lib.stk_partition(N, size, rank, ctypes.byref(tb), ctypes.byref(te), None, None) == 0
                mine = element_owner(N, tb.value, te.value)
                assert all(tb.value <= e + 1 < te.value for e in mine)
                # the lower node is a local column or the ghost row
                assert all(e >= tb.value - 1 for e in mine)
                count[mine] += 1
            assert np.array_equal(count, np.ones(N - 1, dtype=int)), (N, size, count)


# ---- 3. the oracle ---------------------------------------------------------------------------------
def test_oracle_is_zero_on_the_discrete_space():
    """I_h of a function that is P1 in space and linear in time IS that function: every
    norm of the difference is 0 up to the roundings of the oracle's own longdouble sums and of
    the doubles it is fed (nodal values and f, each good to 2^-53): (error)^2 <= 1e-28 of
    (norm)^2."""
    for problem, J in (('square', 2), ('cube', 1)):
        mesh, _, mesh_time, _, _ = problem_helper(problem, J_space=J, J_time=2)
        d = mesh.cells.shape[1] - 1
        coef = [0.3, -1.1, 0.7][:d]
        fn = lambda t, *x: (1.0 + 2.0 * t) * (0.5 + sum(a * c for a, c in zip(coef, x)))
        grad = lambda t, *x: tuple((1.0 + 2.0 * t) * a + 0.0 * x[0] for a in coef)
        # the boundary values are not zero: give the oracle a mesh without boundary
        mesh.boundary = np.zeros(mesh.nv, dtype=bool)
        got = numpy_error_norms(mesh, mesh_time, nodal_values(mesh, mesh_time, fn), fn, grad, times=[0.0, 0.3, 1.0])
        print(problem, got['sq'], got['sq_at'])
        assert got['sq'][0] <= 1e-28 * got['sq'][2] and got['sq'][1] <= 1e-28 * got['sq'][3]
        assert np.all(got['sq_at'] <= 1e-28)
        assert got['sq'][2] > 0.1 and got['sq'][3] > 0.1


def test_oracle_reproduces_the_norm_of_the_exact_solution():
    """U = 0: the 'error' is u itself.  || u ||^2 of square_forced is known in closed form
    (s_11 and s_21 are orthogonal, || s ||^2 = 1/4, || grad s_kl ||^2 = (k^2 + l^2) pi^2 / 4):
        L2(L2)^2 = ((1 - e^-2) / 2 + 1/3) / 4,   L2(H1)^2 = pi^2 (2 (1 - e^-2) / 2 + 5/3) / 4,
    and the conical rule of degree 13 with 7 Gauss points in time reproduces both to 1e-9
    relative at J = 3 (measured 1.5e-16 and 0: its own error).  THE ERROR OF THE DEGREE-4
    RULE the device uses: per cell at most about 2 (2 pi h)^5 / 5! of the largest |u^2| with
    h = the diameter sqrt(2) / 8 of a cell -- 1.0e-2 relative here, which is what is asserted.
    Measured: 6.7e-15 on the L2 norm squared and 4.4e-15 on the H1 one, far below it,
    because THIS integrand is periodic on the square and the mesh uniform (a composite rule
    is then as good as the trapezoidal rule on a period); a general u only has the bound.
    Both figures are printed."""
    mesh, _, mesh_time, data, _ = problem_helper('square_forced', J_space=3, J_time=3)
    zero = np.zeros((mesh_time.nv, len(free_dofs(mesh))))
    fine = numpy_error_norms(mesh, mesh_time, zero, data['exact'], data['exact_grad'], rule=conical_rule(7), nq_time=7)
    own = numpy_error_norms(mesh, mesh_time, zero, data['exact'], data['exact_grad'])
    l2 = ((1.0 - math.exp(-2.0)) / 2.0 + 1.0 / 3.0) / 4.0
    h1 = math.pi**2 * (2.0 * (1.0 - math.exp(-2.0)) / 2.0 + 5.0 / 3.0) / 4.0
    rel = lambda a, b: abs(float(a) - b) / b
    print('degree 13 against the closed form: %.2e, %.2e' % (rel(fine['sq'][2], l2), rel(fine['sq'][3], h1)))
    print('degree 4 against degree 13: %.3e, %.3e'
          % (rel(own['sq'][2], float(fine['sq'][2])), rel(own['sq'][3], float(fine['sq'][3]))))
    assert rel(fine['sq'][2], l2) <= 1e-9 and rel(fine['sq'][3], h1) <= 1e-9
    rule_error = 2.0 * (2.0 * math.pi * math.sqrt(2.0) / 8.0)**5 / 120.0
    assert rel(own['sq'][2], float(fine['sq'][2])) <= rule_error
    assert rel(own['sq'][3], float(fine['sq'][3])) <= rule_error
    # with U = 0 the error IS the reference
    assert own['sq'][0] == own['sq'][2] and own['sq'][1] == own['sq'][3]
    assert abs(own['l2_at'][0]**2 - (math.exp(-2.0) + 1.0) / 4.0) <= rule_error * 0.5


# ---- 4. the SciPy restatements -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scipy_solution(problem, J):
    """The discrete solution (N, M) of the SciPy restatement of `problem` at
    J_time = J_space = J: the solve of the existing host tests' scipy_error, reused by
    import -- their CG is watched for what it returns."""
    import test_forcing_host
    import test_spacetime_load_host
    module, call = {'square_forced': (test_forcing_host, lambda: test_forcing_host.scipy_error(J)),
                    'square_nonseparable': (test_spacetime_load_host,
                                            lambda: test_spacetime_load_host.scipy_error(problem, J))}[problem]
    # the host test module's own name `spla` is pointed at a stand-in that hands everything
    # on to scipy.sparse.linalg and remembers what cg returns; scipy itself is not touched
    real, seen = module.spla, []

    class Watched:
        def __getattr__(self, name):
            return getattr(real, name)

        @staticmethod
        def cg(*args, **kw):
            out = real.cg(*args, **kw)
            seen.append(out[0])
            return out

    module.spla = Watched()
    try:
        call()
    finally:
        module.spla = real
    assert len(seen) == 1
    mesh, _, mesh_time, data, _ = problem_helper(problem, J_space=J, J_time=J)
    return mesh, mesh_time, data, seen[0].reshape(mesh_time.nv, -1)


# l2_l2, l2_h1, l2_at(T) of the SciPy restatements (measured on the CPU by the test below)
PINNED = {
    ('square_forced', 3): (7.5677554994e-03, 3.2672921565e-01, 1.1975390468e-02),
    ('square_forced', 4): (1.9061100523e-03, 1.6394192725e-01, 3.0188751885e-03),
    ('square_nonseparable', 3): (2.9893602657e-03, 1.2448434843e-01, 1.5582215608e-03),
    ('square_nonseparable', 4): (7.5048152084e-04, 6.2337801994e-02, 3.8884590464e-04),
}


def scipy_norms(problem, J):
    mesh, mesh_time, data, U = scipy_solution(problem, J)
    return numpy_error_norms(mesh, mesh_time, U, data['exact'], data['exact_grad'])


@pytest.mark.parametrize('problem', ['square_forced', 'square_nonseparable'])
def test_scipy_restatement_converges_in_the_error_norms(problem):
    """J_time = J_space = 3, 4, norms of u - u_h by the oracle.  Measured on the CPU:
        square_forced        L2(L2) 7.568e-3 -> 1.906e-3 (ratio 3.970; relative 1.73e-2, 4.36e-3),
                             L2(H1) 3.267e-1 -> 1.639e-1 (ratio 1.993; relative 1.31e-1, 6.56e-2),
                             L2 at T 1.198e-2 -> 3.019e-3 (ratio 3.967);
        square_nonseparable  L2(L2) 2.989e-3 -> 7.505e-4 (ratio 3.983; relative 1.06e-2, 2.66e-3),
                             L2(H1) 1.245e-1 -> 6.234e-2 (ratio 1.997; relative 9.88e-2, 4.95e-2),
                             L2 at T 1.558e-3 -> 3.888e-4 (ratio 4.007).
    Theory: second order in L2, first order in the gradient -- the L2 ratio in [3.5, 4.5] as
    the neighbouring convergence tests ask, the H1 ratio in [1.8, 2.2].  The figures are
    pinned (PINNED): the device's end-to-end test compares with them."""
    n3, n4 = scipy_norms(problem, 3), scipy_norms(problem, 4)
    for J, n in ((3, n3), (4, n4)):
        print('%s J = %d: l2_l2 %.10e l2_h1 %.10e l2_at(T) %.10e (relative %.4e, %.4e)'
              % (problem, J, n['l2_l2'], n['l2_h1'], n['l2_at'][0], n['l2_l2'] / n['exact_l2_l2'],
                 n['l2_h1'] / n['exact_l2_h1']))
        want = PINNED[(problem, J)]
        got = (n['l2_l2'], n['l2_h1'], n['l2_at'][0])
        # CG stops at 1e-12 of the residual: the pinned figures hold to 1e-8 relative
        assert all(abs(g - w) <= 1e-8 * w for g, w in zip(got, want)), (got, want)
    print('ratios: L2 %.3f, H1 %.3f, L2 at T %.3f' % (n3['l2_l2'] / n4['l2_l2'], n3['l2_h1'] / n4['l2_h1'],
                                                      n3['l2_at'][0] / n4['l2_at'][0]))
    assert 3.5 <= n3['l2_l2'] / n4['l2_l2'] <= 4.5
    assert 1.8 <= n3['l2_h1'] / n4['l2_h1'] <= 2.2
