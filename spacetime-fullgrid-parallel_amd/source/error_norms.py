"""Error norms of a discrete solution against an exact one, by quadrature on the device
(csrc/err_norms.hip, include/stk.h "space-time error norms"):

    || u - u_h ||  in  L2(I; L2(Omega)),  L2(I; H^1_0(Omega))  and  L2(Omega) at given times,

for a trial-space vector u_h (continuous P1 in time, P1 in space) -- norms of the error
itself, gradient included, not of u_h - I_h u, and without downloading the slab.

* ``ErrorPlan(mesh, mesh_time)``: the mesh, the vertex -> slab-row map, |T| and the
  gradients of the barycentric coordinates on the device, built once; ``points()`` = the
  quadrature points of the mesh's own rule (assembly.simplex_rule), computed once;
  ``element(...)`` = one stk_err_element call.
* ``element_owner``: which time elements a rank integrates (pure NumPy).
* ``error_norms_collective``: the whole computation, all-reduced.

Space: the degree-4 rule of the load vectors.  Time: the four Gauss points per element of
the test-space loads (assembly.time_rule_test_space; degree 7).  Both are exact for the
squares of discrete functions; for a smooth u the quadrature error is far below the
discretisation error it measures.

Scope: vectors of the TRIAL space.  The H^1(I; H^-1) part of the X-norm and test-space
vectors are not served.
"""
import numpy as np

from .p1_plan import MeshPlanHandle


def element_owner(N, t_begin, t_end):
    """The time elements e (0 .. N - 2, between the nodes e and e + 1) that the rank
    owning the nodes [t_begin, t_end) integrates: those whose UPPER node e + 1 it owns.
    Every element has exactly one such rank, whatever the partition; a rank that owns
    node 0 alone integrates none."""
    return np.arange(max(t_begin - 1, 0), max(t_end - 1, 0), dtype=np.int64)


class ErrorPlan:
    """The error-norm engine of libstk on one mesh.  Not for two streams at once: the
    plan owns the tile partials of a call in flight."""
    def __init__(self, mesh, mesh_time):
        from . import _lib
        from .assembly import simplex_rule
        self._lib = _lib
        self.mesh_time = mesh_time
        self.qw, self.ql = (np.ascontiguousarray(a, dtype=np.float64) for a in simplex_rule(mesh))
        self._points = None
        self._plan = MeshPlanHandle(mesh, lambda lib, m, out: lib.stk_err_plan_create(*m, out),
                                    lambda lib, plan: lib.stk_err_plan_destroy(plan))
        self.d, self.nc, self.n_free = self._plan.d, self._plan.nc, self._plan.n_free

    def points(self, ql=None):
        """Device tensor (d, nc, nq): coordinate k of quadrature point q of cell t; of the
        mesh's own rule (kept) or of the barycentric points `ql`.  The doubles of
        DeviceLoadPlan.points."""
        import torch
        _lib = self._lib
        if ql is None and self._points is not None:
            return self._points
        rule = self.ql if ql is None else np.ascontiguousarray(ql, dtype=np.float64)
        assert rule.ndim == 2 and rule.shape[1] == self.d + 1, rule.shape
        out = torch.empty((self.d, self.nc, rule.shape[0]), dtype=torch.float64, device=_lib.compute_device())
        _lib.check(_lib.lib().stk_err_points(_lib.stream(), self._plan, rule.shape[0], rule.ctypes.data, _lib.ptr(out)))
        if ql is None:
            self._points = out
        return out

    def element(self, f, gf, w_lo, w_hi, c, u_lo, stride_lo, u_hi, stride_hi, out4, qw=None, ql=None):
        """One stk_err_element call: f (n_k, nc, nq) and gf (n_k, d, nc, nq) or None, device
        tensors; w_lo, w_hi, c (n_k,) host arrays; u_lo / u_hi device POINTERS (integers) to
        row 0 of the two time nodes with their row strides in doubles; out4 a contiguous
        device tensor of 4 doubles."""
        import torch
        _lib = self._lib
        qw = self.qw if qw is None else np.ascontiguousarray(qw, dtype=np.float64)
        ql = self.ql if ql is None else np.ascontiguousarray(ql, dtype=np.float64)
        w_lo, w_hi, c = (np.ascontiguousarray(a, dtype=np.float64) for a in (w_lo, w_hi, c))
        n_k, nq = len(c), len(qw)
        assert w_lo.shape == w_hi.shape == c.shape == (n_k,) and ql.shape == (nq, self.d + 1)
        assert f.dtype == torch.float64 and f.is_contiguous() and tuple(f.shape) == (n_k, self.nc, nq), tuple(f.shape)
        if gf is not None:
            assert gf.dtype == torch.float64 and gf.is_contiguous() and tuple(gf.shape) == (n_k, self.d, self.nc, nq)
        assert out4.dtype == torch.float64 and out4.is_contiguous() and out4.numel() == 4
        _lib.check(_lib.lib().stk_err_element(
            _lib.stream(), self._plan, nq, qw.ctypes.data, ql.ctypes.data, n_k, w_lo.ctypes.data, w_hi.ctypes.data,
            c.ctypes.data, _lib.ptr(f), _lib.ptr(gf), int(u_lo), int(stride_lo), int(u_hi), int(stride_hi), _lib.ptr(out4)))


def time_rule(mesh_time, nq=4):
    """(s, c): the Gauss points s_k on [0, 1] of assembly.time_rule_test_space and the
    weights c_k = 0.5 h w_k of an element of length h."""
    from .assembly import time_rule_test_space
    s, _ = time_rule_test_space(mesh_time, nq)
    _, w = np.polynomial.legendre.leggauss(nq)
    return s, 0.5 * mesh_time.h * w


def evaluate_exact(plan, exact, exact_grad, t):
    """exact and exact_grad at the times t (n_k,) and the quadrature points of the plan,
    ON THE DEVICE with torch tensors that broadcast, as assembly.fill_test_space_slab
    evaluates a forcing: f (n_k, nc, nq) and gf (n_k, d, nc, nq) or None, contiguous."""
    import torch
    pts = plan.points()
    n_k = len(t)
    shape = (n_k,) + tuple(pts.shape[1:])
    tt = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(pts.device).reshape(n_k, 1, 1)
    full = lambda v: torch.broadcast_to(torch.as_tensor(v, dtype=torch.float64, device=pts.device), shape)
    f = full(exact(tt, *pts)).contiguous()
    gf = None
    if exact_grad is not None:
        parts = exact_grad(tt, *pts)
        assert len(parts) == plan.d, 'exact_grad returns %d arrays on a mesh of dimension %d' % (len(parts), plan.d)
        gf = torch.stack([full(p) for p in parts], dim=1).contiguous()
    return f, gf


def error_norms_collective(plan, vec, exact, exact_grad=None, times=None):
    """The norms of u - u_h for the trial-space vector `vec` (KronVectorMPI) on every rank.

    A rank integrates the time elements whose upper node it owns (element_owner); the
    lower node of its first one is the ghost row X_lo of vec.communicate_bdr().  Per
    element: exact (and exact_grad) at the four Gauss points in time and the quadrature
    points of the mesh, evaluated with torch on the device, and ONE stk_err_element call
    that writes the element's row of a device array (N - 1 + n_times, 4).  A time t of
    `times` (default [T]) lies in element e = min(floor(t / h), N - 2) at s = t / h - e:
    one call with n_k = 1, c = 1 and weights (1 - s, s) by the rank that integrates e.
    The array is all-reduced with the communicator of the vector -- every entry has one
    non-zero contributor, the pattern of KronVectorMPI.dot -- and the element rows are
    added in ascending e on the host (stk_sum_steps): the result does not depend on the
    number of ranks, bit for bit.

    Returns a dict: l2_l2, l2_h1 (the norms of the error), exact_l2_l2, exact_l2_h1 (those
    of u by the same rule), l2_at (array over `times`), per_element ((N - 1, 4): the
    SQUARES err_L2, err_H1, ref_L2, ref_H1 per time element).  The H1 entries are None
    without exact_grad."""
    import torch
    _lib = plan._lib
    mesh_time = plan.mesh_time
    N, h, T = mesh_time.nv, mesh_time.h, mesh_time.T
    assert N == vec.N and N >= 2, (N, vec.N)
    assert vec.M == plan.n_free, (vec.M, plan.n_free)
    times = np.atleast_1d(np.asarray([T] if times is None else times, dtype=np.float64))
    if times.ndim != 1 or not np.all((times >= 0.0) & (times <= T)):
        raise ValueError('times must be a list of times in [0, %g]' % T)
    x = times / h
    e_of = np.minimum(np.floor(x), N - 2).astype(np.int64)
    s_of = x - e_of

    mine = element_owner(N, vec.t_begin, vec.t_end)
    vec.communicate_bdr()  # collective; X_lo = the time row t_begin - 1
    out = torch.zeros((N - 1 + len(times), 4), dtype=torch.float64, device=vec.buf.device)
    base = _lib.ptr(vec.buf)

    def node(n):
        """(pointer to row 0, row stride) of the time node n"""
        if n == vec.t_begin - 1:
            return _lib.ptr(vec.X_lo), 1
        assert vec.t_begin <= n < vec.t_end, (n, vec.t_begin, vec.t_end)
        return base + 8 * int(n - vec.t_begin), vec.ld

    s, c = time_rule(mesh_time)
    for e in mine:
        f, gf = evaluate_exact(plan, exact, exact_grad, h * (e + s))
        plan.element(f, gf, 1.0 - s, s, c, *node(e), *node(e + 1), out[e])
    for i, (e, sv) in enumerate(zip(e_of, s_of)):
        if len(mine) and mine[0] <= e <= mine[-1]:
            f, _ = evaluate_exact(plan, exact, None, times[i:i + 1])
            plan.element(f, None, [1.0 - sv], [sv], [1.0], *node(e), *node(e + 1), out[N - 1 + i])
    vec.dofs_distr.comm.allreduce_tensor_(out)
    rows = out.cpu().numpy()
    per_element = np.ascontiguousarray(rows[:N - 1])
    lib = _lib.lib()
    total = []
    for k in range(4):
        col = np.ascontiguousarray(per_element[:, k])
        total.append(float(lib.stk_sum_steps(col.ctypes.data, N - 1)))
    with_grad = exact_grad is not None
    return {'l2_l2': float(np.sqrt(total[0])),
            'l2_h1': float(np.sqrt(total[1])) if with_grad else None,
            'exact_l2_l2': float(np.sqrt(total[2])),
            'exact_l2_h1': float(np.sqrt(total[3])) if with_grad else None,
            'l2_at': np.sqrt(rows[N - 1:, 0]),
            'per_element': per_element}
