"""The C Krylov loops of the ABI (csrc/krylov.hip) driven from ctypes: stk_pcg_solve_slab
and stk_lanczos_slab on 1..8 ranks (threads, tests/thread_comm.py), the flat
stk_pcg_solve with a real all-reduce, their refusals and early exits.  Needs an MI355X.

Two kinds of operators:
* explicit ones written in torch, T(x)[:, t] = c_t K x[:, t] with K = tridiag(-1, 3, -1)
  (1-D Laplacian plus identity) and c_t depending on the GLOBAL time step (a rank must
  use its t_begin), P = the Jacobi inverse.  The NumPy twins of these operators round
  every entry exactly as the torch ones do, so against oracle/krylov.py (float64 NumPy)
  only the inner products differ;
* the heat equation's WT_S_W and P (HeatEquationMPI, J_space = 6, J_time = 3: N = 9,
  M = 16 129), as tests/mp_parity_worker.py solves it.

What stk.h promises and is asserted here: on slabs, history, iteration count and
iterate are bit for bit those of a one-rank run whatever the number of ranks; the work
sizers cover everything the loops touch; refusals leave the caller's arrays alone.
The deviations the docstrings quote were measured on an MI355X; the assertion messages
carry the measured value."""
import ctypes
import threading

import numpy as np
import pytest
import torch

from conftest import load_golden
from thread_comm import run_ranks

pytestmark = pytest.mark.gpu

RANKS = (1, 2, 3, 4, 8)
SHAPES = [(9, 37), (16, 37), (17, 37), (9, 1000), (16, 1000), (17, 1000)]  # (N, M)
EPS = 1e-6
SENTINEL = -12345.0625


@pytest.fixture(scope='module')
def stk():
    from source import _lib
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _lib.lib()
    return _lib


def _record(tag, dev, bound):
    """One measured deviation against its bound; the message names both."""
    dev = float(dev)
    assert dev < bound, (tag, dev, bound)


def _rel_dev(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a / b - 1.0))) if a.size else 0.0


def _partition(stk, N, size, rank):
    t0, t1 = ctypes.c_int32(), ctypes.c_int32()
    stk.check(stk.lib().stk_partition(N, size, rank, ctypes.byref(t0), ctypes.byref(t1), None, None))
    return t0.value, t1.value - t0.value


def _allreduce_fn(stk, comm):
    """The all-reduce callback a rank hands to the C loop: host doubles -> tensor ->
    ThreadComm.allreduce_tensor_ -> back."""
    def fn(ctx, values, n):
        try:
            a = np.ctypeslib.as_array(values, shape=(n,))
            t = torch.from_numpy(a.copy())
            comm.allreduce_tensor_(t)
            a[:] = t.numpy()
            return 0
        except Exception:  # never let an exception cross the C frame
            return 1
    return stk.ALLREDUCE_FN(fn)


class _Slab:
    """One rank's slab (M rows of ld doubles, time fastest, padding zero) and the device
    arrays its C loop hands to the operator callbacks, known by their raw pointers."""

    def __init__(self, stk, M, N, t_begin, n_loc, ld=None):
        self.stk, self.M, self.N, self.t_begin, self.n_loc = stk, M, N, t_begin, n_loc
        self.ld = n_loc + (n_loc & 1) if ld is None else ld
        self.n = M * self.ld
        self.known = {}

    def vec(self, glob=None):
        """A device slab holding this rank's columns of the (M, N) array `glob`."""
        v = torch.zeros((self.M, self.ld), dtype=torch.float64, device='cuda')
        if glob is not None:
            v[:, :self.n_loc] = torch.from_numpy(
                np.ascontiguousarray(glob[:, self.t_begin:self.t_begin + self.n_loc])).cuda()
        return self.register(v)

    def register(self, v):
        self.known[v.data_ptr()] = v
        return v

    def work(self, size, fill=0.0, tail=0):
        """`size` device doubles (+ `tail` sentinels); the four vectors of the loop are
        its first 4 n doubles."""
        w = torch.full((size + tail,), fill, dtype=torch.float64, device='cuda')
        if tail:
            w[size:] = SENTINEL
        for k in range(4):
            if (k + 1) * self.n <= size:
                self.register(w[k * self.n:(k + 1) * self.n].view(self.M, self.ld))
        return w

    def op(self, f):
        """OPERATOR_FN applying f to the first n_loc columns; padding written as zero."""
        def fn(ctx, stream, x_ptr, y_ptr):
            try:
                x, y = self.known[x_ptr], self.known[y_ptr]
                out = torch.zeros_like(y)
                out[:, :self.n_loc] = f(x[:, :self.n_loc], self.t_begin)
                y.copy_(out)
                return 0
            except Exception:  # never let an exception cross the C frame
                return 1
        return self.stk.OPERATOR_FN(fn)

    def local(self, v):
        return v[:, :self.n_loc].cpu().numpy()


# ---- the explicit operators, in torch (slabs) and NumPy (the whole (M, N) array) ------
def _c_of(N):
    return 1.0 + 0.37 * np.arange(N)


def _K(x):
    y = 3.0 * x
    y[1:] -= x[:-1]
    y[:-1] -= x[1:]
    return y


def _T_dev(c):
    cd = torch.from_numpy(c).cuda()
    return lambda x, t0: _K(x) * cd[t0:t0 + x.shape[1]]


def _P_dev(c):
    pd = torch.from_numpy(1.0 / (3.0 * c)).cuda()
    return lambda x, t0: x * pd[t0:t0 + x.shape[1]]


def _T_np(c):
    return lambda X: _K(X) * c


def _P_np(c):
    p = 1.0 / (3.0 * c)
    return lambda X: X * p


def _rhs(N, M, seed=5):
    return np.random.RandomState(seed + 7 * N + M).rand(M, N) - 0.5


def _pcg_slab(stk, comm, N, M, B, kmax=200, ld_pad=0, work_fill=0.0, tail=64, w0=None):
    """stk_pcg_solve_slab of T w = B on this rank's slab; returns what it computed."""
    lib = stk.lib()
    t0, n_loc = _partition(stk, N, comm.Get_size(), comm.Get_rank())
    s = _Slab(stk, M, N, t0, n_loc, ld=n_loc + (n_loc & 1) + ld_pad)
    c = _c_of(N)
    b, w = s.vec(B), s.vec(w0)
    size = lib.stk_pcg_slab_work_size(M, n_loc, s.ld, N)
    work = s.work(size, work_fill, tail)
    hist = (ctypes.c_double * (kmax + 1))(*([SENTINEL] * (kmax + 1)))
    its = ctypes.c_int32(-1)
    T, P, ar = s.op(_T_dev(c)), s.op(_P_dev(c)), _allreduce_fn(stk, comm)
    stk.check(lib.stk_pcg_solve_slab(stk.stream(), M, n_loc, s.ld, N, t0, T, None, P, None, ar, None,
                                     stk.ptr(b), stk.ptr(w), EPS, kmax, stk.ptr(work), hist,
                                     ctypes.byref(its)))
    torch.cuda.synchronize()
    return dict(its=its.value, hist=np.array(hist[:]), w=s.local(w),
                pad=float(w[:, n_loc:].abs().max()) if s.ld > n_loc else 0.0,
                tail=work[size:].cpu().numpy(), finite=bool(torch.isfinite(w).all()))


def _gather(results, key='w'):
    return np.concatenate([r[key] for r in results], axis=1)


# ---- 1. known answers on the explicit operators -----------------------------------------
@pytest.fixture(scope='module')
def pcg_runs(stk):
    return {(N, M, size): run_ranks(size, lambda comm: _pcg_slab(stk, comm, N, M, _rhs(N, M)), timeout=120.0)
            for N, M in SHAPES for size in RANKS}


def test_pcg_slab_matches_numpy_pcg(stk, pcg_runs):
    """One slab against oracle.krylov.pcg (float64 NumPy) on the same T, P, eps and kmax:
    equal iteration counts, every r.Pr within 1e-13 relative (the operators round as their
    NumPy twins do, so only the inner products differ; measured 4.2e-15 over the six
    shapes), and the returned iterate meets
    the stopping rule when r.Pr is recomputed in NumPy from it (to 1e-6 relative: the
    recursive residual the loop stops on is not the true one)."""
    from oracle.krylov import pcg
    worst = 0.0
    for N, M in SHAPES:
        c, B = _c_of(N), _rhs(N, M)
        got = pcg_runs[(N, M, 1)][0]
        w_ref, its_ref, hist_ref = pcg(_T_np(c), _P_np(c), B.copy(), kmax=200, eps=EPS)
        assert got['its'] == its_ref > 5, (N, M, got['its'], its_ref)
        h = got['hist']
        assert np.all(h[its_ref + 1:] == SENTINEL), (N, M)  # history: its + 1 entries
        worst = max(worst, _rel_dev(h[:its_ref + 1], hist_ref))
        r = B - _T_np(c)(got['w'])
        rpr = float(np.vdot(r, _P_np(c)(r)))
        assert rpr < EPS * EPS * (1 + 1e-6), (N, M, rpr)
        assert np.linalg.norm(got['w'] - w_ref) < 1e-10 * np.linalg.norm(w_ref), (N, M)
    _record('pcg_slab_vs_numpy_history', worst, 1e-13)


def test_pcg_slab_is_independent_of_the_partition(stk, pcg_runs):
    """History, iteration count and gathered iterate on 2, 3, 4 and 8 ranks (odd slabs
    with ld = n_loc + 1 among them) are array_equal to the one-slab run."""
    for N, M in SHAPES:
        one = pcg_runs[(N, M, 1)][0]
        for size in RANKS[1:]:
            got = pcg_runs[(N, M, size)]
            tag = (N, M, size)
            assert all(r['its'] == one['its'] for r in got), tag
            assert all(np.array_equal(r['hist'], one['hist']) for r in got), tag
            assert np.array_equal(_gather(got), one['w']), tag


def test_pcg_slab_work_is_exactly_what_the_sizer_says(stk, pcg_runs):
    """A work array of exactly stk_pcg_slab_work_size doubles, filled with NaN, followed
    by sentinels: the loop writes everything it reads (the result is finite and equal to
    the clean run's), stays inside the size (the sentinels are untouched) and leaves the
    padding of w zero -- with the usual ld and with two more padding columns."""
    for N, M in [(9, 37), (17, 1000)]:
        for size in (1, 3, 8):
            for ld_pad in (0, 2):
                clean = pcg_runs[(N, M, size)]
                got = run_ranks(size, lambda comm: _pcg_slab(stk, comm, N, M, _rhs(N, M), ld_pad=ld_pad,
                                                             work_fill=float('nan'), tail=64), timeout=120.0)
                tag = (N, M, size, ld_pad)
                for r, c in zip(got, clean):
                    assert r['finite'] and r['its'] == c['its'], tag
                    assert np.array_equal(r['hist'], c['hist']), tag
                    assert np.all(r['tail'] == SENTINEL), tag
                    assert r['pad'] == 0.0, tag
                assert np.array_equal(_gather(got), _gather(clean)), tag


def _lanczos_slab(stk, comm, N, M, A, P, W, max_it=200, work_fill=0.0, tail=32):
    """stk_lanczos_slab on this rank's slab; A, P: torch functions of (x, t_begin)."""
    lib = stk.lib()
    t0, n_loc = _partition(stk, N, comm.Get_size(), comm.Get_rank())
    s = _Slab(stk, M, N, t0, n_loc)
    w = s.vec(W)
    size = lib.stk_lanczos_slab_work_size(M, n_loc, s.ld, N)
    work = s.work(size, work_fill, tail)
    alpha = (ctypes.c_double * (max_it + 1))(*([SENTINEL] * (max_it + 1)))
    beta = (ctypes.c_double * max_it)(*([SENTINEL] * max_it))
    lmax, lmin = ctypes.c_double(), ctypes.c_double()
    its, conv = ctypes.c_int32(-1), ctypes.c_int32(-1)
    A_cb, P_cb, ar = s.op(A), s.op(P), _allreduce_fn(stk, comm)
    stk.check(lib.stk_lanczos_slab(stk.stream(), M, n_loc, s.ld, N, t0, A_cb, None, P_cb, None, ar, None,
                                   stk.ptr(w), max_it, 1e-4, 1e-6, stk.ptr(work), alpha, beta,
                                   ctypes.byref(lmax), ctypes.byref(lmin), ctypes.byref(its),
                                   ctypes.byref(conv)))
    torch.cuda.synchronize()
    return dict(its=its.value, conv=conv.value, alpha=np.array(alpha[:]), beta=np.array(beta[:]),
                lmax=lmax.value, lmin=lmin.value, tail=work[size:].cpu().numpy())


def test_lanczos_slab_exact_breakdown(stk):
    """A = 2 I, P = I, a +-1 start vector and M N = 512: every step is exact in binary.
    The start vector spans an invariant subspace (beta_0 = 0): two iterations, alpha =
    [2, 2], beta_0 = 0, lmax = lmin = 2, converged -- on every rank count; nothing past
    iterations / iterations - 1 coefficients and nothing past the work size is written."""
    N, M = 16, 32
    W = np.where(np.random.RandomState(3).rand(M, N) < 0.5, -1.0, 1.0)
    two = lambda x, t0: 2.0 * x
    one = lambda x, t0: x.clone()
    for size in RANKS:
        got = run_ranks(size, lambda comm: _lanczos_slab(stk, comm, N, M, two, one, W, max_it=10,
                                                         work_fill=float('nan'), tail=32), timeout=120.0)
        for r in got:
            assert r['its'] == 2 and r['conv'] == 1, (size, r['its'], r['conv'])
            assert list(r['alpha'][:2]) == [2.0, 2.0] and r['beta'][0] == 0.0, (size, r['alpha'][:3])
            assert np.all(r['alpha'][2:] == SENTINEL) and np.all(r['beta'][1:] == SENTINEL), size
            assert r['lmax'] == r['lmin'] == 2.0, (size, r['lmax'], r['lmin'])
            assert np.all(r['tail'] == SENTINEL), size


def _diag(N, M):
    """Diagonal of A: M N distinct eigenvalues, geometrically spaced in [1, 10],
    scattered over space and time.  (A spread of 100 on the 333 unknowns of N = 9,
    M = 37 takes Lanczos, which does not re-orthogonalise, 92 steps, far into the loss
    of orthogonality: two float64 summation orders then disagree in the first digit of
    alpha.  At 10 it takes 47 steps and two orders agree to 1e-15.)"""
    d = np.geomspace(1.0, 10.0, M * N)
    return d[np.random.RandomState(17).permutation(M * N)].reshape(M, N)


def test_lanczos_slab_matches_numpy_lanczos(stk):
    """A diagonal with geometrically spaced eigenvalues, P = I, against
    oracle.krylov.Lanczos from the same start vector: equal iteration counts, alpha /
    beta / lmax / lmin within test_c_lanczos_matches_python_lanczos's bounds, both
    estimates inside the spectrum (up to the bisection tolerance), and everything
    array_equal across rank counts (the work array sized exactly and NaN-filled)."""
    from oracle.krylov import Lanczos
    for N, M in [(9, 37), (17, 1000)]:
        D = _diag(N, M)
        Dd = torch.from_numpy(D).cuda()
        A = lambda x, t0: x * Dd[:, t0:t0 + x.shape[1]]
        one = lambda x, t0: x.clone()
        W = np.random.RandomState(23).rand(M, N) - 0.5
        ref = Lanczos(lambda X: X * D, lambda X: X.copy(), W.copy())
        runs = {size: run_ranks(size, lambda comm: _lanczos_slab(stk, comm, N, M, A, one, W, work_fill=float('nan'),
                                                                 tail=32), timeout=120.0)
                for size in RANKS}
        got = runs[1][0]
        k = got['its'] - 1
        assert got['conv'] == 1 and ref.converged and got['its'] == ref.iterations > 5, (N, M, got['its'])
        assert np.allclose(got['alpha'][:k], ref.alpha, rtol=1e-8), (N, M)
        assert np.allclose(got['beta'][:k - 1], ref.beta, rtol=1e-7), (N, M)
        assert abs(got['lmax'] - ref.lmax) < 1e-8 * ref.lmax and abs(got['lmin'] - ref.lmin) < 1e-8 * ref.lmin
        assert D.min() * (1 - 1e-6) <= got['lmin'] <= got['lmax'] <= D.max() * (1 + 1e-6), (got['lmin'], got['lmax'])
        assert np.all(got['alpha'][k + 1:] == SENTINEL) and np.all(got['beta'][k:] == SENTINEL)
        for size, rs in runs.items():
            for r in rs:
                assert np.all(r['tail'] == SENTINEL), (N, M, size)
                for key in ('its', 'conv', 'lmax', 'lmin'):
                    assert r[key] == got[key], (N, M, size, key)
                assert np.array_equal(r['alpha'], got['alpha']) and np.array_equal(r['beta'], got['beta'])


def test_lanczos_slab_stops_unconverged_at_max_iterations(stk):
    """max_iterations = 3: converged = 0, iterations = 3, and alpha / beta receive exactly
    the 3 / 2 entries stk.h documents (host arrays one longer, ending in a sentinel)."""
    N, M = 9, 1000
    D = _diag(N, M)
    Dd = torch.from_numpy(D).cuda()
    A = lambda x, t0: x * Dd[:, t0:t0 + x.shape[1]]
    one = lambda x, t0: x.clone()
    W = np.random.RandomState(23).rand(M, N) - 0.5
    for size in (1, 4):
        got = run_ranks(size, lambda comm: _lanczos_slab(stk, comm, N, M, A, one, W, max_it=3), timeout=120.0)
        for r in got:
            assert r['its'] == 3 and r['conv'] == 0, (size, r['its'], r['conv'])
            assert np.all(np.isfinite(r['alpha'][:3])) and r['alpha'][3] == SENTINEL, r['alpha'][:4]
            assert np.all(r['beta'][:2] > 0) and r['beta'][2] == SENTINEL, r['beta'][:3]
            assert 0 < r['lmin'] <= r['lmax'] <= D.max() * (1 + 1e-6)


# ---- 2. the heat operators across thread ranks -----------------------------------------
HEAT_J_SPACE, HEAT_J_TIME = 6, 3
FLAT_RANKS = (1, 2, 4)
_SETUP = threading.Lock()  # plan construction reads process-wide tuning keys: one rank at a time


def _heat_ops(stk, dd, s, ops):
    from source.mpi_vector import KronVectorMPI

    def wrap(op):
        def fn(ctx, stream, x_ptr, y_ptr):
            try:
                s.known[y_ptr].copy_((op @ KronVectorMPI.around(dd, s.known[x_ptr])).buf)
                return 0
            except Exception:  # never let an exception cross the C frame
                return 1
        return stk.OPERATOR_FN(fn)
    return [wrap(op) for op in ops]


def _heat_rank(stk, comm, flat):
    import heateq_mpi as hm
    from source.lanczos import Lanczos
    from source.linalg import PCG
    from source.mpi_vector import KronVectorMPI
    lib = stk.lib()
    with _SETUP:
        h = hm.HeatEquationMPI(J_space=HEAT_J_SPACE, J_time=HEAT_J_TIME, problem='square', comm=comm,
                               wavelettransform='composite', precond='multigrid')
    dd = h.dofs_distr
    N, M, t0, n_loc = h.N, h.M, dd.t_begin, dd.t_end - dd.t_begin
    out = dict(N=N, M=M)
    hist_py = []
    w_py, out['py_its'] = PCG(h.WT_S_W, h.P, h.rhs, history=hist_py)
    out['py_hist'], out['py_w'] = np.asarray(hist_py), w_py.buf[:, :n_loc].cpu().numpy()
    del w_py

    kmax = 200
    s = _Slab(stk, M, N, t0, n_loc)
    assert s.ld == h.rhs.ld
    T, P = _heat_ops(stk, dd, s, (h.WT_S_W, h.P))
    ar = _allreduce_fn(stk, comm)
    b = s.register(h.rhs.buf)

    def solve(slab):
        w = s.vec()
        size = lib.stk_pcg_slab_work_size(M, n_loc, s.ld, N) if slab else lib.stk_pcg_work_size(s.n)
        work = s.work(size)
        hist = (ctypes.c_double * kmax)()
        its = ctypes.c_int32(-1)
        if slab:
            rc = lib.stk_pcg_solve_slab(stk.stream(), M, n_loc, s.ld, N, t0, T, None, P, None, ar, None,
                                        stk.ptr(b), stk.ptr(w), 1e-6, kmax, stk.ptr(work), hist, ctypes.byref(its))
        else:
            rc = lib.stk_pcg_solve(stk.stream(), s.n, T, None, P, None, ar, None, stk.ptr(b), stk.ptr(w),
                                   1e-6, kmax, stk.ptr(work), hist, ctypes.byref(its))
        stk.check(rc)
        return its.value, np.array(hist[:its.value + 1]), s.local(w)

    out['c_its'], out['c_hist'], out['c_w'] = solve(True)
    if flat:
        out['flat_its'], out['flat_hist'], _ = solve(False)

    # the Lanczos estimate from the bench's vector (heateq_mpi_timing.py:81-83)
    X = np.random.RandomState(128).rand(N, M)
    start = s.vec(X.T)
    max_it = 200
    work = s.work(lib.stk_lanczos_slab_work_size(M, n_loc, s.ld, N))
    alpha, beta = (ctypes.c_double * max_it)(), (ctypes.c_double * (max_it - 1))()
    lmax, lmin, its, conv = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32(), ctypes.c_int32()
    stk.check(lib.stk_lanczos_slab(stk.stream(), M, n_loc, s.ld, N, t0, T, None, P, None, ar, None,
                                   stk.ptr(start), max_it, Lanczos.TOL, Lanczos.TOLBISEC, stk.ptr(work), alpha,
                                   beta, ctypes.byref(lmax), ctypes.byref(lmin), ctypes.byref(its),
                                   ctypes.byref(conv)))
    out['lz'] = (its.value, conv.value, np.array(alpha[:]), np.array(beta[:]), lmax.value, lmin.value)
    if comm.Get_size() == 1:
        lz = Lanczos(h.WT_S_W, h.P, w=KronVectorMPI(dd, X[t0:t0 + n_loc]))
        out['py_lz'] = (lz.iterations, lz.converged, lz.alpha.copy(), lz.beta.copy(), lz.lmax, lz.lmin)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def heat_runs(stk):
    runs = {size: run_ranks(size, lambda comm: _heat_rank(stk, comm, size in FLAT_RANKS), timeout=600.0)
            for size in RANKS}
    torch.cuda.empty_cache()
    return runs


def test_heat_pcg_slab_on_thread_ranks(stk, heat_runs):
    """stk_pcg_solve_slab on WT_S_W / P / rhs of J_space = 6, J_time = 3 on 1, 2, 3, 4 and
    8 thread ranks: history, iterations and gathered iterate array_equal to the one-rank
    C run; the C loop against the Python PCG of the same ranks: equal iterations, history
    and iterate within 1e-11 (the scalars are combined by other axpby forms -- measured:
    bit-equal on every rank count, the same kernels rounding the same way); and the
    oracle's trajectory (tests/golden/o1_pcg_square_J3_J6) as tests/mp_parity_worker.py
    gates it (measured 7.1e-12 on the history, 2.5e-15 on the iterate sample)."""
    one = heat_runs[1][0]
    N, M = one['N'], one['M']
    assert (N, M) == (9, 16129)
    w1 = _gather(heat_runs[1], 'c_w')
    worst_h = worst_w = 0.0
    for size, got in heat_runs.items():
        w = _gather(got, 'c_w')
        for r in got:
            assert r['c_its'] == one['c_its'] and np.array_equal(r['c_hist'], one['c_hist']), size
        assert np.array_equal(w, w1), size
        w_py = _gather(got, 'py_w')
        r0 = got[0]
        assert r0['c_its'] == r0['py_its'], (size, r0['c_its'], r0['py_its'])
        worst_h = max(worst_h, _rel_dev(r0['c_hist'], r0['py_hist']))
        worst_w = max(worst_w, np.linalg.norm(w - w_py) / np.linalg.norm(w_py))
    _record('heat_c_slab_pcg_vs_python_pcg_history', worst_h, 1e-11)
    _record('heat_c_slab_pcg_vs_python_pcg_iterate', worst_w, 1e-11)
    g = load_golden('o1_pcg_square_J%d_J%d' % (HEAT_J_TIME, HEAT_J_SPACE))
    assert one['c_its'] == int(g['iters']), (one['c_its'], int(g['iters']))
    _record('heat_c_slab_pcg_vs_oracle_history', _rel_dev(one['c_hist'], g['hist']), 1e-10)
    st, sx = (int(v) for v in g['sample_strides'])
    W = w1.T  # (N, M), the oracle's orientation
    assert abs(np.linalg.norm(W) - g['w_norm']) < 1e-10 * g['w_norm']
    err = np.linalg.norm(W[::st, ::sx] - g['w_sample']) / np.linalg.norm(g['w_sample'])
    _record('heat_c_slab_pcg_vs_oracle_iterate_sample', err, 1e-10)


def test_heat_lanczos_slab_on_thread_ranks(stk, heat_runs):
    """stk_lanczos_slab from the bench vector: alpha, beta, lmax and lmin array_equal
    across rank counts, and within test_c_lanczos_matches_python_lanczos's bounds of
    source.lanczos.Lanczos."""
    its, conv, alpha, beta, lmax, lmin = heat_runs[1][0]['lz']
    for size, got in heat_runs.items():
        for r in got:
            i, c, a, b, hi, lo = r['lz']
            assert (i, c, hi, lo) == (its, conv, lmax, lmin), size
            assert np.array_equal(a, alpha) and np.array_equal(b, beta), size
    p_its, p_conv, p_alpha, p_beta, p_lmax, p_lmin = heat_runs[1][0]['py_lz']
    assert conv == 1 and p_conv and its == p_its > 3, (its, p_its)
    k = its - 1
    assert np.allclose(alpha[:k], p_alpha, rtol=1e-8)
    assert np.allclose(beta[:k - 1], p_beta, rtol=1e-7)
    assert abs(lmax - p_lmax) < 1e-8 * p_lmax and abs(lmin - p_lmin) < 1e-8 * p_lmin
    assert 0 < lmin < lmax


def test_heat_flat_pcg_with_a_real_allreduce(stk, heat_runs):
    """The flat stk_pcg_solve on 2 and 4 ranks, one scalar all-reduced per inner product:
    the same iteration count as one rank, the history within 3e-11 relative of it (not
    bit-equal: the rank partials are added in another order, see dot_shape in
    csrc/krylov.hip; measured 2.6e-12 on 2 ranks, 1.5e-11 on 4, largest on the last,
    smallest r.Pr); and on one rank the slab loop's history within 1e-11 (measured
    3.1e-12: stk_dot and stk_slab_dot sum in different shapes)."""
    one = heat_runs[1][0]
    _record('heat_flat_pcg_1_rank_vs_slab_history', _rel_dev(one['flat_hist'], one['c_hist']), 1e-11)
    for size in FLAT_RANKS[1:]:
        for r in heat_runs[size]:
            assert r['flat_its'] == one['flat_its'], (size, r['flat_its'], one['flat_its'])
            _record('heat_flat_pcg_%d_ranks_vs_1_rank_history' % size, _rel_dev(r['flat_hist'], one['flat_hist']),
                    3e-11)


# ---- 3. refusals, error reporting and early exits ----------------------------------------
class _One:
    """A one-rank call of the slab loops with every caller array pre-filled, so that what
    the loop wrote can be told from what it left."""

    def __init__(self, stk, N=9, M=37):
        self.stk, self.lib, self.N, self.M = stk, stk.lib(), N, M
        self.s = _Slab(stk, M, N, 0, N)
        self.c = _c_of(N)
        self.B = _rhs(N, M)
        self.W0 = np.random.RandomState(9).rand(M, N)
        self.b, self.w = self.s.vec(self.B), self.s.vec(self.W0)
        self.w_before = self.w.clone()
        size = max(self.lib.stk_pcg_slab_work_size(M, N, self.s.ld, N),
                   self.lib.stk_lanczos_slab_work_size(M, N, self.s.ld, N))
        self.work = self.s.work(size, fill=0.75)
        self.work_before = self.work.clone()
        self.hist = (ctypes.c_double * 8)(*([SENTINEL] * 8))
        self.alpha = (ctypes.c_double * 8)(*([SENTINEL] * 8))
        self.beta = (ctypes.c_double * 8)(*([SENTINEL] * 8))
        self.T, self.P = self.s.op(_T_dev(self.c)), self.s.op(_P_dev(self.c))
        self.none = stk.ALLREDUCE_FN()

    def pcg(self, M=None, n_loc=None, ld=None, N=None, t_begin=0, P=None, allreduce=None, b=None, kmax=8):
        its = ctypes.c_int32(-1)
        rc = self.lib.stk_pcg_solve_slab(
            self.stk.stream(), self.M if M is None else M, self.N if n_loc is None else n_loc,
            self.s.ld if ld is None else ld, self.N if N is None else N, t_begin, self.T, None,
            self.P if P is None else P, None, self.none if allreduce is None else allreduce, None,
            self.stk.ptr(self.b if b is None else b), self.stk.ptr(self.w), EPS, kmax, self.stk.ptr(self.work),
            self.hist, ctypes.byref(its))
        torch.cuda.synchronize()
        return rc, its.value

    def lanczos(self, M=None, n_loc=None, ld=None, N=None, t_begin=0, max_it=8, allreduce=None):
        lmax, lmin, its, conv = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32(-1), ctypes.c_int32(-1)
        rc = self.lib.stk_lanczos_slab(
            self.stk.stream(), self.M if M is None else M, self.N if n_loc is None else n_loc,
            self.s.ld if ld is None else ld, self.N if N is None else N, t_begin, self.T, None, self.P, None,
            self.none if allreduce is None else allreduce, None, self.stk.ptr(self.w), max_it, 1e-4, 1e-6,
            self.stk.ptr(self.work), self.alpha, self.beta, ctypes.byref(lmax), ctypes.byref(lmin),
            ctypes.byref(its), ctypes.byref(conv))
        torch.cuda.synchronize()
        return rc

    def error(self):
        return self.lib.stk_last_error().decode()

    def caller_arrays_untouched(self, work=True):
        untouched = (all(v == SENTINEL for v in self.hist) and all(v == SENTINEL for v in self.alpha)
                     and all(v == SENTINEL for v in self.beta) and torch.equal(self.w, self.w_before))
        return untouched and (not work or torch.equal(self.work, self.work_before))


def test_slab_loops_refuse_bad_shapes_and_touch_nothing(stk):
    """Odd ld, ld < n_loc, M = 0, t_begin + n_loc > N, max_iterations = 1 to Lanczos and
    kmax = 0 to PCG: non-zero, an error naming the cause, and history / coefficients / w / work as they
    were."""
    cases = [(dict(ld=9, n_loc=8), 'ld=9 must be even'),
             (dict(ld=8), 'ld=8 is smaller than n_loc=9'),
             (dict(M=0), 'M=0'),
             (dict(t_begin=1), 'time steps [1, 10) of 9')]
    for loop in ('pcg', 'lanczos'):
        for kw, cause in cases:
            one = _One(stk)
            rc = getattr(one, loop)(**kw)
            assert rc != 0 and cause in one.error(), (loop, kw, rc, one.error())
            assert ('stk_%s' % ('pcg_solve_slab' if loop == 'pcg' else 'lanczos_slab')) in one.error()
            assert one.caller_arrays_untouched(), (loop, kw)
    one = _One(stk)
    rc = one.lanczos(max_it=1)
    assert rc != 0 and 'max_iterations=1 too small' in one.error(), (rc, one.error())
    assert one.caller_arrays_untouched()
    one = _One(stk)
    rc, _ = one.pcg(kmax=0)  # history holds kmax entries: not even r.Pr of w0 fits
    assert rc != 0 and 'kmax=0 must be at least 1' in one.error(), (rc, one.error())
    assert one.caller_arrays_untouched()


def test_slab_loops_report_failing_callbacks(stk):
    """An all-reduce callback that returns 5 (PCG and Lanczos) and a failing P in PCG: the
    code comes back, the error names the callback, history / coefficients / w are as they
    were (work may have been used: the loop had started)."""
    five = stk.ALLREDUCE_FN(lambda ctx, values, n: 5)
    one = _One(stk)
    rc, _ = one.pcg(allreduce=five)
    assert rc == 5 and 'stk_pcg_solve: allreduce callback failed (5)' in one.error(), (rc, one.error())
    assert one.caller_arrays_untouched(work=False)
    one = _One(stk)
    rc = one.lanczos(allreduce=five)
    assert rc == 5 and 'stk_lanczos: allreduce callback failed (5)' in one.error(), (rc, one.error())
    assert one.caller_arrays_untouched(work=False)
    one = _One(stk)
    bad = stk.OPERATOR_FN(lambda ctx, stream, x, y: 3)
    rc, _ = one.pcg(P=bad)
    assert rc == 3 and 'operator P failed (3)' in one.error(), (rc, one.error())
    assert one.caller_arrays_untouched(work=False)


def test_pcg_slab_early_exits(stk):
    """b = 0: no iteration, nothing written.  w0 already the solution (b = T w0 through
    the same operator, so r = 0 exactly): no iteration, only history[0] (= 0) written, w
    unchanged.  kmax = 1 and kmax = 4: kmax - 1 iterations, kmax history entries, and
    the same trajectory as oracle.krylov.pcg with that kmax."""
    from oracle.krylov import pcg
    one = _One(stk)
    zero = one.s.vec()
    rc, its = one.pcg(b=zero)
    assert rc == 0 and its == 0 and one.caller_arrays_untouched(work=False)

    one = _One(stk)
    b = one.s.vec()
    b[:, :one.N] = _T_dev(one.c)(one.w[:, :one.N], 0)  # what the T callback computes
    rc, its = one.pcg(b=b)
    assert rc == 0 and its == 0, (rc, its)
    assert one.hist[0] == 0.0 and all(v == SENTINEL for v in one.hist[1:])
    assert torch.equal(one.w, one.w_before)

    for kmax in (1, 4):
        one = _One(stk)
        rc, its = one.pcg(kmax=kmax)
        w_ref, its_ref, hist_ref = pcg(_T_np(one.c), _P_np(one.c), one.B.copy(), w0=one.W0.copy(), kmax=kmax, eps=EPS)
        assert rc == 0 and its == its_ref == kmax - 1, (kmax, rc, its, its_ref)
        assert all(v == SENTINEL for v in one.hist[kmax:]), kmax
        assert _rel_dev(one.hist[:kmax], hist_ref) < 1e-13, kmax
        assert np.linalg.norm(one.s.local(one.w) - w_ref) < 1e-13 * np.linalg.norm(w_ref), kmax


# ---- 4. the device query -------------------------------------------------------------------
def test_device_info_matches_torch(stk):
    """stk_device_info: compute units, wave size and HBM bytes of the current device, as
    torch reports them."""
    n_cu, wave, hbm = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    stk.check(stk.lib().stk_device_info(ctypes.byref(n_cu), ctypes.byref(wave), ctypes.byref(hbm)))
    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    assert n_cu.value == props.multi_processor_count, (n_cu.value, props.multi_processor_count)
    assert wave.value == 64
    assert hbm.value == props.total_memory, (hbm.value, props.total_memory)
