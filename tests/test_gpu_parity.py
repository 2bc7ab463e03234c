"""Parity of the HIP path (through the C ABI, via the reference-shaped Python
classes) against golden vectors produced by the reference's own classes and
against the CPU oracle.  Needs an MI355X.

Tolerance: the north star asks for 1e-10 relative on residuals; single applies
are held to 1e-12 here (they differ from the reference only by the order of
floating-point additions), whole solves in the default arithmetic to 1e-10 on
every r.Pr entry and on the iterates, and to exact equality on iteration
counts; the opt-in arithmetic='fast' to 1e-9 per entry (it measures 4.6e-10)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import csr_from, load_golden, problem_from, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope='module')
def stk():
    from source import _lib
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _lib.lib()
    return _lib


def _vec(dd, X):
    from source.mpi_vector import KronVectorMPI
    return KronVectorMPI(dd, X)


def _np(v):
    return v.X_loc.cpu().numpy()


def _dd(N, M):
    from source.comm import Comm
    from source.mpi_vector import DofDistributionMPI
    return DofDistributionMPI(Comm(distributed=False), N, M)


def _hist_dev(tag, hist, ref, tol):
    """Largest relative deviation of a residual history from the reference's,
    entry by entry; asserted against `tol` and written to
    gpurun_out/parity_history_dev.json (the source of the bounds quoted in
    DESIGN.md section 5: every bound in this file is the north star's 1e-10 or,
    where the measured deviation is larger, about twice the measured one)."""
    import json
    import os
    hist, ref = np.asarray(hist, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert hist.shape == ref.shape, (tag, hist.shape, ref.shape)
    dev = float(np.max(np.abs(hist / ref - 1.0))) if len(ref) else 0.0
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    if os.path.isdir(out):
        path = os.path.join(out, 'parity_history_dev.json')
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[tag] = {'max_rel_dev': dev, 'entries': int(len(ref)), 'asserted_bound': tol}
        json.dump(rec, open(path, 'w'), indent=1, sort_keys=True)
    assert dev < tol, (tag, dev, tol)
    return dev


class _combination_of_two_chains:
    """HeatEquationMPI built inside runs its preconditioner family on the combination ca (R A
    P) + cm (R M P) on every level -- rounds 1-5's default -- instead of handing the members'
    own Galerkin chains to the coarse end (round 6, MultiGridFamily(exact_coarse=True)): for
    tests that compare forms of one arithmetic with each other."""
    def __enter__(self):
        import heateq_mpi as hm
        self.hm, self.default = hm, dict(hm.HeatEquationMPI.ACCURATE)
        hm.HeatEquationMPI.ACCURATE = dict(self.default, member_coarse_matrices=False)

    def __exit__(self, *exc):
        self.hm.HeatEquationMPI.ACCURATE = self.default


def _scalar_dev(tag, dev, tol):
    """One measured deviation, recorded like _hist_dev's and then asserted."""
    import json
    import os
    dev = float(dev)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    if os.path.isdir(out):
        path = os.path.join(out, 'parity_history_dev.json')
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[tag] = {'max_rel_dev': dev, 'entries': 1, 'asserted_bound': tol}
        json.dump(rec, open(path, 'w'), indent=1, sort_keys=True)
    assert dev < tol, (tag, dev, tol)
    return dev


# ---------------------------------------------------------------------------
def test_blas1_and_dot(stk):
    rng = np.random.RandomState(0)
    for N, M in [(9, 49), (33, 1001), (65, 4099)]:
        dd = _dd(N, M)
        X, Y = rng.rand(N, M), rng.rand(N, M)
        x, y = _vec(dd, X), _vec(dd, Y)
        assert abs(x.dot(y) - np.vdot(X, Y)) < 1e-12 * np.vdot(X, Y)
        assert x.dot(y) == x.dot(y)  # deterministic reduction
        z = x + 3.14 * y
        assert relerr(_np(z), X + 3.14 * Y) < 1e-15
        z = x - y
        assert relerr(_np(z), X - Y) < 1e-15
        x += 2.0 * y
        X = X + 2.0 * Y
        assert relerr(_np(x), X) < 1e-15
        x -= 0.5 * y
        X = X - 0.5 * Y
        x *= 1.5
        X = X * 1.5
        x /= 3.0
        X = X / 3.0
        assert relerr(_np(x), X) < 1e-15
        # PCG's direction update in one pass: bit for bit the two steps of the reference
        # (linalg.py:39-40), which NumPy performs with the same two roundings
        p1, p2, zz = x.copy(), x.copy(), _vec(dd, Y)
        p1 *= 0.37
        p1 += zz
        p2.scale_add(0.37, zz)
        assert torch.equal(p1.buf, p2.buf)
        assert np.array_equal(_np(p2), _np(x) * 0.37 + Y)
        w = y / 7.0
        assert relerr(_np(w), Y / 7.0) < 1e-15
        w = -y
        assert relerr(_np(w), -Y) < 1e-15
        # lazily scaled vectors must see the value from before a later mutation
        s = 2.0 * y
        y *= 10.0
        assert relerr(_np(s), 2.0 * Y) < 1e-15
        c = x.copy()
        c *= 0.0
        assert relerr(_np(x), X) < 1e-15


def test_kron_applies_match_reference_golden(stk, g3):
    from source.mpi_kron import (IdentityKronMatMPI, SparseKronIdentityMPI,
                                 SumMPI, TridiagKronIdentityMPI,
                                 TridiagKronMatMPI)
    m = problem_from(g3)
    N, M = int(g3['N']), int(g3['M'])
    dd = _dd(N, M)
    x = _vec(dd, g3['X'])
    LtT = sp.csr_matrix(m['L_t'].T)
    for nm, T, S in [('AtMx', m['A_t'], m['M_x']), ('MtAx', m['M_t'], m['A_x']),
                     ('LtAx', m['L_t'], m['A_x']), ('LtTMx', LtT, m['M_x']),
                     ('GtMx', m['G_t'], m['M_x'])]:
        y = TridiagKronMatMPI(dd, T, S) @ x
        assert relerr(_np(y), g3['kron_' + nm]) < TOL, nm
    op = SumMPI(dd, [
        TridiagKronMatMPI(dd, m['A_t'], m['M_x']),
        TridiagKronMatMPI(dd, m['M_t'], m['A_x'])
    ])
    assert relerr(_np(op @ x), g3['kron_metric']) < TOL
    # 5 fusable terms exercise the group-of-4 + accumulate path
    terms = [(m['A_t'], m['M_x']), (m['M_t'], m['A_x']), (m['L_t'], m['A_x']),
             (LtT, m['M_x']), (m['G_t'], m['M_x'])]
    op5 = SumMPI(dd, [TridiagKronMatMPI(dd, T, S) for T, S in terms])
    want = sum(g3['kron_' + k]
               for k in ('AtMx', 'MtAx', 'LtAx', 'LtTMx', 'GtMx'))
    assert relerr(_np(op5 @ x), want) < TOL
    assert relerr(_np(TridiagKronIdentityMPI(dd, m['A_t']) @ x),
                  g3['tridiag_At']) < TOL
    assert relerr(_np(IdentityKronMatMPI(dd, m['M_x']) @ x),
                  g3['ident_Mx']) < TOL
    assert relerr(_np(SparseKronIdentityMPI(dd, m['A_t']) @ x),
                  g3['sparse_At']) < TOL
    assert relerr(
        _np(SparseKronIdentityMPI(dd, m['A_t'], add_identity=True) @ x),
        g3['sparse_At_plusI']) < TOL
    from source.linop import KronLinOp
    assert relerr(KronLinOp(m['A_t'], m['M_x']) @ g3['X'].reshape(-1),
                  g3['kronlinop_AtMx']) < TOL


def test_kron_known_answer_dense(stk):
    """The reference's own unit test data (mpi_kron_test.py:58-66, 112-128):
    literal tridiagonal time matrix, arange space matrices, dense np.kron."""
    from source.mpi_kron import SumMPI, TridiagKronMatMPI
    mat = np.array([[3.5, 13., 28.5, 50., 77.5], [-5., -23., -53., -95., -149.],
                    [2.5, 11., 25.5, 46., 72.5]])
    T = sp.spdiags(mat, (1, 0, -1), 5, 5).T.copy().tocsr()
    M = 3
    S1 = np.arange(0, M * M).reshape(M, M) * 1.0
    S2 = np.arange(M * M, 2 * M * M).reshape(M, M) * 1.0
    dd = _dd(5, M)
    op = SumMPI(dd, [TridiagKronMatMPI(dd, T, S1), TridiagKronMatMPI(dd, T, S2)])
    assert np.allclose(op.as_global_matrix(), np.kron(T.toarray(), S1 + S2))


def test_wavelets_match_reference_golden(stk, g3):
    from source.mpi_kron import as_matrix
    from source.wavelets import (TransposedWaveletTransformKronIdentityMPI,
                                 WaveletTransformKronIdentityMPI,
                                 WaveletTransformOp)
    N, M, J = int(g3['N']), int(g3['M']), int(g3['J_time'])
    dd = _dd(N, M)
    x = _vec(dd, g3['X'])
    W = WaveletTransformKronIdentityMPI(dd, J)
    WT = TransposedWaveletTransformKronIdentityMPI(dd, J)
    assert np.array_equal(W.levels, g3['levels'])
    assert relerr(_np(W @ x), g3['W']) < TOL
    assert relerr(_np(WT @ x), g3['WT']) < TOL
    # without the one-rank call the operators take the all-to-all form (mode 'transpose', what
    # runs across ranks) and give the same; the per-level composite (mode 'composite') is
    # held to its own bound in test_wavelet_kernels_gpu.py
    W._fused = WT._fused = None
    assert relerr(_np(W @ x), g3['W']) < TOL
    assert relerr(_np(WT @ x), g3['WT']) < TOL


def test_wavelet_op_matrices(stk):
    from source.mpi_kron import as_matrix
    from source.wavelets import WaveletTransformOp
    g = load_golden('g1_wavelets')
    for J in range(1, 6):
        for inter, tag in ((True, 'il'), (False, 'lv')):
            op = WaveletTransformOp(J, interleaved=inter)
            key = 'J%d_%s' % (J, tag)
            assert np.allclose(as_matrix(op), g['W_' + key], rtol=0, atol=1e-14)
            assert np.allclose(as_matrix(op.T), g['WT_' + key], rtol=0,
                               atol=1e-14)
            assert np.array_equal(np.asarray(op.levels), g['levels_' + key])
    # all of this test runs the generic LDS kernel: WaveletTransformOp passes ld = N, and the
    # register kernel wants ld = N + 1 (its own tests: test_wavelet_kernels_gpu.py)
    from oracle import wavelets as ow
    for J in (6, 7, 8):
        op = WaveletTransformOp(J, interleaved=True)
        X = np.random.RandomState(5).rand(2**J + 1, 64 + 37)
        assert relerr(op @ X, ow.apply(J, X)) < TOL
        assert relerr(op.T @ X, ow.apply_transposed(J, X)) < TOL


def test_smoother_classes_as_the_reference_tests_them(stk):
    """source.multigrid.Smoother / PETScSMoother (reference multigrid.py:83-127): the
    reference's own test (multigrid_test.py:40-58: 150 forward resp. backward sweeps
    from zero reach A^-1 y) for both classes, and single calls against the oracle's
    sweep in dof order -- nonzero initial guess, 1-3 sweeps per call, NumPy vectors,
    (n, k) arrays and device slabs, on the square (M = 49 and 16 129) and the L-shape.
    The sweeps are the sequential sweep's arithmetic row by row, with fused
    multiply-adds where NumPy / SciPy round twice: 1e-14 per call, not bits."""
    from oracle.multigrid import Smoother as OracleSmoother
    from source.assembly import space_matrices
    from source.multigrid import PETScSMoother, Smoother
    from source.problem import problem_helper
    g = load_golden('g3_square')
    A = csr_from(g, 'A_x')
    rng = np.random.RandomState(3)
    x = rng.rand(A.shape[1])
    y = A @ x
    for smoother in [Smoother(A), PETScSMoother(A, 1)]:
        x_pre = np.zeros(A.shape[1])
        x_post = np.zeros(A.shape[1])
        for _ in range(150):
            smoother.PreSmooth(x_pre, y)
            smoother.PostSmooth(x_post, y)
        assert np.allclose(x_post, x)
        assert np.allclose(x_pre, x)
    mats = [A, csr_from(load_golden('g3_lshape'), 'A_x'),
            space_matrices(problem_helper('square', J_space=6, J_time=2)[0])[1]]
    for mat in mats:
        n = mat.shape[0]
        for its in (1, 3):
            oracle = OracleSmoother(mat, its=its)
            for cls in (Smoother, PETScSMoother):
                sm = cls(mat, its)
                for backward in (False, True):
                    call = lambda s_, u_, f_: (s_.PostSmooth if backward else s_.PreSmooth)(u_, f_)
                    u0, f = rng.rand(n), rng.rand(n)
                    want = u0.copy()
                    call(oracle, want, f)
                    got = u0.copy()
                    call(sm, got, f)
                    assert relerr(got, want) < 1e-14, (n, its, cls.__name__, backward)
                    # five right-hand sides at once: NumPy (n, 5) and a device slab (n, 6)
                    U0, F = rng.rand(n, 5), rng.rand(n, 5)
                    want = np.ascontiguousarray(U0.T)
                    call(oracle, want, np.ascontiguousarray(F.T))
                    got = U0.copy()
                    call(sm, got, F)
                    assert relerr(got, want.T) < 1e-14
                    ud = torch.zeros((n, 6), dtype=torch.float64, device='cuda')
                    fd = torch.zeros((n, 6), dtype=torch.float64, device='cuda')
                    ud[:, :5], fd[:, :5] = torch.from_numpy(U0).cuda(), torch.from_numpy(F).cuda()
                    call(sm, ud, fd)
                    assert relerr(ud[:, :5].cpu().numpy(), want.T) < 1e-14


def test_gauss_seidel_and_multigrid_match_reference_golden(stk, g3):
    from oracle.multigrid import Smoother
    from source.multigrid import MeshHierarchy, MultiGrid, MultiGridFamily
    m = problem_from(g3)
    b = g3['mg_b']
    hier = MeshHierarchy(P_mats=m['P_mats'])
    M = len(b)
    rng = np.random.RandomState(7)
    # smoother alone, 5 time slices at once, nonzero initial guess
    mg = MultiGrid(m['A_x'], hier, smoothsteps=3, vcycles=2)
    # 5 slices: odd leading dimension -> flat CSR kernels; 6: ELL row engine
    for nsl in (5, 6):
        F, U0 = rng.rand(nsl, M), rng.rand(nsl, M)
        for backward in (False, True):
            ref = U0.copy()
            sm = Smoother(m['A_x'], its=2)
            (sm.PostSmooth if backward else sm.PreSmooth)(ref, F)
            u = stk.to_dev(np.ascontiguousarray(U0.T))
            f = stk.to_dev(np.ascontiguousarray(F.T))
            mg.smooth(hier.J, u, f, its=2, backward=backward)
            assert relerr(u.cpu().numpy().T, ref) < TOL
    for ss in (1, 3):
        for vc in (1, 2):
            mg = MultiGrid(m['A_x'], hier, smoothsteps=ss, vcycles=vc)
            assert relerr(mg @ b, g3['mg_Ax_s%d_v%d' % (ss, vc)]) < 1e-11
            # the reference's own entry point and its counters (multigrid.py:184-197)
            before = mg.num_applies
            assert np.array_equal(mg._matvec(b), mg @ b)
            assert mg.num_applies == before + 2 and mg.time_per_apply() > 0
    fam = MultiGridFamily(m['A_x'], m['M_x'], hier, ca=0.3,
                          cms=[2**j for j in range(4)], smoothsteps=3,
                          vcycles=2)
    assert relerr(fam.members[2] @ b, g3['mg_C2_s3_v2']) < 1e-11


@pytest.mark.parametrize('schur', ['reference', 'fused'])
def test_heat_operators_and_solve_match_reference_golden(stk, g3, schur):
    import heateq_mpi as hm
    from source.lanczos import Lanczos
    from source.linalg import PCG
    from source.mpi_kron import (BlockDiagMPI, CompositeMPI, IdentityMPI,
                                 SumMPI, TridiagKronMatMPI)
    from source.linop import CompositeLinOp
    from source.multigrid import MeshHierarchy, MultiGrid, MultiGridFamily
    from source.wavelets import (TransposedWaveletTransformKronIdentityMPI,
                                 WaveletTransformKronIdentityMPI)
    m = problem_from(g3)
    N, M, J = int(g3['N']), int(g3['M']), int(g3['J_time'])
    dd = _dd(N, M)
    hier = MeshHierarchy(P_mats=m['P_mats'])
    K = MultiGrid(m['A_x'], hier, smoothsteps=3, vcycles=2)
    fam = MultiGridFamily(m['A_x'], m['M_x'], hier, ca=0.3,
                          cms=[2**j for j in range(J + 1)], smoothsteps=3,
                          vcycles=2)
    W = WaveletTransformKronIdentityMPI(dd, J)
    WT = TransposedWaveletTransformKronIdentityMPI(dd, J)
    M_x, A_x = m['M_x'], m['A_x']
    if schur == 'reference':
        S = SumMPI(dd, [
            TridiagKronMatMPI(dd, m['A_t'], CompositeLinOp([M_x, K, M_x])),
            TridiagKronMatMPI(dd, m['L_t'], CompositeLinOp([M_x, K, A_x])),
            TridiagKronMatMPI(dd, sp.csr_matrix(m['L_t'].T),
                              CompositeLinOp([A_x, K, M_x])),
            TridiagKronMatMPI(dd, m['M_t'], CompositeLinOp([A_x, K, A_x])),
            TridiagKronMatMPI(dd, m['G_t'], M_x),
        ])
    else:
        S = hm.SchurMPI(dd, m['A_t'], m['L_t'], m['M_t'], m['G_t'], M_x, A_x, K)
    CAC = [CompositeLinOp([c, A_x, c]) for c in fam.members]
    P = BlockDiagMPI(dd, [CAC[j] for j in W.levels])
    assert P._batched is not None and P._batched[0] == 'family'
    WT_S_W = CompositeMPI(dd, [WT, S, W])
    x = _vec(dd, g3['X'])
    assert relerr(_np(S @ x), g3['S_multigrid']) < 1e-11
    assert relerr(_np(P @ x), g3['P_multigrid']) < 1e-11
    assert relerr(_np(WT_S_W @ x), g3['WTSW_multigrid']) < 1e-11
    # the general (slice by slice) block-diagonal path agrees with the batched
    Pg = BlockDiagMPI(dd, [CAC[j] for j in W.levels])
    Pg._batched = None
    assert relerr(_np(Pg @ x), g3['P_multigrid']) < 1e-11

    rhs = _vec(dd, g3['rhs'])
    rr = []
    w, iters = PCG(WT_S_W, P, rhs, callback=lambda w, r, k: rr.append(r.dot(r)))
    assert iters == int(g3['pcg_iters_multigrid'])
    _hist_dev('golden_%d_%d_%s_rr' % (N, M, schur), rr, g3['pcg_rr_multigrid'], 1e-10)
    assert relerr(_np(w), g3['pcg_w_multigrid']) < 1e-10
    tag = 'golden_%d_%d_%s' % (N, M, schur)
    # 60 unconverged steps of plain CG amplify the last bits of one S apply
    # (the oracle itself sits 7.5e-9 from the reference on g3_square3): held to
    # ten times what the GPU measures (5.8e-9; profiles/r06_parity_history_dev.json),
    # the Lanczos coefficients (2.8e-14) and Ritz values (1.3e-15) likewise
    w2, it2 = PCG(S, IdentityMPI(dd), rhs, kmax=60)
    assert it2 == int(g3['pcg_unprec_iters_multigrid'])
    _scalar_dev(tag + '_unprec_w', relerr(_np(w2), g3['pcg_unprec_w_multigrid']), 6e-8)

    lz = Lanczos(WT_S_W, P, w=_vec(dd, g3['X']))
    assert lz.iterations == int(g3['lz_its_multigrid'])
    _scalar_dev(tag + '_lz_lmax', abs(lz.lmax / g3['lz_lmax_multigrid'] - 1.0), 1e-13)
    _scalar_dev(tag + '_lz_lmin', abs(lz.lmin / g3['lz_lmin_multigrid'] - 1.0), 1e-13)
    assert len(lz.alpha) == len(g3['lz_alpha_multigrid'])
    _hist_dev(tag + '_lz_alpha', lz.alpha, g3['lz_alpha_multigrid'], 1e-12)


@pytest.mark.parametrize('problem,J_space', [('square', 4), ('lshape', 3),
                                             ('cube', 2)])
def test_driver_end_to_end_against_oracle(stk, problem, J_space):
    """heateq_mpi.HeatEquationMPI (build-owned assembly) versus the CPU oracle
    on the same matrices: J_time = 4 (N = 17); square M = 961, lshape M = 705,
    cube M = 343 (15-point mass matrix: the K = 16 ELL width, 8 Gauss-Seidel
    dependency levels)."""
    import heateq_mpi as hm
    from oracle.heat import HeatEquationOracle
    from oracle.krylov import pcg
    from source.linalg import PCG
    h = hm.HeatEquationMPI(J_space=J_space, J_time=4, problem=problem)
    mats = dict(A_t=h.A_t, L_t=h.L_t, M_t=h.M_t, G_t=h.G_t, M_x=h.M_x,
                A_x=h.A_x, P_mats=h.hierarchy.P_mats, u0_t=h.u0_t, u0_x=h.u0_x)
    o = HeatEquationOracle(mats, 4)
    assert relerr(_np(h.rhs), o.rhs()) < 1e-14
    X = np.random.RandomState(128).rand(h.N, h.M)
    x = _vec(h.dofs_distr, X)
    assert relerr(_np(h.S @ x), o.S(X)) < 1e-11
    assert relerr(_np(h.P @ x), o.P(X)) < 1e-11
    hist_o = []
    wo, it_o, hist_o = pcg(o.WT_S_W, o.P, o.rhs())
    hist = []
    w, it = PCG(h.WT_S_W, h.P, h.rhs, history=hist)
    assert it == it_o
    _hist_dev('driver_%s_J%d' % (problem, J_space), hist, hist_o, 1e-10)
    assert relerr(_np(w), wo) < 1e-10


def test_full_size_properties(stk):
    """At bench-like sizes the oracle is too slow; check size-independent
    properties instead: linearity, symmetry of S and P, W^T adjoint of W."""
    import heateq_mpi as hm
    h = hm.HeatEquationMPI(J_space=6, J_time=5)  # N = 33, M = 16129
    dd = h.dofs_distr
    rng = np.random.RandomState(1)
    x, y = _vec(dd, rng.rand(h.N, h.M)), _vec(dd, rng.rand(h.N, h.M))
    for op in (h.S, h.P, h.W, h.WT, h.WT_S_W):
        lhs = op @ (x + 3.14 * y)
        rhs = (op @ x) + 3.14 * (op @ y)
        assert relerr(_np(lhs), _np(rhs)) < 1e-11
    for op in (h.S, h.P, h.WT_S_W):
        a, b = (op @ x).dot(y), x.dot(op @ y)
        assert abs(a - b) < 1e-10 * abs(a)
    a, b = (h.W @ x).dot(y), x.dot(h.WT @ y)
    assert abs(a - b) < 1e-12 * abs(a)
    assert (h.S @ x).dot(x) > 0 and (h.P @ x).dot(x) > 0


def test_abi_refusals_are_reported(stk):
    lib = stk.lib()
    rc = lib.stk_csr_spmm(None, 10, 5, 3, None, None, None, 0.0, None, None, None,
                          1.0, 0.0, None, None)  # ld < n_loc
    assert rc != 0 and b'bad sizes' in lib.stk_last_error()
    rc = lib.stk_wavelet_apply(None, 10, 3, 4, 0, None, None)
    assert rc != 0 and b'ld' in lib.stk_last_error()
    with pytest.raises(stk.StkError):
        stk.ptr(torch.zeros(3, dtype=torch.float64))  # host tensor refused


def test_row_orders_and_ell_workgroups_do_not_change_results(stk):
    """Tile order (assembly hint), reverse Cuthill-McKee (anonymous matrix);
    every persistent-workgroup count of the sliced-ELL kernel: same Kronecker
    apply."""
    import scipy.sparse as sp
    from oracle import kron as okron
    from source.assembly import space_matrices, time_matrices
    from source.mesh import construct_2d_lshape_mesh, construct_interval
    from source.mpi_kron import SumMPI, TridiagKronMatMPI
    mesh, _ = construct_2d_lshape_mesh(5)  # M = 12033 (> RCM threshold)
    M_x, A_x = space_matrices(mesh)
    A_t, L_t, M_t, G_t, _ = time_matrices(construct_interval(2**3))
    N, M = A_t.shape[0], M_x.shape[0]
    assert M > 8192
    dd = _dd(N, M)
    X = np.random.RandomState(3).rand(N, M)
    x = _vec(dd, X)
    want = okron.sum_apply([(A_t, M_x), (M_t, A_x), (L_t, A_x)], X)
    plain = lambda m: sp.csr_matrix(m)  # drops the stk_row_order hint
    try:
        for mk in (lambda m: m, plain):
            for wg in (0, 1, 3):
                stk.check(stk.lib().stk_set_tuning(b'ell_wg_per_cu', wg))
                op = SumMPI(dd, [TridiagKronMatMPI(dd, A_t, mk(M_x)),
                                 TridiagKronMatMPI(dd, M_t, mk(A_x)),
                                 TridiagKronMatMPI(dd, L_t, mk(A_x))])
                assert (op._groups[0].row_ids is not None)
                assert relerr(_np(op @ x), want) < TOL
    finally:
        stk.check(stk.lib().stk_set_tuning(b'ell_wg_per_cu', 0))
    with pytest.raises(stk.StkError):
        stk.check(stk.lib().stk_set_tuning(b'nonsense', 1))


def test_ell_overflow_rows_and_ragged_matrix(stk):
    """Rows longer than the 16 ELL slots spill into the overflow CSR; empty
    rows and a dense row must come out right (ragged input)."""
    import scipy.sparse as sp
    from oracle import kron as okron
    from source.mpi_kron import SumMPI, TridiagKronMatMPI
    rng = np.random.RandomState(11)
    M, N = 300, 9
    S = sp.random(M, M, density=0.02, random_state=rng, format='lil')
    S[5, :] = rng.rand(M)          # dense row -> overflow
    S[17, :40] = rng.rand(40)      # 40 entries -> overflow
    S[100, :] = 0.0                # empty row
    S = sp.csr_matrix(S)
    S.eliminate_zeros()
    S2 = sp.csr_matrix(S.multiply(S > 0.5))
    T = sp.diags([rng.rand(N - 1), rng.rand(N), rng.rand(N - 1)], [-1, 0, 1],
                 format='csr')
    dd = _dd(N, M)
    X = rng.rand(N, M)
    op = SumMPI(dd, [TridiagKronMatMPI(dd, T, S), TridiagKronMatMPI(dd, T.T.tocsr(), S2)])
    assert op._groups[0].ell.ovf_indptr is not None
    want = okron.sum_apply([(T, S), (T.T.tocsr(), S2)], X)
    assert relerr(_np(op @ _vec(dd, X)), want) < TOL


def test_direct_preconditioner_matches_reference_golden(stk, g3):
    """precond='direct' (reference heateq_mpi.py:154-157; its tests
    heateq_mpi_test.py:66-135 use it): InvLinOp blocks, reference-shaped S."""
    from source.linalg import PCG
    from source.linop import CompositeLinOp, InvLinOp
    from source.mpi_kron import (BlockDiagMPI, CompositeMPI, SumMPI,
                                 TridiagKronMatMPI)
    from source.wavelets import (TransposedWaveletTransformKronIdentityMPI,
                                 WaveletTransformKronIdentityMPI)
    m = problem_from(g3)
    N, M, J = int(g3['N']), int(g3['M']), int(g3['J_time'])
    dd = _dd(N, M)
    M_x, A_x = m['M_x'], m['A_x']
    K = InvLinOp(A_x)
    C_j = [InvLinOp(2**j * M_x + 0.3 * A_x) for j in range(J + 1)]
    S = SumMPI(dd, [
        TridiagKronMatMPI(dd, m['A_t'], CompositeLinOp([M_x, K, M_x])),
        TridiagKronMatMPI(dd, m['L_t'], CompositeLinOp([M_x, K, A_x])),
        TridiagKronMatMPI(dd, sp.csr_matrix(m['L_t'].T),
                          CompositeLinOp([A_x, K, M_x])),
        TridiagKronMatMPI(dd, m['M_t'], CompositeLinOp([A_x, K, A_x])),
        TridiagKronMatMPI(dd, m['G_t'], M_x),
    ])
    W = WaveletTransformKronIdentityMPI(dd, J)
    WT = TransposedWaveletTransformKronIdentityMPI(dd, J)
    CAC = [CompositeLinOp([c, A_x, c]) for c in C_j]
    P = BlockDiagMPI(dd, [CAC[j] for j in W.levels])
    WT_S_W = CompositeMPI(dd, [WT, S, W])
    x = _vec(dd, g3['X'])
    assert relerr(_np(S @ x), g3['S_direct']) < 1e-10
    assert relerr(_np(P @ x), g3['P_direct']) < 1e-10
    assert relerr(_np(WT_S_W @ x), g3['WTSW_direct']) < 1e-10
    rr = []
    w, iters = PCG(WT_S_W, P, _vec(dd, g3['rhs']),
                   callback=lambda w, r, k: rr.append(r.dot(r)))
    assert iters == int(g3['pcg_iters_direct'])
    _hist_dev('golden_%d_%d_direct_rr' % (N, M), rr, g3['pcg_rr_direct'], 1e-10)
    assert relerr(_np(w), g3['pcg_w_direct']) < 1e-10


def test_mat_kron_identity_and_original_wavelet_mode(stk):
    """MatKronIdentityMPI through the all-to-all transpose (reference
    mpi_kron_test.py:48-54, 96-109) and the drivers' wavelettransform modes."""
    import heateq_mpi as hm
    from source.mpi_kron import (CompositeMPI, IdentityKronMatMPI,
                                 MatKronIdentityMPI)
    N, M = 9, 16
    dd = _dd(N, M)
    mat_time = np.arange(0, N * N).reshape(N, N) * 1.0
    mat_space = np.arange(0, M * M).reshape(M, M) * 1.0
    X = np.random.RandomState(4).rand(N, M)
    x = _vec(dd, X)
    M_I = MatKronIdentityMPI(dd, mat_time)
    assert relerr(_np(M_I @ x), mat_time @ X) < TOL
    # one rank applies the dense factor to the time columns directly; the reference's
    # route -- transpose, I kron T on the transposed slab, transpose back -- must give
    # the same, also when a transposed "time" row (a rank's share of the space dofs) is
    # longer than the row engine's 1024 time steps (the sizes of the BASELINE configs)
    MatKronIdentityMPI.single_rank_shortcut = False
    try:
        assert relerr(_np(M_I @ x), mat_time @ X) < TOL
        for M_long in (1024, 1025, 2500):
            dl = _dd(N, M_long)
            Xl = np.random.RandomState(5).rand(N, M_long)
            assert relerr(_np(MatKronIdentityMPI(dl, mat_time) @ _vec(dl, Xl)), mat_time @ Xl) < TOL
    finally:
        MatKronIdentityMPI.single_rank_shortcut = True
    I_M = IdentityKronMatMPI(dd, mat_space)
    comp = CompositeMPI(dd, [I_M, M_I])
    want = (np.kron(mat_time, mat_space) @ X.reshape(-1)).reshape(N, M)
    assert relerr(_np(comp @ x), want) < TOL
    # vec.permute: (t, x) -> (x, t) (reference mpi_vector_test.py:31-48)
    vp, _ = x.permute()
    assert np.array_equal(_np(vp), X.T)
    # the three wavelet-transform modes of the drivers give the same solve
    ref = None
    for mode in ('composite', 'interleaved', 'original'):
        h = hm.HeatEquationMPI(J_space=2, J_time=3, wavelettransform=mode)
        xx = _vec(h.dofs_distr, np.random.RandomState(9).rand(h.N, h.M))
        if mode != 'original':  # interleaved numbering: same vectors
            got = _np(h.WT_S_W @ xx)
            ref = got if ref is None else ref
            assert relerr(got, ref) < 1e-11
        from source.linalg import PCG
        w, it = PCG(h.WT_S_W, h.P, h.rhs)
        u = _np(h.W @ w)  # solution in the hat-function basis: mode independent
        if mode == 'composite':
            u_ref, it_ref = u, it
        else:
            assert abs(it - it_ref) <= 1 and relerr(u, u_ref) < 1e-5


def test_reference_family_runs_the_default_arithmetic_too(stk):
    """HeatEquationMPI(family='reference') -- one hierarchy per wavelet level from the
    assembled 2^j M_x + alpha A_x, as reference heateq_mpi.py:147-153 builds them -- gets
    the plan options of arithmetic='accurate' like the batched family (it
    used to run a third, undocumented arithmetic): the r.Pr history of config 1 within
    1e-10 of the oracle's.  Unknown option strings are refused, not silently mapped."""
    import heateq_mpi as hm
    from source.linalg import PCG
    g = load_golden('o1_pcg_square_J3_J6')
    h = hm.HeatEquationMPI(J_space=int(g['J_space']), J_time=int(g['J_time']), family='reference')
    assert h.arithmetic == 'accurate' and h.C_family is None
    for mg in [h.Kinv_x] + h.C_j:
        assert mg._dev.options.get('fast_until_cycle') == 1 and mg._dev.options.get('fast_parts') == 1
    hist = []
    w, it = PCG(h.WT_S_W, h.P, h.rhs, history=hist)
    assert it == int(g['iters'])
    assert _record_history_dev('square_J3_J6_reference_family_accurate', hist, g['hist']) < HIST_RTOL_REFERENCE
    for bad in (dict(family='batch'), dict(schur='fuse')):
        with pytest.raises(AssertionError):
            hm.HeatEquationMPI(J_space=2, J_time=2, **bad)


def test_midsize_solve_matches_oracle_fixture(stk):
    """N = 33, M = 16 129: PCG iteration count and r.Pr history against the CPU
    oracle's trajectory (tests/golden/make_oracle_vectors.py)."""
    import heateq_mpi as hm
    from source.linalg import PCG
    g = load_golden('o1_pcg_square_J5_J6')
    h = hm.HeatEquationMPI(J_space=int(g['J_space']), J_time=int(g['J_time']))
    st, sx = (int(v) for v in g['sample_strides'])
    x = _vec(h.dofs_distr, _bench_vector(h.N, h.M))
    assert relerr(_np(h.S @ x)[::st, ::sx], g['SX_sample']) < 1e-11
    assert relerr(_np(h.P @ x)[::st, ::sx], g['PX_sample']) < 1e-11
    hist = []
    w, it = PCG(h.WT_S_W, h.P, h.rhs, history=hist)
    assert it == int(g['iters'])
    assert _record_history_dev('square_J5_J6', hist, g['hist']) < HIST_RTOL_REFERENCE  # the default arithmetic
    wn = _np(w)
    assert abs(np.linalg.norm(wn) - g['w_norm']) < 1e-10 * g['w_norm']
    assert relerr(wn[::st, ::sx], g['w_sample']) < 1e-10


def test_wide_slab_addressing_matches(stk):
    """Slabs of 4 GiB and more use 64-bit addressing inside the ELL kernels
    (stk_slab<true>).  Forced here on a small problem: S, P and the solve are
    the same as with the buffer-descriptor path."""
    import heateq_mpi as hm
    from source.linalg import PCG
    h = hm.HeatEquationMPI(J_space=3, J_time=3)
    X = np.random.RandomState(5).rand(h.N, h.M)
    x = _vec(h.dofs_distr, X)
    ref = [_np(h.S @ x), _np(h.P @ x)]
    hist0 = []
    w0, it0 = PCG(h.WT_S_W, h.P, h.rhs, history=hist0)
    try:
        for key in (b'ell_force_wide', b'rows_force_wide'):
            stk.check(stk.lib().stk_set_tuning(key, 1))
        assert relerr(_np(h.S @ x), ref[0]) < 1e-14
        assert relerr(_np(h.P @ x), ref[1]) < 1e-14
        hist = []
        w, it = PCG(h.WT_S_W, h.P, h.rhs, history=hist)
        assert it == it0 and np.allclose(hist, hist0, rtol=1e-10, atol=1e-30)
        assert relerr(_np(w), _np(w0)) < 1e-12
    finally:
        for key in (b'ell_force_wide', b'rows_force_wide'):
            stk.check(stk.lib().stk_set_tuning(key, 0))


def test_restricted_residual_in_one_pass_is_exact(stk):
    """(R A) u - R f in ONE pass of a two-matrix row kernel (csrc/rows_ell.hip,
    rows_ell2_kernel; tuning key mg_restrict_one_pass) against the two passes of the row
    engine it replaces -- d = R f, then d = (R A) u - d: the same sums and the same final
    fused multiply-add, so K^-1, S and P must not change by a bit; one matrix and the
    family's per-slice coefficients, slabs of 3 / 9 / 17 / 65 steps (lane, group and
    prefetch instances), 64-bit addressing forced."""
    import heateq_mpi as hm
    for J_time, J_space, wide in ((1, 5, 0), (3, 6, 0), (4, 5, 1), (6, 4, 0)):
        h = hm.HeatEquationMPI(J_space=J_space, J_time=J_time, arithmetic='fast')
        x = _vec(h.dofs_distr, np.random.RandomState(23).rand(h.N, h.M))
        res = []
        try:
            stk.check(stk.lib().stk_set_tuning(b'rows_force_wide', wide))
            for one_pass in (0, 2):  # 2: every plan (the default, 1, leaves K's plans on two passes)
                stk.check(stk.lib().stk_set_tuning(b'mg_restrict_one_pass', one_pass))
                res.append((_np(h.S @ x), _np(h.P @ x)))
        finally:
            stk.check(stk.lib().stk_set_tuning(b'mg_restrict_one_pass', 1))
            stk.check(stk.lib().stk_set_tuning(b'rows_force_wide', 0))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), (J_time, J_space)
        assert np.isfinite(res[1][1]).all()


def test_coarse_subcycle_variants_agree(stk):
    """The coarse end of the V-cycle runs level by level, as one job-list
    kernel on global workspaces, or as one kernel with all level vectors in LDS
    -- on the levels' own ELL copies, or on the uniform copies with the job
    descriptors in LDS and the next job's rows prefetched, 1024 or 512 threads
    per time step (csrc/mg_coarse.hip): same arithmetic in the same order,
    identical output.  The square at J_space = 6 gives a thread several rows of a
    job; the L-shape has rows of 9 entries (12 slots in the uniform form); the
    cube's rows are longer than the uniform form takes."""
    import heateq_mpi as hm
    outs = []
    for problem, J_space in (('square', 5), ('square', 6), ('lshape', 4), ('cube', 2)):
        # (the members' own coarse matrices of the default arithmetic are served by the
        # uniform form alone -- the other forms are A/B switches and run the combination
        # of the two chains: the forms are compared on the combination)
        with _combination_of_two_chains():
            h = hm.HeatEquationMPI(J_space=J_space, J_time=3, problem=problem)
        X = np.random.RandomState(11).rand(h.N, h.M)
        x = _vec(h.dofs_distr, X)
        res = []
        try:
            # the level-by-level path would otherwise form its restricted
            # residuals through R*A (test_restricted_residual_variants_agree),
            # which the job list does not: compare like with like
            stk.check(stk.lib().stk_set_tuning(b'mg_fuse_restrict', 0))
            for fuse, lds, uniform in ((0, 0, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1), (1, 1, 2)):
                stk.check(stk.lib().stk_set_tuning(b'mg_fuse_coarse', fuse))
                stk.check(stk.lib().stk_set_tuning(b'mg_coarse_lds', lds))
                stk.check(stk.lib().stk_set_tuning(b'mg_coarse_uniform', uniform))
                res.append((_np(h.P @ x), _np(h.S @ x)))
        finally:
            stk.check(stk.lib().stk_set_tuning(b'mg_fuse_coarse', 1))
            stk.check(stk.lib().stk_set_tuning(b'mg_coarse_lds', 1))
            stk.check(stk.lib().stk_set_tuning(b'mg_coarse_uniform', 1))
            stk.check(stk.lib().stk_set_tuning(b'mg_fuse_restrict', 1))
        for Pv, Sv in res[1:]:
            assert np.array_equal(Pv, res[0][0]) and np.array_equal(Sv, res[0][1])


# r.Pr histories against the oracle: the bound asserted below, and the measured
# deviations (written to gpurun_out/parity_history_dev.json when that directory
# exists, so that the figure quoted in DESIGN.md section 5 has a source).
# Measured (gpurun_out/parity_history_dev.json, round 2): iteration counts equal
# everywhere; every r.Pr within 5e-11 of the oracle's at J_time = 3 / J_space = 6,
# within 4.7e-10 at the sizes of configs 2-4.  The deviation starts at 1e-15 in the
# first iterations and roughly triples per iteration: CG turns last-bit
# differences (order of additions in dot products and in the regrouped Schur
# complement, the Gauss-Seidel update written as (f_i - sum_{j != i}) / a_ii like
# PETSc's MatSOR instead of u_i += (f_i - sum_j) / a_ii) into differences of alpha
# and beta.  1e-10 on the LAST entries,
# which are 1e-13 of the first, would need bit-identical arithmetic; what is
# asserted is 1e-9 on every entry relative to itself and 1e-10 relative to the
# initial residual.  The latter is set by the FIRST entry r0.P r0: 3e-13 at
# J_space = 6, 5e-12 at 8, 2e-11 at 9.  P applies multigrid to 2^j M + alpha A; the
# reference forms the Galerkin products of that assembled matrix, the family here
# stores R M P and R A P once and combines them per time slice (exactly the
# assembled entries on the finest level, one rounding apart on the coarse ones),
# and the conditioning of the level problems turns that ulp into 1e-11.
HIST_RTOL = 1e-9              # arithmetic='fast' (opt-in): twice the largest deviation measured (4.6e-10)
HIST_RTOL_REFERENCE = 1e-10   # arithmetic='reference' and 'accurate': the north star's bound, per entry
HIST_RTOL_VS_INITIAL = 1e-10


def _record_history_dev(tag, hist, ref):
    import json
    import os
    hist, ref = np.asarray(hist), np.asarray(ref)
    dev = float(np.max(np.abs(hist / ref - 1.0)))
    dev0 = float(np.max(np.abs(hist - ref)) / ref[0])
    assert dev0 < HIST_RTOL_VS_INITIAL, (tag, dev0)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       'gpurun_out')
    if os.path.isdir(out):
        path = os.path.join(out, 'parity_history_dev.json')
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[tag] = {'max_rel_dev_r_dot_Pr': dev, 'iterations': len(hist) - 1,
                    'max_dev_relative_to_initial': dev0,
                    'first_three_rel_dev': [float(v) for v in np.abs(hist / ref - 1.0)[:3]]}
        json.dump(rec, open(path, 'w'), indent=1, sort_keys=True)
    print('history deviation %s: %.2e' % (tag, dev))
    return dev


def _bench_vector(N, M):
    """The bench's input (bench.seeded_slab): the reference's timing vector,
    np.random.seed(128); rand(N, M) (heateq_mpi_timing.py:81-83)."""
    return np.random.RandomState(128).rand(N, M)


def _solve_against_fixture(problem, J_space, J_time, arithmetic):
    import heateq_mpi as hm
    from source.linalg import PCG
    g = load_golden('o1_pcg_%s_J%d_J%d' % (problem, J_time, J_space))
    h = hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem=problem,
                           arithmetic=arithmetic)
    st, sx = (int(v) for v in g['sample_strides'])
    x = _vec(h.dofs_distr, _bench_vector(h.N, h.M))
    assert relerr(_np(h.W @ x)[::st, ::sx], g['WX_sample']) < 1e-13
    assert relerr(_np(h.S @ x)[::st, ::sx], g['SX_sample']) < 1e-10
    assert relerr(_np(h.P @ x)[::st, ::sx], g['PX_sample']) < 1e-10
    del x
    hist = []
    w, it = PCG(h.WT_S_W, h.P, h.rhs, history=hist)
    assert it == int(g['iters']), (it, int(g['iters']))
    tag = '%s_J%d_J%d' % (problem, J_time, J_space) + ('' if arithmetic == 'fast' else '_%s_arithmetic' % arithmetic)
    dev = _record_history_dev(tag, hist, g['hist'])
    assert dev < (HIST_RTOL if arithmetic == 'fast' else HIST_RTOL_REFERENCE), dev
    wn = _np(w)
    assert abs(np.linalg.norm(wn) - g['w_norm']) < 1e-10 * g['w_norm']
    assert relerr(wn[::st, ::sx], g['w_sample']) < (1e-9 if arithmetic == 'fast' else 1e-10)
    return h


@pytest.mark.parametrize('arithmetic', ['fast', 'accurate', 'reference'])
@pytest.mark.parametrize('problem,J_space,J_time', [('square', 6, 3),
                                                    ('square', 8, 5),
                                                    ('square', 9, 6),
                                                    ('lshape', 8, 5)])
def test_baseline_configs_solve_matches_oracle_trajectory(stk, problem, J_space, J_time, arithmetic):
    """BASELINE.json configs 1-4 at full size, the whole solve as the
    reference's integration test compares it (heateq_mpi_test.py:138-189):
    iteration count EQUAL to the CPU oracle's, every r.Pr of the history within
    the bound, the solution on the fixture's sample, plus S, P and W applied
    to the bench's vector on the same sample.  The oracle trajectories are
    fixtures (tests/golden/make_oracle_vectors.py; config 3 takes 11 minutes on
    6 host threads).

    arithmetic='reference' (every regrouping of the build switched off:
    five-term S, one hierarchy per wavelet level from the assembled matrix,
    Gauss-Seidel rows with their diagonal, restricted residual as R (A u - f))
    is held to the north star's 1e-10 on EVERY entry; measured 7e-12 .. 2.1e-11
    (profiles/r03_history_attribution.json).  arithmetic='accurate' switches back
    only the two regroupings that own the gap (Gauss-Seidel rows with their
    diagonal, restricted residual as R (A u - f)) and keeps the fast structure:
    the same 1e-10 on every entry, measured 2.1e-11 .. 5.0e-11
    (profiles/r03_history_attribution_c.json), for 15 % of the solve time.  The
    fast default is held to 1e-9 per entry = twice what it measures (4.6e-10),
    and to 1e-10 relative to the initial residual; DESIGN.md section 5 attributes
    the difference."""
    _solve_against_fixture(problem, J_space, J_time, arithmetic)


@pytest.mark.parametrize('arithmetic', ['fast', 'accurate', 'reference'])
@pytest.mark.parametrize('problem,J_space,J_time', [('cube', 4, 4), ('lshape_jitter', 6, 5)])
def test_second_problem_and_irregular_values_solve_matches_oracle_trajectory(stk, problem, J_space, J_time,
                                                                             arithmetic):
    """The whole solve (reference heateq_mpi_test.py:138-189) on the reference's SECOND
    problem and on matrices whose values do not repeat, against oracle fixtures
    (tests/golden/make_oracle_vectors.py --problem ...): iteration count equal, every
    r.Pr within the bound, the iterate and S / P / W of the bench vector on the sample.
    `cube`, J_space = 4 (reference source/problem.py:21-41): M = 29 791, 15-point rows
    (K = 16 slots), 8 Gauss-Seidel dependency groups, the 15^3 level inside the fused
    coarse kernel, Galerkin products with rows beyond 32 entries.  `lshape_jitter`,
    J_space = 6: every interior vertex moved, so no two entries of M_x, A_x or of any
    Galerkin product repeat (BASELINE config 4's "irregular CSR"; the reference takes
    any CSR, source/mpi_kron.py:135-150) -- S streams row pairs with explicit values,
    its last stage the plain sliced-ELL form, and the family's Gauss-Seidel copies
    carry irregular values through every level."""
    h = _solve_against_fixture(problem, J_space, J_time, arithmetic)
    if problem == 'lshape_jitter' and arithmetic != 'reference':  # (the reference mode runs the five-term S)
        pk = h.S.ell.packed_for(h.rhs.n_loc)
        assert pk.ok and pk.explicit  # the solve above did stream explicit-value pairs



@pytest.mark.parametrize('problem,J_space,J_time', [('square', 9, 6),
                                                    ('lshape', 8, 5),
                                                    ('square', 10, 7)])
def test_baseline_configs_full_size_against_oracle(stk, problem, J_space, J_time):
    """BASELINE.json configs 3, 4 and 5 at their full size (config 5: N = 129,
    M = 4 190 209, a 4.3 GB vector -- slabs of 4 GiB and more, 64-bit addressing
    in every ELL kernel).  The Kronecker metric operator and W / W^T are compared
    with the oracle on the WHOLE vector; S and P, whose oracle needs seconds
    per time slice, on sampled time slices (space operators act slice by slice,
    so (S x)[t] only needs the rows t-1, t, t+1 of the time factors).  Config 5's
    whole solve is held to an oracle fixture too (below)."""
    import heateq_mpi as hm
    from oracle import kron as okron
    from oracle import wavelets as ow
    from oracle.multigrid import MultiGrid as OracleMG
    from source.linalg import PCG
    from source.mpi_kron import SumMPI, TridiagKronMatMPI
    h = hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem=problem)
    dd, N, M = h.dofs_distr, h.N, h.M
    X = np.random.RandomState(128).rand(N, M)
    x = _vec(dd, X)
    # the bench's operator, whole output
    op = SumMPI(dd, [TridiagKronMatMPI(dd, h.A_t, h.M_x),
                     TridiagKronMatMPI(dd, h.M_t, h.A_x)])
    assert relerr(_np(op @ x), okron.sum_apply([(h.A_t, h.M_x), (h.M_t, h.A_x)], X)) < 1e-13
    assert relerr(_np(h.W @ x), ow.apply(J_time, X)) < 1e-13
    assert relerr(_np(h.WT @ x), ow.apply_transposed(J_time, X)) < 1e-13
    # S and P on sampled time slices
    P_mats = h.hierarchy.P_mats
    levels = ow.levels(J_time, interleaved=True)
    sample = [0, N // 2 + 1]
    Sx = _np(h.S @ x)[sample]
    Px = _np(h.P @ x)[sample]
    K = OracleMG(h.A_x, P_mats, 3, 2)
    Mx, Ax = h.M_x, h.A_x
    want = np.zeros((len(sample), M))
    for T, ops in [(h.A_t, [Mx, K, Mx]), (h.L_t, [Mx, K, Ax]),
                   (sp.csr_matrix(h.L_t.T), [Ax, K, Mx]), (h.M_t, [Ax, K, Ax]),
                   (h.G_t, [Mx])]:  # heateq_mpi.py:166-181
        Z = sp.csr_matrix(T)[sample] @ X
        want += okron.composite_space(ops, Z.T).T
    assert relerr(Sx, want) < 1e-10
    for k, t in enumerate(sample):
        C = OracleMG(sp.csr_matrix(2.0**levels[t] * Mx + 0.3 * Ax), P_mats, 3, 2)
        assert relerr(Px[k], C @ (Ax @ (C @ X[t]))) < 1e-10
    del Sx, Px, X, x
    hist = []
    w, iters = PCG(h.WT_S_W, h.P, h.rhs, history=hist)
    assert 10 <= iters <= 16 and hist[-1] < 1e-12
    assert all(b < a for a, b in zip(hist, hist[1:]))
    if (problem, J_space, J_time) == ('square', 10, 7):
        # config 5's oracle fixture (tests/golden/make_oracle_vectors.py --lean on the
        # host: chunked S, in-place PCG, hours of CPU).  Round 5 ran it to convergence:
        # the WHOLE trajectory -- iteration count, every r.Pr, the final iterate -- as
        # the reference's integration test compares it (heateq_mpi_test.py:138-189),
        # the iterate after five iterations, and S, P, W of the bench's vector on the
        # fixture's sample.  (A fixture that stops at kmax holds the head only: rounds
        # 3-4.)
        g = load_golden('o1_pcg_square_J7_J10')
        st, sx = (int(v) for v in g['sample_strides'])
        head = len(g['hist'])
        whole = int(g['iters']) + 1 < int(g['kmax'])  # the oracle stopped on r.Pr < 1e-12
        assert head >= 6
        if whole:
            assert iters == int(g['iters']), (iters, int(g['iters']))
            _hist_dev('config5_whole_accurate', hist, g['hist'], 1e-10)  # the default arithmetic
            wn = _np(w)
            assert abs(np.linalg.norm(wn) - g['w_norm']) < 1e-10 * g['w_norm']
            assert relerr(wn[::st, ::sx], g['w_sample']) < 1e-10
            del wn
        else:
            assert head == int(g['kmax'])
            _hist_dev('config5_head_accurate', hist[:head], g['hist'], 1e-10)
        del w
        xb = _vec(dd, _bench_vector(N, M))
        assert relerr(_np(h.W @ xb)[::st, ::sx], g['WX_sample']) < 1e-13
        assert relerr(_np(h.S @ xb)[::st, ::sx], g['SX_sample']) < 1e-10
        assert relerr(_np(h.P @ xb)[::st, ::sx], g['PX_sample']) < 1e-10
        del xb, h
        torch.cuda.empty_cache()
        # the reference-arithmetic mode: 1e-10 per entry on the same trajectory, the
        # iterate after five iterations (where the fixture has it) and at the end
        h = hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem=problem, arithmetic='reference')
        if 'w5_sample' in g.files:
            hist = []
            w, iters = PCG(h.WT_S_W, h.P, h.rhs, kmax=6, history=hist)
            assert iters == 5
            _hist_dev('config5_head_reference_arithmetic', hist, g['hist'][:6], 1e-10)
            wn = _np(w)
            assert abs(np.linalg.norm(wn) - g['w5_norm']) < 1e-10 * g['w5_norm']
            assert relerr(wn[::st, ::sx], g['w5_sample']) < 1e-10
            del w, wn
        hist = []
        w, iters = PCG(h.WT_S_W, h.P, h.rhs, kmax=int(g['kmax']), history=hist)
        assert iters == int(g['iters'])
        _hist_dev('config5_%s_reference_arithmetic' % ('whole' if whole else 'head'), hist, g['hist'], 1e-10)
        wn = _np(w)
        assert abs(np.linalg.norm(wn) - g['w_norm']) < 1e-10 * g['w_norm']
        assert relerr(wn[::st, ::sx], g['w_sample']) < 1e-10


def test_serial_kron_linop_rectangular_and_operator_factors(stk):
    """KronLinOp (reference linop.py:6-15) with a rectangular sparse time
    factor, a dense one and a LinearOperator one, against numpy.kron."""
    from source.linop import KronLinOp
    from source.wavelets import WaveletTransformOp
    rng = np.random.RandomState(2)
    B = sp.random(23, 17, density=0.3, random_state=rng, format='csr')
    for A in (sp.random(6, 9, density=0.5, random_state=rng, format='csr'),
              rng.rand(9, 5), WaveletTransformOp(3), WaveletTransformOp(3).T):
        dense_A = A.toarray() if sp.issparse(A) else (
            A if isinstance(A, np.ndarray) else A @ np.eye(A.shape[1]))
        op = KronLinOp(A, B)
        x = rng.rand(op.shape[1])
        assert op.shape == (dense_A.shape[0] * 23, dense_A.shape[1] * 17)
        assert relerr(op @ x, np.kron(dense_A, B.toarray()) @ x) < 1e-13
    # BlockDiagLinOp (linop.py:29-44): repeated blocks are batched, mixed
    # block sizes take the block-by-block path
    from source.linop import BlockDiagLinOp
    C1 = sp.random(11, 11, density=0.4, random_state=rng, format='csr')
    C2 = sp.random(11, 11, density=0.4, random_state=rng, format='csr')
    C3 = sp.random(7, 7, density=0.5, random_state=rng, format='csr')
    for blocks in ([C1, C2, C1, C1], [C1, C3, C1]):
        op = BlockDiagLinOp(blocks)
        x = rng.rand(op.shape[1])
        assert relerr(op @ x, sp.block_diag(blocks) @ x) < 1e-14
    # BlockLinOp (linop.py:47-65): a 2 x 3 grid of rectangular blocks
    from source.linop import BlockLinOp
    grid = [[sp.random(5, 4, density=0.6, random_state=rng, format='csr'),
             sp.random(5, 7, density=0.6, random_state=rng, format='csr'),
             sp.random(5, 3, density=0.6, random_state=rng, format='csr')],
            [sp.random(8, 4, density=0.6, random_state=rng, format='csr'),
             sp.random(8, 7, density=0.6, random_state=rng, format='csr'),
             sp.random(8, 3, density=0.6, random_state=rng, format='csr')]]
    op = BlockLinOp(grid)
    x = rng.rand(op.shape[1])
    assert relerr(op @ x, sp.bmat(grid) @ x) < 1e-14


@pytest.mark.parametrize('precond', ['multigrid', 'direct'])
def test_serial_driver_against_oracle(stk, precond):
    """heateq.HeatEquation (the reference's serial wiring, heateq.py:18-107) on
    the device versus its CPU oracle, and versus the parallel driver's S."""
    import heateq as hs
    import heateq_mpi as hm
    from oracle.heat_serial import HeatSerialOracle
    from oracle.krylov import pcg
    from source.assembly import prolongation_matrices
    from source.linalg import PCG
    from source.mesh import construct_2d_square_mesh
    J_space, J_time = 3, 3
    h = hs.HeatEquation(J_space=J_space, J_time=J_time, precond=precond)
    mats = dict(h.time_mats, M_x=h.M_x, A_x=h.A_x, u0_x=h.u0_x,
                P_mats=prolongation_matrices(construct_2d_square_mesh(J_space)[0]))
    o = HeatSerialOracle(mats, J_time, precond=precond)
    x = np.random.RandomState(4).rand(h.N * h.M)
    assert relerr(h.B @ x, o.B(x)) < 1e-13
    assert relerr(h.S @ x, o.S(x)) < 1e-11
    assert relerr(h.P @ x, o.P(x)) < 1e-11
    assert relerr(h.WT_S_W @ x, o.WT_S_W(x)) < 1e-11
    assert relerr(h.f, o.f()) < 1e-15
    hist = []
    w, iters = PCG(h.WT_S_W, h.P, h.WT @ h.f, history=hist)
    wo, iters_o, hist_o = pcg(o.WT_S_W, o.P, o.WT(o.f()))
    assert iters == iters_o
    _hist_dev('serial_driver_%s' % precond, hist, hist_o, 1e-10)
    assert relerr(w, wo) < 1e-10
    # the parallel driver builds the same Schur complement from five terms
    hp = hm.HeatEquationMPI(J_space=J_space, J_time=J_time, precond=precond)
    xv = _vec(hp.dofs_distr, x.reshape(h.N, h.M))
    assert relerr(_np(hp.S @ xv).reshape(-1), h.S @ x) < 1e-11


@pytest.mark.parametrize('precond', ['multigrid', 'direct'])
def test_serial_operators_on_device_vectors(stk, precond):
    """The serial operators (reference linop.py:6-65, heateq.py:37-91) applied to device
    vectors: KronLinOp, sums and products of them, the Schur complement written as a
    function and BlockDiagLinOp map a one-rank KronVectorMPI to one -- the doubles of
    the flat-NumPy-vector path where the same kernels run (everything but the block
    diagonal, whose host path hands each block an (M, k) array of its own stride) --
    and HeatEquation.solve(), device-resident between one upload and one download,
    gives the iteration count and the history of the host-vector wiring within 1e-10
    of the oracle's."""
    import heateq as hs
    from oracle.heat_serial import HeatSerialOracle
    from oracle.krylov import pcg
    from source.assembly import prolongation_matrices
    from source.linalg import PCG
    from source.linop import DeviceLinearOperator, device_vector, host_vector
    from source.mesh import construct_2d_square_mesh
    from source.mpi_vector import KronVectorMPI
    J_space, J_time = 3, 3
    h = hs.HeatEquation(J_space=J_space, J_time=J_time, precond=precond)
    x = np.random.RandomState(5).rand(h.N * h.M)
    xd = device_vector(x, h.N)
    assert np.array_equal(host_vector(xd), x)
    for name in ('B', 'G', 'W', 'WT', 'S'):
        op = getattr(h, name)
        assert isinstance(op, DeviceLinearOperator), name
        yd = op @ xd
        assert isinstance(yd, KronVectorMPI) and yd.N * yd.M == op.shape[0], name
        assert np.array_equal(host_vector(yd), op @ x), name
    y = h.B @ x  # a vector of the test space: another number of time steps
    yd = device_vector(y, h.N_Y)
    assert np.array_equal(host_vector(h.K @ yd), h.K @ y)
    assert np.array_equal(host_vector(h.BT @ yd), h.BT @ y)
    for name in ('P', 'WT_S_W'):
        op = getattr(h, name)
        assert relerr(host_vector(op @ xd), op @ x) < 1e-12, name
    # mixed use keeps SciPy's rules: a product with a plain LinearOperator is one
    from scipy.sparse.linalg import LinearOperator, aslinearoperator
    import scipy.sparse as sp
    mixed = h.G @ aslinearoperator(sp.identity(h.N * h.M, format='csr'))
    assert isinstance(mixed, LinearOperator) and not isinstance(mixed, DeviceLinearOperator)
    assert relerr(mixed @ x, h.G @ x) < 1e-15
    # the solve
    seen = []
    u, iters = h.solve(callback=lambda w, r, k: seen.append(type(w)))
    u_host, iters_host = h.solve(on_host=True)
    assert iters == iters_host and seen and all(t is KronVectorMPI for t in seen)
    assert isinstance(u, np.ndarray) and relerr(u, u_host) < 1e-10
    hist = []
    PCG(h.WT_S_W, h.P, h.WT @ device_vector(h.f, h.N), history=hist)
    mats = dict(h.time_mats, M_x=h.M_x, A_x=h.A_x, u0_x=h.u0_x,
                P_mats=prolongation_matrices(construct_2d_square_mesh(J_space)[0]))
    o = HeatSerialOracle(mats, J_time, precond=precond)
    wo, iters_o, hist_o = pcg(o.WT_S_W, o.P, o.WT(o.f()))
    assert iters == iters_o
    _hist_dev('serial_driver_on_device_%s' % precond, hist, hist_o, 1e-10)
    assert relerr(u, o.W(wo)) < 1e-10
    e_alg, e_y = h.errors(u)  # device vectors inside; against the host-vector formulas
    residual, defect = h.f - h.S @ u, h.g_vec - h.B @ u
    assert abs(e_alg - residual @ (h.P @ residual)) <= 1e-9 * e_alg + 1e-24
    assert abs(e_y - defect @ (h.K @ defect)) <= 1e-12 * e_y


def test_c_pcg_solve_matches_python_pcg(stk):
    """stk_pcg_solve (C ABI, reference linalg.py:6-42) driven through ctypes
    callbacks into the same operators as the Python PCG: identical iteration
    count, r.Pr history and solution."""
    import ctypes
    import heateq_mpi as hm
    from source.linalg import PCG
    from source.mpi_vector import KronVectorMPI
    h = hm.HeatEquationMPI(J_space=3, J_time=3)
    dd = h.dofs_distr
    hist_py = []
    w_py, it_py = PCG(h.WT_S_W, h.P, h.rhs, history=hist_py)

    lib = stk.lib()
    n = h.rhs.buf.numel()
    work = torch.zeros(lib.stk_pcg_work_size(n), dtype=torch.float64, device='cuda')
    w = KronVectorMPI(dd)
    # the callbacks receive raw device pointers into `work`, b and w
    known = {}
    for k in range(4):
        view = work[k * n:(k + 1) * n].view(h.M, -1)
        known[view.data_ptr()] = view
    known[w.buf.data_ptr()] = w.buf
    known[h.rhs.buf.data_ptr()] = h.rhs.buf

    def wrap(op):
        def fn(ctx, stream, x_ptr, y_ptr):
            try:
                vin, vout = KronVectorMPI(dd), KronVectorMPI(dd)
                vin._buf = known[x_ptr]
                out = op @ vin
                known[y_ptr].copy_(out.buf)
                return 0
            except Exception:  # never let an exception cross the C frame
                return 1
        return stk.OPERATOR_FN(fn)

    T_cb, P_cb = wrap(h.WT_S_W), wrap(h.P)
    kmax = 100
    history = (ctypes.c_double * kmax)()
    iters = ctypes.c_int32()
    stk.check(lib.stk_pcg_solve(stk.stream(), n, T_cb, None, P_cb, None,
                                stk.ALLREDUCE_FN(), None, stk.ptr(h.rhs.buf),
                                stk.ptr(w.buf), 1e-6, kmax, stk.ptr(work),
                                history, ctypes.byref(iters)))
    assert iters.value == it_py
    # the same kernels driven from C instead of Python: the recurrences only differ
    # in where the scalars are combined
    _hist_dev('c_pcg_vs_python_pcg', list(history)[:it_py + 1], hist_py, 1e-11)
    assert relerr(_np(w), _np(w_py)) < 1e-11


def test_c_lanczos_matches_python_lanczos(stk):
    """stk_lanczos (C ABI, reference lanczos.py:87-159) driven through ctypes
    callbacks into the same operators as the Python Lanczos: identical iteration
    count, recurrence coefficients and eigenvalue brackets."""
    import ctypes
    import heateq_mpi as hm
    from source.lanczos import Lanczos
    from source.mpi_vector import KronVectorMPI
    h = hm.HeatEquationMPI(J_space=3, J_time=3)
    dd = h.dofs_distr
    rng = np.random.default_rng(11)
    start = KronVectorMPI(dd)
    start.buf[:, :start.n_loc] = torch.from_numpy(
        2.0 * rng.random((h.M, start.n_loc)) - 1.0).cuda()
    w_py = KronVectorMPI(dd)
    w_py.buf.copy_(start.buf)
    lz = Lanczos(h.WT_S_W, h.P, w=w_py)

    lib = stk.lib()
    n = start.buf.numel()
    work = torch.zeros(lib.stk_lanczos_work_size(n), dtype=torch.float64, device='cuda')
    known = {start.buf.data_ptr(): start.buf}
    for k in range(4):
        view = work[k * n:(k + 1) * n].view(h.M, -1)
        known[view.data_ptr()] = view

    def wrap(op):
        def fn(ctx, stream, x_ptr, y_ptr):
            try:
                vin = KronVectorMPI(dd)
                vin._buf = known[x_ptr]
                known[y_ptr].copy_((op @ vin).buf)
                return 0
            except Exception:  # never let an exception cross the C frame
                return 1
        return stk.OPERATOR_FN(fn)

    A_cb, P_cb = wrap(h.WT_S_W), wrap(h.P)
    kmax = 200
    alpha = (ctypes.c_double * kmax)()
    beta = (ctypes.c_double * (kmax - 1))()
    lmax, lmin = ctypes.c_double(), ctypes.c_double()
    its, conv = ctypes.c_int32(), ctypes.c_int32()
    stk.check(lib.stk_lanczos(stk.stream(), n, A_cb, None, P_cb, None,
                              stk.ALLREDUCE_FN(), None, stk.ptr(start.buf), kmax,
                              Lanczos.TOL, Lanczos.TOLBISEC, stk.ptr(work), alpha, beta,
                              ctypes.byref(lmax), ctypes.byref(lmin),
                              ctypes.byref(its), ctypes.byref(conv)))
    assert conv.value == 1 and lz.converged
    assert its.value == lz.iterations
    k = its.value - 1
    assert np.allclose(list(alpha)[:k], lz.alpha, rtol=1e-8)
    assert np.allclose(list(beta)[:k - 1], lz.beta, rtol=1e-7)
    assert abs(lmax.value - lz.lmax) < 1e-8 * lz.lmax
    assert abs(lmin.value - lz.lmin) < 1e-8 * lz.lmin
    # a failing callback is reported, not swallowed
    bad = stk.OPERATOR_FN(lambda ctx, stream, x, y: 7)
    rc = lib.stk_lanczos(stk.stream(), n, bad, None, P_cb, None, stk.ALLREDUCE_FN(),
                         None, stk.ptr(start.buf), kmax, 1e-4, 1e-6, stk.ptr(work),
                         None, None, ctypes.byref(lmax), ctypes.byref(lmin),
                         ctypes.byref(its), ctypes.byref(conv))
    assert rc == 7 and b'operator A failed' in lib.stk_last_error()


def test_c_abi_timing_counters(stk):
    """stk_timing_*: per-class call counts and device seconds of the apply entry
    points (the C-side counterpart of LinearOperatorMPI.num_applies /
    time_applies, reference mpi_kron.py:23-36), against what one S apply, one W
    apply and one dot are known to enqueue, and against the HIP-event time of the
    whole sequence."""
    import ctypes
    import heateq_mpi as hm
    lib = stk.lib()
    h = hm.HeatEquationMPI(J_space=4, J_time=4)
    x = h.rhs.copy()
    h.S @ x
    h.W @ x  # plans and workspaces exist now

    def read(name):
        calls, seconds = ctypes.c_int64(), ctypes.c_double()
        stk.check(lib.stk_timing_get(name.encode(), ctypes.byref(calls), ctypes.byref(seconds)))
        return calls.value, seconds.value

    try:
        # one stream: the sum of the classes' device times is then bounded by the
        # time of the whole sequence (S's two K applies overlap on two streams
        # otherwise, each timed on its own)
        hm.SchurMPI.two_streams = False
        stk.check(lib.stk_timing_enable(1))
        stk.check(lib.stk_timing_reset())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h.S @ x
        h.W @ x
        x.dot(x)
        e1.record()
        torch.cuda.synchronize()
        whole = e0.elapsed_time(e1) * 1e-3
        kron, wav, mg, blas = read('kron'), read('wavelet'), read('multigrid'), read('blas1')
        assert kron[0] == 3 and mg[0] == 2 and wav[0] == 1  # SchurMPI: 3 fused passes, 2 K applies
        assert blas[0] >= 1
        for calls, seconds in (kron, wav, mg, blas):
            assert 0.0 < seconds < whole
        assert mg[1] > kron[1] > 0.0  # two V-cycle applies outweigh three Kronecker passes
        assert kron[1] + wav[1] + mg[1] <= whole * 1.001
        stk.check(lib.stk_timing_reset())
        assert read('kron') == (0, 0.0)
        stk.check(lib.stk_timing_enable(0))
        h.W @ x
        assert read('wavelet') == (0, 0.0)  # disabled: nothing recorded
        assert lib.stk_timing_get(b'nonsense', None, None) != 0
        assert b'unknown class' in lib.stk_last_error()
    finally:
        lib.stk_timing_enable(0)
        hm.SchurMPI.two_streams = True


def test_restricted_residual_variants_agree(stk):
    """d = R (A u - f) in two steps, or as (R A) u - R f with the precomputed
    product R A (stk_mg_level.ell_ra): same V-cycle up to rounding."""
    import heateq_mpi as hm
    for problem, J_space in (('square', 5), ('lshape', 4)):
        # (arithmetic='fast': its plans follow the process-wide key; the default
        # arithmetic pins the two-step form per plan)
        h = hm.HeatEquationMPI(J_space=J_space, J_time=3, problem=problem, arithmetic='fast')
        x = _vec(h.dofs_distr, np.random.RandomState(12).rand(h.N, h.M))
        res = []
        try:
            for fuse in (0, 1):
                stk.check(stk.lib().stk_set_tuning(b'mg_fuse_restrict', fuse))
                res.append((_np(h.P @ x), _np(h.S @ x)))
        finally:
            stk.check(stk.lib().stk_set_tuning(b'mg_fuse_restrict', 1))
        assert relerr(res[1][0], res[0][0]) < 1e-13
        assert relerr(res[1][1], res[0][1]) < 1e-13
        assert not np.array_equal(res[1][0], res[0][0])  # the fused path did run
        # the per-level window of the fused form (what the default arithmetic uses to
        # keep the two-step form on the finest level only): an empty window is the
        # two-step form, the full one the fused form, bit for bit
        J = h.hierarchy.J
        plans = (h.Kinv_x._dev, h.C_family._dev)
        try:
            for lo, hi, same_as in ((0, -1, 0), (0, 1 << 30, 1), (0, J - 1, None)):
                for dev in plans:
                    dev.set_option('fuse_restrict_min_level', lo)
                    dev.set_option('fuse_restrict_max_level', hi)
                got = _np(h.P @ x)
                if same_as is not None:
                    assert np.array_equal(got, res[same_as][0]), (lo, hi)
                else:  # fused below the finest level only (at this size those levels run
                    # inside the fused coarse launch, which always takes the two steps)
                    assert relerr(got, res[0][0]) < 1e-13
                    assert not np.array_equal(got, res[1][0])
        finally:
            for dev in plans:
                dev.set_option('fuse_restrict_min_level', 0)
                dev.set_option('fuse_restrict_max_level', 1 << 30)
    # Gauss-Seidel row forms by level (multigrid.GS_DIAG_FREE_LEVELS): "no level
    # diagonal-free" is the plan GS_DIAG_FREE = False builds
    from source import multigrid as mgmod
    from source.assembly import space_matrices
    from source.multigrid import MeshHierarchy, MultiGrid
    from source.problem import problem_helper
    mesh = problem_helper('square', J_space=4, J_time=2)[0]
    A_x = space_matrices(mesh)[1]
    hier = MeshHierarchy(mesh)
    F = np.random.RandomState(3).rand(A_x.shape[0], 6)
    out = {}
    try:
        for name, flag, levels in (('free', True, None), ('full', False, None),
                                   ('none free', True, lambda j, Jf: False),
                                   ('free below the finest', True, lambda j, Jf: j < Jf)):
            mgmod.GS_DIAG_FREE, mgmod.GS_DIAG_FREE_LEVELS = flag, levels
            mg = MultiGrid(A_x, hier, smoothsteps=3, vcycles=2)
            out[name] = mg @ F
            # an odd number of columns takes the CSR kernels (mg.hip gs_group_kernel,
            # two-step restricted residual, no fused coarse launch): the same row form
            out[name + ', csr'] = mg @ F[:, :5]
            assert relerr(out[name + ', csr'], out[name][:, :5]) < 1e-13, name
    finally:
        mgmod.GS_DIAG_FREE, mgmod.GS_DIAG_FREE_LEVELS = True, None
    assert np.array_equal(out['none free'], out['full'])
    assert not np.array_equal(out['free'], out['full'])
    assert not np.array_equal(out['free below the finest'], out['full'])
    assert not np.array_equal(out['free below the finest'], out['free'])
    assert relerr(out['free below the finest'], out['full']) < 1e-13
    assert np.array_equal(out['none free, csr'], out['full, csr'])
    assert not np.array_equal(out['free, csr'], out['full, csr'])


def test_solve_is_reproducible_run_to_run(stk):
    """No kernel of the path uses atomics or an order that depends on scheduling
    (two-stage dot products, one writer per output element), S runs two V-cycle
    chains on two HIP streams and the set-up builds its plans in worker threads:
    two solves of two separately built operators give the same bits, and so do
    repeated applies."""
    import heateq_mpi as hm
    from source.linalg import PCG
    runs = []
    for rep in range(2):
        h = hm.HeatEquationMPI(J_space=6, J_time=4, problem='square')
        x = _vec(h.dofs_distr, np.random.RandomState(77).rand(h.N, h.M))
        applies = [(_np(h.S @ x), _np(h.P @ x), _np(h.WT_S_W @ x)) for _ in range(3)]
        for k in range(3):
            assert np.array_equal(applies[1][k], applies[0][k]) and np.array_equal(applies[2][k], applies[0][k])
        hist = []
        w, it = PCG(h.WT_S_W, h.P, h.rhs, history=hist)
        runs.append((it, np.asarray(hist), _np(w), applies[0]))
        del h
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][2], runs[1][2])
    for k in range(3):
        assert np.array_equal(runs[0][3][k], runs[1][3][k])


def test_reference_forms_only_where_the_gap_is_owned(stk):
    """The default arithmetic keeps the reference's forms for the last V-cycle's
    restricted residual and post-smoothing on the finest level (plan options
    fast_until_cycle / fast_parts, the alternative sweep copies of
    stk_mg_level.ell_fwd_alt / ell_bwd_alt).  With every V-cycle declared fast the
    plan reproduces arithmetic='fast' bit for bit; with none, the plan that has
    the reference's forms on the whole finest level; the default lies between."""
    import heateq_mpi as hm
    from source import multigrid as mgmod
    for problem, J_space in (('square', 6), ('lshape', 5)):
        fast = hm.HeatEquationMPI(J_space=J_space, J_time=3, problem=problem, arithmetic='fast')
        x = _vec(fast.dofs_distr, np.random.RandomState(21).rand(fast.N, fast.M))
        want_fast = (_np(fast.P @ x), _np(fast.S @ x))
        del fast
        # the reference's forms on the whole finest level, no alternative copies
        mgmod.GS_DIAG_FREE_LEVELS = lambda level, finest: level < finest
        try:
            whole = hm.HeatEquationMPI(J_space=J_space, J_time=3, problem=problem, arithmetic='fast')
        finally:
            mgmod.GS_DIAG_FREE_LEVELS = None
        for dev in (whole.Kinv_x._dev, whole.C_family._dev):
            dev.set_option('fuse_restrict_max_level', whole.hierarchy.J - 1)
        want_whole = (_np(whole.P @ x), _np(whole.S @ x))
        del whole
        with _combination_of_two_chains():  # (the fast arithmetic's coarse matrices)
            h = hm.HeatEquationMPI(J_space=J_space, J_time=3, problem=problem)  # arithmetic='accurate'
        plans = (h.Kinv_x._dev, h.C_family._dev)
        default = (_np(h.P @ x), _np(h.S @ x))

        def run(until, parts):
            for dev in plans:
                dev.set_option('fast_until_cycle', until)
                dev.set_option('fast_parts', parts)
            return _np(h.P @ x), _np(h.S @ x)

        all_fast, none_fast = run(2, 0), run(0, 0)
        for k in range(2):
            assert np.array_equal(all_fast[k], want_fast[k]), (problem, k)
            assert np.array_equal(none_fast[k], want_whole[k]), (problem, k)
            assert not np.array_equal(default[k], want_fast[k]) and not np.array_equal(default[k], want_whole[k])
            assert relerr(default[k], want_whole[k]) < 1e-13
        again = run(1, 1)  # the default's options
        assert np.array_equal(again[0], default[0]) and np.array_equal(again[1], default[1])


def _lib_dev(a):
    from source import _lib
    return _lib.to_dev(np.ascontiguousarray(a))


def test_kron_ell_randomised_shapes(stk):
    """stk_kron_ell_apply / stk_kron_ell_ghost_apply on random ragged matrices,
    slab lengths 1..21, one to three terms, with and without ghost rows, beta
    0 or not, identity time factors: against dense NumPy.  Walks through the
    K / NPF / overflow / wide-row instances of the kernel."""
    from source.linop import EllMatrices
    rng = np.random.RandomState(2024)
    for case in range(40):
        M = int(rng.randint(3, 400))
        n_loc = int(rng.randint(1, 22))
        ld = n_loc + (n_loc & 1)
        nt = int(rng.randint(1, 4))
        width = int(rng.choice([3, 6, 9, 14, 20]))  # 20 > 16: overflow rows
        dens = min(1.0, width / M)
        base = sp.random(M, M, density=dens, random_state=rng, format='csr')
        base = sp.csr_matrix(base + sp.eye(M))
        mats = []
        for k in range(nt):
            m = base.copy()
            m.data = rng.rand(m.nnz)
            mats.append(m)
        ell = EllMatrices(mats)
        shared = bool(rng.randint(2))
        xs = [rng.rand(M, n_loc) for _ in range(1 if shared else nt)]
        lo = rng.rand(M) if rng.randint(2) else None
        hi = rng.rand(M) if rng.randint(2) else None
        beta = float(rng.choice([0.0, 0.5]))
        y0 = rng.rand(M, n_loc)
        specs, want = [], beta * y0
        for k in range(nt):
            X = xs[0] if shared else xs[k]
            if rng.randint(4) == 0:
                tri, T = None, np.eye(n_loc)
                sub0 = sup1 = 0.0
            else:
                t = rng.rand(3, n_loc)
                T = np.diag(t[1]) + np.diag(t[0, 1:], -1) + np.diag(t[2, :-1], 1)
                tri, sub0, sup1 = _lib_dev(t), t[0, 0], t[2, -1]
            Z = mats[k] @ X  # (M, n_loc): space factor on every time column
            want = want + Z @ T.T
            if tri is not None and lo is not None:
                want[:, 0] += sub0 * (mats[k] @ lo)
            if tri is not None and hi is not None:
                want[:, -1] += sup1 * (mats[k] @ hi)
            specs.append((tri, k, X, lo, hi))
        dev = {}

        def slab(a):
            key = id(a)
            if key not in dev:
                s_ = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
                s_[:, :n_loc] = torch.from_numpy(a).cuda()
                dev[key] = s_
            return dev[key]

        glo = None if lo is None else torch.from_numpy(lo).cuda()
        ghi = None if hi is None else torch.from_numpy(hi).cuda()
        dspecs = [(tri, k, slab(X), glo, ghi) for tri, k, X, _, _ in specs]
        y = slab(y0.copy())
        ell.apply(dspecs, n_loc, ld, beta, y)
        got = y[:, :n_loc].cpu().numpy()
        assert relerr(got, want) < 1e-13, (case, M, n_loc, nt, width, shared)
        if ld > n_loc:
            assert float(y[:, n_loc:].abs().max()) == 0.0  # padding stays zero


def test_kron_pack_randomised_shapes(stk):
    """stk_kron_pack_apply (packed slot stream, dictionary of value tuples,
    ghost time steps fused) on random matrices whose entries come from a small
    set of values: against dense NumPy, and bit for bit against the plain ELL
    form (stk_kron_ell_apply + stk_kron_ell_ghost_apply) on the same inputs.
    Slab lengths 1..40 walk through the lanes-per-row / rows-per-group / NPF
    instances; matrices with too many distinct values must be refused by the
    planner (it keeps the plain form)."""
    from source.linop import EllMatrices
    rng = np.random.RandomState(77)
    for case in range(40):
        M = int(rng.randint(3, 600))
        n_loc = int(rng.choice([1, 2, 3, 8, 9, 16, 17, 33, 40]))
        ld = n_loc + (n_loc & 1)
        nt = int(rng.randint(1, 4))
        width = int(rng.choice([3, 6, 9, 14]))
        base = sp.random(M, M, density=min(1.0, width / M), random_state=rng,
                         format='csr')
        base = sp.csr_matrix(base + sp.eye(M))
        palette = rng.randn(int(rng.randint(1, 9)))
        mats = []
        for k in range(nt):
            m = base.copy()
            m.data = palette[rng.randint(len(palette), size=m.nnz)]
            mats.append(m)
        ell = EllMatrices(mats)
        if ell.ovf_indptr is not None:
            assert not ell.packed.ok
            continue
        # codes: value tuples (+ "no entry"), per row of a unit when rows were paired
        assert ell.packed.ok
        assert ell.packed.n_codes <= (len(palette)**nt + 1)**ell.packed.rows_per_unit
        X = rng.rand(M, n_loc)
        lo = rng.rand(M) if rng.randint(2) else None
        hi = rng.rand(M) if rng.randint(2) else None
        beta = float(rng.choice([0.0, 0.5]))
        y0 = rng.rand(M, n_loc)
        want, tris = beta * y0, []
        for k in range(nt):
            if rng.randint(4) == 0:
                tri, T, sub0, sup1 = None, np.eye(n_loc), 0.0, 0.0
            else:
                t = rng.rand(3, n_loc)
                T = np.diag(t[1]) + np.diag(t[0, 1:], -1) + np.diag(t[2, :-1], 1)
                tri, sub0, sup1 = _lib_dev(t), t[0, 0], t[2, -1]
            want = want + (mats[k] @ X) @ T.T
            if tri is not None and lo is not None:
                want[:, 0] += sub0 * (mats[k] @ lo)
            if tri is not None and hi is not None:
                want[:, -1] += sup1 * (mats[k] @ hi)
            tris.append(tri)

        def slab(a):
            s_ = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
            s_[:, :n_loc] = torch.from_numpy(a).cuda()
            return s_

        x = slab(X)
        glo = None if lo is None else torch.from_numpy(lo).cuda()
        ghi = None if hi is None else torch.from_numpy(hi).cuda()
        gh = None
        if glo is not None or ghi is not None:
            gh = torch.empty((M, 2), dtype=torch.float64, device='cuda')
            stk.check(stk.lib().stk_interleave_ghosts(
                stk.stream(), M, stk.ptr(glo), stk.ptr(ghi), stk.ptr(gh)))
            z = torch.zeros(M, dtype=torch.float64, device='cuda')
            assert torch.equal(gh[:, 0], z if glo is None else glo)
            assert torch.equal(gh[:, 1], z if ghi is None else ghi)
        y = slab(y0)
        ell.packed.apply([(tris[k], k) for k in range(nt)], x, gh, n_loc, ld,
                         beta, y)
        got = y[:, :n_loc].cpu().numpy()
        assert relerr(got, want) < 1e-13, (case, M, n_loc, nt, width)
        if ld > n_loc:
            assert float(y[:, n_loc:].abs().max()) == 0.0  # padding stays zero
        y_plain = slab(y0)
        ell.apply([(tris[k], k, x, glo, ghi) for k in range(nt)], n_loc, ld,
                  beta, y_plain)
        # same arithmetic in the same order -- with ghost rows too: the plain form
        # recomputes its first and last step in a second kernel, in the main
        # kernel's order of operations (round 6; rounds 1-5 added a share: 1e-14)
        assert torch.equal(y, y_plain), (case, M, n_loc, nt)
    # too many distinct values: the planner keeps the plain form
    m = sp.random(300, 300, density=0.02, random_state=rng, format='csr')
    m = sp.csr_matrix(m + sp.eye(300))
    m.data = rng.rand(m.nnz)
    e = EllMatrices([m])
    assert e.ovf_indptr is not None or not e.packed.ok or e.packed.n_codes <= 512


def _blocks(N, size):
    """DofDistributionMPI's blocks (reference mpi_vector.py:17-34): N // size steps
    each, the remainder to the LAST ranks."""
    base, extra = divmod(N, size)
    out, start = [], 0
    for p in range(size):
        stop = start + base + (1 if p >= size - extra else 0)
        out.append((start, stop))
        start = stop
    return out


def test_slab_dot_does_not_depend_on_the_partition(stk):
    """stk_slab_dot: the per-time-step sums of a slab are the same doubles wherever
    the time axis is cut (the sum over the spatial index has one shape, a function of M
    alone), so KronVectorMPI.dot returns ONE value on 1, 2, 3, 4 or 8 ranks -- the
    reference's (and rounds 1-5's) slab-by-slab sum moves the history of a solve by
    4.6e-11 between 1 and 8 ranks.  Slab lengths 1 .. 300 walk through several row
    blocks per workgroup, several items per thread and two column ranges."""
    lib = stk.lib()
    rng = np.random.RandomState(5)

    def steps_of(Xs, Ys, N, t_begin):
        M, n_loc = Xs.shape
        ld = n_loc + (n_loc & 1)
        x = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
        y = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
        x[:, :n_loc], y[:, :n_loc] = torch.from_numpy(Xs).cuda(), torch.from_numpy(Ys).cuda()
        work = torch.empty(int(lib.stk_slab_dot_work_size(M, n_loc)), dtype=torch.float64, device='cuda')
        out = torch.full((N,), 7.0, dtype=torch.float64, device='cuda')  # the other steps must come out as zero
        stk.check(lib.stk_slab_dot(stk.stream(), M, n_loc, ld, stk.ptr(x), stk.ptr(y), stk.ptr(work), N, t_begin,
                                   stk.ptr(out)))
        return out.cpu().numpy()

    for M, N in [(1, 5), (7, 9), (255, 17), (256, 33), (257, 33), (1000, 65), (4099, 129), (70001, 9), (300, 300)]:
        X, Y = rng.randn(M, N), rng.randn(M, N)
        whole = steps_of(X, Y, N, 0)
        exact = np.einsum('it,it->t', X, Y)
        assert np.allclose(whole, exact, rtol=0, atol=1e-13 * np.abs(X * Y).sum(axis=0).max())
        for size in (2, 3, 4, 8):
            if size > N:
                continue
            total = np.zeros(N)
            for b, e in _blocks(N, size):
                part = steps_of(np.ascontiguousarray(X[:, b:e]), np.ascontiguousarray(Y[:, b:e]), N, b)
                assert np.all(part[:b] == 0.0) and np.all(part[e:] == 0.0)
                total += part  # what the all-reduce does: every entry has one contributor
            assert np.array_equal(total, whole), (M, N, size)
        host = np.ascontiguousarray(whole)
        s = 0.0
        for v in whole:
            s += v
        assert lib.stk_sum_steps(host.ctypes.data_as(ctypes.c_void_p), N) == s
    # the vector class: one value however it is cut
    from source.mpi_vector import DofDistributionMPI, KronVectorMPI

    class _Cut:  # rank `rank` of `size`, no transport: the all-reduce is done by hand below
        def __init__(self, rank, size):
            self.rank, self.size, self.parts = rank, size, None

        def Get_rank(self):
            return self.rank

        def Get_size(self):
            return self.size

        def allreduce_tensor_(self, t):
            self.parts = t.clone()
            return t

    N, M = 33, 961
    X, Y = rng.rand(N, M), rng.rand(N, M)
    one = _vec(_dd(N, M), X).dot(_vec(_dd(N, M), Y))
    assert abs(one - np.vdot(X, Y)) < 1e-13 * np.vdot(X, Y)
    for size in (2, 4, 8):
        steps = torch.zeros(N, dtype=torch.float64, device='cuda')
        for r in range(size):
            dd = DofDistributionMPI(_Cut(r, size), N, M)
            KronVectorMPI(dd, X[dd.t_begin:dd.t_end]).dot(KronVectorMPI(dd, Y[dd.t_begin:dd.t_end]))
            steps += dd.comm.parts
        total = 0.0
        for v in steps.tolist():
            total += v
        assert total == one, (size, total, one)


def test_kron_apply_does_not_depend_on_the_partition(stk):
    """The Kronecker sum on time slabs -- the one-pass form with ghost lanes, the
    overlapped form (pass without ghost steps + stk_kron_pack_ghost_apply) and the
    plain sliced-ELL form (stk_kron_ell_apply + _ghost_apply) -- gives, on every
    slab of 2, 3, 4, 5 and 8 ranks, bit for bit the rows of the ONE-RANK apply: the
    time stencil has one order of operations in every form (rounds
    1-5 added the ghost rows' share last, an order no interior step has).  Slabs of one
    step (both ghost rows meet in it), odd and even lengths, row pairs, one to three
    terms, an identity time factor among them."""
    from source.assembly import space_matrices
    from source.linop import EllMatrices
    from source.problem import problem_helper
    rng = np.random.RandomState(99)
    M_x, A_x = space_matrices(problem_helper('square', J_space=3, J_time=2)[0])
    mats = [M_x, A_x, sp.csr_matrix(M_x + 0.3 * A_x)]
    ell = EllMatrices(mats, [M_x])
    M = ell.M
    forms = [('one row per slot row', ell.packed_variant(1)), ('row pairs', ell.packed_variant(2))]
    assert all(f.ok for _, f in forms)

    def slab(a):
        n = a.shape[1]
        s_ = torch.zeros((M, n + (n & 1)), dtype=torch.float64, device='cuda')
        s_[:, :n] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return s_

    for N, nt, identity in [(5, 2, False), (9, 2, False), (17, 3, True), (33, 1, False), (65, 2, False),
                            (66, 3, False)]:
        X = rng.rand(M, N)
        tris = [None if (identity and k == 1) else rng.rand(3, N) for k in range(nt)]
        ld = N + (N & 1)
        x = slab(X)
        whole = {}
        for name, form in forms:
            y = slab(np.zeros((M, N)))
            form.apply([(None if t is None else _lib_dev(t), k) for k, t in enumerate(tris)], x, None, N, ld, 0.0, y)
            whole[name] = y[:, :N].clone()
        y = slab(np.zeros((M, N)))
        ell.apply([(None if t is None else _lib_dev(t), k, x, None, None) for k, t in enumerate(tris)], N, ld, 0.0, y)
        whole['plain'] = y[:, :N].clone()
        assert torch.equal(whole['plain'], whole['row pairs']) and torch.equal(whole['plain'],
                                                                              whole['one row per slot row'])
        T = [np.eye(N) if t is None else np.diag(t[1]) + np.diag(t[0, 1:], -1) + np.diag(t[2, :-1], 1) for t in tris]
        want = sum((mats[k] @ X) @ T[k].T for k in range(nt))
        assert relerr(whole['plain'].cpu().numpy(), want) < 1e-13
        for size in (2, 3, 4, 5, 8):
            if size > N:
                continue
            for b, e in _blocks(N, size):
                n_loc, ldl = e - b, (e - b) + ((e - b) & 1)
                xs = slab(X[:, b:e])
                lo = torch.from_numpy(np.ascontiguousarray(X[:, b - 1])).cuda() if b > 0 else None
                hi = torch.from_numpy(np.ascontiguousarray(X[:, e])).cuda() if e < N else None
                local = [None if t is None else _lib_dev(np.ascontiguousarray(t[:, b:e])) for t in tris]
                specs = [(local[k], k) for k in range(nt)]
                gh = None
                if lo is not None or hi is not None:
                    gh = torch.zeros((M, 2), dtype=torch.float64, device='cuda')
                    if lo is not None:
                        gh[:, 0] = lo
                    if hi is not None:
                        gh[:, 1] = hi
                for name, form in forms:
                    ref = whole[name][:, b:e]
                    y1 = slab(rng.rand(M, n_loc))
                    form.apply(specs, xs, gh, n_loc, ldl, 0.0, y1)
                    assert torch.equal(y1[:, :n_loc], ref), (name, 'ghost lanes', N, size, b, e)
                    y2 = slab(rng.rand(M, n_loc))
                    form.apply(specs, xs, None, n_loc, ldl, 0.0, y2)
                    form.apply_ghost(specs, xs, lo, hi, n_loc, ldl, y2)
                    assert torch.equal(y2[:, :n_loc], ref), (name, 'overlapped', N, size, b, e)
                    if ldl > n_loc:
                        assert float(y2[:, n_loc:].abs().max()) == 0.0
                    # ... and from the compact records of the pack kernel and the interleaved
                    # received rows (stk_halo_pack_records, stk_kron_pack_boundary_apply): what
                    # the operator classes run
                    if gh is not None:
                        rec = torch.empty((M, 4), dtype=torch.float64, device='cuda')
                        first = torch.empty(M, dtype=torch.float64, device='cuda')
                        last = torch.empty(M, dtype=torch.float64, device='cuda')
                        stk.check(stk.lib().stk_halo_pack_records(
                            stk.stream(), M, n_loc, ldl, stk.ptr(xs), stk.ptr(first), 1, stk.ptr(last), 1,
                            stk.ptr(rec)))
                        assert torch.equal(first, xs[:, 0]) and torch.equal(last, xs[:, n_loc - 1])
                        assert torch.equal(rec[:, 0], xs[:, 0]) and torch.equal(rec[:, 3], xs[:, n_loc - 1])
                        assert torch.equal(rec[:, 1], xs[:, min(1, n_loc - 1)])
                        assert torch.equal(rec[:, 2], xs[:, max(n_loc - 2, 0)])
                        y2b = slab(rng.rand(M, n_loc))
                        form.apply(specs, xs, None, n_loc, ldl, 0.0, y2b)
                        form.apply_boundary(specs, rec, gh, lo is not None, hi is not None, n_loc, ldl, y2b)
                        assert torch.equal(y2b, y2), (name, 'records', N, size, b, e)
                y3 = slab(rng.rand(M, n_loc))
                ell.apply([(local[k], k, xs, lo, hi) for k in range(nt)], n_loc, ldl, 0.0, y3)
                assert torch.equal(y3[:, :n_loc], whole['plain'][:, b:e]), ('plain', N, size, b, e)
                y4 = slab(rng.rand(M, n_loc))
                ell.apply_local([(local[k], k, xs, None, None) for k in range(nt)], n_loc, ldl, 0.0, y4)
                ell.apply_ghost([(local[k], k, xs, lo, hi) for k in range(nt)], n_loc, ldl, y4)
                assert torch.equal(y4, y3), ('plain, overlapped', N, size, b, e)
                # beta != 0 on a slab with neighbours: the one-call form keeps the old
                # boundary entries it scales (y = beta y0 + A x, rounded as on one rank)
                y0 = rng.rand(M, n_loc)
                y5, y6 = slab(y0), slab(y0)
                ell.apply([(local[k], k, xs, lo, hi) for k in range(nt)], n_loc, ldl, 0.5, y5)
                two = forms[1][1]
                two.apply(specs, xs, gh, n_loc, ldl, 0.5, y6)
                assert torch.equal(y5, y6), ('beta', N, size, b, e)
                assert relerr(y5[:, :n_loc].cpu().numpy(), 0.5 * y0 + want[:, b:e]) < 1e-13


def test_kron_pack_row_pairs(stk):
    """The row-pair form of stk_kron_pack_apply (two matrix rows per slot row,
    the union of their columns gathered once) on the P1 matrices of the square
    and the L-shape and on banded matrices with 5-entry rows: rows really are
    paired, the result is bit for bit that of the one-row form (same accumulation
    order, absent columns add exact zeros) and agrees with dense NumPy; ghost time
    steps, 1-3 terms, beta, slab lengths through the lane / group / prefetch
    instances."""
    from source.assembly import space_matrices
    from source.linop import EllMatrices
    from source.problem import problem_helper
    rng = np.random.RandomState(123)
    families = []
    for problem, J in (('square', 2), ('square', 4), ('lshape', 3)):
        M_x, A_x = space_matrices(problem_helper(problem, J_space=J, J_time=2)[0])
        families.append((problem, [M_x, A_x, sp.csr_matrix(M_x + 0.3 * A_x)]))
    n = 23 * 17
    band = sp.diags([rng.choice([1.0, -2.0, 0.5], size=n - abs(o)) for o in (-17, -1, 0, 1, 17)],
                    (-17, -1, 0, 1, 17), format='csr')
    families.append(('band5', [band, sp.csr_matrix(band.T), sp.csr_matrix(band + band.T)]))
    offs9 = (-18, -17, -16, -1, 0, 1, 16, 17, 18)  # 9-point stencil: pairs of 12 slots
    nine = sp.diags([rng.choice([1.0, -2.0, 0.5, 3.0], size=n - abs(o)) for o in offs9], offs9, format='csr')
    families.append(('nine', [nine, sp.csr_matrix(nine.T), sp.csr_matrix(nine + 2.0 * nine.T)]))
    seen_pairs = 0
    for name, mats_all in families:
        for n_loc in (1, 2, 8, 9, 17, 33, 65, 129):
            nt = int(rng.randint(1, 4))
            mats = mats_all[:nt]
            ell = EllMatrices(mats, [mats_all[0]])
            one, two = ell.packed_variant(1), ell.packed_variant(2)
            assert one.ok and one.rows_per_unit == 1
            assert two.ok and two.rows_per_unit == 2, (name, two.ok)
            M = ell.M
            assert two.n_units < 0.7 * M and two.K in (8, 10, 12)
            seen_pairs += M - two.n_units
            ld = n_loc + (n_loc & 1)
            X = rng.rand(M, n_loc)
            lo = rng.rand(M) if rng.randint(2) else None
            hi = rng.rand(M) if rng.randint(2) else None
            beta = float(rng.choice([0.0, 0.5]))
            y0 = rng.rand(M, n_loc)
            want, specs = beta * y0, []
            for k in range(nt):
                t = rng.rand(3, n_loc)
                T = np.diag(t[1]) + np.diag(t[0, 1:], -1) + np.diag(t[2, :-1], 1)
                want = want + (mats[k] @ X) @ T.T
                if lo is not None:
                    want[:, 0] += t[0, 0] * (mats[k] @ lo)
                if hi is not None:
                    want[:, -1] += t[2, -1] * (mats[k] @ hi)
                specs.append((_lib_dev(t), k))

            def slab(a):
                s_ = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
                s_[:, :n_loc] = torch.from_numpy(a).cuda()
                return s_

            x, gh = slab(X), None
            if lo is not None or hi is not None:
                gh = torch.zeros((M, 2), dtype=torch.float64, device='cuda')
                if lo is not None:
                    gh[:, 0] = torch.from_numpy(lo).cuda()
                if hi is not None:
                    gh[:, 1] = torch.from_numpy(hi).cuda()
            y1, y2 = slab(y0), slab(y0)
            one.apply(specs, x, gh, n_loc, ld, beta, y1)
            two.apply(specs, x, gh, n_loc, ld, beta, y2)
            assert torch.equal(y1, y2), (name, n_loc, nt)
            assert relerr(y2[:, :n_loc].cpu().numpy(), want) < 1e-13, (name, n_loc, nt)
            if ld > n_loc:
                assert float(y2[:, n_loc:].abs().max()) == 0.0
            # the overlapped form of several ranks (reference mpi_kron.py:193-200): the
            # pass WITHOUT the ghost steps (beta = 0), then the first and last step
            # recomputed with the received rows as they arrive
            # (stk_kron_pack_ghost_apply) -- bit for bit the one-pass form
            if gh is not None:
                dev_lo = None if lo is None else torch.from_numpy(lo).cuda()
                dev_hi = None if hi is None else torch.from_numpy(hi).cuda()
                y2z = slab(y0)
                two.apply(specs, x, gh, n_loc, ld, 0.0, y2z)
                for form in (one, two):
                    y3 = slab(y0)
                    form.apply(specs, x, None, n_loc, ld, 0.0, y3)
                    form.apply_ghost(specs, x, dev_lo, dev_hi, n_loc, ld, y3)
                    assert torch.equal(y3, y2z), (name, n_loc, nt, float((y3 - y2z).abs().max()))
    assert seen_pairs > 0
    # rows that share nothing stay alone: the planner keeps the one-row form
    circ = lambda k: sp.csr_matrix((np.ones(64), (np.arange(64), (np.arange(64) + k) % 64)), shape=(64, 64))
    scattered = sp.csr_matrix(circ(0) + circ(13) + circ(-13) + circ(29) + circ(-29))
    e = EllMatrices([scattered])
    assert e.packed.ok and e.packed.rows_per_unit == 1


def test_kron_pack_inputs_per_term(stk):
    """stk_kron_pack_apply_multi: every term gathers from a slab of its own on the
    one packed slot stream (the last stage of SchurMPI: (I kron M_x) v1 + (I kron
    A_x) v2 + (G_t kron M_x) x, reference heateq_mpi.py:166-181).  Bit for bit the
    plain sliced-ELL form it replaces (stk_kron_ell_apply: same sums per row, terms
    added in the same order) for the Schur shape, and dense NumPy for random time
    factors -- among them factors with a single entry, whose term only a few lanes
    gather; one row and row pairs per slot row; 2 and 3 terms, beta, slab lengths
    through the lane / group / prefetch instances.  Three forms of the pass: a lane
    group per term (round 5: csrc/kron_pack_multi.hip) without and with the
    caller's statement of the time steps each factor reads (`steps`), and round 4's
    turn-taking lanes (tuning key pack_multi_lanes = 0) -- all three bit for bit the
    same."""
    from source import _lib
    from source.assembly import space_matrices
    from source.linop import EllMatrices, time_factor_steps
    from source.problem import problem_helper
    rng = np.random.RandomState(77)
    families = []
    for problem, J in (('square', 2), ('square', 4), ('lshape', 3)):
        M_x, A_x = space_matrices(problem_helper(problem, J_space=J, J_time=2)[0])
        families.append((problem, [M_x, A_x]))
    for name, mats in families:
        ell = EllMatrices(mats, [mats[0]])
        M = ell.M
        for n_loc in (1, 2, 8, 9, 17, 33, 65, 129):
            ld = n_loc + (n_loc & 1)

            def slab(a):
                s_ = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
                s_[:, :n_loc] = torch.from_numpy(a).cuda()
                return s_

            for shape in ('schur', 'random2', 'random3', 'single'):
                nt = 2 if shape == 'random2' else 3
                Xs = [rng.rand(M, n_loc) for _ in range(nt)]
                tris, which = [], [int(rng.randint(2)) for _ in range(nt)]
                if shape == 'schur':
                    which = [0, 1, 0]
                    g = np.zeros((3, n_loc))
                    g[1, 0] = 1.0  # G_t = e_0 e_0^T (reference heateq_mpi.py:86-88)
                    tris = [None, None, g]
                elif shape == 'single':
                    for k in range(nt):  # one entry somewhere in the band
                        t = np.zeros((3, n_loc))
                        d, c = int(rng.randint(3)), int(rng.randint(n_loc))
                        if n_loc > 1:
                            c = min(max(c, 1 if d == 0 else 0), n_loc - 2 if d == 2 else n_loc - 1)
                            t[d, c] = 1.5
                        else:
                            t[1, 0] = 1.5
                        tris.append(t)
                else:
                    tris = [rng.rand(3, n_loc) if rng.randint(3) else None for _ in range(nt)]
                beta = float(rng.choice([0.0, 0.5]))
                y0 = rng.rand(M, n_loc)
                want = beta * y0
                for k in range(nt):
                    Z = mats[which[k]] @ Xs[k]
                    if tris[k] is not None:
                        t = tris[k]
                        T = np.diag(t[1]) + np.diag(t[0, 1:], -1) + np.diag(t[2, :-1], 1)
                        Z = Z @ T.T
                    want = want + Z
                dev_tri = [None if t is None else _lib_dev(t) for t in tris]
                xs = [slab(X) for X in Xs]
                y_plain = slab(y0)
                ell.apply([(dev_tri[k], which[k], xs[k], None, None) for k in range(nt)],
                          n_loc, ld, beta, y_plain)
                for rows in (1, 2):
                    form = ell.packed_variant(rows)
                    assert form.ok and form.rows_per_unit == rows and not form.explicit
                    tag = (name, n_loc, shape, rows)
                    specs_ = [(dev_tri[k], which[k], xs[k]) for k in range(nt)]
                    y, y_steps, y_turns, y_auto = slab(y0), slab(y0), slab(y0), slab(y0)
                    try:
                        # 2: a lane group per term whatever the slab (1, the default, takes
                        # it from 24 steps on or beyond the Infinity Cache), 0: turns
                        _lib.check(_lib.lib().stk_set_tuning(b'pack_multi_lanes', 2))
                        form.apply_multi(specs_, n_loc, ld, beta, y)
                        form.apply_multi(specs_, n_loc, ld, beta, y_steps,
                                         steps=[time_factor_steps(t) for t in tris])
                        _lib.check(_lib.lib().stk_set_tuning(b'pack_multi_lanes', 0))
                        form.apply_multi(specs_, n_loc, ld, beta, y_turns)
                    finally:
                        _lib.check(_lib.lib().stk_set_tuning(b'pack_multi_lanes', 1))
                    form.apply_multi(specs_, n_loc, ld, beta, y_auto)
                    # the entry point without stated steps, called by its own name
                    y_direct = slab(y0)
                    _lib.check(_lib.lib().stk_kron_pack_apply_multi(
                        _lib.stream(), ctypes.byref(form.pattern), n_loc, ld, nt,
                        form._terms([(dev_tri[k], which[k]) for k in range(nt)]),
                        (ctypes.c_void_p * nt)(*[_lib.ptr(x) for x in xs]), beta, _lib.ptr(y_direct)))
                    assert torch.equal(y_steps, y), tag
                    assert torch.equal(y_auto, y), tag
                    assert torch.equal(y_direct, y), tag
                    assert torch.equal(y_turns, y), tag
                    assert relerr(y[:, :n_loc].cpu().numpy(), want) < 1e-13, tag
                    if shape == 'schur':
                        assert torch.equal(y, y_plain), tag
                    else:
                        assert float((y - y_plain).abs().max()) <= 1e-13 * float(y_plain.abs().max()), tag
                    if ld > n_loc:
                        assert float(y[:, n_loc:].abs().max()) == 0.0
    # The stated time steps are trusted: a range that omits a step a factor reads
    # silently drops that step's contribution.  The tuning key "pack_check_steps" makes
    # the entry point fetch the factors and refuse such a range -- and lets
    # the honest ranges of time_factor_steps through.
    name, mats = families[0]
    ell = EllMatrices(mats, [mats[0]])
    M, n_loc, ld = ell.M, 9, 10
    g = np.zeros((3, n_loc))
    g[1, 0], g[0, 5] = 1.0, 2.0  # reads the steps 0 and 4
    tri = _lib_dev(g)
    xs = [torch.from_numpy(np.ascontiguousarray(np.pad(rng.rand(M, n_loc), ((0, 0), (0, 1))))).cuda() for _ in range(3)]
    specs_ = [(None, 0, xs[0]), (None, 1, xs[1]), (tri, 0, xs[2])]
    y = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
    form = ell.packed_variant(2)
    assert time_factor_steps(g) == (0, 5)
    try:
        _lib.check(_lib.lib().stk_set_tuning(b'pack_check_steps', 1))
        form.apply_multi(specs_, n_loc, ld, 0.0, y, steps=[None, None, (0, 5)])
        with pytest.raises(_lib.StkError, match='reads time step 4'):
            form.apply_multi(specs_, n_loc, ld, 0.0, y, steps=[None, None, (0, 2)])
    finally:
        _lib.check(_lib.lib().stk_set_tuning(b'pack_check_steps', 0))


def test_kron_pack_explicit_value_pairs(stk):
    """Row pairs WITHOUT a dictionary (stk_pack_pattern.vals): matrices whose
    values do not repeat -- P1 on a jittered L-shape (BASELINE config 4's
    "unstructured spatial mesh, irregular CSR"; the reference takes any CSR,
    mpi_kron.py:135-150) and banded matrices with random entries.  The planner
    must take the explicit form, rows must really be paired, and the result must
    agree with the one-row plain form (stk_kron_ell_apply) to the last bits and
    with dense NumPy; ghost lanes, the overlapped ghost share, 1-3 terms, beta, slab lengths
    through the lane / group / prefetch instances."""
    from source.assembly import space_matrices
    from source.linop import EllMatrices
    from source.problem import problem_helper
    rng = np.random.RandomState(321)
    families = []
    for J in (2, 4):
        M_x, A_x = space_matrices(problem_helper('lshape_jitter', J_space=J, J_time=2)[0])
        families.append(('lshape_jitter%d' % J, [M_x, A_x, sp.csr_matrix(M_x + 0.3 * A_x)]))
    n = 23 * 17
    offs = (-17, -1, 0, 1, 17)
    band = sp.diags([rng.rand(n - abs(o)) + 0.1 for o in offs], offs, format='csr')
    families.append(('band5_random', [band, sp.csr_matrix(band.T), sp.csr_matrix(band + 2.0 * band.T)]))
    for name, mats_all in families:
        for n_loc in (1, 2, 8, 9, 17, 33, 65, 129):
            nt = int(rng.randint(1, 4))
            mats = mats_all[:nt]
            ell = EllMatrices(mats, [mats_all[0]])
            two = ell.packed_variant(2)
            assert two.ok and two.explicit and two.rows_per_unit == 2, (name, two.ok)
            assert not ell.packed_variant(1).ok  # no dictionary for these values
            M = ell.M
            assert two.n_units < 0.7 * M and two.K in (8, 10, 12)
            ld = n_loc + (n_loc & 1)
            X = rng.rand(M, n_loc)
            lo = rng.rand(M) if rng.randint(2) else None
            hi = rng.rand(M) if rng.randint(2) else None
            beta = float(rng.choice([0.0, 0.5]))
            y0 = rng.rand(M, n_loc)
            want, specs, plain = beta * y0, [], []

            def slab(a):
                s_ = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
                s_[:, :n_loc] = torch.from_numpy(a).cuda()
                return s_

            x = slab(X)
            dev_lo = None if lo is None else torch.from_numpy(lo).cuda()
            dev_hi = None if hi is None else torch.from_numpy(hi).cuda()
            for k in range(nt):
                t = rng.rand(3, n_loc)
                T = np.diag(t[1]) + np.diag(t[0, 1:], -1) + np.diag(t[2, :-1], 1)
                want = want + (mats[k] @ X) @ T.T
                if lo is not None:
                    want[:, 0] += t[0, 0] * (mats[k] @ lo)
                if hi is not None:
                    want[:, -1] += t[2, -1] * (mats[k] @ hi)
                td = _lib_dev(t)
                specs.append((td, k))
                plain.append((td, k, x, dev_lo, dev_hi))
            gh = None
            if lo is not None or hi is not None:
                gh = torch.zeros((M, 2), dtype=torch.float64, device='cuda')
                if lo is not None:
                    gh[:, 0] = dev_lo
                if hi is not None:
                    gh[:, 1] = dev_hi
            y1, y2 = slab(y0), slab(y0)
            ell.apply(plain, n_loc, ld, beta, y1)
            two.apply(specs, x, gh, n_loc, ld, beta, y2)
            assert relerr(y2[:, :n_loc].cpu().numpy(), want) < 1e-13, (name, n_loc, nt)
            # the space-factor sums are those of the plain form; the two kernels
            # combine terms and time stencil in their own order: last bits only
            assert float((y1 - y2).abs().max()) <= 4e-15 * float(y1.abs().max()), (name, n_loc, nt)
            if ld > n_loc:
                assert float(y2[:, n_loc:].abs().max()) == 0.0
            if gh is not None:
                y2z, y3 = slab(y0), slab(y0)
                two.apply(specs, x, gh, n_loc, ld, 0.0, y2z)
                two.apply(specs, x, None, n_loc, ld, 0.0, y3)
                two.apply_ghost(specs, x, dev_lo, dev_hi, n_loc, ld, y3)
                assert torch.equal(y3, y2z), (name, n_loc, nt)
    # the operator classes pick the form up by themselves
    from source.mpi_kron import SumMPI, TridiagKronMatMPI
    M_x, A_x = space_matrices(problem_helper('lshape_jitter', J_space=3, J_time=2)[0])
    N = 33
    A_t = sp.diags([rng.rand(N - 1), rng.rand(N), rng.rand(N - 1)], (-1, 0, 1), format='csr')
    M_t = sp.diags([rng.rand(N - 1), rng.rand(N), rng.rand(N - 1)], (-1, 0, 1), format='csr')
    dd = _dd(N, M_x.shape[0])
    op = SumMPI(dd, [TridiagKronMatMPI(dd, A_t, M_x), TridiagKronMatMPI(dd, M_t, A_x)])
    assert 'explicit' in op._groups[0].kernel_name(N)
    Xh = rng.rand(N, M_x.shape[0])
    want = A_t @ Xh @ M_x.T + M_t @ Xh @ A_x.T
    assert relerr(_np(op @ _vec(dd, Xh)), want) < 1e-13


def test_row_engine_randomised_shapes(stk):
    """stk_ell_spmm on random rectangular matrices: y = alpha (ca A + cm[t] M) x
    + beta z for every slot count, with and without the second value array,
    z absent / separate / aliasing y, odd slab lengths padded to even."""
    import ctypes
    from source.linop import EllRowsMatrix, union_pattern
    rng = np.random.RandomState(7)
    lib = stk.lib()
    done = 0
    for case in range(60):
        rows, cols = int(rng.randint(1, 300)), int(rng.randint(1, 300))
        n_loc = int(rng.randint(1, 20))
        ld = n_loc + (n_loc & 1)
        width = int(rng.choice([1, 2, 4, 6, 8, 11, 15, 19]))
        A = sp.random(rows, cols, density=min(1.0, width / cols),
                      random_state=rng, format='csr')
        Mm = A.copy()
        Mm.data = rng.rand(Mm.nnz)
        has_m = bool(rng.randint(2))
        indptr, indices, vals = union_pattern([A, Mm])
        e = EllRowsMatrix(indptr, indices, vals[0], vals[1] if has_m else None,
                          rng.permutation(rows))
        if not e.ok:  # a random row came out wider than the widest slot count
            continue
        done += 1
        ca, alpha = float(rng.rand() + 0.5), float(rng.rand() + 0.5)
        cm = rng.rand(n_loc)
        X, Z = rng.rand(cols, n_loc), rng.rand(rows, n_loc)
        mode = int(rng.randint(3))  # 0: no z, 1: separate z, 2: z aliases y
        beta = 0.0 if mode == 0 else float(rng.rand() + 0.5)
        want = np.empty((rows, n_loc))
        for t in range(n_loc):
            mat = ca * A + (cm[t] * Mm if has_m else 0 * Mm)
            want[:, t] = alpha * (mat @ X[:, t]) + beta * Z[:, t]

        def slab(a, n):
            s_ = torch.zeros((n, ld), dtype=torch.float64, device='cuda')
            s_[:, :n_loc] = torch.from_numpy(a).cuda()
            return s_

        x, z = slab(X, cols), slab(Z, rows)
        y = z if mode == 2 else torch.full((rows, ld), np.nan,
                                           dtype=torch.float64, device='cuda')
        cmd = _lib_dev(cm) if has_m else None
        stk.check(lib.stk_ell_spmm(stk.stream(), ctypes.byref(e.struct), n_loc,
                                   ld, cols, ca, stk.ptr(cmd), stk.ptr(x), alpha,
                                   beta, stk.ptr(z) if mode else None,
                                   stk.ptr(y)))
        got = y[:, :n_loc].cpu().numpy()
        assert relerr(got, want) < 1e-13, (case, rows, cols, n_loc, width, has_m, mode)
        if ld > n_loc:
            assert float(y[:, n_loc:].abs().max()) == 0.0
    assert done >= 30


def test_multigrid_on_random_algebraic_hierarchies(stk):
    """MultiGrid on hierarchies that come from no mesh: random SPD matrices in
    random order (deep Gauss-Seidel dependency chains, rows wider than the ELL
    slots on some levels) and random aggregation-type prolongations, two or
    three levels, on slabs with several time columns: against the oracle."""
    from oracle.multigrid import MultiGrid as OracleMG
    from source.multigrid import MeshHierarchy, MultiGrid
    rng = np.random.RandomState(99)
    for case in range(12):
        sizes = [int(rng.randint(2, 6))]
        for _ in range(int(rng.randint(1, 3))):
            sizes.append(sizes[-1] * int(rng.randint(2, 5)) + int(rng.randint(0, 4)))
        n = sizes[-1]
        B = sp.random(n, n, density=min(1.0, rng.choice([2, 5, 12]) / n),
                      random_state=rng, format='csr')
        A = sp.csr_matrix(B @ B.T + sp.diags(rng.rand(n) + 1.0))
        P_mats = []
        for nc, nf in zip(sizes[:-1], sizes[1:]):
            r = np.arange(nf)
            c1, c2 = rng.randint(0, nc, nf), rng.randint(0, nc, nf)
            # every coarse dof is the first parent of at least one fine dof:
            # P has full column rank, the Galerkin matrices stay SPD
            c1[rng.permutation(nf)[:nc]] = np.arange(nc)
            P = sp.csr_matrix((np.concatenate([np.ones(nf), 0.5 * rng.rand(nf)]),
                               (np.concatenate([r, r]), np.concatenate([c1, c2]))),
                              shape=(nf, nc))
            P_mats.append(P)
        ss, vc = int(rng.randint(1, 4)), int(rng.randint(1, 3))
        mg = MultiGrid(A, MeshHierarchy(P_mats=P_mats), smoothsteps=ss, vcycles=vc)
        omg = OracleMG(A, P_mats, ss, vc)
        k = int(rng.randint(1, 8))
        Bv = rng.rand(n, k)
        assert relerr(mg @ Bv, omg @ Bv) < 1e-11, (case, sizes, ss, vc, k)


def test_zero_start_first_sweep_is_exact(stk):
    """The first forward sweep of a level visit, run on the per-group matrices
    that drop the products with not yet updated (zero) neighbours and without
    zeroing u first (stk_mg_level.ell_fwd0), gives bitwise the same V-cycle."""
    import heateq_mpi as hm
    for problem, J_space in (('square', 5), ('lshape', 4), ('cube', 2)):
        h = hm.HeatEquationMPI(J_space=J_space, J_time=3, problem=problem)
        x = _vec(h.dofs_distr, np.random.RandomState(13).rand(h.N, h.M))
        res = []
        try:
            for zs in (0, 1):
                stk.check(stk.lib().stk_set_tuning(b'mg_zero_start', zs))
                # poison the allocator's free blocks: the zero-start path must
                # not depend on what the output buffers contain
                junk = torch.full((h.M, 2 * h.N + 8), float('nan'),
                                  dtype=torch.float64, device='cuda')
                del junk
                res.append((_np(h.P @ x), _np(h.S @ x)))
        finally:
            stk.check(stk.lib().stk_set_tuning(b'mg_zero_start', 1))
        assert np.array_equal(res[0][0], res[1][0])
        assert np.array_equal(res[0][1], res[1][1])


def test_device_plan_construction_matches_host(stk):
    """the Galerkin products R A P (reference multigrid.py:142-145) and
    the sliced-ELL copies of a hierarchy are made on the device (stk_csr_galerkin,
    stk_ell_from_csr).  The products must be BIT FOR BIT SciPy's `R @ A @ P` --
    pattern and values, on the square, the L-shape and the cube, for mass and
    stiffness down the whole hierarchy -- and the ELL copies exactly the arrays the
    NumPy planner builds (plain, Gauss-Seidel with and without the diagonal among
    the slots, zero-start copies with their padding rule)."""
    from source import multigrid as mgm
    from source.assembly import prolongation_matrices, space_matrices
    from source.linop import EllRowsMatrix, union_pattern
    from source.problem import problem_helper
    rng = np.random.RandomState(4)
    for problem, J in (('square', 5), ('lshape', 4), ('cube', 2)):
        mesh = problem_helper(problem, J_space=J, J_time=2)[0]
        M_x, A_x = space_matrices(mesh)
        P_mats = [sp.csr_matrix(P) for P in prolongation_matrices(mesh)]
        for mat in (A_x, M_x, sp.csr_matrix(4.0 * M_x + 0.3 * A_x)):
            fine = sp.csr_matrix(mat)
            for P in reversed(P_mats):
                R = P.T.tocsr()
                want = sp.csr_matrix(R @ fine @ P)
                want.sort_indices()
                got = mgm.galerkin_product(R, fine, P)
                if R.shape[0] >= 64:
                    assert got.has_sorted_indices
                assert np.array_equal(got.indptr, want.indptr), (problem, R.shape)
                assert np.array_equal(got.indices, want.indices)
                assert np.array_equal(got.data, want.data), (problem, R.shape,
                                                             np.abs(got.data - want.data).max())
                ra_want = sp.csr_matrix(R @ fine)
                ra_want.sort_indices()
                ra = mgm.galerkin_product(R, fine, None)
                assert (np.array_equal(ra.indptr, ra_want.indptr) and np.array_equal(ra.indices, ra_want.indices)
                        and np.array_equal(ra.data, ra_want.data)), (problem, R.shape, 'R A')
                # the dependency groups of the sweeps: device relaxation = NumPy loop
                if fine.shape[0] >= 64:
                    fs = sp.csr_matrix(fine)
                    fs.sort_indices()
                    ip, ix = fs.indptr.astype(np.int32), fs.indices.astype(np.int32)
                    for bw in (False, True):
                        p_h, r_h = mgm.gauss_seidel_schedule(ip, ix, bw)
                        p_d, r_d = mgm.gauss_seidel_schedule(ip, ix, bw, on_device=(stk.to_dev(ip), stk.to_dev(ix)))
                        assert np.array_equal(p_h, p_d) and np.array_equal(r_h, r_d)
                fine = want
        # ELL copies: the device builder against the NumPy builder, array by array
        indptr, indices, vals = union_pattern([A_x, M_x])
        n = len(indptr) - 1
        order = rng.permutation(n)
        grp = rng.randint(0, 4, size=n)
        rows_of = np.repeat(np.arange(n), np.diff(indptr))
        kept = np.bincount(rows_of[grp[indices] < grp[rows_of]], minlength=n)
        for kw in (dict(), dict(diag=True), dict(dia_values=True),
                   dict(dia_values=True, earlier_group=grp, kept_counts=kept, pad_col=-1),
                   dict(pad_col=3)):
            for vm in (vals[1], None):
                sub = order[:max(1, n // 3)]
                dev = EllRowsMatrix(indptr, indices, vals[0], vm, sub, **kw)
                dev.check()
                host = EllRowsMatrix.__new__(EllRowsMatrix)
                host._build_with_numpy(indptr, indices, vals[0], vm, np.asarray(sub, dtype=np.int64), dev.K,
                                       kw.get('diag', False), kw.get('pad_col', 0),
                                       kw.get('diag', False) or kw.get('dia_values') is not None,
                                       kw.get('earlier_group'))
                for name in ('idx', 'va', 'vm', 'dia_a', 'dia_m'):
                    a, b = getattr(dev, name), getattr(host, name)
                    assert (a is None) == (b is None), (problem, kw.keys(), name)
                    if a is not None:
                        assert torch.equal(a, b.to(a.device)), (problem, list(kw), name)


def test_two_stream_multigrid_pair_is_exact(stk):
    """S applies K to two independent right-hand sides; MultiGrid.apply_pair runs
    the two V-cycle chains side by side on two HIP streams (twin plan = second set
    of level workspaces).  Results must be bit for bit those of two applies on one
    stream, buffers must survive the caching allocator across streams (repeated
    with fresh allocations), and S itself must not depend on the switch.

    The library also takes a COLUMN RANGE of a wider slab (stk_mg_apply,
    stk_ell_spmm: pointer inside a row, ld of the whole slab, the per-slice cm /
    kind tables offset alike): two ranges through C A C, called through the C ABI on
    the family's plan and A_x's row-engine copy, give P of the whole slab bit for
    bit -- also with mg_zero_start = 0, whose level-wide memset must stay inside the
    columns of its own range."""
    import heateq_mpi as hm
    h = hm.HeatEquationMPI(J_space=5, J_time=4)
    K = h.Kinv_x
    rng = np.random.RandomState(31)
    n_loc, M = h.N, h.M
    for rep in range(6):
        a = _vec(h.dofs_distr, rng.rand(n_loc, M)).buf
        b = _vec(h.dofs_distr, rng.rand(n_loc, M)).buf
        want = (K.apply(a, n_loc=n_loc).clone(), K.apply(b, n_loc=n_loc).clone())
        got = K.apply_pair(a, b, n_loc=n_loc)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), rep
        del a, b, got  # released while the side stream may still hold them
        junk = [torch.rand((M, n_loc + (n_loc & 1)), dtype=torch.float64, device='cuda') for _ in range(3)]
        del junk
    lib = stk.lib()

    def cac_by_column_ranges(hh, x):
        _, fam, (cm, kind), mid = hh.P._batched
        n_loc, ld = x.n_loc, x.ld
        plan, rows = fam._dev.ensure_plan(ld), mid._ell_form()
        half = ((n_loc + 1) // 2 + 1) & ~1  # even: the second range starts on a 16-byte pair
        t1, t2 = torch.empty_like(x.buf), torch.empty_like(x.buf)
        out = x._like()
        out.buf.fill_(float('nan'))  # a column that no range wrote must not pass by luck
        at = lambda t, off: stk.ptr(t) + t.element_size() * off
        for off, n in ((0, half), (half, n_loc - half)):
            def family(src, dst):
                stk.check(lib.stk_mg_apply(plan, stk.stream(), n, ld, fam.ca, at(cm, off), at(kind, off),
                                           at(src, off), at(dst, off)))

            family(x.buf, t1)
            stk.check(lib.stk_ell_spmm(stk.stream(), ctypes.byref(rows.struct), n, ld, hh.M, 1.0, None,
                                       at(t1, off), 1.0, 0.0, None, at(t2, off)))
            family(t2, out.buf)
        return _np(out)

    for J_time in (4, 3, 5):  # 17, 9 and 33 time steps: odd slabs, uneven ranges
        hh = h if J_time == 4 else hm.HeatEquationMPI(J_space=4, J_time=J_time)
        x = _vec(hh.dofs_distr, rng.rand(hh.N, hh.M))
        try:
            y_two, p_whole = _np(hh.S @ x), _np(hh.P @ x)
            p_ranges = cac_by_column_ranges(hh, x)
            stk.check(lib.stk_set_tuning(b'mg_zero_start', 0))
            p_ranges_memset = cac_by_column_ranges(hh, x)
            stk.check(lib.stk_set_tuning(b'mg_zero_start', 1))
            hm.SchurMPI.two_streams = False
            x._invalidate()
            y_one = _np(hh.S @ x)
        finally:
            hm.SchurMPI.two_streams = True
            stk.check(lib.stk_set_tuning(b'mg_zero_start', 1))
        assert np.array_equal(y_two, y_one), J_time
        assert np.array_equal(p_ranges, p_whole), J_time
        assert np.array_equal(p_ranges_memset, p_whole), J_time


def test_strip_wise_sweeps_are_exact(stk):
    """Smoothing run strip by strip (ALL sweeps and dependency groups on one
    strip of bands before the next, every stage shifted by one band: mg.hip)
    updates every row from exactly the same values as level-wide group passes:
    bitwise the same V-cycle.  Strip widths from a few wide strips down to strips
    thinner than the skew of their stages; the plan must really have taken the
    strip path (launch counter), on the cube too."""
    import heateq_mpi as hm
    # (the cube needs J_space = 4: its 15^3 level runs inside the fused coarse kernel)
    for problem, J_space in (('square', 6), ('lshape', 5), ('cube', 4)):
        h = hm.HeatEquationMPI(J_space=J_space, J_time=3, problem=problem)
        x = _vec(h.dofs_distr, np.random.RandomState(14).rand(h.N, h.M))
        res = []
        try:
            # level working sets here are a few MB: strip_mb = 1 gives several
            # strips; width 0 lifts the lower bound on a strip's width
            for strip_mb, width in ((0, 2), (1, 2), (1, 0), (2, 1)):
                stk.check(stk.lib().stk_set_tuning(b'mg_strip_mb', strip_mb))
                stk.check(stk.lib().stk_set_tuning(b'mg_strip_width', width))
                stk.check(stk.lib().stk_set_tuning(b'mg_strips_used', 0))
                res.append((_np(h.P @ x), _np(h.S @ x)))
                if strip_mb == 1 and (width == 0 or problem != 'cube'):
                    # at least two strips of >= 3 stages ran from a strip table
                    rc = stk.lib().stk_set_tuning(b'mg_strips_used', 6)
                    assert rc == 0, (problem, strip_mb, width,
                                     stk.lib().stk_last_error().decode())
        finally:
            stk.check(stk.lib().stk_set_tuning(b'mg_strip_mb', 250))
            stk.check(stk.lib().stk_set_tuning(b'mg_strip_width', 2))
        for Pv, Sv in res[1:]:
            assert np.array_equal(Pv, res[0][0]) and np.array_equal(Sv, res[0][1])


def test_band_merge_does_not_change_a_bit(stk):
    """Bands of several mesh rows for the strip-wise sweeps (MultiGridFamily(band_merge);
    ADVICE r5): coarser bands keep "coupled
    rows at most one band apart", so the V-cycle is the same to the bit for merge = 1, 6
    and 64, at two slab lengths, from the Python planner and from the C planner -- and
    the fine levels still run strip by strip (launch counter) unless the merge leaves
    fewer than two bands."""
    from source.assembly import space_matrices
    from source.multigrid import MeshHierarchy, MultiGridFamily
    from source.problem import problem_helper
    mesh = problem_helper('square', J_space=6, J_time=2)[0]
    M_x, A_x = space_matrices(mesh)
    hier = MeshHierarchy(mesh)
    cms = [1.0, 2.0, 4.0, 8.0]
    rng = np.random.RandomState(21)
    lib = stk.lib()
    try:
        stk.check(lib.stk_set_tuning(b'mg_strip_mb', 1))  # several strips on a 16 129-row level
        stk.check(lib.stk_set_tuning(b'mg_strip_width', 0))
        for n_loc in (9, 34):
            X = rng.rand(A_x.shape[0], n_loc)
            x = torch.zeros((A_x.shape[0], n_loc + (n_loc & 1)), dtype=torch.float64, device='cuda')
            x[:, :n_loc] = torch.from_numpy(X).cuda()
            members = [k % len(cms) for k in range(n_loc)]
            out = {}
            for merge in (1, 6, 64):
                fam = MultiGridFamily(A_x, M_x, hier, ca=0.3, cms=cms, smoothsteps=3, vcycles=2, band_merge=merge)
                cm, kind = fam.slice_tables(members)
                stk.check(lib.stk_set_tuning(b'mg_strips_used', 0))
                out[merge] = fam.apply(x, n_loc=n_loc, cm=cm, kind=kind).clone()
                if merge <= 6:  # 127 mesh rows: 127 / 21 bands, strips of several bands
                    assert lib.stk_set_tuning(b'mg_strips_used', 6) == 0, (merge, lib.stk_last_error().decode())
            assert torch.equal(out[1], out[6]) and torch.equal(out[1], out[64]), n_loc
    finally:
        stk.check(lib.stk_set_tuning(b'mg_strip_mb', 250))
        stk.check(lib.stk_set_tuning(b'mg_strip_width', 2))


def test_family_members_run_on_their_own_coarse_matrices(stk):
    """MultiGridFamily(exact_coarse=True): the coarse end of the batched V-cycle runs, for
    every time slice, on the Galerkin chain of THAT slice's assembled matrix cm M + ca A
    -- what the reference builds one MultiGrid per wavelet level from
    (heateq_mpi.py:97-98, 147-153) -- instead of the combination of the two shared
    chains (member_chains, stk_mg_set_member_matrices).  The chains formed on the device
    are bit for bit SciPy's R @ C @ P chains (after the noise drop); with them a member's
    V-cycle agrees with MultiGrid(assembled matrix) far better than with the combination
    wherever the hierarchy is deep enough for the difference to show (it grows fourfold
    per level down)."""
    from source.assembly import space_matrices
    from source.multigrid import (MeshHierarchy, MultiGrid, MultiGridFamily, _drop_roundoff,
                                  member_chains)
    from source.problem import problem_helper
    rng = np.random.RandomState(4)
    for problem, J_space in (('square', 5), ('lshape', 5), ('square', 7)):
        mesh = problem_helper(problem, J_space=J_space, J_time=2)[0]
        M_x, A_x = space_matrices(mesh)
        hier = MeshHierarchy(mesh)
        ca, cms = 0.3, [1.0, 8.0, 128.0]
        chains = member_chains(hier, A_x, M_x, ca, cms)
        assert chains is not None
        for k, cm in enumerate(cms):
            C = sp.csr_matrix(cm * M_x + ca * A_x)
            for j in reversed(range(hier.J)):
                C = sp.csr_matrix(hier.R_mats[j] @ C @ hier.P_mats[j])
                C.sort_indices()
                C = _drop_roundoff(C)
                if j in chains[k]:
                    got = chains[k][j]
                    assert np.array_equal(got.indptr, C.indptr) and np.array_equal(got.indices, C.indices)
                    assert np.array_equal(got.data, C.data), (problem, k, j)
            assert 0 in chains[k] and 1 in chains[k]
        n = A_x.shape[0]
        x = torch.zeros((n, 6), dtype=torch.float64, device='cuda')
        x[:, :5] = torch.from_numpy(rng.rand(n, 5)).cuda()
        devs = {}
        for exact in (False, True):
            fam = MultiGridFamily(A_x, M_x, hier, ca=ca, cms=cms, smoothsteps=3, vcycles=2,
                                  fuse_restrict=False, gs_rows='full', exact_coarse=exact)
            worst = 0.0
            for k, cm in enumerate(cms):
                ref = MultiGrid(sp.csr_matrix(cm * M_x + ca * A_x), hier, smoothsteps=3, vcycles=2,
                                fuse_restrict=False, gs_rows='full')
                y = fam.members[k].apply(x, n_loc=5)
                yr = ref.apply(x, n_loc=5)
                worst = max(worst, float((y - yr).abs().max() / yr.abs().max()))
            assert fam._dev.member_levels == (min(hier.J - 1, 5) if exact else 0), fam._dev.member_levels
            devs[exact] = worst
        # every coarse level inside the fused kernel: nothing but the members' own matrices
        # is left below the finest level, which is the assembled matrix in both
        if hier.J - 1 <= 5:
            assert devs[True] == 0.0, (problem, J_space, devs)
        else:
            assert devs[True] < 0.3 * devs[False], (problem, J_space, devs)
        _scalar_dev('family_member_vs_assembled_%s_J%d' % (problem, J_space), devs[True], 1e-12)


def test_coupling_bands_are_verified(stk):
    """The bands the strip-wise smoothing relies on (coupled rows at most one
    band apart) are checked on the pattern: a matrix with a long-range entry
    loses its banding (coarser bands, or none) instead of silently breaking the
    sweep order, and the V-cycle stays the oracle's."""
    from oracle.multigrid import MultiGrid as OracleMG
    from source.assembly import prolongation_matrices, space_matrices
    from source.multigrid import MeshHierarchy, MultiGrid, coupling_bands
    from source.problem import problem_helper
    mesh = problem_helper('square', J_space=5, J_time=2)[0]
    M_x, A_x = space_matrices(mesh)
    n = A_x.shape[0]
    hier = MeshHierarchy(mesh)
    band = coupling_bands(hier.coords, A_x.indptr, A_x.indices)
    assert band is not None and band.max() + 1 == 63  # the mesh rows
    # couple the first and the last dof: no thin banding along y survives
    B = sp.lil_matrix(A_x)
    far = int(np.argmax(hier.coords[:n, -1]))
    near = int(np.argmin(hier.coords[:n, -1]))
    B[near, far] = B[far, near] = -1e-3
    B = sp.csr_matrix(B)
    b2 = coupling_bands(hier.coords, B.indptr, B.indices)
    rows_of = np.repeat(np.arange(n), np.diff(B.indptr))
    assert b2 is None or np.abs(b2[rows_of] - b2[B.indices]).max() <= 1
    try:
        stk.check(stk.lib().stk_set_tuning(b'mg_strip_mb', 1))
        stk.check(stk.lib().stk_set_tuning(b'mg_strip_width', 0))
        mg = MultiGrid(B, hier, smoothsteps=3, vcycles=2)
        F = np.random.RandomState(3).rand(n, 6)
        got = (mg @ F)
    finally:
        stk.check(stk.lib().stk_set_tuning(b'mg_strip_mb', 250))
        stk.check(stk.lib().stk_set_tuning(b'mg_strip_width', 2))
    want = OracleMG(B, prolongation_matrices(mesh), 3, 2) @ F
    assert relerr(got, want) < 1e-12


def _decode_blob(text):
    """The reference's result record: base64(zlib(pickle(per-rank list)))
    printed as 'data: ...' (heateq_mpi.py:308-312, heateq_mpi_timing.py:124-128)."""
    import base64
    import pickle
    import zlib
    line = [ln for ln in text.splitlines() if ln.startswith('data: ')][-1]
    return pickle.loads(zlib.decompress(base64.b64decode(line[len('data: '):])))


def test_driver_telemetry_records(stk, capsys):
    """Row f3: the timing driver and the solve driver print the reference's
    fields and gather the per-rank record into the base64 blob (reference
    heateq_mpi_timing.py:62-128, heateq_mpi.py:259-312).  The blob is decoded and
    its per-operator keys, apply counts and timings (HIP events on the launch
    stream) are checked."""
    import heateq_mpi
    import heateq_mpi_timing
    from source.mpi_kron import LinearOperatorMPI
    iters = 3
    try:
        heateq_mpi_timing.main(['--J_time=3', '--J_space=3', '--iters=%d' % iters])
        out = capsys.readouterr().out
        for field in ('Creating mesh with 3 time refines and 3 space refines.',
                      'N = 9. M = 225.', 'Constructed bilinear forms in',
                      'Completed %d iters steps.' % iters, 'Total time:'):
            assert field in out, field
        for name in ('W:  ', 'S:  ', 'WT: ', 'P:  '):  # print_time_per_apply
            assert name in out
        ranks = _decode_blob(out)
        assert len(ranks) == 1 and ranks[0]['rank'] == 0
        rec = ranks[0]
        assert rec['time_total'] > 0 and rec['mem_after_timing'] > 0
        for name in ('W', 'S', 'WT', 'P'):
            r = rec[name]
            assert sorted(r) == ['num_applies', 'time_applies', 'time_applies_iter',
                                 'time_communication', 'time_communication_iter',
                                 'time_total']
            assert r['num_applies'] == iters
            assert len(r['time_applies_iter']) == iters == len(r['time_communication_iter'])
            assert all(t > 0 for t in r['time_applies_iter'])
            assert abs(sum(r['time_applies_iter']) - r['time_applies']) < 1e-9
            assert r['time_communication'] == 0  # one rank: no halo
            assert r['time_total'] >= r['time_applies']
        # device times: S (two multigrid applies inside) costs more than W
        assert rec['S']['time_applies'] > rec['W']['time_applies']

        h, w, its, hist = heateq_mpi.main(['--J_time=3', '--J_space=3'])
        out = capsys.readouterr().out
        assert 'Completed in %d PCG steps.' % its in out and 'Total solve time:' in out
        rec = _decode_blob(out)[0]
        assert rec['iters'] == its and len(rec['r_dot_Pr']) == its + 1
        assert rec['N'] == 9 and rec['M'] == 225 and rec['args']['J_time'] == 3
        assert rec['solve_time'] > 0 and rec['mem_after_solve'] > 0
        # PCG applies T once for the initial residual and once per iteration; P alike
        # (reference linalg.py:20-34)
        for name in ('W', 'S', 'WT', 'WT_S_W', 'P'):
            assert rec[name]['num_applies'] == its + 1, (name, rec[name])
            assert rec[name]['time_applies'] > 0
        assert rec['WT_S_W']['time_applies'] >= rec['S']['time_applies']
    finally:
        LinearOperatorMPI.sync_timing = False


def test_kron_plan_from_csr_through_ctypes_only(stk):
    """Row b: the fast path without any Python planner.  stk_kron_plan_create
    gets the host CSR arrays of the factors (and a row order), builds union
    pattern, sliced ELL, dictionary and packed words inside libstk, and
    stk_kron_plan_apply runs the operator -- only ctypes calls and device
    buffers here.  Against dense NumPy, and bit for bit against the Python-planned
    forms; matrices with too many distinct values / over-long rows take the plain
    ELL form inside the same call."""
    import ctypes
    from source.linop import EllMatrices
    lib = stk.lib()
    rng = np.random.RandomState(99)
    for case in range(12):
        M = int(rng.randint(5, 500))
        n_loc = int(rng.choice([1, 4, 9, 16, 33]))
        ld = n_loc + (n_loc & 1)
        n_mats = int(rng.randint(1, 4))
        width = int(rng.choice([3, 6, 9, 14, 20]))  # 20: overflow rows
        base = sp.csr_matrix(sp.random(M, M, density=min(1.0, width / M),
                                       random_state=rng, format='csr') + sp.eye(M))
        few = case % 2 == 0  # dictionary-sized value sets on even cases
        palette = rng.randn(5)
        mats = []
        for k in range(n_mats):
            m = base.copy()
            m.data = (palette[rng.randint(5, size=m.nnz)] if few else rng.rand(m.nnz))
            if k == 1:  # patterns differ: drop some entries of the second matrix
                m.data[rng.rand(m.nnz) < 0.3] = 0.0
                m.eliminate_zeros()
            m.sort_indices()
            mats.append(m)
        order = rng.permutation(M).astype(np.int32) if case % 3 else None
        keep = [(m.indptr.astype(np.int32), m.indices.astype(np.int32),
                 m.data.astype(np.float64)) for m in mats]
        arr = lambda j: (ctypes.c_void_p * n_mats)(*[k[j].ctypes.data for k in keep])
        plan = ctypes.c_void_p()
        stk.check(lib.stk_kron_plan_create(
            M, n_mats, arr(0), arr(1), arr(2),
            None if order is None else order.ctypes.data, ctypes.byref(plan)))
        K, nc, packed = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        nnz = ctypes.c_int64()
        rpu = ctypes.c_int32()
        stk.check(lib.stk_kron_plan_info(plan, ctypes.byref(K), ctypes.byref(nc),
                                         ctypes.byref(packed), ctypes.byref(nnz),
                                         ctypes.byref(rpu)))
        pattern = sum(sp.csr_matrix((np.ones(m.nnz), m.indices, m.indptr), shape=m.shape)
                      for m in mats)
        assert nnz.value == sp.csr_matrix(pattern).nnz
        nt = int(rng.randint(1, 4))
        X, y0 = rng.rand(M, n_loc), rng.rand(M, n_loc)
        lo = rng.rand(M) if rng.randint(2) else None
        hi = rng.rand(M) if rng.randint(2) else None
        beta = float(rng.choice([0.0, 0.5]))
        terms = (stk.KronPackTerm * nt)()
        want, keep_tri = beta * y0, []
        for k in range(nt):
            mat = int(rng.randint(n_mats))
            t = rng.rand(3, n_loc)
            T = np.diag(t[1]) + np.diag(t[0, 1:], -1) + np.diag(t[2, :-1], 1)
            dev = _lib_dev(t)
            keep_tri.append(dev)
            terms[k].tri, terms[k].mat = dev.data_ptr(), mat
            want = want + (mats[mat] @ X) @ T.T
            if lo is not None:
                want[:, 0] += t[0, 0] * (mats[mat] @ lo)
            if hi is not None:
                want[:, -1] += t[2, -1] * (mats[mat] @ hi)

        def slab(a):
            s_ = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
            s_[:, :n_loc] = torch.from_numpy(a).cuda()
            return s_

        x, y = slab(X), slab(y0)
        glo = None if lo is None else torch.from_numpy(lo).cuda()
        ghi = None if hi is None else torch.from_numpy(hi).cuda()
        work = torch.empty((M, 2), dtype=torch.float64, device='cuda')
        stk.check(lib.stk_kron_plan_apply(plan, stk.stream(), n_loc, ld, nt, terms,
                                          stk.ptr(x), stk.ptr(glo), stk.ptr(ghi),
                                          stk.ptr(work), beta, stk.ptr(y)))
        got = y[:, :n_loc].cpu().numpy()
        assert relerr(got, want) < 1e-13, (case, M, n_loc, n_mats, width, few)
        if ld > n_loc:
            assert float(y[:, n_loc:].abs().max()) == 0.0
        # the Python-planned form of the same matrices, same row order
        if order is not None:
            for m in mats:
                m.stk_row_order = order
        ell = EllMatrices(mats)
        assert ell.K == K.value and ell.packed.ok == bool(packed.value)
        if ell.packed.ok:  # both planners pair the same rows
            assert ell.packed.rows_per_unit == rpu.value, (case, rpu.value)
        y_py = slab(y0)
        specs = [(keep_tri[k], terms[k].mat) for k in range(nt)]
        if ell.packed.ok:
            gh = None
            if glo is not None or ghi is not None:
                gh = torch.empty((M, 2), dtype=torch.float64, device='cuda')
                stk.check(lib.stk_interleave_ghosts(stk.stream(), M, stk.ptr(glo),
                                                    stk.ptr(ghi), stk.ptr(gh)))
            ell.packed.apply(specs, x, gh, n_loc, ld, beta, y_py)
        else:
            ell.apply([(tri, k, x, glo, ghi) for tri, k in specs], n_loc, ld, beta, y_py)
        assert torch.equal(y, y_py), (case, float((y - y_py).abs().max()))
        stk.check(lib.stk_kron_plan_destroy(plan))
    # mesh matrices in their tile order: the library pairs neighbouring rows, and
    # keeps one row per slot row when told to ("pack_rows"); same bits either way
    from source.assembly import space_matrices
    from source.problem import problem_helper
    M_x, A_x = space_matrices(problem_helper('lshape', J_space=3, J_time=2)[0])
    order = np.asarray(M_x.stk_row_order, dtype=np.int32)
    mats = [sp.csr_matrix(M_x), sp.csr_matrix(A_x)]
    for m in mats:
        m.sort_indices()
    keep = [(m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.astype(np.float64))
            for m in mats]
    arr = lambda j: (ctypes.c_void_p * 2)(*[k[j].ctypes.data for k in keep])
    M, n_loc, ld = M_x.shape[0], 33, 34  # long enough for the plan to use its pair form
    x = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
    x[:, :n_loc] = torch.from_numpy(rng.rand(M, n_loc)).cuda()
    t = [_lib_dev(rng.rand(3, n_loc)) for _ in range(2)]
    terms = (stk.KronPackTerm * 2)()
    for k in range(2):
        terms[k].tri, terms[k].mat = t[k].data_ptr(), k
    out = {}
    for rows in (2, 1):
        stk.check(lib.stk_set_tuning(b'pack_rows', rows))
        plan = ctypes.c_void_p()
        stk.check(lib.stk_kron_plan_create(M, 2, arr(0), arr(1), arr(2), order.ctypes.data,
                                           ctypes.byref(plan)))
        rpu, K = ctypes.c_int32(), ctypes.c_int32()
        stk.check(lib.stk_kron_plan_info(plan, ctypes.byref(K), None, None, None, ctypes.byref(rpu)))
        assert rpu.value == rows and K.value == 7
        y = torch.full_like(x, 9.0)
        stk.check(lib.stk_kron_plan_apply(plan, stk.stream(), n_loc, ld, 2, terms, stk.ptr(x),
                                          None, None, None, 0.0, stk.ptr(y)))
        out[rows] = y
        stk.check(lib.stk_kron_plan_destroy(plan))
    stk.check(lib.stk_set_tuning(b'pack_rows', 2))
    assert torch.equal(out[1], out[2])
    ell = EllMatrices([M_x, A_x], [M_x])
    y_py = torch.full_like(x, 4.0)
    ell.packed.apply([(t[0], 0), (t[1], 1)], x, None, n_loc, ld, 0.0, y_py)
    assert ell.packed.rows_per_unit == 2 and torch.equal(out[2], y_py)
    # argument errors come back as status + message, not as a crash
    plan = ctypes.c_void_p()
    bad = np.array([0, 0, 1], dtype=np.int32)  # not a permutation
    m = sp.identity(3, format='csr')
    ip, ix, dv = m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data
    one = lambda a: (ctypes.c_void_p * 1)(a.ctypes.data)
    assert lib.stk_kron_plan_create(3, 1, one(ip), one(ix), one(dv), bad.ctypes.data,
                                    ctypes.byref(plan)) != 0
    assert b'permutation' in lib.stk_last_error()


def test_kron_plan_without_dictionary_through_ctypes_only(stk):
    """stk_kron_plan_create on matrices whose values do not repeat (jittered
    L-shape): the C planner reports no dictionary but row pairs (explicit values),
    and stk_kron_plan_apply / _ghost_apply agree with dense NumPy and, bit for bit,
    with the Python-planned explicit form -- for a subset and a permutation of the
    plan's matrices as terms, with and without ghost rows, long and short slabs."""
    import ctypes
    from source.assembly import space_matrices
    from source.linop import EllMatrices
    from source.problem import problem_helper
    lib = stk.lib()
    rng = np.random.RandomState(99)
    M_x, A_x = space_matrices(problem_helper('lshape_jitter', J_space=3, J_time=2)[0])
    mats = [sp.csr_matrix(m) for m in (M_x, A_x, M_x + 0.5 * A_x)]
    M = M_x.shape[0]
    keep = [(m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.astype(np.float64)) for m in mats]
    arr = lambda j: (ctypes.c_void_p * len(mats))(*[k[j].ctypes.data for k in keep])
    order = np.asarray(M_x.stk_row_order, dtype=np.int32)
    plan = ctypes.c_void_p()
    stk.check(lib.stk_kron_plan_create(M, len(mats), arr(0), arr(1), arr(2), order.ctypes.data, ctypes.byref(plan)))
    K, codes, packed, rpu = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    stk.check(lib.stk_kron_plan_info(plan, ctypes.byref(K), ctypes.byref(codes), ctypes.byref(packed), None,
                                     ctypes.byref(rpu)))
    assert packed.value == 0 and rpu.value == 2 and K.value == 7
    try:
        for n_loc, use in [(33, (0, 1)), (65, (2, 0)), (24, (1,)), (40, (0, 1, 2)), (9, (0, 1))]:
            ld = n_loc + (n_loc & 1)
            X = rng.rand(M, n_loc)
            lo, hi = rng.rand(M), rng.rand(M)
            x = torch.zeros((M, ld), dtype=torch.float64, device='cuda')
            x[:, :n_loc] = torch.from_numpy(X).cuda()
            d_lo, d_hi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
            work = torch.empty((M, 2), dtype=torch.float64, device='cuda')
            tris, terms = [], (stk.KronPackTerm * len(use))()
            want = np.zeros((M, n_loc))
            for k, m in enumerate(use):
                t = rng.rand(3, n_loc)
                T = np.diag(t[1]) + np.diag(t[0, 1:], -1) + np.diag(t[2, :-1], 1)
                want += (mats[m] @ X) @ T.T
                want[:, 0] += t[0, 0] * (mats[m] @ lo)
                want[:, -1] += t[2, -1] * (mats[m] @ hi)
                tris.append(_lib_dev(t))
                terms[k].tri, terms[k].mat = stk.ptr(tris[-1]), m
            y = torch.full((M, ld), float('nan'), dtype=torch.float64, device='cuda')
            stk.check(lib.stk_kron_plan_apply(plan, stk.stream(), n_loc, ld, len(use), terms, stk.ptr(x),
                                              stk.ptr(d_lo), stk.ptr(d_hi), stk.ptr(work), 0.0, stk.ptr(y)))
            assert relerr(y[:, :n_loc].cpu().numpy(), want) < 1e-13, (n_loc, use)
            # the overlapped form: without ghost rows, then their share
            y2 = torch.full((M, ld), float('nan'), dtype=torch.float64, device='cuda')
            stk.check(lib.stk_kron_plan_apply(plan, stk.stream(), n_loc, ld, len(use), terms, stk.ptr(x), None,
                                              None, None, 0.0, stk.ptr(y2)))
            stk.check(lib.stk_kron_plan_ghost_apply(plan, stk.stream(), n_loc, ld, len(use), terms, stk.ptr(x),
                                                    stk.ptr(d_lo), stk.ptr(d_hi), stk.ptr(y2)))
            assert relerr(y2[:, :n_loc].cpu().numpy(), want) < 1e-13, (n_loc, use)
            assert torch.equal(y2, y)  # pass + boundary steps = the call with the received rows, bit for bit
            # ... and the boundary steps from the records of the pack kernel (the fast form;
            # the slab form again on plans without a packed stream)
            rec = torch.empty((M, 4), dtype=torch.float64, device='cuda')
            stk.check(lib.stk_halo_pack_records(stk.stream(), M, n_loc, ld, stk.ptr(x), None, 1, None, 1,
                                                stk.ptr(rec)))
            y2r = torch.full((M, ld), float('nan'), dtype=torch.float64, device='cuda')
            stk.check(lib.stk_kron_plan_apply(plan, stk.stream(), n_loc, ld, len(use), terms, stk.ptr(x), None,
                                              None, None, 0.0, stk.ptr(y2r)))
            stk.check(lib.stk_kron_plan_boundary_apply(plan, stk.stream(), n_loc, ld, len(use), terms, stk.ptr(x),
                                                       stk.ptr(rec), stk.ptr(d_lo), stk.ptr(d_hi), stk.ptr(work),
                                                       stk.ptr(y2r)))
            assert torch.equal(y2r, y), (n_loc, use)
            if n_loc >= 24:  # the Python planner's explicit pairs: the same kernel on the same arrays
                ell = EllMatrices([mats[m] for m in use], [M_x])
                two = ell.packed_variant(2)
                assert two.ok and two.explicit
                gh = torch.stack([d_lo, d_hi], dim=1).contiguous()
                y3 = torch.empty_like(y)
                two.apply([(tris[k], k) for k in range(len(use))], x, gh, n_loc, ld, 0.0, y3)
                assert torch.equal(y, y3), (n_loc, use)
    finally:
        stk.check(lib.stk_kron_plan_destroy(plan))


def test_multigrid_plan_from_csr_through_ctypes_only(stk):
    """Row b / f1: the multigrid plan without any Python planner.
    stk_mg_create_from_csr gets the finest-level CSR matrices and the
    prolongations as host arrays, forms the Galerkin products, schedules, ELL
    copies, bands and coarse inverses inside libstk; stk_mg_apply then runs the
    V-cycles.  Only ctypes calls and device buffers here.  Against the CPU
    oracle's MultiGrid, and against the Python-planned plan of the same inputs;
    single matrix (K = A^-1) and family (2^j M + alpha A), with and without
    coordinates (breadth-first bands), strip-wise smoothing forced on."""
    import ctypes
    from oracle.multigrid import MultiGrid as OracleMG
    from source.assembly import prolongation_matrices, space_matrices
    from source.multigrid import MeshHierarchy, MultiGrid, MultiGridFamily
    from source.problem import problem_helper
    lib = stk.lib()

    def host(m):
        m = sp.csr_matrix(m)
        m.sort_indices()
        arrs = (m.indptr.astype(np.int32), m.indices.astype(np.int32),
                m.data.astype(np.float64))
        return stk.CsrHost(m.shape[0], m.shape[1], arrs[0].ctypes.data,
                           arrs[1].ctypes.data, arrs[2].ctypes.data), arrs

    for problem, J_space in (('square', 4), ('lshape', 3), ('cube', 2)):
        mesh = problem_helper(problem, J_space=J_space, J_time=2)[0]
        M_x, A_x = space_matrices(mesh)
        hier = MeshHierarchy(mesh)
        P_mats = prolongation_matrices(mesh)
        n = A_x.shape[0]
        n_loc, ld = 7, 8
        F = np.random.RandomState(31).rand(n, n_loc)
        f = torch.zeros((n, ld), dtype=torch.float64, device='cuda')
        f[:, :n_loc] = torch.from_numpy(F).cuda()
        coords = np.ascontiguousarray(hier.coords, dtype=np.float64)
        Ps = [host(P) for P in P_mats]
        P_arr = (stk.CsrHost * len(Ps))(*[p[0] for p in Ps])
        a_h, a_keep = host(A_x)
        m_h, m_keep = host(M_x)
        try:
            stk.check(lib.stk_set_tuning(b'mg_strip_mb', 1))
            stk.check(lib.stk_set_tuning(b'mg_strip_width', 0))
            for with_coords in (True, False):
                # --- one matrix: K = MultiGrid(A_x), 3 sweeps, 2 V-cycles
                plan = ctypes.c_void_p()
                stk.check(lib.stk_mg_create_from_csr(
                    len(P_mats) + 1, ctypes.byref(a_h), None, P_arr,
                    coords.ctypes.data if with_coords else None, coords.shape[1],
                    3, 2, 1.0, 0, None, ld, ctypes.byref(plan)))
                u = torch.empty_like(f)
                stk.check(lib.stk_mg_apply(plan, stk.stream(), n_loc, ld, 1.0, None,
                                           None, stk.ptr(f), stk.ptr(u)))
                got = u[:, :n_loc].cpu().numpy()
                want = OracleMG(A_x, P_mats, 3, 2) @ F
                assert relerr(got, want) < 1e-12, (problem, with_coords)
                # the Python-planned plan on the SAME slab (`op @ F` would upload an
                # (n, 7) slab, and an odd row stride takes the flat CSR kernels, whose
                # sums run in another order)
                py = MultiGrid(A_x, hier, smoothsteps=3, vcycles=2).apply(f, n_loc=n_loc)[:, :n_loc].cpu().numpy()
                assert relerr(got, py) < 1e-13, (problem, with_coords)
                # (the Galerkin matrices, schedules and ELL copies of the two planners
                # agree bit for bit; the coarsest level's dense inverse comes from LAPACK
                # in one and from Gauss-Jordan in the other -- the same for a 1 x 1 level 0)
                if A_x.shape[0] and hier.P_mats[0].shape[1] == 1:
                    assert np.array_equal(got, py), (problem, with_coords)
                stk.check(lib.stk_mg_destroy(plan))
                # ... and with the caller's inverse handed over (stk_mg_set_coarse_inverse:
                # numpy.linalg.inv, what the Python planner takes) the two planners'
                # V-cycles are EQUAL
                INV = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int32, ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(ctypes.c_double), ctypes.c_void_p)

                def lapack_inverse(n0, a_ptr, inv_ptr, user):
                    a = np.ctypeslib.as_array(a_ptr, shape=(n0, n0))
                    np.ctypeslib.as_array(inv_ptr, shape=(n0, n0))[...] = np.linalg.inv(a)
                    return 0

                hook = INV(lapack_inverse)
                stk.check(lib.stk_mg_set_coarse_inverse(ctypes.cast(hook, ctypes.c_void_p), None))
                try:
                    plan = ctypes.c_void_p()
                    stk.check(lib.stk_mg_create_from_csr(
                        len(P_mats) + 1, ctypes.byref(a_h), None, P_arr,
                        coords.ctypes.data if with_coords else None, coords.shape[1],
                        3, 2, 1.0, 0, None, ld, ctypes.byref(plan)))
                finally:
                    stk.check(lib.stk_mg_set_coarse_inverse(None, None))
                u_eq = torch.empty_like(f)
                stk.check(lib.stk_mg_apply(plan, stk.stream(), n_loc, ld, 1.0, None,
                                           None, stk.ptr(f), stk.ptr(u_eq)))
                assert np.array_equal(u_eq[:, :n_loc].cpu().numpy(), py), (problem, with_coords)
                stk.check(lib.stk_mg_destroy(plan))
                # --- the same plan with the default arithmetic of HeatEquationMPI
                # ('accurate'): Gauss-Seidel rows with their diagonal (plan-time key
                # "mg_gs_diag_free" = 0) and the restricted residual as R (A u - f)
                from source import multigrid as mgmod
                stk.check(lib.stk_set_tuning(b'mg_gs_diag_free', 0))
                try:
                    plan = ctypes.c_void_p()
                    stk.check(lib.stk_mg_create_from_csr(
                        len(P_mats) + 1, ctypes.byref(a_h), None, P_arr,
                        coords.ctypes.data if with_coords else None, coords.shape[1],
                        3, 2, 1.0, 0, None, ld, ctypes.byref(plan)))
                finally:
                    stk.check(lib.stk_set_tuning(b'mg_gs_diag_free', 1))
                stk.check(lib.stk_mg_set_option(plan, b'fuse_restrict', 0))
                u2 = torch.empty_like(f)
                stk.check(lib.stk_mg_apply(plan, stk.stream(), n_loc, ld, 1.0, None,
                                           None, stk.ptr(f), stk.ptr(u2)))
                got2 = u2[:, :n_loc].cpu().numpy()
                assert relerr(got2, want) < 1e-12, (problem, with_coords)
                assert not np.array_equal(got2, got)  # another arithmetic did run
                mgmod.GS_DIAG_FREE = False
                try:
                    py2 = MultiGrid(A_x, hier, smoothsteps=3, vcycles=2, fuse_restrict=False) @ F
                finally:
                    mgmod.GS_DIAG_FREE = True
                assert relerr(got2, py2) < 1e-13, (problem, with_coords)
                stk.check(lib.stk_mg_destroy(plan))
                # --- and with those forms only where the history's gap is owned: key 2
                # (finest level: rows with their diagonal + the diagonal-free copies as
                # the alternative form) and the plan options of the default arithmetic
                stk.check(lib.stk_set_tuning(b'mg_gs_diag_free', 2))
                try:
                    plan = ctypes.c_void_p()
                    stk.check(lib.stk_mg_create_from_csr(
                        len(P_mats) + 1, ctypes.byref(a_h), None, P_arr,
                        coords.ctypes.data if with_coords else None, coords.shape[1],
                        3, 2, 1.0, 0, None, ld, ctypes.byref(plan)))
                finally:
                    stk.check(lib.stk_set_tuning(b'mg_gs_diag_free', 1))
                for key, value in ((b'fuse_restrict_max_level', len(P_mats) - 1),
                                   (b'fast_until_cycle', 1), (b'fast_parts', 1)):
                    stk.check(lib.stk_mg_set_option(plan, key, value))
                u3 = torch.empty_like(f)
                stk.check(lib.stk_mg_apply(plan, stk.stream(), n_loc, ld, 1.0, None,
                                           None, stk.ptr(f), stk.ptr(u3)))
                got3 = u3[:, :n_loc].cpu().numpy()
                assert relerr(got3, want) < 1e-12, (problem, with_coords)
                assert not np.array_equal(got3, got) and not np.array_equal(got3, got2)
                # every V-cycle declared fast: the diagonal-free plan's result, bit for bit
                stk.check(lib.stk_mg_set_option(plan, b'fast_until_cycle', 2))
                stk.check(lib.stk_mg_apply(plan, stk.stream(), n_loc, ld, 1.0, None,
                                           None, stk.ptr(f), stk.ptr(u3)))
                assert np.array_equal(u3[:, :n_loc].cpu().numpy(), got), (problem, with_coords)
                stk.check(lib.stk_mg_destroy(plan))
                # --- a family: C_j = (2^j M + 0.3 A)^-1, per-slice coefficients
                cms = np.array([1.0, 2.0, 4.0])
                plan = ctypes.c_void_p()
                stk.check(lib.stk_mg_create_from_csr(
                    len(P_mats) + 1, ctypes.byref(a_h), ctypes.byref(m_h), P_arr,
                    coords.ctypes.data if with_coords else None, coords.shape[1],
                    3, 2, 0.3, len(cms), cms.ctypes.data, ld, ctypes.byref(plan)))
                member = [0, 1, 2, 1, 0, 2, 2]
                cm = stk.to_dev(cms[member])
                kind = stk.to_dev(np.array([k + 1 for k in member], dtype=np.int32))
                stk.check(lib.stk_mg_apply(plan, stk.stream(), n_loc, ld, 0.3,
                                           stk.ptr(cm), stk.ptr(kind), stk.ptr(f),
                                           stk.ptr(u)))
                got = u[:, :n_loc].cpu().numpy()
                for t, k in enumerate(member):
                    C = OracleMG(sp.csr_matrix(cms[k] * M_x + 0.3 * A_x), P_mats, 3, 2)
                    assert relerr(got[:, t], C @ F[:, t]) < 1e-12, (problem, t)
                stk.check(lib.stk_mg_destroy(plan))
        finally:
            stk.check(lib.stk_set_tuning(b'mg_strip_mb', 250))
            stk.check(lib.stk_set_tuning(b'mg_strip_width', 2))
    # a matrix without a diagonal entry is refused with a message
    bad, keep = host(sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 2.0]])))
    plan = ctypes.c_void_p()
    assert lib.stk_mg_create_from_csr(1, ctypes.byref(bad), None, None, None, 2, 1,
                                      1, 1.0, 0, None, 2, ctypes.byref(plan)) != 0
    assert b'diagonal' in lib.stk_last_error()


def test_slab_storage_through_ctypes_only(stk):
    """vector alloc / upload / download for a host that owns no
    device allocator (KronVectorMPI.__init__, scatter, gather:
    mpi_vector.py:62-71, 124-138), called through ctypes with host buffers and
    raw device pointers only -- no torch tensor involved -- and checked through a
    libstk kernel that consumes the slab (stk_axpby on the flat array)."""
    import ctypes
    lib = stk.lib()
    rng = np.random.RandomState(5)
    for M, n_loc in [(1, 1), (37, 9), (1000, 33), (4099, 64), (513, 65)]:
        ld, slab = ctypes.c_int32(), ctypes.c_void_p()
        stk.check(lib.stk_slab_alloc(M, n_loc, ctypes.byref(ld), ctypes.byref(slab)))
        assert ld.value == lib.stk_slab_ld(n_loc) == n_loc + (n_loc & 1)
        X = rng.rand(n_loc, M)
        stk.check(lib.stk_slab_upload(None, M, n_loc, ld.value, X.ctypes.data, slab))
        # y = 2 x + 0 y in place on the flat array: padding stays zero
        stk.check(lib.stk_axpby(None, M * ld.value, 2.0, slab, 0.0, slab))
        Y = np.full((n_loc, M), np.nan)
        stk.check(lib.stk_slab_download(None, M, n_loc, ld.value, slab, Y.ctypes.data))
        assert np.array_equal(Y, 2.0 * X)
        stk.check(lib.stk_slab_free(slab))
    assert lib.stk_slab_alloc(0, 3, ctypes.byref(ld), ctypes.byref(slab)) != 0


def test_byte_moving_kernels(stk):
    """stk_transpose (with zero padding), stk_halo_pack at strides 1 and 2,
    stk_slab_extract_time_rows, stk_copy_block and stk_outer against NumPy:
    pure data movement, bit-exact."""
    import torch
    lib = stk.lib()
    rng = np.random.RandomState(6)
    dev = stk.compute_device()
    for M, n_loc in [(5, 1), (130, 9), (1027, 33), (300, 65)]:
        ld = n_loc + (n_loc & 1)
        X = rng.rand(n_loc, M)
        src = torch.from_numpy(X).to(dev)
        slab = torch.full((M, ld), float('nan'), dtype=torch.float64, device=dev)
        stk.transpose(src, n_loc, M, M, slab, ld, zero_to=ld)
        want = np.zeros((M, ld))
        want[:, :n_loc] = X.T
        assert np.array_equal(slab.cpu().numpy(), want)
        back = torch.empty((n_loc, M), dtype=torch.float64, device=dev)
        stk.transpose(slab, M, n_loc, ld, back, M)
        assert np.array_equal(back.cpu().numpy(), X)
        # halo rows: contiguous, and interleaved into a ghost buffer
        send = torch.zeros((2, M), dtype=torch.float64, device=dev)
        stk.check(lib.stk_halo_pack(stk.stream(), M, n_loc, ld, stk.ptr(slab),
                                    stk.ptr(send[0]), 1, stk.ptr(send[1]), 1))
        assert np.array_equal(send.cpu().numpy(), X[[0, n_loc - 1]])
        gh = torch.zeros((M, 2), dtype=torch.float64, device=dev)
        # as a neighbour pair would: my LAST row is the upper rank's lo entry,
        # my FIRST row the lower rank's hi entry
        stk.check(lib.stk_halo_pack(stk.stream(), M, n_loc, ld, stk.ptr(slab),
                                    stk.ptr(gh) + 8, 2, stk.ptr(gh), 2))
        assert np.array_equal(gh.cpu().numpy(), np.stack([X[n_loc - 1], X[0]], axis=1))
        only = torch.zeros(M, dtype=torch.float64, device=dev)
        stk.check(lib.stk_halo_pack(stk.stream(), M, n_loc, ld, stk.ptr(slab), None, 1,
                                    stk.ptr(only), 1))
        assert np.array_equal(only.cpu().numpy(), X[n_loc - 1])
        rows = sorted(set(int(t) for t in rng.randint(0, n_loc, size=3)))
        idx = stk.to_dev(np.asarray(rows, dtype=np.int32))
        out = torch.empty((len(rows), M), dtype=torch.float64, device=dev)
        stk.check(lib.stk_slab_extract_time_rows(stk.stream(), M, len(rows), stk.ptr(idx),
                                                 stk.ptr(slab), ld, stk.ptr(out), M))
        assert np.array_equal(out.cpu().numpy(), X[rows])
        # a block of rows to another leading dimension
        r0, r1, nc = M // 3, M, max(1, n_loc - 1)
        blk = torch.zeros((r1 - r0, nc + 3), dtype=torch.float64, device=dev)
        stk.copy_block(slab, r1 - r0, nc, ld, blk, nc + 3, src_off=r0 * ld)
        assert np.array_equal(blk.cpu().numpy()[:, :nc], want[r0:r1, :nc])
        assert not blk.cpu().numpy()[:, nc:].any()
        u_t, u_x = rng.rand(n_loc), rng.rand(M)
        y = torch.full((M, ld), float('nan'), dtype=torch.float64, device=dev)
        d_t, d_x = stk.to_dev(u_t), stk.to_dev(u_x)  # kept alive across the launch
        stk.check(lib.stk_outer(stk.stream(), M, n_loc, ld, stk.ptr(d_t), stk.ptr(d_x),
                                stk.ptr(y)))
        wy = np.zeros((M, ld))
        wy[:, :n_loc] = np.kron(u_t, u_x).reshape(n_loc, M).T
        assert np.array_equal(y.cpu().numpy(), wy)
    assert lib.stk_halo_pack(stk.stream(), 4, 2, 2, stk.ptr(slab), None, 1, None, 1) != 0


def test_direct_inverse_above_the_dense_limit(stk):
    """InvLinOp on systems too large for a dense inverse (reference linop.py:18-26 is
    size-agnostic SuperLU): SuperLU's factors applied ON THE DEVICE -- permutations
    and the two level-scheduled triangular solves of stk_lu_solve, all time steps at
    once -- against SciPy's solve of the same factorisation; the columns of the result
    do not depend on the slab length (one shape of every row's sum); the host
    round trip of rounds 1-5 (host_solve) still returns SciPy's doubles.  Square at
    J_space = 6 (M = 16 129: config 1's size) and the L-shape (M = 12 033); then the
    whole solve of config 1 with precond='direct' (reference heateq_mpi.py:154-157,
    heateq_mpi_test.py:66-135) against the oracle's direct trajectory."""
    from scipy.sparse.linalg import splu
    from source.assembly import space_matrices
    from source.linop import InvLinOp
    from source.problem import problem_helper
    rng = np.random.RandomState(11)
    for problem, coef in (('square', 4.0), ('square', 0.0), ('lshape', 1.0)):
        mesh, _, _, _, _ = problem_helper(problem, J_space=6, J_time=1)
        M_x, A_x = space_matrices(mesh)
        mat = sp.csr_matrix(coef * M_x + 0.3 * A_x)
        M = mat.shape[0]
        assert M > InvLinOp.MAX_ROWS
        op = InvLinOp(mat)
        assert op._dense is None
        lv_l, lv_u, launches = op.levels()
        # the narrow levels near the root are one dense block: a few dozen launches
        assert lv_l > 100 and lv_u > 100 and op.n_top > 100 and launches < 0.1 * (lv_l + lv_u), (lv_l, lv_u, launches)
        InvLinOp.dense_top = False  # (the plan is built at construction)
        try:
            by_levels = InvLinOp(mat)
        finally:
            InvLinOp.dense_top = True
        assert by_levels.n_top == 0 and by_levels.levels()[2] > launches
        lu = splu(sp.csc_matrix(mat), options={"SymmetricMode": True}, permc_spec="MMD_AT_PLUS_A")
        cols = {}
        for n_loc in (5, 2, 9, 33):
            X = rng.rand(n_loc, M)
            X[0] = np.linspace(0.0, 1.0, M)  # a column every slab length shares
            x = _vec(_dd(n_loc, M), X)
            y = op.apply(x.buf, n_loc=n_loc)
            got = y[:, :n_loc].t().cpu().numpy()
            want = lu.solve(X.T.copy()).T
            assert relerr(got, want) < 1e-13, (problem, n_loc, relerr(got, want))
            assert relerr((mat @ got.T).T, X) < 1e-12
            assert not y[:, n_loc:].cpu().numpy().any()
            cols[n_loc] = got[0].copy()
            y_in_place = x.buf.clone()
            op.apply(y_in_place, out=y_in_place, n_loc=n_loc)
            assert torch.equal(y_in_place, y)
            # every level by itself (no dense top): the same solution to rounding
            y_levels = by_levels.apply(x.buf, n_loc=n_loc)
            assert relerr(y_levels[:, :n_loc].t().cpu().numpy(), want) < 1e-13
        assert all(np.array_equal(cols[5], c) for c in cols.values())
        op.host_solve = True
        y = op.apply(x.buf, n_loc=n_loc)
        assert np.array_equal(y[:, :n_loc].t().cpu().numpy(), want)
    import heateq_mpi as hm
    from source.linalg import PCG
    g = load_golden('o1_pcg_square_J3_J6_direct')
    h = hm.HeatEquationMPI(J_space=6, J_time=3, precond='direct')
    assert h.Kinv_x._dense is None and not h.Kinv_x.host_solve
    st, sx = (int(v) for v in g['sample_strides'])
    x = _vec(h.dofs_distr, _bench_vector(h.N, h.M))
    assert relerr(_np(h.S @ x)[::st, ::sx], g['SX_sample']) < 1e-11
    assert relerr(_np(h.P @ x)[::st, ::sx], g['PX_sample']) < 1e-11
    hist = []
    w, it = PCG(h.WT_S_W, h.P, h.rhs, history=hist)
    assert it == int(g['iters']), (it, int(g['iters']))
    _hist_dev('config1_direct_preconditioner', hist, g['hist'], 1e-10)
    wn = _np(w)
    assert abs(np.linalg.norm(wn) - g['w_norm']) < 1e-10 * g['w_norm']
    assert relerr(wn[::st, ::sx], g['w_sample']) < 1e-10
