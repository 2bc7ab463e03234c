#!/usr/bin/env python3
"""Generates tests/golden/f1_forcing_*.npz: the forced heat problems solved by the
REFERENCE's own classes, wired as its serial driver (reference heateq.py:40-102).

Run in the build container only (it needs the reference checkout make_golden.py
names, which never travels to the GPU box):

    python tests/golden/make_forcing_golden.py

Nothing of the reference is copied.  The stand-ins for mpi4py / petsc4py and the
duck-typed hierarchy come from make_golden.py; the reference's KronLinOp,
CompositeLinOp, BlockDiagLinOp, MultiGrid, WaveletTransformOp and PCG are imported
and fed this build's host matrices and load vectors (source/assembly.py,
source/problem.py), where the reference's driver asks NGSolve.  Stored per problem:
the load vector g on the test space, f = B^T K g + u0, the wavelet coefficients w
(the serial driver's level-by-level numbering), u = W w, the iteration count, the
r.Pr history (initial residual and every iteration) and the two error numbers of
the driver's last line -- the X-norm algebraic error r.Pr with r = f - S u and the
Y' estimator (g - B u)^T K (g - B u) (heateq.py:154-155).  A fixture whose g would
exceed LARGE doubles keeps f and u only: g is this build's own assembly (the tests
rebuild it), w is u in another basis.
"""
import importlib
import os
import sys
import types

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

# name of the fixture, problem, J_time, J_space
F1_PROBLEMS = [
    ('f1_forcing_square_J3_J3', 'square_forced', 3, 3),
    ('f1_forcing_square_J4_J4', 'square_forced', 4, 4),
    ('f1_forcing_cube_J2_J2', 'cube_forced', 2, 2),
]

LARGE = 8192  # doubles of g above which a fixture leaves g and w out


def load_build_package():
    """This build's `source` package under another name (the name `source` stays
    free for the reference's): problem.py imports its mesh module relatively."""
    pkg = types.ModuleType('amd_source')
    pkg.__path__ = [mg.PKG]
    sys.modules['amd_source'] = pkg
    mesh = importlib.import_module('amd_source.mesh')
    mesh.REFINE_NUMPY = True  # the generator does not load libstk
    return (importlib.import_module('amd_source.problem'),
            importlib.import_module('amd_source.assembly'))


def main():
    mg.install_standins()
    problem, asm = load_build_package()
    sys.path.insert(0, mg.REF)
    from source.linalg import PCG
    from source.linop import BlockDiagLinOp, CompositeLinOp, KronLinOp
    from source.multigrid import MultiGrid
    from source.wavelets import WaveletTransformOp
    import source.linop as ref_linop

    # BlockDiagLinOp leaves the dtype to SciPy, whose current versions find it by
    # applying the operator to an int8 zero vector -- which the reference's matvec
    # cannot add floats to.  Name the dtype for it; the matvec itself runs untouched.
    ref_linop.LinearOperator = lambda matvec, shape: sp.linalg.LinearOperator(
        shape, matvec=matvec, dtype=np.float64)

    out_dir = os.environ.get('STK_GOLDEN_OUT', HERE)
    for name, pname, J_time, J_space in F1_PROBLEMS:
        mesh_space, bc, mesh_time, data, _ = problem.problem_helper(pname, J_space=J_space, J_time=J_time)
        A_t, L_t, M_t, G_t, u0_t = asm.time_matrices(mesh_time)
        M_Y, Minv_Y, B1_t, B2_t = asm.time_matrices_test_space(mesh_time)
        M_x, A_x = asm.space_matrices(mesh_space, scipy_path=True)
        hier = mg.Hierarchy(asm.prolongation_matrices(mesh_space))
        N, M = A_t.shape[0], M_x.shape[0]
        mk = lambda m: MultiGrid(m, hier, smoothsteps=3, vcycles=2)
        alpha = 0.3

        # heateq.py:52-91
        B = KronLinOp(B1_t, M_x) + KronLinOp(B2_t, A_x)
        BT = KronLinOp(sp.csr_matrix(B1_t.T), M_x) + KronLinOp(sp.csr_matrix(B2_t.T), A_x)
        G = KronLinOp(G_t, M_x)
        K = KronLinOp(Minv_Y, mk(A_x))
        W_t = WaveletTransformOp(J_time)
        W = KronLinOp(W_t, sp.eye(M, format='csr'))
        WT = KronLinOp(W_t.T, sp.eye(M, format='csr'))
        C_j = [mk(sp.csr_matrix(2**j * M_x + alpha * A_x)) for j in range(J_time + 1)]
        CAC_j = [CompositeLinOp([C_j[j], A_x, C_j[j]]) for j in range(J_time + 1)]
        P = BlockDiagLinOp([CAC_j[j] for j in W_t.levels])
        S = sp.linalg.LinearOperator(G.shape, matvec=lambda v: BT @ (K @ (B @ v)) + G @ v)
        WT_S_W = WT @ S @ W

        # heateq.py:93-102, the loads from this build's assembly
        g = np.zeros(K.shape[0])
        for g_t, g_x in data['g']:
            g += np.kron(asm.time_load_test_space(mesh_time, g_t),
                         asm.space_load(mesh_space, g_x, numpy_path=True))
        u0_x = asm.space_load(mesh_space, data['u0'], numpy_path=True)
        f = BT @ (K @ g) + np.kron(u0_t, u0_x)

        # heateq.py:146-155
        history = []
        rhs = WT @ f
        history.append(float(rhs @ (P @ rhs)))  # r.Pr of the initial residual (w0 = 0)
        w, iters = PCG(WT_S_W, P, rhs, callback=lambda w_, r, k: history.append(float(r @ (P @ r))))
        u = W @ w
        res = f - S @ u
        defect = g - B @ u
        path = os.path.join(out_dir, name + '.npz')
        vectors = dict(f=f, u=u) if g.size > LARGE else dict(g=g, f=f, w=w, u=u)
        np.savez_compressed(path, J_time=J_time, J_space=J_space, N=N, M=M, iters=iters, **vectors,
                            r_dot_Pr=np.array(history),
                            error_alg=float(res @ (P @ res)),
                            error_Yprime=float(defect @ (K @ defect)))
        print('wrote', os.path.relpath(path, mg.REPO), '%.1f kB' % (os.path.getsize(path) / 1024),
              'iters', iters, 'Yprime', float(defect @ (K @ defect)))


if __name__ == '__main__':
    main()
