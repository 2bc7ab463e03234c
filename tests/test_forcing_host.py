"""Forcing terms, host side (no GPU): the time factor of the load vector, the fixtures
made by the reference's own classes (tests/golden/make_forcing_golden.py), and a SciPy
restatement of the forced problem against its exact solution -- the one check that
pins sign and scale of g, which no parity between two paths of this build can."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from conftest import load_golden, relerr

from source.assembly import (element_blocks, space_load, space_matrices, time_load_test_space,
                             time_matrices, time_matrices_test_space)
from source.problem import problem_helper

F1 = ['f1_forcing_square_J3_J3', 'f1_forcing_square_J4_J4', 'f1_forcing_cube_J2_J2']


def host_problem(problem, J_time, J_space):
    """Host matrices and loads of a forced problem, as the drivers assemble them."""
    mesh_space, _, mesh_time, data, _ = problem_helper(problem, J_space=J_space, J_time=J_time)
    A_t, L_t, M_t, G_t, u0_t = time_matrices(mesh_time)
    M_Y, Minv_Y, B1_t, B2_t = time_matrices_test_space(mesh_time)
    M_x, A_x = space_matrices(mesh_space, scipy_path=True)
    g = sum(np.kron(time_load_test_space(mesh_time, g_t), space_load(mesh_space, g_x, numpy_path=True))
            for g_t, g_x in data['g'])
    u0_x = space_load(mesh_space, data['u0'], numpy_path=True)
    return dict(mesh_space=mesh_space, mesh_time=mesh_time, data=data, M_t=M_t, G_t=G_t, u0_t=u0_t,
                Minv_Y=Minv_Y, B1_t=B1_t, B2_t=B2_t, M_x=M_x, A_x=A_x, g=g, u0_x=u0_x)


# ---- 1. the time load ---------------------------------------------------------------
@pytest.mark.parametrize('J_time', [3, 5])
def test_time_load_against_a_12_point_rule(J_time):
    """4 Gauss points integrate g_t * psi exactly up to degree 7; for the two smooth g_t
    of the forced problems on elements of h <= 1/8 the remainder, h^9 (4!)^4 / (9 (8!)^3)
    max|(g_t psi)^(8)| = 4e-18, is below one rounding of the entries (~ h / 2)."""
    _, _, mesh_time, data, _ = problem_helper('square_forced', J_space=1, J_time=J_time)
    _, _, _, data3, _ = problem_helper('cube_forced', J_space=1, J_time=J_time)
    ne, h = mesh_time.nv - 1, mesh_time.h
    q, w = np.polynomial.legendre.leggauss(12)
    s = 0.5 * (q + 1.0)
    for g_t in [pair[0] for pair in data['g'] + data3['g']]:
        got = time_load_test_space(mesh_time, g_t)
        assert got.shape == (2 * ne,)
        want = np.empty(2 * ne)
        whole = np.empty(ne)
        for e in range(ne):
            f = g_t(h * (e + s)) * 0.5 * h * w
            want[2 * e], want[2 * e + 1], whole[e] = f @ (1 - s), f @ s, f.sum()
        assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-14
        # psi_{e,0} + psi_{e,1} = 1 on the element
        assert np.max(np.abs(got[0::2] + got[1::2] - whole) / np.abs(whole)) <= 1e-14


def test_time_load_ordering_matches_the_test_space_matrices():
    """B2_t 1 = int psi_{e,a}: the load of the constant 1 in the ordering 2e + a."""
    _, _, mesh_time, _, _ = problem_helper('square_forced', J_space=1, J_time=3)
    _, _, _, B2_t = time_matrices_test_space(mesh_time)
    one = time_load_test_space(mesh_time, lambda t: np.ones_like(t))
    assert np.allclose(one, B2_t @ np.ones(mesh_time.nv), rtol=1e-15, atol=0)
    # and a function that tells the two ends of an element apart
    lin = time_load_test_space(mesh_time, lambda t: t)
    nodes = mesh_time.h * np.arange(mesh_time.nv)
    assert np.allclose(lin, B2_t @ nodes, rtol=1e-14, atol=1e-17)


def test_element_blocks_rebuild_the_time_factors():
    _, _, mesh_time, _, _ = problem_helper('square_forced', J_space=1, J_time=3)
    M_Y, Minv_Y, B1_t, B2_t = time_matrices_test_space(mesh_time)
    ne = mesh_time.nv - 1
    for mat, step in ((B1_t, 1), (B2_t, 1), (Minv_Y, 2), (M_Y, 2)):
        blk = element_blocks(mat)
        dense = np.zeros(mat.shape)
        for e in range(ne):
            dense[2 * e:2 * e + 2, step * e:step * e + 2] = blk[e]
        assert np.array_equal(dense, mat.toarray())


# ---- 2. the fixtures of the reference's classes -------------------------------------
@pytest.mark.parametrize('name', F1)
def test_fixture_loads_and_right_hand_side(name):
    """g of the fixture is this build's host assembly; f = B^T K g + u0 and the Y'
    number are restated on the CPU oracle's serial wiring (oracle/heat_serial.py, the
    reference's multigrid arithmetic)."""
    from oracle.heat_serial import HeatSerialOracle
    from source.assembly import prolongation_matrices
    g = load_golden(name)
    problem = 'cube_forced' if 'cube' in name else 'square_forced'
    J_time, J_space = int(g['J_time']), int(g['J_space'])
    h = host_problem(problem, J_time, J_space)
    assert (int(g['N']), int(g['M'])) == (h['G_t'].shape[0], h['M_x'].shape[0])
    g_vec = g['g'] if 'g' in g.files else h['g']  # the larger fixtures leave g out: this build's assembly
    assert relerr(h['g'], g_vec) <= 1e-13
    o = HeatSerialOracle(dict(G_t=h['G_t'], u0_t=h['u0_t'], Minv_Y=h['Minv_Y'], B1_t=h['B1_t'],
                              B2_t=h['B2_t'], M_x=h['M_x'], A_x=h['A_x'], u0_x=h['u0_x'],
                              P_mats=prolongation_matrices(h['mesh_space'])), J_time)
    f = o.BT(o.K(g_vec)) + o.f()
    assert relerr(f, g['f']) <= 1e-11
    defect = g_vec - o.B(g['u'])
    assert abs(defect @ o.K(defect) - float(g['error_Yprime'])) <= 1e-9 * float(g['error_Yprime'])
    hist = g['r_dot_Pr']
    assert len(hist) == int(g['iters']) + 1 and hist[-1] < 1e-12 <= hist[-2]


# ---- the choice between the fused and the composed element kernels ----------------------
def test_fused_form_is_chosen_by_the_kernels_own_lds_count():
    """ElementKronMatMPI.fused_fits asks the library (stk_kron_pack_elem_lds_bytes(), host
    code) what ONE slot row costs a workgroup: all 8 n_el block doubles, the dictionary,
    2 * rows_per_unit sums per node or test-space column.  On the square's pair plan
    (K = 10, rows_per_unit = 2) J_time = 9 on one rank -- 513 nodes, 512 elements -- is
    beyond the 64 KiB in the transpose (32 832 + 32 768 bytes of sums and blocks alone)
    and must take the composed form; J_time = 8 fits both ways."""
    from source import _lib
    from source.mpi_kron import ElementKronMatMPI

    def pattern(K, rows_per_unit, n_codes=16):
        return _lib.PackPattern(1 << 20, K, 20, n_codes, 2, rows_per_unit, 1 << 19, None, None, None, None)

    lds = lambda pat, n_el, n_loc, t: _lib.lib().stk_kron_pack_elem_lds_bytes(pat, n_el, n_loc, t)
    pairs = pattern(10, 2)
    assert lds(pairs, 512, 513, 1) > 65536 >= 2 * 2 * 1026 * 8 + 8 * 512 * 8 - 64
    assert lds(pairs, 512, 513, 1) >= 2 * 2 * 1026 * 8 + 8 * 512 * 8
    assert not ElementKronMatMPI.fused_fits(pairs, 512, 513, True)
    assert ElementKronMatMPI.fused_fits(pairs, 512, 513, False)       # forward: 513 + 3 sums per row
    assert not ElementKronMatMPI.fused_fits(pairs, 768, 769, False)   # ... but not at 769 nodes
    assert ElementKronMatMPI.fused_fits(pairs, 256, 257, True) and ElementKronMatMPI.fused_fits(pairs, 256, 257, False)
    # rank 0 of 2 at J_time = 10: 512 nodes, 512 elements
    assert not ElementKronMatMPI.fused_fits(pairs, 512, 512, True)
    # single rows carry half the sums: 512 elements fit, 1023 nodes need more than 512 lanes
    single = pattern(7, 1)
    assert ElementKronMatMPI.fused_fits(single, 512, 513, True)
    assert lds(single, 1024, 1025, 1) == -1 and not ElementKronMatMPI.fused_fits(single, 1024, 1025, True)
    # monotone in the slab length
    sizes = [lds(pairs, n, n + 1, 1) for n in range(1, 513)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))


# ---- 3. SciPy restatement against the exact solution --------------------------------
def scipy_error(J):
    """Relative (M_t kron M_x) error of the discrete solution of square_forced at
    J_time = J_space = J against the nodal values of the exact solution: S u = f with
    S = B^T K B + G, f = B^T K g + u0, K = Minv_Y kron A_x^-1 exactly (splu), every
    Kronecker product written out with sp.kron, CG to 1e-12."""
    h = host_problem('square_forced', J, J)
    N, M = h['G_t'].shape[0], h['M_x'].shape[0]
    B = sp.kron(h['B1_t'], h['M_x']) + sp.kron(h['B2_t'], h['A_x'])
    G = sp.kron(h['G_t'], h['M_x'])
    lu = spla.splu(sp.csc_matrix(h['A_x']))
    NY = h['Minv_Y'].shape[0]

    def K(y):
        Z = h['Minv_Y'] @ y.reshape(NY, M)
        return lu.solve(np.ascontiguousarray(Z.T)).T.reshape(-1)

    S = spla.LinearOperator((N * M, N * M), matvec=lambda v: B.T @ K(B @ v) + G @ v, dtype=np.float64)
    f = B.T @ K(h['g']) + np.kron(h['u0_t'], h['u0_x'])
    # preconditioner: (M_t + G_t) kron A_x^-1 ... any SPD one will do; I_t kron A_x^-1
    Pre = spla.LinearOperator((N * M, N * M), dtype=np.float64,
                              matvec=lambda v: lu.solve(np.ascontiguousarray(v.reshape(N, M).T)).T.reshape(-1))
    u, info = spla.cg(S, f, rtol=1e-12, atol=0.0, M=Pre, maxiter=20000)
    assert info == 0, info
    from source.assembly import free_dofs
    pts = h['mesh_space'].points[free_dofs(h['mesh_space'])]
    t = h['mesh_time'].h * np.arange(N)
    exact = h['data']['exact'](t[:, None], pts[None, :, 0], pts[None, :, 1]).reshape(-1)
    MM = sp.kron(h['M_t'], h['M_x'])
    e = u - exact
    return np.sqrt(e @ (MM @ e)) / np.sqrt(exact @ (MM @ exact))


def test_scipy_restatement_converges_to_the_exact_solution():
    """Measured on the CPU: 1.88e-2 at J = 2, 4.84e-3 at J = 3, 1.21e-3 at J = 4, 3.03e-4
    at J = 5: second order, ratio 4.0 per level.  A wrong sign or scale of either pair of
    g stalls the error at the size of the missing term."""
    e3, e4 = scipy_error(3), scipy_error(4)
    print('relative M_t kron M_x error: J=3 %.4e, J=4 %.4e, ratio %.3f' % (e3, e4, e3 / e4))
    assert 3.5 <= e3 / e4 <= 4.5
    assert e4 <= 1.5e-3
