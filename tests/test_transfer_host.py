"""The level transfer on the host: the contract as a NumPy loop (``numpy_prolong``, which the GPU
tests import), the parent table against the multigrid's prolongation matrices, the window
arithmetic of the C ABI's refusals, the nestedness check and the argument checks of
``solve(x0=)`` -- nothing here needs a GPU."""
import copy
import functools

import numpy as np
import pytest

from source.assembly import prolongation_matrices
from source.problem import jitter, problem_helper
from source.transfer import MAX_A, check_nested, identity_rows, parent_rows, time_levels, window

# (problem, coarse J_space, fine J_space): square 0 -> 1 has M_c = 1
CASES = {'square01': ('square', 0, 1), 'square23': ('square', 2, 3), 'lshape23': ('lshape', 2, 3),
         'cube12': ('cube', 1, 2)}


# ---- the contract -------------------------------------------------------------------------------------------------------
def numpy_space(parents, uc_col):
    """s_i(q) of one coarse column `uc_col` (M_c,) for all fine rows: (p, p) copies, anything
    else is (A + B) * 0.5 with 0.0 for an absent parent ((-1, -1): both absent, 0.0)."""
    p0, p1 = parents[:, 0].astype(np.int64), parents[:, 1].astype(np.int64)
    if len(uc_col) == 0:
        assert np.all(p0 == -1) and np.all(p1 == -1)
        return np.zeros(len(parents))
    with np.errstate(all='ignore'):
        A = np.where(p0 >= 0, uc_col[np.maximum(p0, 0)], 0.0)
        B = np.where(p1 >= 0, uc_col[np.maximum(p1, 0)], 0.0)
        return np.where((p0 == p1) & (p0 >= 0), uc_col[np.maximum(p0, 0)], (A + B) * 0.5)


def numpy_prolong(parents, a, uc, qc_first, k_first, n_cols):
    """The contract of include/stk.h "level transfer" as a loop over the fine columns: `uc`
    (M_c, n_cc) holds the coarse columns qc_first ..; returns (M_f, n_cols), the fine columns
    k_first ...  Every operation is one rounded NumPy operation; column q + 1 is not touched
    where rem == 0."""
    parents = np.asarray(parents)
    assert parents.ndim == 2 and parents.shape[1] == 2
    uc = np.asarray(uc, dtype=np.float64)
    out = np.empty((len(parents), n_cols))
    for c in range(n_cols):
        k = k_first + c
        q, rem = k >> a, k & ((1 << a) - 1)
        s0 = numpy_space(parents, uc[:, q - qc_first])
        if rem == 0:
            out[:, c] = s0
            continue
        w1 = rem / 2.0**a
        w0 = 1.0 - w1
        s1 = numpy_space(parents, uc[:, q + 1 - qc_first])
        with np.errstate(all='ignore'):
            out[:, c] = w0 * s0 + w1 * s1
    return out


def numpy_chain(tables, a, uc):
    """Several space levels on a whole coarse vector `uc` (M_c, N_c): a = 0 on the coarse time
    mesh for all but the last table, which carries the time refinement."""
    N_c = uc.shape[1]
    for table in tables[:-1]:
        uc = numpy_prolong(table, 0, uc, 0, 0, N_c)
    return numpy_prolong(tables[-1], a, uc, 0, 0, ((N_c - 1) << a) + 1)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@functools.lru_cache(maxsize=None)
def meshes(problem, J_space, J_time=1):
    """(mesh_space, mesh_time) of a problem; shared, not to be changed."""
    mesh, _, mesh_time = problem_helper(problem, J_space=J_space, J_time=J_time)[:3]
    return mesh, mesh_time


@functools.lru_cache(maxsize=None)
def case_table(case):
    """(parents (M_f, 2) int32, M_c) of a case."""
    problem, Jc, Jf = CASES[case]
    mesh = meshes(problem, Jf)[0]
    table = parent_rows(mesh)
    M_c = int(np.count_nonzero(~mesh.boundary[:mesh.nverts[-2]]))
    return table, M_c


def dyadic(rng, shape):
    """Multiples of 1/64 of modest size: sums and halves of them are exact."""
    return rng.randint(-512, 513, size=shape) / 64.0


# ---- the parent table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_parent_rows_are_the_prolongation_matrix(case):
    problem, Jc, Jf = CASES[case]
    mesh = meshes(problem, Jf)[0]
    table, M_c = case_table(case)
    P = prolongation_matrices(mesh)[-1]
    assert table.dtype == np.int32 and table.shape == (P.shape[0], 2) and P.shape[1] == M_c
    assert table.min() >= -1 and table.max() < M_c
    dense = np.zeros(P.shape)
    for i, (p0, p1) in enumerate(table):
        if p0 == p1 and p0 >= 0:
            assert i < M_c and p0 == i  # the coarse level's own vertices come first
            dense[i, p0] = 1.0
        else:
            for p in (p0, p1):
                if p >= 0:
                    dense[i, p] = 0.5
    assert np.array_equal(dense, P.toarray())
    # every free row: one entry of 1.0, or at most two of 0.5
    for row in P.toarray():
        nz = row[row != 0.0]
        assert (len(nz) == 1 and nz[0] == 1.0) or (len(nz) <= 2 and np.all(nz == 0.5))
    # a condition on the inputs: rows with BOTH parents on the boundary, and with exactly one
    absent = (table == -1).sum(axis=1)
    assert np.count_nonzero(absent == 2) >= 1 and np.count_nonzero(absent == 1) >= 1, np.bincount(absent)
    if case == 'square01':
        assert M_c == 1
    # P x on dyadic data: the matrix product and the loop add and halve the same exact numbers
    rng = np.random.RandomState(11)
    x = dyadic(rng, (M_c, 3))
    assert np.array_equal(P @ x, numpy_prolong(table, 0, x, 0, 0, 3))
    # the given level of a deeper mesh is the last level of the shallower one
    coarse = meshes(problem, Jc)[0]
    if coarse.J >= 1 and np.count_nonzero(~coarse.boundary[:coarse.nverts[-2]]) > 0:
        assert np.array_equal(parent_rows(mesh, mesh.J - 1), parent_rows(coarse))
    with pytest.raises(ValueError, match='no coarser level'):
        parent_rows(mesh, 0)
    with pytest.raises(ValueError, match='no coarser level'):
        parent_rows(mesh, mesh.J + 1)


def test_identity_rows_copy():
    table = identity_rows(5)
    assert table.dtype == np.int32 and table.tolist() == [[i, i] for i in range(5)]
    x = np.random.RandomState(1).randn(5, 3)
    assert np.array_equal(numpy_prolong(table, 0, x, 0, 0, 3), x)
    assert identity_rows(0).shape == (0, 2)


def test_the_loop_in_time():
    """a levels in one shot on an identity table: nodes copy, midpoints interpolate with exact
    weights, and a NaN in column q + 1 does not reach a column with rem == 0."""
    table = identity_rows(2)
    uc = np.array([[1.0, 3.0, np.nan], [0.0, -8.0, 8.0]])
    got = numpy_prolong(table, 2, uc, 0, 0, 9)
    assert got[0, :5].tolist() == [1.0, 1.5, 2.0, 2.5, 3.0] and np.isnan(got[0, 5:]).all()
    assert got[1].tolist() == [0.0, -2.0, -4.0, -6.0, -8.0, -4.0, 0.0, 4.0, 8.0]
    # a window that ends exactly on a node reads no column beyond it
    assert numpy_prolong(table, 2, uc[:, :2], 0, 0, 5)[0].tolist() == [1.0, 1.5, 2.0, 2.5, 3.0]
    with pytest.raises(IndexError):
        numpy_prolong(table, 2, uc[:, :2], 0, 0, 6)
    # from the middle: coarse columns 1 .., fine columns 6 ..
    assert numpy_prolong(table, 2, uc[:, 1:], 1, 6, 3)[1].tolist() == [0.0, 4.0, 8.0]


# ---- the window of the refusals --------------------------------------------------------------------------------------
def test_window_arithmetic():
    for a in range(0, 5):
        for k_first in range(0, 20):
            for n_cols in range(1, 20):
                read = set()
                for k in range(k_first, k_first + n_cols):
                    read.add(k >> a)
                    if k & ((1 << a) - 1):
                        read.add((k >> a) + 1)
                assert window(a, k_first, n_cols) == (min(read), max(read)), (a, k_first, n_cols)
    assert window(1, 0, 65) == (0, 32) and window(1, 0, 64) == (0, 32) and window(1, 1, 1) == (0, 1)
    assert window(0, 7, 3) == (7, 9) and window(3, 8, 1) == (1, 1) and window(3, 8, 2) == (1, 2)


def test_time_levels():
    assert [time_levels(3, n) for n in (3, 5, 9, 17)] == [0, 1, 2, 3]
    assert time_levels(2, 257) == MAX_A
    for coarse, fine in ((3, 4), (3, 7), (5, 3), (4, 10), (2, 513), (1, 1)):
        with pytest.raises(ValueError, match='2\\^a times the elements'):
            time_levels(coarse, fine)


# ---- nestedness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_the_coarser_mesh_is_the_prefix_of_the_finer(case):
    problem, Jc, Jf = CASES[case]
    assert check_nested(meshes(problem, Jc, 1), meshes(problem, Jf, 2)) == (1, Jf - Jc)
    assert check_nested(meshes(problem, Jf, 2), meshes(problem, Jf, 2)) == (0, 0)
    assert check_nested(meshes(problem, Jc, 1), meshes(problem, Jf, 3)) == (2, Jf - Jc)


def test_meshes_that_are_not_nested_are_refused():
    coarse, fine = meshes('lshape', 2, 1), meshes('lshape', 3, 2)
    moved = jitter(copy.deepcopy(coarse[0]))
    assert not np.array_equal(moved.points, coarse[0].points)
    with pytest.raises(ValueError, match='coarse points are not the prefix'):
        check_nested((moved, coarse[1]), fine)
    with pytest.raises(ValueError, match='coarse points are not the prefix'):
        check_nested(coarse, (jitter(copy.deepcopy(fine[0])), fine[1]))
    longer = copy.deepcopy(coarse[1])
    longer.T = 2.0
    with pytest.raises(ValueError, match='time intervals differ'):
        check_nested((coarse[0], longer), fine)
    from source.mesh import construct_interval
    with pytest.raises(ValueError, match='2\\^a times the elements'):
        check_nested((coarse[0], construct_interval(N=3)), fine)
    with pytest.raises(ValueError, match='2\\^a times the elements'):  # the finer time mesh as the coarse one
        check_nested((coarse[0], meshes('lshape', 2, 3)[1]), fine)
    with pytest.raises(ValueError, match='not nested: levels'):  # the finer space mesh as the coarse one
        check_nested((fine[0], coarse[1]), (coarse[0], fine[1]))
    with pytest.raises(ValueError, match='not nested'):  # another domain
        check_nested(meshes('square', 2, 1), fine)
    flagged = copy.deepcopy(coarse[0])
    flagged.boundary = flagged.boundary.copy()
    flagged.boundary[np.flatnonzero(~flagged.boundary)[0]] = True
    with pytest.raises(ValueError, match='coarse boundary are not the prefix'):
        check_nested((flagged, coarse[1]), fine)


def test_prolong_from_refuses_before_a_plan_is_built():
    """Both drivers' prolong_from goes through source.transfer.prolong_from: meshes that are not
    nested raise before the coarse vector is looked at and before anything is cached."""
    from source.postprocess import PostProcessing

    class Recorder(PostProcessing):
        def __init__(self, pair):
            self._init_postprocessing(pair[0], pair[1], {})
            self.calls = []

        def _trial_vector(self, u, who):
            self.calls.append(who)
            return u

        def _adjoint_target(self, out):
            self.calls.append('target')
            return None, out

    fine, other = Recorder(meshes('lshape', 3, 2)), Recorder(meshes('square', 2, 1))
    assert fine.transfer_plans == {}
    with pytest.raises(ValueError, match='not nested'):
        fine.prolong_from(other, object())
    assert fine.transfer_plans == {} and fine.calls == [] and other.calls == []


# ---- solve(x0=) -------------------------------------------------------------------------------------------------------------
def test_solve_refuses_a_start_of_the_wrong_space():
    import heateq
    import heateq_mpi as hm
    from source.comm import Comm
    from source.mpi_vector import DofDistributionMPI, KronVectorMPI
    N, M = 5, 7
    comm = Comm(distributed=False)
    heat = hm.HeatEquationMPI.__new__(hm.HeatEquationMPI)
    heat.N, heat.M = N, M
    heat.f = KronVectorMPI(DofDistributionMPI(comm, N, M))
    for shape in ((N + 1, M), (N, M + 1)):
        with pytest.raises(AssertionError, match='x0= takes a vector of the trial space'):
            heat.solve(x0=KronVectorMPI(DofDistributionMPI(comm, *shape)))
    with pytest.raises(AssertionError, match='x0= takes a vector of the trial space'):
        heat.solve(x0=np.zeros(N * M))  # the time-parallel driver takes no flat vector
    serial = heateq.HeatEquation.__new__(heateq.HeatEquation)
    serial.N, serial.M, serial.f = N, M, np.zeros(N * M)
    for on_host in (False, True):
        with pytest.raises(AssertionError, match='x0= takes a vector of the trial space'):
            serial.solve(x0=np.zeros(N * M + 1), on_host=on_host)
        with pytest.raises(AssertionError, match='x0= takes a vector of the trial space'):
            serial.solve(x0=KronVectorMPI(DofDistributionMPI(comm, N + 1, M)), on_host=on_host)


def test_nested_levels_of_the_command_line():
    from source import driver
    assert driver.nested_levels(3, 3, 0) == []
    assert driver.nested_levels(3, 4, 2) == [(1, 2), (2, 3)]
    with pytest.raises(SystemExit, match='there is no level'):
        driver.nested_levels(3, 1, 2)
    with pytest.raises(SystemExit, match='fewer than the 8 ranks'):
        driver.nested_levels(3, 3, 1, size=8)  # J_time = 2: five nodes
    assert driver.nested_levels(4, 4, 1, size=8) == [(3, 3)]
