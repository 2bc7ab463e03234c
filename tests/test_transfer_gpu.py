"""The level transfer on the device (csrc/transfer.hip, source/transfer.py) against the NumPy
contract of tests/test_transfer_host.py -- array_equal, NaN-aware: the kernel on the four mesh
pairs at every edge of the time rule, window, stride and alignment, non-finite input, every
launch form, the refusals, the public call of both drivers, its independence of the number of
ranks, solve(x0=), the drivers' --nested, and the torch composition the timing tool compares
with."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_transfer_host import CASES, case_table, meshes, numpy_chain, numpy_prolong, same

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 123.25


def _dev(a):
    from source import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(_lib.compute_device())


@functools.lru_cache(maxsize=None)
def _level(case):
    """(the device plan of a case's space level, its table, M_c)."""
    from source.transfer import _PlanHandle
    table, M_c = case_table(case)
    return _PlanHandle(table, M_c), table, M_c


def _prolong(level, a, uc, qc_first, k_first, n_cols, ld=None, ldc=None, off_out=0, off_uc=0):
    """stk_transfer_prolong on fresh buffers: `uc` (M_c, n_cc) NumPy, the coarse columns from
    qc_first, at row stride ldc with NaN between the rows, based `off_uc` doubles into its
    buffer; out at row stride ld, pre-filled with SENTINEL, based `off_out` doubles in.
    Returns (the (M_f, n_cols) result, True iff every other double of the out buffer still
    holds SENTINEL)."""
    from source.transfer import prolong_scan
    M_f, (M_c, n_cc) = level.M_fine, uc.shape
    ld = n_cols + (n_cols & 1) if ld is None else ld
    ldc = n_cc if ldc is None else ldc
    src = np.full(off_uc + max(M_c, 1) * ldc + 1, np.nan)
    if M_c:
        src[off_uc:off_uc + M_c * ldc].reshape(M_c, ldc)[:, :n_cc] = uc
    src, dst = _dev(src), _dev(np.full(off_out + M_f * ld + 1, SENTINEL))
    prolong_scan(level, a, src.data_ptr() + 8 * off_uc, ldc, qc_first, n_cc, dst.data_ptr() + 8 * off_out, ld, k_first,
                 n_cols)
    flat = dst.cpu().numpy()
    body = flat[off_out:off_out + M_f * ld].reshape(M_f, ld)
    kept = bool(np.all(body[:, n_cols:] == SENTINEL)) and bool(np.all(flat[:off_out] == SENTINEL)) and bool(
        np.all(flat[off_out + M_f * ld:] == SENTINEL))
    return body[:, :n_cols].copy(), kept


class _tile:
    """The kernel's launch form for the block: rows per workgroup, LDS in KiB (stk_transfer_tile)."""
    def __init__(self, rows, kib):
        self.shape = (rows, kib)

    def __enter__(self):
        from source import _lib
        _lib.check(_lib.lib().stk_transfer_tile(*self.shape))

    def __exit__(self, *exc):
        from source import _lib
        _lib.check(_lib.lib().stk_transfer_tile(0, 0))


# ---- 1. the device is the contract ------------------------------------------------------------------------------------
N_COARSE = 5  # coarse time nodes of the kernel tests: 4 elements


@pytest.mark.parametrize('a', [0, 1, 2, 3])
@pytest.mark.parametrize('case', sorted(CASES))
def test_device_is_the_contract(case, a):
    """n_cols in {1, 2, 2^a, 2^a + 1, all}; k_first odd and even, on a coarse node and off it; the
    coarse window exactly what the rules read (so a last column with rem == 0 has no q + 1 in
    the window) and one column wider at either end; ld = n_cols, odd, even and beyond; out and uc
    based at +8 bytes; the pads and the doubles around out unchanged."""
    from source.transfer import window
    level, table, M_c = _level(case)
    rng = np.random.RandomState(100 * a + len(case))
    whole = rng.randn(M_c, N_COARSE)
    n_fine = ((N_COARSE - 1) << a) + 1
    seen = {'ends_on_node': 0, 'ends_off_node': 0, 'odd_first': 0, 'odd_ld': 0, 'even_ld': 0, 'wide_ld': 0,
            'shifted_out': 0, 'shifted_uc': 0}
    number = 0
    for n_cols in sorted({1, 2, 1 << a, (1 << a) + 1, n_fine}):
        for k_first in sorted({0, 1, 1 << a, (1 << a) + 1, n_fine - n_cols}):
            if k_first + n_cols > n_fine:
                continue
            for widen in (0, 1):
                number += 1
                q0, q1 = window(a, k_first, n_cols)
                lo, hi = max(q0 - widen, 0), min(q1 + widen, N_COARSE - 1)
                ld = n_cols + (0, 1, 2, 5)[number % 4]
                ldc = (hi - lo + 1) + (0, 3)[number % 2]
                off_out, off_uc = ((0, 0), (1, 0), (0, 1), (1, 1))[(number // 2) % 4]
                got, kept = _prolong(level, a, whole[:, lo:hi + 1], lo, k_first, n_cols, ld, ldc, off_out, off_uc)
                want = numpy_prolong(table, a, whole[:, lo:hi + 1], lo, k_first, n_cols)
                assert same(got, want) and kept, (n_cols, k_first, widen, ld, ldc, off_out, off_uc)
                last_rem = (k_first + n_cols - 1) & ((1 << a) - 1)
                seen['ends_on_node' if last_rem == 0 and not widen else 'ends_off_node'] += 1
                seen['odd_first'] += k_first & 1
                seen['odd_ld' if ld & 1 else 'even_ld'] += 1
                seen['wide_ld'] += ld > n_cols + 1
                seen['shifted_out'] += off_out
                seen['shifted_uc'] += off_uc
    assert all(seen.values()), seen
    assert not np.isnan(want).any()  # no NaN from between the coarse rows came in


def test_no_coarse_rows_gives_zeros():
    """M_c = 0: every parent is -1 and the result is 0.0 everywhere, pads untouched."""
    from source.transfer import _PlanHandle
    level = _PlanHandle(np.full((70, 2), -1, dtype=np.int32), 0)
    for a, n_cols in ((0, 3), (1, 5), (2, 4)):
        got, kept = _prolong(level, a, np.zeros((0, 4)), 0, 1, n_cols)
        assert got.shape == (70, n_cols) and np.all(got == 0.0) and kept


# ---- 2. NaN and +-inf ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['cube12', 'square23'])
def test_non_finite_values_give_what_the_loop_gives(case):
    level, table, M_c = _level(case)
    rng = np.random.RandomState(2)
    uc = rng.randn(M_c, N_COARSE)
    uc[rng.rand(M_c, N_COARSE) < 0.1] = np.nan
    uc[rng.rand(M_c, N_COARSE) < 0.1] = np.inf
    uc[rng.rand(M_c, N_COARSE) < 0.1] = -np.inf
    uc[:, 0], uc[:, 1] = 1.0, np.nan  # a NaN in column q + 1 must not reach the node q
    for a in (0, 1, 2):
        n_fine = ((N_COARSE - 1) << a) + 1
        got, kept = _prolong(level, a, uc, 0, 0, n_fine)
        want = numpy_prolong(table, a, uc, 0, 0, n_fine)
        assert same(got, want) and kept, a
        assert not np.isnan(got[:, 0]).any() and np.isnan(got[:, 1 << a]).sum() > 0
        if a:
            assert np.isnan(got[table[:, 0] >= 0, 1]).all()
        assert np.isinf(got).any()


# ---- 3. every launch form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,kib', [(64, 64), (128, 64), (256, 64), (64, 1), (128, 1), (256, 1), (256, 16), (64, 4)])
def test_every_launch_form_gives_the_one_shot_doubles(rows, kib):
    """64 .. 256 rows per workgroup; 1 KiB of LDS forces chunks of a single column at a = 0 and of
    2^a columns above, 4 and 16 KiB (an LDS stride of 7 and 5) chunks whose last one is shorter; out
    aligned and not."""
    level, table, M_c = _level('lshape23')
    uc = np.random.RandomState(3).randn(M_c, 9)
    for a in (0, 1, 3):
        n_fine = (8 << a) + 1
        for k_first, n_cols, off_out in ((0, n_fine, 0), (3, n_fine - 4, 1), (1, min(n_fine - 1, 6), 0)):
            want = numpy_prolong(table, a, uc, 0, k_first, n_cols)
            with _tile(rows, kib):
                got, kept = _prolong(level, a, uc, 0, k_first, n_cols, off_out=off_out)
            assert same(got, want) and kept, (a, k_first, n_cols, off_out)


def test_a_call_cut_into_column_ranges_is_the_one_call():
    level, table, M_c = _level('square23')
    uc = np.random.RandomState(4).randn(M_c, 5)
    a, n_fine = 2, 17
    whole, _ = _prolong(level, a, uc, 0, 0, n_fine)
    assert same(whole, numpy_prolong(table, a, uc, 0, 0, n_fine))
    for cut in range(1, n_fine):
        left, kept_l = _prolong(level, a, uc, 0, 0, cut)
        right, kept_r = _prolong(level, a, uc, 0, cut, n_fine - cut)
        assert kept_l and kept_r and same(np.concatenate([left, right], axis=1), whole), cut


def test_tile_setter_refuses_other_shapes_and_changes_nothing():
    from source import _lib
    lib = _lib.lib()
    level, table, M_c = _level('square23')
    uc = np.random.RandomState(5).randn(M_c, 5)
    before, _ = _prolong(level, 1, uc, 0, 0, 9)
    for rows, kib, name in ((100, 64, 'rows'), (-64, 0, 'rows'), (512, 0, 'rows'), (256, 65, 'lds_kib'), (256, -1, 'lds_kib')):
        assert lib.stk_transfer_tile(rows, kib) != 0 and name in lib.stk_last_error().decode(), (rows, kib)
        after, kept = _prolong(level, 1, uc, 0, 0, 9)
        assert same(after, before) and kept
    assert lib.stk_transfer_tile(0, 0) == 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_out_untouched():
    from source import _lib
    lib = _lib.lib()
    level, table, M_c = _level('square23')
    a, n_cols, n_cc = 1, 6, 4  # the fine columns 2 .. 7 read the coarse columns 1 .. 4
    uc, out = _dev(np.random.RandomState(6).randn(M_c, n_cc)), _dev(np.full((level.M_fine, n_cols), SENTINEL))
    st = _lib.stream()
    good = dict(plan=level, a=a, uc=uc.data_ptr(), ldc=n_cc, qc_first=1, n_cc=n_cc, out=out.data_ptr(), ld=n_cols,
                k_first=2, n_cols=n_cols)
    order = ('plan', 'a', 'uc', 'ldc', 'qc_first', 'n_cc', 'out', 'ld', 'k_first', 'n_cols')
    cases = [
        (' plan is null', dict(plan=None)), (' uc is null', dict(uc=None)), (' out is null', dict(out=None)),
        (' a = -1', dict(a=-1)), (' a = 9', dict(a=9)), (' n_cc = -1', dict(n_cc=-1)), (' n_cols = -1', dict(n_cols=-1)),
        (' qc_first = -1', dict(qc_first=-1)), (' k_first = -1', dict(k_first=-1)),
        (' ldc = 3 is below n_cc', dict(ldc=n_cc - 1)), (' ld = 5 is below n_cols', dict(ld=n_cols - 1)),
        (' = [2, 5) does not cover', dict(qc_first=2, n_cc=n_cc - 1)),  # short by one at the lower end
        (' = [1, 4) does not cover', dict(n_cc=n_cc - 1)),  # ... at the upper end: column 7 has rem != 0
        (' = [1, 5) does not cover', dict(n_cols=n_cols + 2, ld=n_cols + 2)),  # column 9 reads the coarse column 5
    ]
    for name, change in cases:
        args = dict(good, **change)
        rc = lib.stk_transfer_prolong(st, *[args[k] for k in order])
        text = lib.stk_last_error().decode()
        assert rc != 0 and 'stk_transfer_prolong' in text and name in text, (name, change, rc, text)
        with pytest.raises(_lib.StkError):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the no-op leaves it too; a window that ends on a node needs no column beyond it
    assert lib.stk_transfer_prolong(st, *[dict(good, n_cols=0)[k] for k in order]) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert lib.stk_transfer_prolong(st, *[dict(good, n_cols=5, n_cc=3)[k] for k in order]) == 0  # columns 2 .. 6
    assert lib.stk_transfer_prolong(st, *[good[k] for k in order]) == 0
    assert same(out.cpu().numpy(), numpy_prolong(table, a, uc.cpu().numpy(), 1, 2, n_cols))


def test_the_plan_refuses_indices_outside_the_coarse_level():
    from source import _lib
    from source.transfer import _PlanHandle
    table, M_c = case_table('square23')
    lib = _lib.lib()
    for row, pair, text in ((40, (M_c, 3), 'not in [-1, M_coarse'), (41, (2, M_c), 'not in [-1, M_coarse'),
                            (40, (-2, 3), 'not in [-1, M_coarse'), (40, (3, -2), 'not in [-1, M_coarse'),
                            (0, (-1, -1), 'a copy pair without a row to copy')):
        bad = table.copy()
        bad[row] = pair
        with pytest.raises(_lib.StkError, match='stk_transfer_plan_create'):
            _PlanHandle(bad, M_c)
        assert text in lib.stk_last_error().decode() and 'parents[%d]' % row in lib.stk_last_error().decode()
    assert (table[M_c:] == -1).all(axis=1).any()  # between two boundary vertices it is allowed
    _PlanHandle(table, M_c)
    with pytest.raises(_lib.StkError, match='M_coarse'):
        _PlanHandle(table[:0], -1)


# ---- 5. the public call ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solver(problem, J, comm=None):
    """Shared, not to be changed.  J = J_space = J_time."""
    import heateq_mpi as hm
    from source.comm import Comm
    return hm.HeatEquationMPI(J_space=J, J_time=J, problem=problem, comm=Comm(distributed=False) if comm is None else comm)


@functools.lru_cache(maxsize=None)
def _serial(problem, J):
    import heateq
    return heateq.HeatEquation(J_space=J, J_time=J, problem=problem)


def _tables(mesh, levels):
    from source.transfer import parent_rows
    return [parent_rows(mesh, l) for l in range(mesh.J - levels + 1, mesh.J + 1)]


@pytest.mark.parametrize('problem,Jc,Jf', [('square_forced', 2, 3), ('square_forced', 3, 4), ('cube_forced', 1, 2),
                                           ('square_forced', 1, 3)])
def test_prolong_from_is_the_loop_and_the_same_function(problem, Jc, Jf):
    """P u_c equals the chained rule of the contract on the gathered vectors (J 1 -> 3: two space
    levels and two time levels at once), and it is the SAME function: sampled at random interior
    points and times, both sides are combinations of at most 2 (d + 1) terms with weights in
    [0, 1], rounded term by term -- a few ulps of max |u_c|, bounded here by 1e-13 max |u_c|."""
    from source import driver
    from source.mpi_vector import KronVectorMPI
    coarse, fine = _solver(problem, Jc), _solver(problem, Jf)
    u_c = driver.seeded_vector(coarse, KronVectorMPI)
    got = fine.prolong_from(coarse, u_c)
    assert isinstance(got, KronVectorMPI) and got.dofs_distr is fine.dofs_distr
    X_c = u_c.X_loc.cpu().numpy()  # (N_c, M_c)
    want = numpy_chain(_tables(fine._sample_meshes[0], Jf - Jc), Jf - Jc, np.ascontiguousarray(X_c.T))
    assert same(got.X_loc.cpu().numpy().T, want)
    assert bool((got.buf[:, got.n_loc:] == 0.0).all())  # the pad column
    key = (2**Jc, Jc + 1)
    assert list(fine.transfer_plans) == [key] or key in fine.transfer_plans
    plan = fine.transfer_plans[key][0]
    assert fine.prolong_from(coarse, u_c).buf.equal(got.buf) and fine.transfer_plans[key][0] is plan  # cached
    d = fine._sample_meshes[0].points.shape[1]
    rng = np.random.RandomState(50 + Jf)
    points, times = 0.02 + 0.96 * rng.rand(200, d), rng.rand(7)
    times[0], times[-1] = 0.0, 1.0
    on_fine, on_coarse = fine.sample(got, times, points), coarse.sample(u_c, times, points)
    gap, size = float((on_fine - on_coarse).abs().max()), float(np.abs(X_c).max())
    print('%s J %d -> %d: sample(fine, P u_c) against sample(coarse, u_c): %.3e of max|u_c| %.3e' % (problem, Jc, Jf, gap, size))
    assert not bool(torch.isnan(on_fine).any()) and gap <= 1e-13 * size
    with pytest.raises(ValueError, match='2\\^a times the elements'):
        coarse.prolong_from(fine, got)  # downwards is no prolongation
    with pytest.raises(AssertionError, match='trial space'):
        fine.prolong_from(coarse, got)


def test_serial_driver_takes_flat_and_device_vectors():
    from source import driver
    from source.linop import device_vector, host_vector
    from source.mpi_vector import KronVectorMPI
    coarse, fine = _solver('square_forced', 2), _solver('square_forced', 3)
    u_c = driver.seeded_vector(coarse, KronVectorMPI)
    want = fine.prolong_from(coarse, u_c).X_loc.cpu().numpy().reshape(-1)
    flat = u_c.X_loc.cpu().numpy().reshape(-1)
    s_coarse, s_fine = _serial('square_forced', 2), _serial('square_forced', 3)
    from_flat = s_fine.prolong_from(s_coarse, flat)
    from_device = s_fine.prolong_from(s_coarse, device_vector(flat, s_coarse.N))
    assert isinstance(from_flat, KronVectorMPI) and len(s_fine.transfer_plans) == 1
    assert same(host_vector(from_flat), want) and same(host_vector(from_device), want)
    # ... and across the two classes: the meshes decide, not the class
    assert same(host_vector(s_fine.prolong_from(coarse, u_c)), want)
    with pytest.raises(AssertionError, match='trial space'):
        s_fine.prolong_from(s_coarse, np.zeros(3 * s_coarse.N))


# ---- 6. rank independence -------------------------------------------------------------------------------------------
def _rank_run(comm, J_time, J_coarse):
    """This rank's columns of P u_c, J_space 2 -> 3 on the square, and its first column."""
    from source.comm import Comm
    from source.mpi_vector import DofDistributionMPI, KronVectorMPI
    from source.transfer import TransferPlan, prolong_collective
    comm = Comm(distributed=False) if comm is None else comm
    plan = TransferPlan(meshes('square', 2, J_coarse), meshes('square', 3, J_time))
    cd = DofDistributionMPI(comm, plan.N_coarse, plan.M_coarse)
    fd = DofDistributionMPI(comm, plan.N_fine, plan.M_fine)
    rows = np.stack([np.random.RandomState(900 + t).randn(plan.M_coarse) for t in range(cd.t_begin, cd.t_end)])
    out = prolong_collective(plan, KronVectorMPI(cd, rows), fd)
    torch.cuda.synchronize()
    return out.X_loc.cpu().numpy(), fd.t_begin


@functools.lru_cache(maxsize=None)
def _one_rank(J_time, J_coarse):
    return _rank_run(None, J_time, J_coarse)[0]


@pytest.mark.parametrize('J_time,J_coarse,ranks', [(3, 2, 2), (3, 2, 3), (3, 2, 4), (4, 3, 8)])
def test_prolongation_does_not_depend_on_the_number_of_ranks(J_time, J_coarse, ranks):
    from thread_comm import run_ranks
    one = _one_rank(J_time, J_coarse)
    got = run_ranks(ranks, lambda comm: _rank_run(comm, J_time, J_coarse))
    table = case_table('square23')[0]
    coarse = np.stack([np.random.RandomState(900 + t).randn(table.max() + 1) for t in range(2**J_coarse + 1)])
    assert same(one.T, numpy_prolong(table, J_time - J_coarse, coarse.T, 0, 0, 2**J_time + 1))
    at = 0
    for block, t_begin in got:
        assert t_begin == at and same(block, one[at:at + len(block)]), (ranks, t_begin)
        at += len(block)
    assert at == 2**J_time + 1
    if ranks == 3:  # nine nodes in blocks of three: a window that starts at an odd column
        assert any(t_begin & 1 for _, t_begin in got)


# ---- 7. solve(x0=) ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cold(J):
    """(u, iterations, history, error norms) of solve() on square_forced; shared."""
    heat, history = _solver('square_forced', J), []
    u, iters = heat.solve(history=history)
    return u, iters, history, heat.error_norms(u)


def _agree_to_three_digits(norms, cold):
    for key in ('l2_l2', 'l2_h1'):
        print('%s: %.9e against the cold solve\'s %.9e' % (key, norms[key], cold[key]))
        assert abs(norms[key] - cold[key]) <= 5e-4 * abs(cold[key]), key


def test_solve_from_zero_is_solve():
    from source.mpi_vector import KronVectorMPI
    heat = _solver('square_forced', 3)
    u, iters, history, _ = _cold(3)
    again = []
    v, n = heat.solve(x0=KronVectorMPI(heat.dofs_distr), history=again)
    assert n == iters and again == history and bool((v.buf == u.buf).all())


def test_solve_from_the_solution_takes_no_step():
    heat = _solver('square_forced', 3)
    tight, _ = heat.solve(eps=1e-9)
    history = []
    u, iters = heat.solve(x0=tight, eps=1e-6, history=history)
    print('r.Pr of the correction from a solve to eps = 1e-9: %.3e' % history[0])
    assert iters == 0 and len(history) == 1 and history[0] < 1e-12
    assert bool((u.buf == tight.buf).all())


def test_solve_from_the_prolonged_coarse_solution():
    coarse, heat = _solver('square_forced', 2), _solver('square_forced', 3)
    u_c, _ = coarse.solve()
    history = []
    u, iters = heat.solve(x0=heat.prolong_from(coarse, u_c), history=history)
    _, cold_iters, cold_history, cold_norms = _cold(3)
    print('nested start: %d PCG steps, r.Pr %.3e -> %.3e; cold start: %d steps, r.Pr %.3e -> %.3e'
          % (iters, history[0], history[-1], cold_iters, cold_history[0], cold_history[-1]))
    assert history[0] < cold_history[0] and history[-1] < 1e-12
    _agree_to_three_digits(heat.error_norms(u), cold_norms)


# ---- 8. the drivers' --nested ----------------------------------------------------------------------------------------------
def test_drivers_solve_nested(monkeypatch, capsys):
    import heateq
    import heateq_mpi as hm
    from source.mpi_kron import LinearOperatorMPI
    monkeypatch.setattr(LinearOperatorMPI, 'sync_timing', LinearOperatorMPI.sync_timing)  # main() sets it
    common = ['--J_time', '3', '--J_space', '3', '--problem', 'square_forced']
    cold_norms = _cold(3)[3]
    for name, main in (('mpi', hm.main), ('serial', heateq.main)):
        capsys.readouterr()
        plain = main(common)
        printed = capsys.readouterr().out
        assert 'nested' not in printed.lower()  # the option is taken off the command line the drivers print
        assert plain[0].transfer_plans == {}
        again = main(common + ['--nested', '0'])
        arguments = lambda text: [line for line in text.splitlines() if line.startswith('Arguments:')]  # noqa: E731
        zero = capsys.readouterr().out
        assert 'nested' not in zero.lower() and len(arguments(zero)) == 1 and arguments(zero) == arguments(printed)
        assert again[2] == plain[2] and again[0].transfer_plans == {}
        res = main(common + ['--nested', '1'])
        printed = capsys.readouterr().out
        lines = [line for line in printed.splitlines() if line.startswith('Nested level')]
        assert len(lines) == 2 and 'J_time = 2, J_space = 2' in lines[0] and 'from zero' in lines[0], printed
        assert 'J_time = 3, J_space = 3' in lines[1] and 'from zero' not in lines[1], printed
        print('%s: %s' % (name, lines))
        heat, u = res[0], res[1]
        assert len(heat.transfer_plans) == 1
        _agree_to_three_digits(heat.error_norms(u), cold_norms)
    with pytest.raises(SystemExit, match='there is no level'):
        hm.main(common + ['--nested', '4'])
    with pytest.raises(SystemExit, match='at least 0'):
        heateq.main(common + ['--nested', '-1'])
    with pytest.raises(SystemExit, match='problem with forcing'):
        hm.main(['--J_time', '2', '--J_space', '2', '--problem', 'square', '--nested', '1'])


# ---- 9. the torch composition of the timing tool ----------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location('transfer_time', os.path.join(REPO, 'tools', 'transfer_time.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_timed_composition_computes_what_the_kernel_computes():
    from source.transfer import TransferPlan, parent_rows, prolong_window
    coarse, fine = meshes('square', 3, 2), meshes('square', 4, 3)
    plan = TransferPlan(coarse, fine)
    assert (plan.a, plan.s, plan.N_coarse, plan.N_fine) == (1, 1, 5, 9)
    table = parent_rows(fine[0])
    uc = torch.randn((plan.M_coarse, 5), dtype=torch.float64, device=_dev(np.zeros(1)).device)
    out = torch.full((plan.M_fine, 10), SENTINEL, dtype=torch.float64, device=uc.device)
    prolong_window(plan, uc, 5, 5, out, 10, 0, 9)
    ref = _tool().torch_composition(_dev(table.astype(np.int64)), 1, uc, torch.full_like(out, SENTINEL))
    assert torch.equal(out, ref) and bool((out[:, 9] == SENTINEL).all())
    assert same(out[:, :9].cpu().numpy(), numpy_prolong(table, 1, uc.cpu().numpy(), 0, 0, 9))
