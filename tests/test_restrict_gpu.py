"""The restriction P^T on the device (csrc/transfer.hip, source/transfer.py) against the NumPy
contract of tests/test_restrict_host.py -- array_equal, NaN-aware: the kernel on the four mesh
pairs at every edge of the stencils, window, stride and alignment, the longest folds, synthetic
tables, non-finite input, every launch form and cut, the refusals, the public call of both
drivers, the adjoint identities with prolong_from and sample_along_adjoint, its independence of
the number of ranks, solve_nested(rhs=), the drivers' --nested_rhs, and the torch composition the
timing tool compares with."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_restrict_host import (N_COARSE, SYNTHETIC, numpy_children, numpy_restrict, numpy_restrict_chain,
                                numpy_space_T, numpy_time_T)
from test_transfer_host import CASES, case_table, dyadic, meshes, numpy_chain, same

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 123.25


def _dev(a):
    from source import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(_lib.compute_device())


@functools.lru_cache(maxsize=None)
def _level(case):
    """(the device plan of the transposed space level of a case, its table, M_c)."""
    from source.transfer import _RestrictHandle
    table, M_c = case_table(case) if case in CASES else SYNTHETIC[case]()
    return _RestrictHandle(table, M_c), table, M_c


def _restrict(level, a, f, k_first, n_fine, q_first, n_qc, ld=None, ldc=None, off_out=0, off_f=0, rows=None):
    """stk_transfer_restrict (`level` a plan) or stk_transfer_restrict_time (`level` None, over
    `rows` rows) on fresh buffers: `f` (M_f, n_cols) NumPy, the fine columns from k_first, at row
    stride ld with NaN between the rows, based `off_f` doubles into its buffer; out at row
    stride ldc, pre-filled with SENTINEL, based `off_out` doubles in.  Returns (the (M_c, n_qc)
    result, True iff every other double of the out buffer still holds SENTINEL)."""
    from source.transfer import restrict_scan, restrict_time_scan
    M_f, n_cols = f.shape
    M_c = rows if level is None else level.M_coarse
    ld = n_cols if ld is None else ld
    ldc = n_qc if ldc is None else ldc
    src = np.full(off_f + max(M_f, 1) * ld + 1, np.nan)
    if M_f:
        src[off_f:off_f + M_f * ld].reshape(M_f, ld)[:, :n_cols] = f
    src, dst = _dev(src), _dev(np.full(off_out + M_c * ldc + 1, SENTINEL))
    if level is None:
        restrict_time_scan(M_c, a, src.data_ptr() + 8 * off_f, ld, k_first, n_cols, n_fine,
                           dst.data_ptr() + 8 * off_out, ldc, q_first, n_qc)
    else:
        restrict_scan(level, a, src.data_ptr() + 8 * off_f, ld, k_first, n_cols, n_fine,
                      dst.data_ptr() + 8 * off_out, ldc, q_first, n_qc)
    flat = dst.cpu().numpy()
    body = flat[off_out:off_out + M_c * ldc].reshape(M_c, ldc)
    kept = bool(np.all(body[:, n_qc:] == SENTINEL)) and bool(np.all(flat[:off_out] == SENTINEL)) and bool(
        np.all(flat[off_out + M_c * ldc:] == SENTINEL))
    return body[:, :n_qc].copy(), kept


class _tile:
    """The kernel's launch form for the block: rows per workgroup, LDS in KiB (stk_restrict_tile)."""
    def __init__(self, rows, kib):
        self.shape = (rows, kib)

    def __enter__(self):
        from source import _lib
        _lib.check(_lib.lib().stk_restrict_tile(*self.shape))

    def __exit__(self, *exc):
        from source import _lib
        _lib.check(_lib.lib().stk_restrict_tile(0, 0))


# ---- 1. the device is the contract ------------------------------------------------------------------------------------
@pytest.mark.parametrize('a', [0, 1, 2, 3])
@pytest.mark.parametrize('case', sorted(CASES))
def test_device_is_the_contract(case, a):
    """n_qc in {1, 2, all}; q_first at node 0, interior and such that the last node closes the
    range (one-sided stencils at both ends); the fine window exactly what the stencils read and one
    column wider at either end; ld and ldc tight, odd, even and beyond; f and out based at +8
    bytes; the pads and the doubles around out unchanged."""
    from source.transfer import stencil_window
    level, table, M_c = _level(case)
    rng = np.random.RandomState(100 * a + len(case))
    n_fine = ((N_COARSE - 1) << a) + 1
    whole = rng.randn(len(table), n_fine)
    seen = {'first_node': 0, 'interior': 0, 'last_node': 0, 'exact_window': 0, 'wider_window': 0, 'odd_ld': 0,
            'even_ld': 0, 'tight_ld': 0, 'wide_ld': 0, 'tight_ldc': 0, 'odd_ldc': 0, 'even_ldc': 0, 'wide_ldc': 0,
            'shifted_out': 0, 'shifted_f': 0, 'odd_k_first': 0}
    number = 0
    want = None
    for n_qc in (1, 2, N_COARSE):
        for q_first in sorted({0, 1, 2, N_COARSE - n_qc}):
            if q_first + n_qc > N_COARSE:
                continue
            for widen in (0, 1):
                number += 1
                k_lo, k_hi = stencil_window(a, q_first, n_qc, n_fine)
                lo, hi = max(k_lo - widen, 0), min(k_hi + widen, n_fine - 1)
                n_cols = hi - lo + 1
                ld = n_cols + (0, 1, 2, 5)[number % 4]
                ldc = n_qc + (0, 1, 2, 5)[(number // 2) % 4]
                off_out, off_f = ((0, 0), (1, 0), (0, 1), (1, 1))[(number // 3) % 4]
                got, kept = _restrict(level, a, whole[:, lo:hi + 1], lo, n_fine, q_first, n_qc, ld, ldc, off_out, off_f)
                want = numpy_restrict(table, M_c, a, whole[:, lo:hi + 1], lo, n_fine, q_first, n_qc)
                assert same(got, want) and kept, (n_qc, q_first, widen, ld, ldc, off_out, off_f)
                seen['first_node'] += q_first == 0
                seen['last_node'] += q_first + n_qc == N_COARSE
                seen['interior'] += q_first > 0 and q_first + n_qc < N_COARSE
                seen['exact_window' if (lo, hi) == (k_lo, k_hi) else 'wider_window'] += 1
                seen['odd_ld' if ld & 1 else 'even_ld'] += 1
                seen['tight_ld'] += ld == n_cols
                seen['wide_ld'] += ld > n_cols + 1
                seen['odd_ldc' if ldc & 1 else 'even_ldc'] += 1
                seen['tight_ldc'] += ldc == n_qc
                seen['wide_ldc'] += ldc > n_qc + 1
                seen['shifted_out'] += off_out
                seen['shifted_f'] += off_f
                seen['odd_k_first'] += lo & 1
    assert all(seen.values()), seen
    assert not np.isnan(want).any()  # no NaN from between the fine rows came in


@pytest.mark.parametrize('n_coarse', [2, 3])
def test_the_longest_folds(n_coarse):
    """a = 8: one-sided stencils of 256 terms (two coarse nodes) and, with a node between them,
    the full stencil of 511; in space and time on square 0 -> 1 (M_c = 1) and in time only."""
    a, n_fine = 8, ((n_coarse - 1) << 8) + 1
    level, table, M_c = _level('square01')
    f = np.random.RandomState(8).randn(len(table), n_fine)
    got, kept = _restrict(level, a, f, 0, n_fine, 0, n_coarse)
    assert same(got, numpy_restrict(table, M_c, a, f, 0, n_fine, 0, n_coarse)) and kept
    got, kept = _restrict(None, a, f, 0, n_fine, 0, n_coarse, rows=len(table))
    assert same(got, numpy_time_T(a, f, 0, n_fine, 0, n_coarse)) and kept
    # the last coarse node alone, from exactly its 256 columns, based at an odd column
    got, kept = _restrict(level, a, f[:, n_fine - 256:], n_fine - 256, n_fine, n_coarse - 1, 1)
    assert same(got, numpy_restrict(table, M_c, a, f, 0, n_fine, n_coarse - 1, 1)) and kept


# ---- 2. synthetic tables -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(SYNTHETIC))
def test_synthetic_tables(name):
    """Rows with 0 and 1 entries and one with 301 (longer than a wavefront and than a tile), more
    coarse rows than fine ones, an identity table, M_c = 0 (a no-op) and M_f = 0 (zeros)."""
    level, table, M_c = _level(name)
    rng = np.random.RandomState(len(name))
    for a, n_coarse in ((0, 3), (1, 3), (2, 2)):
        n_fine = ((n_coarse - 1) << a) + 1
        f = rng.randn(len(table), n_fine)
        for rows in (0, 4):  # the default tile and one that M_c = 7 and 9 are no multiple of
            with _tile(rows, 0):
                got, kept = _restrict(level, a, f, 0, n_fine, 0, n_coarse)
            assert got.shape == (M_c, n_coarse) and kept
            assert same(got, numpy_restrict(table, M_c, a, f, 0, n_fine, 0, n_coarse)), (a, rows)
        if name == 'no_fine_rows':
            assert np.all(got == 0.0) and M_c == 4
        if name == 'identity' and a == 0:
            assert same(got, f)


# ---- 3. NaN and +-inf ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['cube12', 'square23'])
def test_non_finite_values_give_what_the_loop_gives(case):
    level, table, M_c = _level(case)
    rng = np.random.RandomState(2)
    lists = numpy_children(table, M_c)
    for a in (0, 1, 2):
        n_fine = ((N_COARSE - 1) << a) + 1
        # one NaN: it reaches exactly the coarse rows that list its row, in the stencils that hold its column
        f = rng.randn(len(table), n_fine)
        row, col = len(table) - 3, n_fine // 2 + 1
        f[row, col] = np.nan
        got, kept = _restrict(level, a, f, 0, n_fine, 0, N_COARSE)
        assert same(got, numpy_restrict(table, M_c, a, f, 0, n_fine, 0, N_COARSE)) and kept, a
        listing = [j for j in range(M_c) if row in [i for i, _ in lists[j]]]
        holding = [q for q in range(N_COARSE) if abs(col - (q << a)) < (1 << a)]
        assert listing and holding
        reached = np.zeros((M_c, N_COARSE), dtype=bool)
        reached[np.ix_(listing, holding)] = True
        assert np.array_equal(np.isnan(got), reached)
        # inf - inf within one coarse row gives the loop's NaN, a lone inf stays inf
        f = rng.randn(len(table), n_fine)
        j = max(range(M_c), key=lambda j: len(lists[j]))
        (i1, _), (i2, _) = lists[j][0], lists[j][-1]
        assert i1 != i2
        f[i1, 0], f[i2, 0], f[i1, n_fine - 1] = np.inf, -np.inf, -np.inf
        got, kept = _restrict(level, a, f, 0, n_fine, 0, N_COARSE)
        want = numpy_restrict(table, M_c, a, f, 0, n_fine, 0, N_COARSE)
        assert same(got, want) and kept, a
        assert np.isnan(got[j, 0]) and got[j, N_COARSE - 1] == -np.inf and not np.isnan(f).any()
        # many of them
        f[rng.rand(*f.shape) < 0.02] = np.nan
        f[rng.rand(*f.shape) < 0.05] = np.inf
        f[rng.rand(*f.shape) < 0.05] = -np.inf
        got, kept = _restrict(level, a, f, 0, n_fine, 0, N_COARSE)
        assert same(got, numpy_restrict(table, M_c, a, f, 0, n_fine, 0, N_COARSE)) and kept, a


# ---- 4. launch forms and cuts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,kib', [(1, 64), (4, 64), (32, 64), (64, 64), (256, 64), (256, 1), (64, 1), (7, 1), (1, 1),
                                      (64, 4), (256, 16)])
def test_every_launch_form_gives_the_one_shot_doubles(rows, kib):
    """1 .. 256 rows per workgroup; 1 KiB of LDS forces chunks of a single coarse column and
    tiles of fewer rows (at a = 3 and 64 rows: 8 rows of one stencil), 4 and 16 KiB chunks whose
    last one is shorter; out aligned and not."""
    level, table, M_c = _level('lshape23')
    for a in (0, 1, 3):
        n_fine = (8 << a) + 1
        f = np.random.RandomState(3 + a).randn(len(table), n_fine)
        for q_first, n_qc, off_out in ((0, 9, 0), (2, 5, 1), (8, 1, 0)):
            want = numpy_restrict(table, M_c, a, f, 0, n_fine, q_first, n_qc)
            with _tile(rows, kib):
                got, kept = _restrict(level, a, f, 0, n_fine, q_first, n_qc, off_out=off_out)
            assert same(got, want) and kept, (a, q_first, n_qc, off_out)


def test_a_call_cut_into_column_ranges_is_the_one_call():
    from source.transfer import stencil_window
    level, table, M_c = _level('square23')
    a, n_fine = 2, 17
    f = np.random.RandomState(4).randn(len(table), n_fine)
    whole, _ = _restrict(level, a, f, 0, n_fine, 0, N_COARSE)
    assert same(whole, numpy_restrict(table, M_c, a, f, 0, n_fine, 0, N_COARSE))
    for cut in range(1, N_COARSE):
        parts = []
        for q_first, n_qc in ((0, cut), (cut, N_COARSE - cut)):
            lo, hi = stencil_window(a, q_first, n_qc, n_fine)
            part, kept = _restrict(level, a, f[:, lo:hi + 1], lo, n_fine, q_first, n_qc)
            assert kept
            parts.append(part)
        assert same(np.concatenate(parts, axis=1), whole), cut


@pytest.mark.parametrize('case', ['square23', 'cube12'])
def test_space_then_time_is_the_fused_call(case):
    """What the multi-rank route rests on: "space with a = 0" followed by "time only" gives the
    doubles of the one call, and so does space on column blocks written side by side."""
    level, table, M_c = _level(case)
    for a in (1, 3):
        n_fine = ((N_COARSE - 1) << a) + 1
        f = np.random.RandomState(5 + a).randn(len(table), n_fine)
        f[3, 2] = np.inf
        fused, _ = _restrict(level, a, f, 0, n_fine, 0, N_COARSE)
        blocks = [_restrict(level, 0, f[:, k:k + n], k, n_fine, k, n)[0] for k, n in ((0, 3), (3, n_fine - 3))]
        space = np.concatenate(blocks, axis=1)
        assert same(space, numpy_space_T(table, M_c, f))
        split, kept = _restrict(None, a, space, 0, n_fine, 0, N_COARSE, rows=M_c)
        assert same(split, fused) and kept, a


def test_tile_setter_refuses_other_shapes_and_changes_nothing():
    from source import _lib
    lib = _lib.lib()
    level, table, M_c = _level('square23')
    f = np.random.RandomState(5).randn(len(table), 9)
    before, _ = _restrict(level, 1, f, 0, 9, 0, 5)
    for rows, kib, name in ((-1, 64, 'rows'), (257, 0, 'rows'), (32, 65, 'lds_kib'), (32, -1, 'lds_kib')):
        assert lib.stk_restrict_tile(rows, kib) != 0 and name in lib.stk_last_error().decode(), (rows, kib)
        after, kept = _restrict(level, 1, f, 0, 9, 0, 5)
        assert same(after, before) and kept
    assert lib.stk_restrict_tile(0, 0) == 0


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_out_untouched():
    from source import _lib
    lib = _lib.lib()
    level, table, M_c = _level('square23')
    a, n_fine, q_first, n_qc = 1, 9, 1, 2  # the coarse columns 1 .. 2 read the fine columns 1 .. 5
    n_cols = 5
    f = _dev(np.random.RandomState(6).randn(len(table), n_cols))
    out = _dev(np.full((M_c, n_qc), SENTINEL))
    st = _lib.stream()
    good = dict(plan=level, a=a, f=f.data_ptr(), ld=n_cols, k_first=1, n_cols=n_cols, n_fine=n_fine, out=out.data_ptr(),
                ldc=n_qc, q_first=q_first, n_qc=n_qc)
    order = ('plan', 'a', 'f', 'ld', 'k_first', 'n_cols', 'n_fine', 'out', 'ldc', 'q_first', 'n_qc')
    cases = [
        (' plan is null', dict(plan=None)), (' f is null', dict(f=None)), (' out is null', dict(out=None)),
        (' a = -1', dict(a=-1)), (' a = 9', dict(a=9)), (' n_cols = -1', dict(n_cols=-1)), (' n_qc = -1', dict(n_qc=-1)),
        (' n_fine = -1', dict(n_fine=-1)), (' k_first = -1', dict(k_first=-1)), (' q_first = -1', dict(q_first=-1)),
        (' ld = 4 is below n_cols', dict(ld=n_cols - 1)), (' ldc = 1 is below n_qc', dict(ldc=n_qc - 1)),
        (' n_fine = 10: n_fine - 1 is no multiple of 2^a', dict(n_fine=10)),
        (' = [4, 6) reach beyond the last coarse node 4', dict(q_first=4, k_first=7)),
        (' = [2, 6) does not cover', dict(k_first=2, n_cols=4, ld=4)),  # short by one at the lower end
        (' = [1, 5) does not cover', dict(n_cols=4)),  # ... at the upper end
        (' = [1, 6) does not cover the columns [0, 5]', dict(q_first=0, n_qc=3, ldc=3)),  # node 0 reads column 0
    ]
    for name, change in cases:
        args = dict(good, **change)
        rc = lib.stk_transfer_restrict(st, *[args[k] for k in order])
        text = lib.stk_last_error().decode()
        assert rc != 0 and 'stk_transfer_restrict:' in text and name in text, (name, change, rc, text)
        with pytest.raises(_lib.StkError):
            _lib.check(rc)
        if 'plan' not in change:  # the time-only form makes the same checks
            rc = lib.stk_transfer_restrict_time(st, len(table), *[args[k] for k in order[1:]])
            text = lib.stk_last_error().decode()
            assert rc != 0 and 'stk_transfer_restrict_time:' in text and name in text, (name, change, rc, text)
    assert lib.stk_transfer_restrict_time(st, -1, *[good[k] for k in order[1:]]) != 0
    assert ' M = -1' in lib.stk_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the no-op leaves it too; the last node's one-sided stencil needs no column beyond the mesh
    assert lib.stk_transfer_restrict(st, *[dict(good, n_qc=0)[k] for k in order]) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert lib.stk_transfer_restrict(st, *[dict(good, q_first=3, k_first=5, n_cols=4)[k] for k in order]) == 0
    assert lib.stk_transfer_restrict(st, *[good[k] for k in order]) == 0
    assert same(out.cpu().numpy(), numpy_restrict(table, M_c, a, f.cpu().numpy(), 1, n_fine, q_first, n_qc))


def test_the_plan_refuses_indices_outside_the_coarse_level():
    from source import _lib
    from source.transfer import _RestrictHandle
    table, M_c = case_table('square23')
    lib = _lib.lib()
    for row, pair, text in ((40, (M_c, 3), 'not in [-1, M_coarse'), (41, (2, M_c), 'not in [-1, M_coarse'),
                            (40, (-2, 3), 'not in [-1, M_coarse'), (40, (3, -2), 'not in [-1, M_coarse'),
                            (0, (-1, -1), 'a copy pair without a row to copy')):
        bad = table.copy()
        bad[row] = pair
        with pytest.raises(_lib.StkError, match='stk_restrict_plan_create'):
            _RestrictHandle(bad, M_c)
        assert text in lib.stk_last_error().decode() and 'parents[%d]' % row in lib.stk_last_error().decode()
    _RestrictHandle(table, M_c)
    with pytest.raises(_lib.StkError, match='M_coarse'):
        _RestrictHandle(table[:0], -1)


# ---- 6. the public call ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solver(problem, J_space, J_time):
    """Shared, not to be changed."""
    import heateq_mpi as hm
    from source.comm import Comm
    return hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem=problem, comm=Comm(distributed=False))


@functools.lru_cache(maxsize=None)
def _serial(problem, J_space, J_time):
    import heateq
    return heateq.HeatEquation(J_space=J_space, J_time=J_time, problem=problem)


def _tables(mesh, levels):
    from source.transfer import parent_rows
    tables = [parent_rows(mesh, l) for l in range(mesh.J - levels + 1, mesh.J + 1)]
    free = ~np.asarray(mesh.boundary, dtype=bool)
    sizes = [int(np.count_nonzero(free[:mesh.nverts[l]])) for l in range(mesh.J - levels, mesh.J)]
    return tables, sizes


def _vector(heat, X):
    """(N, M) NumPy as a KronVectorMPI of a one-rank driver."""
    from source.mpi_vector import KronVectorMPI
    return KronVectorMPI(heat.dofs_distr, X)


J_TIME = 2


@pytest.mark.parametrize('a', [0, 1])
@pytest.mark.parametrize('problem,Jc,Jf', [('square_forced', 2, 3), ('square_forced', 1, 3), ('lshape', 2, 3),
                                           ('cube_forced', 1, 2)])
def test_restrict_to_is_the_loop_and_the_adjoint_of_prolong_from(problem, Jc, Jf, a):
    """P^T f equals the chained loop (J_space 1 -> 3: two space levels), and through the public
    calls <P u, f> == <u, P^T f> as an equality of doubles on dyadic data."""
    from source.mpi_vector import KronVectorMPI
    coarse, fine = _solver(problem, Jc, J_TIME - a), _solver(problem, Jf, J_TIME)
    rng = np.random.RandomState(10 * Jf + a)
    F = rng.randn(fine.N, fine.M)
    got = fine.restrict_to(coarse, _vector(fine, F))
    assert isinstance(got, KronVectorMPI) and got.dofs_distr is coarse.dofs_distr
    tables, sizes = _tables(fine._sample_meshes[0], Jf - Jc)
    want = numpy_restrict_chain(tables, sizes, a, np.ascontiguousarray(F.T))
    assert same(got.X_loc.cpu().numpy().T, want)
    assert bool((got.buf[:, got.n_loc:] == 0.0).all())  # the pad column
    key = (2**(J_TIME - a), Jc + 1)
    plan = fine.transfer_plans[key][0]
    assert fine.restrict_to(coarse, _vector(fine, F)).buf.equal(got.buf) and fine.transfer_plans[key][0] is plan  # cached
    # the adjoint identity, exactly: dyadic data
    U, F = dyadic(rng, (coarse.N, coarse.M)), dyadic(rng, (fine.N, fine.M))
    Pu = fine.prolong_from(coarse, _vector(coarse, U)).X_loc.cpu().numpy()
    PTf = fine.restrict_to(coarse, _vector(fine, F)).X_loc.cpu().numpy()
    assert same(Pu.T, numpy_chain(tables, a, np.ascontiguousarray(U.T)))
    assert float(np.sum(Pu * F)) == float(np.sum(U * PTf))
    with pytest.raises(ValueError, match='2\\^a times the elements|not nested'):
        coarse.restrict_to(fine, _vector(coarse, U))  # upwards is no restriction
    with pytest.raises(AssertionError, match='trial space'):
        fine.restrict_to(coarse, _vector(coarse, U))


def test_the_transposed_tables_are_built_by_the_first_restriction():
    from source.transfer import TransferPlan
    plan = TransferPlan(meshes('square', 2, 1), meshes('square', 3, 2))
    assert plan._transposed is None
    u = torch.zeros((plan.M_coarse, plan.N_coarse), dtype=torch.float64, device=_dev(np.zeros(1)).device)
    from source.transfer import prolong_window, restrict_window
    out = torch.empty((plan.M_fine, plan.N_fine), dtype=torch.float64, device=u.device)
    prolong_window(plan, u, plan.N_coarse, plan.N_coarse, out, plan.N_fine, 0, plan.N_fine)
    assert plan._transposed is None  # a run that only prolongs builds nothing of it
    restrict_window(plan, out, plan.N_fine, 0, plan.N_fine, u, plan.N_coarse, 0, plan.N_coarse)
    assert len(plan._transposed) == 1 and bool((u == 0.0).all())


def test_serial_driver_takes_flat_and_device_vectors():
    from source.linop import device_vector, host_vector
    from source.mpi_vector import KronVectorMPI
    coarse, fine = _solver('square_forced', 2, J_TIME - 1), _solver('square_forced', 3, J_TIME)
    F = np.random.RandomState(12).randn(fine.N, fine.M)
    want = fine.restrict_to(coarse, _vector(fine, F)).X_loc.cpu().numpy().reshape(-1)
    s_coarse, s_fine = _serial('square_forced', 2, J_TIME - 1), _serial('square_forced', 3, J_TIME)
    flat = F.reshape(-1)
    from_flat = s_fine.restrict_to(s_coarse, flat)
    from_device = s_fine.restrict_to(s_coarse, device_vector(flat, s_fine.N))
    assert isinstance(from_flat, KronVectorMPI) and len(s_fine.transfer_plans) == 1
    assert same(host_vector(from_flat), want) and same(host_vector(from_device), want)
    assert same(host_vector(s_fine.restrict_to(coarse, flat)), want)  # the meshes decide, not the class
    with pytest.raises(AssertionError, match='trial space'):
        s_fine.restrict_to(s_coarse, np.zeros(3 * s_fine.N))


def test_sampling_the_coarse_function_is_sampling_its_prolongation():
    """E_c = E_f P, so E_c^T w = P^T E_f^T w: one level down in space and in time, 64 random
    pairs inside the mesh.  Fewer than 200 rounded operations lie on any entry's path (64 pairs,
    a = 1, at most 15 entries per row): 200 * 2^-53 = 2.2e-14, bounded by 1e-13 max(E_c^T |w|)."""
    coarse, fine = _solver('square_forced', 2, J_TIME - 1), _solver('square_forced', 3, J_TIME)
    rng = np.random.RandomState(64)
    points, times, w = 0.02 + 0.96 * rng.rand(64, 2), rng.rand(64), rng.randn(64)
    on_fine, used_f = fine.sample_along_adjoint(w, times, points)
    on_coarse, used_c = coarse.sample_along_adjoint(w, times, points)
    size, _ = coarse.sample_along_adjoint(np.abs(w), times, points)
    assert bool(used_f.all()) and bool(used_c.all())
    got = fine.restrict_to(coarse, on_fine)
    gap = float((got.X_loc - on_coarse.X_loc).abs().max())
    bound = 1e-13 * float(size.X_loc.max())
    print('P^T E_f^T w against E_c^T w: largest gap %.3e, bound %.3e' % (gap, bound))
    assert not bool(torch.isnan(got.X_loc).any()) and float(on_coarse.X_loc.abs().max()) > 0.0
    assert gap <= bound


# ---- 7. rank independence -------------------------------------------------------------------------------------------
def _rank_run(comm, J_time, J_coarse, Js_coarse):
    """This rank's columns of P^T f, J_space Js_coarse -> 3 on the square, and its first column."""
    from source.comm import Comm
    from source.mpi_vector import DofDistributionMPI, KronVectorMPI
    from source.transfer import TransferPlan, restrict_collective
    comm = Comm(distributed=False) if comm is None else comm
    plan = TransferPlan(meshes('square', Js_coarse, J_coarse), meshes('square', 3, J_time))
    cd = DofDistributionMPI(comm, plan.N_coarse, plan.M_coarse)
    fd = DofDistributionMPI(comm, plan.N_fine, plan.M_fine)
    rows = np.stack([np.random.RandomState(900 + t).randn(plan.M_fine) for t in range(fd.t_begin, fd.t_end)])
    out = restrict_collective(plan, KronVectorMPI(fd, rows), cd)
    torch.cuda.synchronize()
    return out.X_loc.cpu().numpy(), cd.t_begin, fd.t_begin


@functools.lru_cache(maxsize=None)
def _one_rank(J_time, J_coarse, Js_coarse):
    return _rank_run(None, J_time, J_coarse, Js_coarse)[0]


@pytest.mark.parametrize('J_time,J_coarse,ranks,Js_coarse', [(3, 2, 2, 2), (3, 2, 3, 2), (3, 2, 4, 2), (4, 3, 8, 2),
                                                             (3, 2, 3, 1), (3, 3, 3, 3)])
def test_restriction_does_not_depend_on_the_number_of_ranks(J_time, J_coarse, ranks, Js_coarse):
    from source.transfer import parent_rows
    from thread_comm import run_ranks
    one = _one_rank(J_time, J_coarse, Js_coarse)
    got = run_ranks(ranks, lambda comm: _rank_run(comm, J_time, J_coarse, Js_coarse))
    mesh = meshes('square', 3, J_time)[0]
    fine = np.stack([np.random.RandomState(900 + t).randn(int(np.count_nonzero(~mesh.boundary)))
                     for t in range(2**J_time + 1)])
    if Js_coarse < 3:
        tables, sizes = _tables(mesh, 3 - Js_coarse)
        assert same(one.T, numpy_restrict_chain(tables, sizes, J_time - J_coarse, np.ascontiguousarray(fine.T)))
    else:
        assert same(one, fine)  # the same discretisation: a copy
    at = 0
    for block, t_begin, _ in got:
        assert t_begin == at and same(block, one[at:at + len(block)]), (ranks, t_begin)
        at += len(block)
    assert at == 2**J_coarse + 1
    if ranks == 3 and J_time == 3:  # nine nodes in blocks of three: a fine window that starts at an odd column
        assert any(f_begin & 1 for _, _, f_begin in got)


# ---- 8. solve_nested(rhs=) and the drivers' --nested_rhs -------------------------------------------------------------
def _agree_to_three_digits(norms, cold):
    for key in ('l2_l2', 'l2_h1'):
        print('%s: %.9e against the cold solve\'s %.9e' % (key, norms[key], cold[key]))
        assert abs(norms[key] - cold[key]) <= 5e-4 * abs(cold[key]), key


def test_solve_nested_for_a_functional_of_point_data(capsys):
    """The nested misfit-gradient solve: E^T w exists only as a fine vector; the coarser level
    solves for P^T E^T w, the fine level from its prolonged solution."""
    from source import driver
    heat = _solver('square_forced', 3, 3)
    rng = np.random.RandomState(21)
    points, times, w = 0.05 + 0.9 * rng.rand(32, 2), rng.rand(32), rng.randn(32)
    vec, used = heat.sample_along_adjoint(w, times, points)
    assert bool(used.all())
    cold_history = []
    cold, cold_iters = heat.solve(rhs=vec, history=cold_history)
    history = []
    capsys.readouterr()
    u, iters, counts = driver.solve_nested(heat, lambda J_time, J_space: _solver('square_forced', J_space, J_time),
                                           [(2, 2)], rhs=vec, history=history)
    lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith('Nested level')]
    assert len(lines) == 2 and 'J_time = 2, J_space = 2' in lines[0] and 'from zero' in lines[0]
    assert 'for the restricted right-hand side' in lines[0] and 'for the given right-hand side' in lines[1]
    assert [c[:2] for c in counts] == [(2, 2), (3, 3)] and counts[-1][2] == iters
    print('nested start: %d PCG steps, r.Pr %.3e -> %.3e; cold start: %d steps, r.Pr %.3e -> %.3e'
          % (iters, history[0], history[-1], cold_iters, cold_history[0], cold_history[-1]))
    assert history[0] < cold_history[0] and history[-1] < 1e-12
    _agree_to_three_digits(heat.error_norms(u), heat.error_norms(cold))


def test_drivers_nested_rhs(monkeypatch, capsys):
    import heateq
    import heateq_mpi as hm
    from source.mpi_kron import LinearOperatorMPI
    monkeypatch.setattr(LinearOperatorMPI, 'sync_timing', LinearOperatorMPI.sync_timing)  # main() sets it
    common = ['--J_time', '3', '--J_space', '3', '--problem', 'square_forced']
    kept = lambda text: [line for line in text.splitlines()  # noqa: E731
                         if line.startswith('Nested level') or line.startswith('Arguments:')]
    capsys.readouterr()
    today = hm.main(common + ['--nested', '1'])
    printed_today = capsys.readouterr().out
    own = hm.main(common + ['--nested', '1', '--nested_rhs', 'own'])
    printed_own = capsys.readouterr().out
    assert kept(printed_own) == kept(printed_today) and len(kept(printed_own)) == 3 and own[2] == today[2]
    assert 'nested' not in ''.join(line for line in kept(printed_own) if line.startswith('Arguments:')).lower()
    assert 'restricted' not in printed_own and bool((own[1].buf == today[1].buf).all())
    cold_norms = today[0].error_norms(today[0].solve()[0])
    for name, main in (('mpi', hm.main), ('serial', heateq.main)):
        res = main(common + ['--nested', '1', '--nested_rhs', 'restricted'])
        lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith('Nested level')]
        print('%s: %s' % (name, lines))
        assert len(lines) == 2 and 'J_time = 2, J_space = 2' in lines[0] and 'from zero' in lines[0]
        assert 'for the restricted right-hand side' in lines[0] and 'for the given right-hand side' in lines[1]
        heat, u = res[0], res[1]
        assert len(heat.transfer_plans) == 1
        _agree_to_three_digits(heat.error_norms(u), cold_norms)
    with pytest.raises(SystemExit, match='own or restricted'):
        hm.main(common + ['--nested', '1', '--nested_rhs', 'injected'])


# ---- 9. the torch composition of the timing tool ----------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location('restrict_time', os.path.join(REPO, 'tools', 'restrict_time.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_timed_composition_computes_what_the_kernel_computes():
    """The composition's summation order is unknown: entrywise within K 2^-53 (|P|^T |f|), K = the
    terms of the longest sum (the longest row of the table times the stencil) plus two."""
    from source.transfer import TransferPlan, children_rows, parent_rows, restrict_window
    coarse, fine = meshes('square', 3, 2), meshes('square', 4, 3)
    plan = TransferPlan(coarse, fine)
    assert (plan.a, plan.s, plan.N_coarse, plan.N_fine) == (1, 1, 5, 9)
    table = parent_rows(fine[0])
    ptr, _ = children_rows(table, plan.M_coarse)
    K = int(np.diff(ptr).max()) * ((2 << plan.a) - 1) + 2
    assert K == 7 * 3 + 2
    tool = _tool()
    device = _dev(np.zeros(1)).device
    f = torch.randn((plan.M_fine, 9), dtype=torch.float64, device=device)
    out = torch.full((plan.M_coarse, 6), SENTINEL, dtype=torch.float64, device=device)
    restrict_window(plan, f, 9, 0, 9, out, 6, 0, 5)
    PxT, PtT = tool.space_matrix_T(table, plan.M_coarse, device), tool.time_matrix_T(1, 5, device)
    ref, size = tool.torch_composition(PxT, PtT, f), tool.torch_composition(PxT, PtT, f.abs())
    assert bool((out[:, 5] == SENTINEL).all())
    assert same(out[:, :5].cpu().numpy(), numpy_restrict(table, plan.M_coarse, 1, f.cpu().numpy(), 0, 9, 0, 5))
    gap = float(((out[:, :5] - ref).abs() / size).max())
    print('kernel against the torch composition: largest gap %.3e of |P|^T |f|, bound %.3e' % (gap, K * 2.0**-53))
    assert bool(((out[:, :5] - ref).abs() <= K * 2.0**-53 * size).all())
    # time only
    ref_t = tool.torch_composition(None, PtT, f)
    out_t = torch.empty((plan.M_fine, 5), dtype=torch.float64, device=device)
    from source.transfer import restrict_time_scan
    restrict_time_scan(plan.M_fine, 1, f, 9, 0, 9, 9, out_t, 5, 0, 5)
    assert bool(((out_t - ref_t).abs() <= 5 * 2.0**-53 * tool.torch_composition(None, PtT, f.abs())).all())
