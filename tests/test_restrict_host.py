"""The restriction P^T on the host: the contract as a NumPy loop (``numpy_restrict``, which the
GPU tests import), its exactness against the prolongation (the adjoint identity on dyadic data,
the transposed multigrid matrix at a = 0), the transposed table of stk_transfer_children against
a NumPy construction, the stencil-window arithmetic of the C ABI's refusals and the refusal of
``restrict_to`` on meshes that are not nested -- nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest

from source.assembly import prolongation_matrices
from source.transfer import MAX_A, identity_rows, stencil_window

from test_transfer_host import CASES, case_table, dyadic, meshes, numpy_prolong, same

N_COARSE = 5


# ---- the contract -------------------------------------------------------------------------------------------------------
def numpy_children(parents, M_c):
    """Per coarse row the list of (fine row, weight) in ascending fine row."""
    lists = [[] for _ in range(M_c)]
    for i, (p0, p1) in enumerate(np.asarray(parents).tolist()):
        if p0 == p1:
            if p0 >= 0:
                lists[p0].append((i, 1.0))
        else:
            for p in (p0, p1):
                if p >= 0:
                    lists[p].append((i, 0.5))
    return lists


def numpy_space_T(parents, M_c, f):
    """g (M_c, n_cols) of `f` (M_f, n_cols): per coarse row the left fold of w * f_i over its
    entries, the first term starting the sum; 0.0 for a row without entries."""
    f = np.asarray(f, dtype=np.float64)
    g = np.zeros((M_c, f.shape[1]))
    with np.errstate(all='ignore'):
        for j, entries in enumerate(numpy_children(parents, M_c)):
            for number, (i, w) in enumerate(entries):
                term = w * f[i]
                g[j] = term if number == 0 else g[j] + term
    return g


def numpy_time_T(a, g, k_first, n_fine, q_first, n_qc):
    """out (M, n_qc) of `g` (M, n_cols), the fine columns k_first ..: per coarse column q the left
    fold over its stencil, ascending k, of w(k) * g(k), the first term starting the sum."""
    g = np.asarray(g, dtype=np.float64)
    assert (n_fine - 1) % (1 << a) == 0
    out = np.empty((g.shape[0], n_qc))
    with np.errstate(all='ignore'):
        for c in range(n_qc):
            q = q_first + c
            kc = q << a
            lo, hi = max(0, ((q - 1) << a) + 1), min(n_fine - 1, ((q + 1) << a) - 1)
            for k in range(lo, hi + 1):
                if k == kc:
                    w = 1.0
                elif k < kc:
                    w = (k - ((q - 1) << a)) / 2.0**a
                else:
                    w = 1.0 - (k - kc) / 2.0**a
                term = w * g[:, k - k_first]
                out[:, c] = term if k == lo else out[:, c] + term
    return out


def numpy_restrict(parents, M_c, a, f, k_first, n_fine, q_first, n_qc):
    """The contract of include/stk.h "restriction": `f` (M_f, n_cols) holds the fine columns
    k_first ..; returns (M_c, n_qc), the coarse columns q_first ...  Space first, then time;
    every operation is one rounded NumPy operation."""
    return numpy_time_T(a, numpy_space_T(parents, M_c, f), k_first, n_fine, q_first, n_qc)


def numpy_restrict_chain(tables, sizes, a, f):
    """Several space levels on a whole fine vector `f` (M_f, N_f): tables and the rows `sizes`
    below each of them, the coarsest first; the LAST table acts first and carries `a`."""
    N_f = f.shape[1]
    N_c = ((N_f - 1) >> a) + 1
    f = numpy_restrict(tables[-1], sizes[-1], a, f, 0, N_f, 0, N_c)
    for table, M_c in zip(tables[-2::-1], sizes[-2::-1]):
        f = numpy_restrict(table, M_c, 0, f, 0, N_c, 0, N_c)
    return f


def entries_of(parents, M_c):
    """(ptr, entries) of the C ABI's encoding from the NumPy lists."""
    lists = numpy_children(parents, M_c)
    ptr = np.zeros(M_c + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(entries) for entries in lists])
    flat = [(i << 1) | (1 if w == 0.5 else 0) for entries in lists for i, w in entries]
    return ptr, np.asarray(flat, dtype=np.int32).reshape(-1)


def big_row_table():
    """(parents, M_c = 7): coarse row 3 has its own fine row and 300 children -- longer than a
    wavefront and than a tile --, its neighbour row 4 exactly one entry, rows 5 and 6 none (their
    fine rows copy row 1)."""
    M_c = 7
    rows = [(j, j) for j in range(M_c)]
    rows += [(3, -1)] * 150 + [(3, 2)] * 100 + [(0, 3)] * 50 + [(-1, -1)] * 3
    table = np.asarray(rows, dtype=np.int32)
    table[5], table[6] = (1, 1), (1, 1)
    return table, M_c


SYNTHETIC = {
    'identity': lambda: (identity_rows(9), 9),
    'no_coarse_rows': lambda: (np.full((6, 2), -1, dtype=np.int32), 0),
    'more_coarse_than_fine': lambda: (np.asarray([[0, 0], [1, 1], [0, 5], [-1, 7]], dtype=np.int32), 9),
    'big_row': big_row_table,
    'no_fine_rows': lambda: (np.zeros((0, 2), dtype=np.int32), 4),
}


# ---- exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_the_loop_is_the_adjoint_of_the_prolongation(case):
    """On dyadic data every product and sum is exact, so sum (P u) . f == sum u . (P^T f) as an
    equality of doubles; at a = 0 the transposed multigrid matrix gives the loop's doubles."""
    table, M_c = case_table(case)
    rng = np.random.RandomState(7)
    for a in range(4):
        n_fine = ((N_COARSE - 1) << a) + 1
        u, f = dyadic(rng, (M_c, N_COARSE)), dyadic(rng, (len(table), n_fine))
        Pu = numpy_prolong(table, a, u, 0, 0, n_fine)
        PTf = numpy_restrict(table, M_c, a, f, 0, n_fine, 0, N_COARSE)
        assert PTf.shape == (M_c, N_COARSE)
        assert float(np.sum(Pu * f)) == float(np.sum(u * PTf)), a
    problem, Jc, Jf = CASES[case]
    P = prolongation_matrices(meshes(problem, Jf)[0])[-1]
    f = dyadic(rng, (len(table), 3))
    assert np.array_equal(P.T @ f, numpy_restrict(table, M_c, 0, f, 0, 3, 0, 3))
    # a = 0 is space alone; an identity table is time alone, and a copy at a = 0
    g = rng.randn(len(table), 4)
    assert same(numpy_restrict(identity_rows(len(table)), len(table), 0, g, 0, 4, 0, 4), g)
    # a window: the columns 1 .. 2 from exactly the fine columns they read
    a, n_fine = 2, 17
    f = rng.randn(len(table), n_fine)
    whole = numpy_restrict(table, M_c, a, f, 0, n_fine, 0, N_COARSE)
    k_lo, k_hi = stencil_window(a, 1, 2, n_fine)
    assert same(numpy_restrict(table, M_c, a, f[:, k_lo:k_hi + 1], k_lo, n_fine, 1, 2), whole[:, 1:3])


def test_the_loop_in_time():
    out = numpy_time_T(1, np.asarray([[1.0, 2.0, 4.0, 8.0, 16.0]]), 0, 5, 0, 3)
    assert out.tolist() == [[1.0 + 0.5 * 2.0, 0.5 * 2.0 + 4.0 + 0.5 * 8.0, 0.5 * 8.0 + 16.0]]
    # a NaN reaches exactly the stencils that hold its column
    g = np.ones((1, 9))
    g[0, 3] = np.nan
    assert np.isnan(numpy_time_T(2, g, 0, 9, 0, 3)[0]).tolist() == [True, True, False]
    assert np.isnan(numpy_time_T(1, g, 0, 9, 0, 5)[0]).tolist() == [False, True, True, False, False]


# ---- the transposed table -------------------------------------------------------------------------------------------------
def _tables():
    for case in sorted(CASES):
        yield (case,) + case_table(case)
    for name in sorted(SYNTHETIC):
        yield (name,) + SYNTHETIC[name]()


def test_children_rows_are_the_numpy_construction():
    from source.transfer import children_rows
    lengths = {}
    for name, table, M_c in _tables():
        ptr, entries = children_rows(table, M_c)
        want_ptr, want = entries_of(table, M_c)
        assert ptr.dtype == np.int64 and entries.dtype == np.int32, name
        assert np.array_equal(ptr, want_ptr) and np.array_equal(entries, want), name
        for j in range(M_c):  # ascending fine rows per coarse row
            rows = entries[ptr[j]:ptr[j + 1]] >> 1
            assert np.all(np.diff(rows) > 0), (name, j)
        lengths[name] = np.diff(ptr)
    assert lengths['square23'].max() == 7 and lengths['lshape23'].max() == 7 and lengths['cube12'].max() == 15
    assert lengths['identity'].tolist() == [1] * 9 and len(lengths['no_coarse_rows']) == 0
    assert (lengths['more_coarse_than_fine'] == 0).sum() == 5 and lengths['no_fine_rows'].tolist() == [0] * 4
    assert lengths['big_row'][3] == 301 and lengths['big_row'][4] == 1 and lengths['big_row'][5:].tolist() == [0, 0]


def test_children_rows_do_not_depend_on_the_host_threads(monkeypatch):
    from source.transfer import children_rows
    rng = np.random.RandomState(3)
    M_c, M_f = 5000, 40000  # above the 16384 items below which one thread works
    table = rng.randint(-1, M_c, size=(M_f, 2)).astype(np.int32)
    table[:M_c] = np.arange(M_c, dtype=np.int32)[:, None]
    want_ptr, want = entries_of(table, M_c)
    for threads in ('1', '3', '8'):
        monkeypatch.setenv('STK_HOST_THREADS', threads)
        ptr, entries = children_rows(table, M_c)
        assert np.array_equal(ptr, want_ptr) and np.array_equal(entries, want), threads


def test_children_rows_share_the_index_refusals():
    from source import _lib
    from source.transfer import children_rows
    table, M_c = case_table('square23')
    lib = _lib.lib()
    for row, pair, text in ((40, (M_c, 3), 'not in [-1, M_coarse'), (41, (2, M_c), 'not in [-1, M_coarse'),
                            (40, (-2, 3), 'not in [-1, M_coarse'), (40, (3, -2), 'not in [-1, M_coarse'),
                            (0, (-1, -1), 'a copy pair without a row to copy')):
        bad = table.copy()
        bad[row] = pair
        with pytest.raises(_lib.StkError, match='stk_transfer_children'):
            children_rows(bad, M_c)
        assert text in lib.stk_last_error().decode() and 'parents[%d]' % row in lib.stk_last_error().decode()
    with pytest.raises(_lib.StkError, match='M_coarse'):
        children_rows(table[:0], -1)
    ptr = np.full(M_c + 1, 77, dtype=np.int64)
    # an M_fine the encoding cannot hold is refused before the table is read
    assert _lib.STK_RESTRICT_MAX_M_FINE == 2**30
    rc = lib.stk_transfer_children(2**30 + 1, M_c, None, ptr.ctypes.data, None)
    assert rc != 0 and 'parents is null' in lib.stk_last_error().decode()
    for args, text in (((len(table), M_c, table.ctypes.data, None, ptr.ctypes.data), 'ptr is null'),
                       ((len(table), M_c, table.ctypes.data, ptr.ctypes.data, None), 'entries is null')):
        assert lib.stk_transfer_children(*args) != 0 and text in lib.stk_last_error().decode()
    assert np.all(ptr == 77)


# ---- the window of the refusals ---------------------------------------------------------------------------------------
def test_stencil_window_arithmetic():
    for a in range(0, 4):
        for n_coarse in (2, 3, 6):
            n_fine = ((n_coarse - 1) << a) + 1
            for q_first in range(n_coarse):
                for n_qc in range(1, n_coarse - q_first + 1):
                    read = set()
                    for q in range(q_first, q_first + n_qc):
                        for k in range(n_fine):  # every fine node whose prolongation weight on q is not 0
                            if abs(k - (q << a)) < (1 << a):
                                read.add(k)
                    assert stencil_window(a, q_first, n_qc, n_fine) == (min(read), max(read)), (a, q_first, n_qc)
    assert stencil_window(1, 0, 33, 65) == (0, 64) and stencil_window(1, 1, 1, 65) == (1, 3)
    assert stencil_window(0, 4, 2, 9) == (4, 5) and stencil_window(MAX_A, 1, 1, 257) == (1, 256)
    assert stencil_window(MAX_A, 0, 1, 257) == (0, 255)
    for bad in ((1, 0, 1, 4), (1, 2, 2, 5)):  # n_fine - 1 no multiple of 2^a; a q beyond the last node
        with pytest.raises(AssertionError):
            stencil_window(*bad)


# ---- the public call ---------------------------------------------------------------------------------------------------
def test_restrict_to_refuses_before_a_plan_is_built():
    """Both drivers' restrict_to goes through source.transfer.restrict_to: meshes that are not
    nested raise before the vector is looked at and before anything is cached."""
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
    with pytest.raises(ValueError, match='not nested'):
        fine.restrict_to(other, object())
    assert fine.transfer_plans == {} and fine.calls == [] and other.calls == []
    with pytest.raises(ValueError, match='2\\^a times the elements'):  # upwards is no restriction
        other.restrict_to(Recorder(meshes('square', 3, 2)), object())


def test_nested_rhs_of_the_command_line():
    import argparse

    from source import driver
    parser = argparse.ArgumentParser()
    for flag, kind, default, text in driver.POST_OPTIONS:
        parser.add_argument('--' + flag, type=kind, default=default, help=text)
    args, asked = driver.take_post_options(parser.parse_args([]))
    assert asked['nested'] is None and not hasattr(args, 'nested_rhs')
    args, asked = driver.take_post_options(parser.parse_args(['--nested', '1']))
    assert asked['nested'].nested_rhs == 'own'
    args, asked = driver.take_post_options(parser.parse_args(['--nested', '1', '--nested_rhs', 'restricted']))
    assert asked['nested'].nested_rhs == 'restricted'
    with pytest.raises(SystemExit, match='own or restricted'):
        driver.take_post_options(parser.parse_args(['--nested', '1', '--nested_rhs', 'injected']))
