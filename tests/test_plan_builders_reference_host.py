"""What tests/test_plan_builders_gpu.py measures the plan builders on the device with
(csrc/ell_build.hip: stk_csr_galerkin, stk_ell_from_csr, stk_gs_depth_step): a catalogue of small
synthetic CSR matrices, the references, and the checks, run where there is no GPU, that every case
does what it is in the catalogue for.

Galerkin cases (`GALERKIN`, name -> (R, A, P or None, cap)).  The reference is SciPy's own
`(R @ A) @ P` with sorted rows; the matrices are built with sp.csr_matrix((data, indices, indptr))
from row entries in a shuffled order and are never canonicalised (SciPy's csr_matmat, and the kernel,
traverse the rows as stored).  All have nc >= 64 coarse rows (below that galerkin_product stays on
the host), nc in 64, 65, 129: one full workgroup, one thread of a second, three.

    cancel-nc*        small integers: some sums of R A and some of (R A) P are exactly zero and are
                      not emitted ("exact zero is not emitted", csr_matmat; copied by galerkin_kernel)
    roundings-nc*     randn on the same patterns: every sum rounds, the order of the additions shows
    ra-64 / ra-65 / ra-70   P = NULL, cap = 64: a row of R A with exactly 64 / 65 / 70 distinct columns
    rap-cap{1,16,32}-fits / -over   a row of R A P with exactly cap / cap + 1 columns
    excess-cancels-in-rap     cap + 1 touched columns, one of them a sum that is exactly zero
    excess-cancels-in-ra      an entry of R A that is exactly zero leads to rows of P nothing else reaches
    empty-nc*         an empty row of R, an empty row of A that R reaches, an empty row of P

`galerkin_overflow` states what *overflow receives (include/stk.h): per row, the number of distinct
columns its products TOUCH -- those whose sum cancels, and those reached only through a cancelled
entry of R A, included -- where that exceeds cap; 65 where R A or R A P touches more than 64; the
largest over the rows.

ELL cases (`ell_cases()`): one matrix with rows of 0 entries, rows without their diagonal, unsorted
rows and a second value array, through every combination of order (None, a permutation, a subset
with repeats), pad_col (0, 3, -1), grp, strip_diag, vm and K (the longest kept row, one short of it).
The reference is `ell_loop`, a per-row loop; EllRowsMatrix._build_with_numpy is checked against it
here (on a matrix with a full diagonal where it records the diagonal: it asserts one).

Depth cases (`DEPTH`): the reference is the longest-path recurrence over the rows in dof order
(`depth_ref`); `depth_step_ref` restates one relaxation.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

CAP = 64


# ---- CSR matrices from rows as listed ---------------------------------------------------------------
def csr_rows(rows, n_cols):
    """rows: per row a list of (col, value) in the order they are to be stored."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    indices = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    data = np.array([v for r in rows for _, v in r], dtype=np.float64)
    m = sp.csr_matrix((data, indices, indptr), shape=(len(rows), n_cols))
    assert m.indices is indices or np.array_equal(m.indices, indices)  # as stored: not sorted
    return m


def with_values(m, values):
    return sp.csr_matrix((np.asarray(values, dtype=np.float64), m.indices, m.indptr), shape=m.shape)


def _pattern(m):
    out = sp.csr_matrix((np.ones(len(m.indices)), m.indices, m.indptr), shape=m.shape)
    return out


def touched(R, A, P):
    """Distinct columns the products of each row touch in R A and in (R A) P: no cancellation."""
    ra = sp.csr_matrix(_pattern(R) @ _pattern(A))
    rap = ra if P is None else sp.csr_matrix(ra @ _pattern(P))
    return np.diff(ra.indptr), np.diff(rap.indptr)


def galerkin_overflow_rows(R, A, P, cap):
    ta, tc = touched(R, A, P)
    return np.where((ta > CAP) | (tc > CAP), CAP + 1, np.where(tc > cap, tc, 0))


def galerkin_overflow(R, A, P, cap):
    return int(galerkin_overflow_rows(R, A, P, cap).max())


def galerkin_ref(R, A, P):
    out = sp.csr_matrix(R @ A if P is None else (R @ A) @ P)
    out.sort_indices()
    return out


def _banded(nc, seed, values):
    """R (nc, 2 nc), A (2 nc, 2 nc), P (2 nc, nc) on banded patterns, rows stored shuffled."""
    rng, nf = np.random.RandomState(seed), 2 * nc

    def rows(n, cols_of):
        out = []
        for i in range(n):
            cols = sorted(set(cols_of(i)))
            rng.shuffle(cols)
            out.append([(c, values(rng)) for c in cols])
        return out
    R = csr_rows(rows(nc, lambda i: [(2 * i + d) % nf for d in (-1, 0, 1)]), nf)
    A = csr_rows(rows(nf, lambda j: [(j + d) % nf for d in (-2, -1, 0, 1, 2) if d == 0 or rng.rand() < 0.8]), nf)
    P = csr_rows(rows(nf, lambda l: [(l // 2 + d) % nc for d in (0, 1)]), nc)
    return R, A, P


def _ints(rng):
    return float(rng.choice([-2, -1, 1, 2]))


def _randn(rng):
    return float(rng.randn())


def _wide_ra(width, nc=64):
    """P = NULL: row 5 of R A has `width` distinct columns (two rows of A, 40 + the rest), the others 3."""
    rng, n_cols = np.random.RandomState(width), 96
    r_rows = [[(i, _randn(rng)), ((i + 7) % nc, _randn(rng))] for i in range(nc)]
    a_rows = [[((3 * j + k) % n_cols, _randn(rng)) for k in (2, 0)] for j in range(nc)]
    cols = list(rng.permutation(n_cols)[:width])
    a_rows[5] = [(int(c), _randn(rng)) for c in cols[:40]]
    a_rows[12] = [(int(c), _randn(rng)) for c in cols[40:]] + [(int(cols[0]), _randn(rng))]  # one shared column
    return csr_rows(r_rows, nc), csr_rows(a_rows, n_cols), None, CAP


def _wide_rap(cap, width, nc=65, cancel=None):
    """R picks fine rows i and i + nc, A is diagonal, so row i of R A P is the union of rows i and
    i + nc of P: `width` distinct columns in row 3 (one of them shared), at most cap elsewhere."""
    rng, nf = np.random.RandomState(100 * cap + width), 2 * nc
    val = _ints if cancel else _randn
    r_rows = [[(i + nc, val(rng)), (i, val(rng))] for i in range(nc)]
    a_rows = [[(j, val(rng))] for j in range(nf)]
    p_rows = [[((l % nc + k) % nc, val(rng)) for k in range(1 + (l < nc and cap > 1))][::-1] for l in range(nf)]
    if cap == 1:
        p_rows = [[(l % nc, val(rng))] for l in range(nf)]
    cols = [int(c) for c in rng.permutation(nc)[:width]]
    half = (width + 1) // 2
    p_rows[3] = [(c, val(rng)) for c in cols[:half]]
    p_rows[3 + nc] = [(c, val(rng)) for c in cols[half - 1:]]  # cols[half - 1] is in both
    if width == 1:
        p_rows[3 + nc] = [(cols[0], val(rng))]
    if cancel == 'rap':  # t = (r a) of the two fine rows; their shares of the shared column cancel
        r_rows[3], a_rows[3], a_rows[3 + nc] = [(3 + nc, 1.0), (3, 1.0)], [(3, 2.0)], [(3 + nc, 2.0)]
        p_rows[3][-1], p_rows[3 + nc][0] = (cols[half - 1], 3.0), (cols[half - 1], -3.0)
    return csr_rows(r_rows, nf), csr_rows(a_rows, nf), csr_rows(p_rows, nc), cap


def _excess_in_ra(cap=16, nc=64):
    """Row 9 of R A: the entry at fine column 40 is 1 * 5 + (-1) * 5 = 0, and row 40 of P has 5 columns
    that nothing else of the row reaches; the entry at column 41 leads to cap columns."""
    rng, nf = np.random.RandomState(9), 2 * nc
    r_rows = [[(i, _ints(rng))] for i in range(nc)]
    a_rows = [[(j, _ints(rng))] for j in range(nf)]
    p_rows = [[(l % nc, _ints(rng))] for l in range(nf)]
    r_rows[9] = [(72, 1.0), (70, 1.0), (71, -1.0)]
    a_rows[70], a_rows[71], a_rows[72] = [(40, 5.0)], [(40, 5.0)], [(41, 3.0)]
    p_rows[40] = [(c, 1.0) for c in (50, 49, 48, 47, 46)]
    p_rows[41] = [(c, 2.0) for c in range(cap)][::-1]
    return csr_rows(r_rows, nf), csr_rows(a_rows, nf), csr_rows(p_rows, nc), cap


def _empty(nc):
    R, A, P = _banded(nc, 70 + nc, _randn)

    def cut(m, gone):
        rows = [[] if i in gone else list(zip(m.indices[m.indptr[i]:m.indptr[i + 1]], m.data[m.indptr[i]:m.indptr[i + 1]]))
                for i in range(m.shape[0])]
        return csr_rows(rows, m.shape[1])
    return cut(R, {0, 17, nc - 1}), cut(A, {2, 34, 35, 36}), cut(P, {0, 33, 2 * nc - 1}), 16


def _build_galerkin():
    cases = {}
    for nc in (64, 65, 129):
        R, A, P = _banded(nc, nc, _ints)
        cases['cancel-nc%d' % nc] = (R, A, P, 16)
        cases['cancel-ra-nc%d' % nc] = (R, A, None, 32)
        g = np.random.RandomState(nc + 1)
        Rr, Ar, Pr = (with_values(m, g.randn(m.nnz)) for m in (R, A, P))
        cases['roundings-nc%d' % nc] = (Rr, Ar, Pr, 16)
        cases['roundings-ra-nc%d' % nc] = (Rr, Ar, None, 32)
        cases['empty-nc%d' % nc] = _empty(nc)
        e = cases['empty-nc%d' % nc]
        cases['empty-ra-nc%d' % nc] = (e[0], e[1], None, 32)
    for width in (64, 65, 70):
        cases['ra-%d' % width] = _wide_ra(width)
    for cap, nc in ((1, 64), (16, 65), (32, 129)):
        cases['rap-cap%d-fits' % cap] = _wide_rap(cap, cap, nc)
        cases['rap-cap%d-over' % cap] = _wide_rap(cap, cap + 1, nc)
    cases['rap-64'] = _wide_rap(CAP, 64, 129)
    cases['rap-65'] = _wide_rap(CAP, 65, 129)
    cases['excess-cancels-in-rap'] = _wide_rap(16, 17, 65, cancel='rap')
    cases['excess-cancels-in-ra'] = _excess_in_ra()
    return cases


GALERKIN = _build_galerkin()
OVERFLOWS = {'ra-65': 65, 'ra-70': 65, 'rap-cap1-over': 2, 'rap-cap16-over': 17, 'rap-cap32-over': 33, 'rap-65': 65,
             'excess-cancels-in-rap': 17, 'excess-cancels-in-ra': 21}


# ---- ELL copies -----------------------------------------------------------------------------------------
def ell_loop(indptr, indices, va, vm, order, K, strip_diag, grp, pad_col):
    """stk_ell_from_csr by a per-row loop -> dict(idx, va, vm, dia_a, dia_m, overflow, fits)."""
    order = np.arange(len(indptr) - 1) if order is None else np.asarray(order)
    n_pos = len(order)
    out = dict(idx=np.zeros((n_pos, K), np.int32), va=np.zeros((n_pos, K)), vm=None if vm is None else np.zeros((n_pos, K)),
               dia_a=np.zeros(n_pos), dia_m=None if vm is None else np.zeros(n_pos), overflow=0,
               fits=np.ones(n_pos, dtype=bool))
    for pos, row in enumerate(order):
        ent = [e for e in range(indptr[row], indptr[row + 1])]
        for e in ent:
            if indices[e] == row:
                out['dia_a'][pos] = va[e]
                if vm is not None:
                    out['dia_m'][pos] = vm[e]
        kept = [e for e in ent if not (strip_diag and indices[e] == row)
                and (grp is None or grp[indices[e]] < grp[row])]
        if len(kept) > K:
            out['overflow'], out['fits'][pos] = max(out['overflow'], len(kept)), False
        pad = pad_col if pad_col >= 0 else (indices[kept[0]] if kept else row)
        out['idx'][pos] = pad
        for s, e in enumerate(kept[:K]):
            out['idx'][pos, s], out['va'][pos, s] = indices[e], va[e]
            if vm is not None:
                out['vm'][pos, s] = vm[e]
    return out


def kept_counts(indptr, indices, order, strip_diag, grp):
    n = len(indptr) - 1
    rows_of = np.repeat(np.arange(n), np.diff(indptr))
    keep = np.ones(len(indices), dtype=bool)
    if strip_diag:
        keep &= indices != rows_of
    if grp is not None:
        keep &= grp[indices] < grp[rows_of]
    counts = np.bincount(rows_of[keep], minlength=n)
    return counts if order is None else counts[np.asarray(order)]


@functools.lru_cache(maxsize=None)
def ell_matrix(full_diagonal=False):
    """(indptr, indices, va, vm, grp) of 41 rows: rows 4 and 40 empty, rows 7, 8 and 20 without their
    diagonal (none of them with `full_diagonal`), every row stored in a shuffled order."""
    rng, n = np.random.RandomState(41), 41
    rows = []
    for i in range(n):
        cols = set(int(c) for c in rng.randint(0, n, size=rng.randint(1, 8))) | {i}
        if not full_diagonal:
            if i in (7, 8, 20):
                cols.discard(i)
                cols.add((i + 5) % n)
            if i in (4, 40):
                cols = set()
        cols = sorted(cols)
        rng.shuffle(cols)
        rows.append([(c, float(rng.randn())) for c in cols])
    m = csr_rows(rows, n)
    return m.indptr.copy(), m.indices.copy(), m.data.copy(), rng.randn(m.nnz), rng.randint(0, 4, size=n).astype(np.int32)


def ell_orders(n):
    rng = np.random.RandomState(2)
    return {'none': None, 'perm': rng.permutation(n).astype(np.int32),
            'subset': np.array([40, 7, 7, 3, 4, 20, 3, 39, 0, 8, 8, 8, 12], dtype=np.int32)}


def ell_cases(full_diagonal=False):
    """[(name, kwargs of ell_loop without the matrix)]: every combination, K the longest kept row
    of the listed rows (`fit`) or one short of it (`short`, where that is still a slot)."""
    indptr, indices, va, vm, grp = ell_matrix(full_diagonal)
    out = []
    for oname, order in ell_orders(len(indptr) - 1).items():
        for pad_col in (0, 3, -1):
            for use_grp in (False, True):
                for strip in (0, 1):
                    for use_vm in (False, True):
                        g = grp if use_grp else None
                        kmax = int(kept_counts(indptr, indices, order, strip, g).max())
                        for kind, K in (('fit', max(kmax, 1)), ('short', kmax - 1)):
                            if K < 1:
                                continue
                            name = '%s-pad%d-grp%d-strip%d-vm%d-%s' % (oname, pad_col, use_grp, strip, use_vm, kind)
                            out.append((name, dict(order=order, K=K, strip_diag=strip, grp=g, pad_col=pad_col,
                                                   vm=vm if use_vm else None)))
    return out


def long_ell_matrix(n=1048577):
    """Two entries per row stored as (i, i - 1) (row 0: the diagonal alone): n_pos past one
    grid-stride pass of 4096 x 256 rows, K = 2."""
    i = np.arange(n, dtype=np.int32)
    indptr = np.concatenate([[0, 1], 1 + 2 * np.arange(1, n)]).astype(np.int32)
    indices = np.concatenate([[0], np.stack([i[1:], i[1:] - 1], axis=1).ravel()]).astype(np.int32)
    va = np.arange(1, len(indices) + 1, dtype=np.float64)
    return indptr, indices, va


# ---- Gauss-Seidel depths -----------------------------------------------------------------------------------
def depth_ref(indptr, indices, backward):
    """Longest path to every row in the dependency DAG, rows in dof order (reverse for backward)."""
    n = len(indptr) - 1
    ip, ix = indptr.tolist(), indices.tolist()
    d = [0] * n
    for i in (range(n - 1, -1, -1) if backward else range(n)):
        best = 0
        for j in ix[ip[i]:ip[i + 1]]:
            if (j > i) if backward else (j < i):
                if d[j] + 1 > best:
                    best = d[j] + 1
        d[i] = best
    return np.array(d, dtype=np.int32)


def depth_step_ref(indptr, indices, backward, depth):
    """One relaxation: depth_out[i] = max over the neighbours i waits for of depth_in[j] + 1."""
    n = len(indptr) - 1
    rows_of = np.repeat(np.arange(n), np.diff(indptr))
    dep = indices > rows_of if backward else indices < rows_of
    new = np.zeros(n, dtype=np.int32)
    np.maximum.at(new, rows_of[dep], depth[indices[dep]] + 1)
    return new


def _pattern_rows(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return indptr, np.array([c for r in rows for c in r], dtype=np.int32)


def _random_pattern(n, seed, symmetric):
    rng = np.random.RandomState(seed)
    rows = [set() for _ in range(n)]
    for i in range(n):
        for j in rng.randint(max(0, i - 6), min(n, i + 7), size=rng.randint(0, 5)):
            rows[i].add(int(j))
            if symmetric:
                rows[int(j)].add(i)
    out = []
    for i, r in enumerate(rows):
        r = sorted(r)
        rng.shuffle(r)
        out.append(r)
    return _pattern_rows(out)


@functools.lru_cache(maxsize=None)
def depth_case(name):
    if name == 'chain-300':
        return _pattern_rows([[j for j in (i + 1, i, i - 1) if 0 <= j < 300] for i in range(300)])
    if name == 'star':
        return _pattern_rows([list(range(99, -1, -1))] + [[i, 0] for i in range(1, 100)])
    if name == 'short-chains-1048577':
        n = 1048577
        i = np.arange(n, dtype=np.int32)
        lo = np.where(i % 4 == 0, i, i - 1)  # a chain of 4 starts at every multiple of 4
        hi = np.where((i % 4 == 3) | (i == n - 1), i, i + 1)
        return np.arange(0, 2 * n + 1, 2, dtype=np.int32), np.stack([hi, lo], axis=1).ravel().astype(np.int32)
    if name == 'unsymmetric':
        return _random_pattern(200, 5, False)
    if name == 'empty-rows':
        ip, ix = _random_pattern(120, 6, True)
        rows = [[] if i % 7 == 3 else ix[ip[i]:ip[i + 1]].tolist() for i in range(120)]
        return _pattern_rows(rows)
    if name == 'n1':
        return _pattern_rows([[0]])
    if name == 'n1-empty':
        return _pattern_rows([[]])
    if name.startswith('n'):
        return _random_pattern(int(name[1:]), int(name[1:]), True)
    raise KeyError(name)


DEPTH = ('chain-300', 'star', 'short-chains-1048577', 'unsymmetric', 'empty-rows', 'n1', 'n1-empty', 'n255', 'n256', 'n257')


@functools.lru_cache(maxsize=None)
def depth_want(name, backward):
    ip, ix = depth_case(name)
    d = depth_ref(ip, ix, backward)
    d.setflags(write=False)
    return d


# ---- the catalogue does what it is for ---------------------------------------------------------------------
def _unsorted(m):
    return any(np.any(np.diff(m.indices[a:b]) < 0) for a, b in zip(m.indptr[:-1], m.indptr[1:]))


@pytest.mark.parametrize('name', sorted(GALERKIN))
def test_galerkin_catalogue(name):
    R, A, P, cap = GALERKIN[name]
    nc = R.shape[0]
    assert nc in (64, 65, 129) and R.indptr.dtype == np.int32 and R.indices.dtype == np.int32
    assert _unsorted(R) and (name.startswith(('ra-', 'rap-', 'excess')) or _unsorted(A))
    for m in (R, A) + (() if P is None else (P,)):
        assert not m.has_canonical_format or not _unsorted(m)
        for a, b in zip(m.indptr[:-1], m.indptr[1:]):
            assert len(set(m.indices[a:b].tolist())) == b - a  # no entry twice in a row
    want, ra = galerkin_ref(R, A, P), galerkin_ref(R, A, None)
    ta, tc = touched(R, A, P)
    ov = galerkin_overflow(R, A, P, cap)
    assert ov == OVERFLOWS.get(name, 0), (name, ov)
    counts = np.diff(want.indptr)
    if ov == 0:
        assert tc.max() <= cap and ta.max() <= CAP and counts.max() <= cap
    if name.startswith('cancel'):
        assert ra.nnz < ta.sum(), 'no sum of R A cancels'
        if P is not None:
            assert want.nnz < tc.sum() and np.any(counts < np.diff(sp.csr_matrix(_pattern(ra) @ _pattern(P)).indptr)), \
                'no sum of (R A) P cancels'
        assert np.all(want.data != 0.0)
    if name.startswith('roundings'):
        assert want.nnz == tc.sum()
        other = sp.csr_matrix(R @ (A @ P)) if P is not None else None  # another order: other roundings
        if other is not None:
            other.sort_indices()
            assert np.array_equal(other.indices, want.indices) and np.any(other.data != want.data)
    if name.startswith('ra-'):
        assert P is None and cap == CAP and ta.max() == int(name[3:]) and (ta == ta.max()).sum() == 1
    if name.startswith('rap-'):
        width = dict(fits=cap, over=cap + 1).get(name.split('-')[-1]) or int(name[4:])
        assert tc.max() == width and counts.max() == width
        assert (tc == width).sum() == 1 or (cap == 1 and width == 1)  # cap = 1: every row is as wide as cap
    if name == 'excess-cancels-in-rap':
        assert tc.max() == cap + 1 and counts.max() == cap and ta.max() == 2 and np.diff(ra.indptr).min() == 2
    if name == 'excess-cancels-in-ra':
        assert tc[9] == 21 and counts[9] == cap == counts.max() and ta[9] == 2 and np.diff(ra.indptr)[9] == 1
    if name.startswith('empty'):
        assert np.any(np.diff(R.indptr) == 0) and np.any(np.diff(A.indptr) == 0)
        reached = np.zeros(A.shape[0], dtype=bool)
        reached[R.indices] = True
        assert np.any(reached & (np.diff(A.indptr) == 0)), 'no empty row of A is reached'
        assert counts.min() == 0
        if P is not None:
            hit = np.zeros(P.shape[0], dtype=bool)
            hit[ra.indices] = True
            assert np.any(hit & (np.diff(P.indptr) == 0)), 'no empty row of P is reached'


def test_galerkin_catalogue_is_complete():
    names = set(GALERKIN)
    assert {n for n in names if GALERKIN[n][0].shape[0] == 64} and set(OVERFLOWS) <= names
    for kind in ('cancel', 'roundings', 'empty'):
        assert {'%s-nc%d' % (kind, nc) for nc in (64, 65, 129)} <= names
    assert {GALERKIN[n][3] for n in names if n.startswith('rap-cap')} == {1, 16, 32}


@pytest.mark.parametrize('full_diagonal', (False, True))
def test_numpy_ell_builder_is_the_per_row_loop(full_diagonal):
    from source.linop import EllRowsMatrix
    indptr, indices, va, vm_all, grp = ell_matrix(full_diagonal)
    n = len(indptr) - 1
    counts = np.diff(indptr)
    rows_of = np.repeat(np.arange(n), counts)
    if not full_diagonal:
        assert (counts == 0).sum() == 2 and sorted(set(range(n)) - set(rows_of[indices == rows_of]) - {4, 40}) == [7, 8, 20]
    assert any(np.any(np.diff(indices[a:b]) < 0) for a, b in zip(indptr[:-1], indptr[1:]))
    cases = ell_cases(full_diagonal)
    assert len(cases) > 100 and any(c[0].endswith('short') for c in cases)
    for name, kw in cases:
        want = ell_loop(indptr, indices, va, **kw)
        kmax = int(kept_counts(indptr, indices, kw['order'], kw['strip_diag'], kw['grp']).max())
        assert want['overflow'] == (kmax if kmax > kw['K'] else 0), name
        assert (kw['K'] == max(kmax, 1)) == name.endswith('fit') and (kw['K'] == kmax - 1) == name.endswith('short')
        host = EllRowsMatrix.__new__(EllRowsMatrix)
        order = np.arange(n) if kw['order'] is None else kw['order'].astype(np.int64)
        host._build_with_numpy(indptr, indices, va, kw['vm'], order, kw['K'], bool(kw['strip_diag']), kw['pad_col'],
                               full_diagonal, kw['grp'])
        fits = want['fits']
        for key in ('idx', 'va', 'vm') + (('dia_a', 'dia_m') if full_diagonal else ()):
            a, b = getattr(host, key), want[key]
            assert (a is None) == (b is None), (name, key)
            if a is not None:
                assert np.array_equal(a.cpu().numpy()[fits], b[fits]), (name, key)
        if full_diagonal:
            assert np.all(want['dia_a'] != 0.0)
        elif kw['order'] is None:
            assert np.all(want['dia_a'][[4, 7, 8, 20, 40]] == 0.0)
    # the long case: the loop on its first rows vouches for the builder on all of them
    ip, ix, v = long_ell_matrix(4099)
    want = ell_loop(ip, ix, v, None, None, 2, 0, None, -1)
    host = EllRowsMatrix.__new__(EllRowsMatrix)
    host._build_with_numpy(ip, ix, v, None, np.arange(4099), 2, False, -1, True, None)
    assert want['overflow'] == 0 and np.array_equal(host.idx.cpu().numpy(), want['idx'])
    assert np.array_equal(host.va.cpu().numpy(), want['va']) and np.array_equal(host.dia_a.cpu().numpy(), want['dia_a'])
    assert np.array_equal(want['idx'][:2], [[0, 0], [1, 0]])


@pytest.mark.parametrize('name', DEPTH)
def test_depth_catalogue(name):
    from source import multigrid as mgm
    ip, ix = depth_case(name)
    n = len(ip) - 1
    for backward in (False, True):
        want = depth_want(name, backward)
        # the relaxation from zero reaches the recurrence in max(depth) steps, and then reports no change
        d, steps = np.zeros(n, dtype=np.int32), 0
        while True:
            new = depth_step_ref(ip, ix, backward, d)
            if np.array_equal(new, d):
                break
            d, steps = new, steps + 1
        assert np.array_equal(d, want) and steps == want.max(), (name, backward)
        ptr, rows = mgm.gauss_seidel_schedule(ip, ix, backward)
        p2, r2 = mgm._groups_by_depth(want.astype(np.int64), n, backward)
        assert np.array_equal(ptr, p2) and np.array_equal(rows, r2)
    fw, bw = depth_want(name, False), depth_want(name, True)
    if name == 'chain-300':
        assert np.array_equal(fw, np.arange(300)) and np.array_equal(bw, np.arange(299, -1, -1))
    if name == 'star':
        assert fw.tolist() == [0] + [1] * 99 and bw.tolist() == [1] + [0] * 99
    if name == 'short-chains-1048577':
        assert n == 1048577 > 4096 * 256 and np.array_equal(fw, np.arange(n) % 4) and bw[-1] == 0 and bw[0] == 3
    if name == 'unsymmetric':
        a = sp.csr_matrix((np.ones(len(ix)), ix, ip), shape=(n, n))
        assert (a != a.T).nnz > 0 and fw.max() > 8
    if name == 'empty-rows':
        assert (np.diff(ip) == 0).sum() >= 10
    if name.startswith('n1'):
        assert n == 1 and fw.tolist() == [0] and bw.tolist() == [0]
