"""The device LU solve (csrc/sptrsv.hip) on factors built so that every switch point of its
launch plan is crossed, and the single-factor applies (csrc/kron.hip: stk_csr_spmm,
stk_time_csr_apply, stk_time_dense_apply; csrc/blas1.hip: stk_slab_gather_columns /
_scatter_columns, the odd tail of stk_axpbyz) through the ABI alone.  Needs an MI355X.

Reference and bounds: tests/test_lu_reference_host.py (np.longdouble; U = 2^-53, gamma_n =
n U / (1 - n U)).  Level by level the solve is held to the backward bound of a
substitution, |c - L U z| <= (g_L + g_U + g_L g_U) |L| |U| |z|.  With a dense top (explicit
inverses of diagonal blocks) there is no such bound; its forward error, over max |x_ref|,
may be 16 max(e_host, U) with the whole top inverted (csrc/sptrsv.hip documents 5-10 times
substitution for a block six times larger than any here; 16 is that rounded up to a power of
two) and 4 max(e_host, U) with blocks of at most 64 rows ("the accuracy of substitution";
the headroom covers another order of summation), e_host being the forward error of a float64
substitution on the host.  The applies:

    stk_csr_spmm          gamma_{k+4} (|alpha| sum (|ca a| + |cm_t m|) |x| + |beta z|)
    stk_time_csr_apply    gamma_{k+1} (sum |v| |x| + [add_identity] |x_t|)
    stk_time_dense_apply  gamma_{n_in} sum |T| |x|
    stk_axpbyz            gamma_2 (|a x| + |b y|)

(the identity of stk_time_csr_apply is the start of the accumulator: no rounding of its
own, but every later rounding is relative to a sum that holds it, so it is one of the k + 1
terms).  Data movement, padding and every "same doubles" claim are bit for bit.  Every test
prints its largest error in units of its bound; DESIGN.md 3.8 records the figures."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import test_lu_reference_host as ref
from test_lu_reference_host import LD, U, gamma

pytestmark = pytest.mark.gpu

N_LOCS = (1, 2, 3, 16, 17, 33)
GUARD, SENTINEL = 3, 7.25
WHOLE, BLOCKS = 16.0, 4.0  # forward error of the dense-top form in units of max(e_host, U)
NAN = float('nan')


@pytest.fixture(scope='module')
def stk():
    from source import _lib
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _lib.lib()
    return _lib


def _dev(a):
    from source import _lib
    return _lib.to_dev(a)


def _filled(shape, value=NAN):
    return torch.full(shape, value, dtype=torch.float64, device='cuda')


def _guarded(rows, ld):
    """A NaN-filled (rows, ld) slab between sentinel rows; (buffer, the slab's view)."""
    buf = _filled((rows + 2 * GUARD, ld))
    buf[:GUARD] = SENTINEL
    buf[GUARD + rows:] = SENTINEL
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf, rows):
    h = buf.cpu().numpy()
    return np.all(h[:GUARD] == SENTINEL) and np.all(h[GUARD + rows:] == SENTINEL)


def _last_error(stk):
    return stk.lib().stk_last_error().decode()


def _refused(stk, rc, *words):
    msg = _last_error(stk)
    assert rc != 0 and msg and all(w in msg for w in words), (rc, msg, words)


# ---- plans ------------------------------------------------------------------------------
class _Plan:
    """stk_lu_create on a pair of factors; solves between sentinel rows."""
    def __init__(self, stk, f):
        self.stk, self.lib, self.f = stk, stk.lib(), f
        self.args = [f.L.indptr, f.L.indices, f.L.data, f.U.indptr, f.U.indices, f.U.data]
        ptrs = [a.ctypes.data for a in self.args] + [None if p is None else p.ctypes.data for p in (f.perm_r, f.perm_c)]
        self.plan = ctypes.c_void_p()
        stk.check(self.lib.stk_lu_create(f.n, *ptrs, ctypes.byref(self.plan)))

    def info(self):
        out = [ctypes.c_int32() for _ in range(3)]
        self.stk.check(self.lib.stk_lu_info(self.plan, *[ctypes.byref(v) for v in out]))
        return tuple(v.value for v in out)

    def top_rows(self):
        n_top = ctypes.c_int32()
        self.stk.check(self.lib.stk_lu_top_rows(self.plan, ctypes.byref(n_top), None))
        rows = np.empty(n_top.value, dtype=np.int32)
        self.stk.check(self.lib.stk_lu_top_rows(self.plan, ctypes.byref(n_top), rows.ctypes.data))
        return rows

    def set_top(self, block, claimed=None):
        """The production inversion (source/linop.py) on the factors as they were handed over;
        `claimed`: the block size the library is told, where it is to refuse it."""
        from source.linop import invert_top_blocks
        rows = self.top_rows()
        blocks = invert_top_blocks(self.f.L, self.f.U, rows, min(block, len(rows)))
        return self.lib.stk_lu_set_top_inverse(self.plan, self.stk.ptr(blocks[0]), self.stk.ptr(blocks[1]),
                                               block if claimed is None else claimed)

    def solve(self, B, ld, in_place=False):
        """x (n, ld) of b = B (n, n_loc); x and work NaN-filled between sentinel rows, b's
        padding NaN."""
        n, n_loc = B.shape
        xbuf, x = _guarded(n, ld)
        wbuf, w = _guarded(n, ld)
        if in_place:
            b = x
        else:
            b = _filled((n, ld))
        b[:, :n_loc] = _dev(B)
        self.stk.check(self.lib.stk_lu_solve(self.plan, self.stk.stream(), n_loc, ld, b.data_ptr(), x.data_ptr(),
                                             w.data_ptr()))
        assert _guards_intact(xbuf, n) and _guards_intact(wbuf, n), (self.f.name, n_loc, ld)
        return x.cpu().numpy()

    def close(self):
        self.lib.stk_lu_destroy(self.plan)


def _exercise(solve, B, what, n_locs=N_LOCS):
    """Every slab length (ascending: each call needs more scratch than the one before) with
    ld = n_loc, n_loc + 1, n_loc + 3 (the padding loop runs 0, 1 and 3 times): padding zero out
    of a NaN-filled x, sentinels untouched (in `solve`), b == x and a second run the same
    doubles, and -- the right-hand sides being the leading columns of one array -- every column
    the same doubles on every slab length and ld.  Returns the widest result."""
    results = {}
    for n_loc in n_locs:
        for ld in (n_loc, n_loc + 1, n_loc + 3):
            X = solve(B[:, :n_loc], ld)
            assert np.all(np.isfinite(X[:, :n_loc])), what + (n_loc, ld)
            assert not X[:, n_loc:].any(), what + (n_loc, ld, 'padding')
            results[n_loc, ld] = X[:, :n_loc]
            assert np.array_equal(solve(B[:, :n_loc], ld), X), what + (n_loc, ld, 'second run')
            assert np.array_equal(solve(B[:, :n_loc], ld, in_place=True), X), what + (n_loc, ld, 'b == x')
    widest = results[n_locs[-1], n_locs[-1]]
    for (n_loc, ld), X in results.items():
        assert np.array_equal(X, widest[:, :n_loc]), what + (n_loc, ld, 'columns differ between slabs')
    return widest


def _mid_block(n_top):
    return 64 if n_top > 64 else 7  # both leave a ragged last block on every top here


def _check_plan(stk, case, n_locs=N_LOCS):
    """One pair of factors: the plan's shape against the host model, the solve level by
    level against the backward bound, then -- where the plan has a dense top -- with diagonal
    blocks of 1, 7 or 64 (ragged last block) and all rows against the host yardstick."""
    f, B, X_ref, e_host = ref.host_yardstick(*case)
    if n_locs[-1] != B.shape[1]:
        B = f.rhs(n_locs[-1])
        X_ref = None
    plan = _Plan(stk, f)
    worst = {}
    try:
        shape = ref.plan_shape(f)
        assert plan.info() == (shape['levels_L'], shape['levels_U'], shape['launches']), (f.name, plan.info(), shape)
        rows = plan.top_rows()
        assert np.array_equal(rows, shape['top_rows']), (f.name, len(rows), shape['n_top'])
        X = _exercise(plan.solve, B, (f.name, 'levels'), n_locs)
        worst['levels'] = ref.residual_ratio(f, B, X)
        assert worst['levels'] <= 1.0, (f.name, worst)
        if not len(rows):
            dummy = _filled((4, 4), 0.0)
            _refused(stk, plan.lib.stk_lu_set_top_inverse(plan.plan, dummy.data_ptr(), dummy.data_ptr(), 4),
                     'no dense top')
        else:
            for block in (1, _mid_block(len(rows)), len(rows)):
                stk.check(plan.set_top(block))
                assert plan.info()[2] == ref.plan_shape(f, block)['launches'], (f.name, block)
                X = _exercise(plan.solve, B, (f.name, 'block', block), n_locs)
                key, allowed = ('whole', WHOLE) if block >= len(rows) else ('blocks', BLOCKS)
                worst[key] = max(worst.get(key, 0.0), ref.forward_error(X, X_ref) / max(e_host, U))
                assert worst[key] <= allowed, (f.name, block, worst, e_host)
    finally:
        plan.close()
    print(_figures(f.name, worst, e_host))
    return shape, worst


def _figures(name, worst, e_host):
    """`levels` in units of the backward bound; `whole` (may be 16) and `blocks` (may be 4) in
    units of the yardstick max(e_host, U)."""
    parts = ['%s %.3f%s' % (k, v, {'whole': ' of 16', 'blocks': ' of 4'}.get(k, '')) for k, v in sorted(worst.items())]
    return '%s: %s (e_host %.2e)' % (name, ', '.join(parts), e_host)


# ---- 1. factors built by hand -------------------------------------------------------------
@pytest.mark.parametrize('case', ref.with_perms(ref.CHAINS), ids=ref.case_id)
def test_chain(stk, case):
    """L unit lower bidiagonal, U upper bidiagonal, L's diagonal implicit and explicit, with
    identity (NULL) and independent random perm_r != perm_c.  n = 1: one row.  n = 15: 15
    narrow levels in ONE workgroup per factor (2 launches) and no top, one level short of
    `n_levels - d0 >= 16`.  n = 16, 20: the dense-top conditions just met; the top is all rows,
    the head is EMPTY (L_head / U_head without rows, d_S a plain permuted copy), blocks of 7
    leave a ragged last block, block = 1 is substitution through the block kernel.  With the
    diagonal implicit the inverse of a unit block must carry its ones (invert_top_blocks)."""
    f = ref.host_yardstick(*case)[0]
    shape, _ = _check_plan(stk, case)
    assert shape['n_top'] == (f.n if f.n >= 16 else 0)
    assert (shape['levels_L'], shape['levels_U']) == (f.n, f.n)
    if f.n < 16:
        assert shape['launches'] == 2


@pytest.mark.parametrize('case', ref.with_perms(ref.COMBS), ids=ref.case_id)
def test_comb(stk, case):
    """Leaves without L entries, then a chain of rows that each read the row before and 5
    leaves.  64 leaves: the level of WIDE = 64 rows is a launch of its own over the chip, d0 =
    1, the top is the chain of 20, the head one wide level in either factor.  63 leaves: one
    row short of WIDE, d0 = 0 and the top is all 83 rows (ragged blocks of 64 + 19).  A chain
    of 15 behind 64 leaves: 15 levels from d0 on, no top.  The last leaf AFTER the chain, read
    by the chain's last row in U: U's rows of S reach outside S (not closed), no top, and
    stk_lu_set_top_inverse refuses."""
    shape, _ = _check_plan(stk, case)
    n_leaf, n_chain, late = case[1], case[2], len(case) > 3 and case[3] is True
    expect = 0 if (late or n_chain < 16) else (n_chain if n_leaf >= 64 else n_leaf + n_chain)
    assert shape['n_top'] == expect and shape['d0'] == (1 if n_leaf >= 64 else 0)
    assert shape['closed'] == (not late)


@pytest.mark.parametrize('perm', ((), ('perm',)), ids=('identity', 'perm'))
@pytest.mark.parametrize('ell', ref.ROW_LENGTHS)
def test_row_lengths(stk, ell, perm):
    """Row i of L has min(i, ell) entries, U the same mirrored, n = 400: every row length 0
    .. ell on both sides of SP = 16 lanes per item and of the 4 x SP unrolled gather (`e + 3*SP
    < e1`: 47, 48, 49, 63, 64, 65 entries without the diagonal, and the tail loop behind it);
    ell = 0 is one wide level per factor.  The dense top (all 400 rows, 400 levels) runs with
    blocks of 1, of 64 (ragged: 6 x 64 + 16) and whole."""
    shape, _ = _check_plan(stk, (ref.row_lengths, ell) + perm)
    assert shape['n_top'] == (400 if ell else 0)


@pytest.mark.parametrize('perm', ((), ('perm',)), ids=('identity', 'perm'))
def test_grid_cap(stk, perm):
    """4100 rows without L entries and 4100 that each read 3 of them (U mirrored): two wide
    levels per factor.  At n_loc = 65 a level has 266 500 items, more than the 262 144 that
    one pass of the capped grid of 4096 workgroups serves: the second trip runs (x and work
    are NaN-filled, a row left out stays NaN)."""
    assert 4100 * 65 > 4096 * 1024 // 16 > 4100 * 33
    shape, _ = _check_plan(stk, (ref.grid_cap,) + perm, n_locs=N_LOCS + (65,))
    assert shape['n_top'] == 0 and shape['launches'] == 4


# ---- 2. factors from SuperLU --------------------------------------------------------------
def test_superlu_random_unsymmetric(stk):
    """sp.random(300, 300, 0.02) + diag(0.5 .. 1.5) through default splu, the reference's own
    call: perm_r != perm_c, an unsymmetric pattern, long rows, and a U that is NOT closed over
    S -- no dense top, every level walked."""
    f = ref.superlu_random()
    assert not np.array_equal(f.perm_r, f.perm_c)
    shape, _ = _check_plan(stk, (ref.superlu_random,))
    assert shape['n_top'] == 0


def test_laplacian_through_invlinop(stk):
    """The 31 x 31 five-point Laplacian (961 rows) through InvLinOp itself (MAX_ROWS = 0): a
    closed U and a dense top behind wide levels, with TOP_BLOCK = whole, 64 (ragged last
    block) and 1, and with dense_top = False; against the bounds above and against
    InvLinOp.host_solve (SuperLU's own solve: the device may differ from it by its own
    allowance plus SuperLU's measured error against the longdouble solution)."""
    from source.linop import InvLinOp
    f, B, X_ref, e_host = ref.host_yardstick(ref.superlu_laplacian)
    mat = ref.laplacian()
    saved = (InvLinOp.MAX_ROWS, InvLinOp.dense_top, InvLinOp.TOP_BLOCK)

    def build(dense_top, block):
        InvLinOp.MAX_ROWS, InvLinOp.dense_top, InvLinOp.TOP_BLOCK = 0, dense_top, block
        try:
            return InvLinOp(mat)
        finally:
            InvLinOp.MAX_ROWS, InvLinOp.dense_top, InvLinOp.TOP_BLOCK = saved

    def solver(op):
        def solve(Bc, ld, in_place=False):
            n, n_loc = Bc.shape
            xbuf, x = _guarded(n, ld)
            b = x if in_place else _filled((n, ld))
            b[:, :n_loc] = _dev(Bc)
            op.apply(b, out=x, n_loc=n_loc)
            assert _guards_intact(xbuf, n)
            return x.cpu().numpy()
        return solve

    host = build(True, saved[2])
    assert host._dense is None and np.array_equal(host.lu.perm_r, f.perm_r) and np.array_equal(host.lu.perm_c, f.perm_c)
    assert abs(sp.csr_matrix(host.lu.L) - f.L).nnz == 0 and abs(sp.csr_matrix(host.lu.U) - f.U).nnz == 0
    shape = ref.plan_shape(f)
    assert shape['closed'] and shape['d0'] > 0 and host.n_top == shape['n_top'] > 64
    assert host.levels() == (shape['levels_L'], shape['levels_U'], ref.plan_shape(f, shape['n_top'])['launches'])
    worst = {}
    by_levels = build(False, saved[2])
    assert by_levels.n_top == 0 and by_levels.levels()[2] == shape['launches']
    X = _exercise(solver(by_levels), B, (f.name, 'levels'))
    worst['levels'] = ref.residual_ratio(f, B, X)
    assert worst['levels'] <= 1.0, worst
    host.host_solve = True
    X_host = solver(host)(B, B.shape[1] + 1)[:, :B.shape[1]]
    assert np.array_equal(X_host, host.lu.solve(B))  # a round trip of SciPy's doubles
    e_superlu = ref.forward_error(X_host, X_ref)
    scale = float(np.max(np.abs(X_ref)))
    for block in (saved[2], 64, 1):
        op = build(True, block)
        assert op.n_top == shape['n_top'] and op.levels()[2] == ref.plan_shape(f, block)['launches']
        X = _exercise(solver(op), B, (f.name, 'block', block))
        key, allowed = ('whole', WHOLE) if block >= op.n_top else ('blocks', BLOCKS)
        worst[key] = max(worst.get(key, 0.0), ref.forward_error(X, X_ref) / max(e_host, U))
        assert worst[key] <= allowed, (block, worst, e_host)
        assert np.max(np.abs(X - X_host)) / scale <= allowed * max(e_host, U) + e_superlu, block
    print(_figures(f.name, worst, e_host) + ', SuperLU %.2e' % e_superlu)


# ---- 3. refusals --------------------------------------------------------------------------
def test_lu_refusals(stk):
    """Every refusal of the LU entry points returns non-zero with a message."""
    lib = stk.lib()
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    ok_L = (i32([0, 1, 3]), i32([0, 0, 1]), f64([1.0, 0.5, 1.0]))
    ok_U = (i32([0, 2, 3]), i32([0, 1, 1]), f64([2.0, 0.5, 3.0]))

    def create(L=ok_L, Um=ok_U, perm_r=None, perm_c=None, n=2):
        plan = ctypes.c_void_p()
        keep = list(L) + list(Um) + [perm_r, perm_c]
        rc = lib.stk_lu_create(n, *[None if a is None else a.ctypes.data for a in keep], ctypes.byref(plan))
        if rc == 0:
            lib.stk_lu_destroy(plan)
        return rc

    assert create() == 0
    _refused(stk, create(L=(i32([0, 2, 3]), i32([0, 1, 1]), f64([1.0, 0.5, 1.0]))), 'L has an entry on the wrong side')
    _refused(stk, create(Um=(i32([0, 1, 3]), i32([0, 0, 1]), f64([2.0, 0.5, 3.0]))), 'U has an entry on the wrong side')
    _refused(stk, create(Um=(i32([0, 2, 2]), i32([0, 1]), f64([2.0, 0.5]))), 'zero diagonal in row 1 of U')
    _refused(stk, create(Um=(i32([0, 2, 3]), i32([0, 1, 1]), f64([2.0, 0.5, 0.0]))), 'zero diagonal in row 1 of U')
    _refused(stk, create(perm_r=i32([0, 0])), 'not a permutation')
    _refused(stk, create(perm_c=i32([0, 2])), 'not a permutation')
    _refused(stk, create(n=0), 'n=0')

    plan = _Plan(stk, ref.chain(15))
    try:
        x, b, w = _filled((15, 4), 1.0), _filled((15, 4), 1.0), _filled((15, 4), 1.0)
        solve = lambda n_loc, ld, b_, x_, w_: lib.stk_lu_solve(plan.plan, stk.stream(), n_loc, ld, b_.data_ptr(),
                                                               x_.data_ptr(), w_.data_ptr())
        assert solve(3, 4, b, x, w) == 0
        _refused(stk, solve(3, 4, b, x, b), 'work aliases')
        _refused(stk, solve(3, 4, b, x, x), 'work aliases')
        _refused(stk, solve(5, 4, b, x, w), 'bad sizes')
        _refused(stk, solve(0, 4, b, x, w), 'bad sizes')
        assert len(plan.top_rows()) == 0
        _refused(stk, lib.stk_lu_set_top_inverse(plan.plan, x.data_ptr(), x.data_ptr(), 4), 'no dense top')
    finally:
        plan.close()
    plan = _Plan(stk, ref.chain(16))
    try:
        assert len(plan.top_rows()) == 16
        _refused(stk, plan.set_top(16, claimed=0), 'blocks of 0 rows')
        _refused(stk, plan.set_top(16, claimed=8193), 'blocks of 8193 rows')
        stk.check(plan.set_top(8192))
    finally:
        plan.close()
    torch.cuda.synchronize()


# ---- 4. the single-factor applies ---------------------------------------------------------
def _ratio(got, want, bound, what):
    """The largest |got - want| in units of the bound (a zero bound admits no error)."""
    assert np.all(np.isfinite(got)), what
    err = np.abs(got.astype(LD) - want)
    assert np.all(err[bound == 0] == 0), what
    pos = bound > 0
    worst = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
    assert worst <= 1.0, what + (worst,)
    return worst


SPMM_LENGTHS = (0, 1, 7, 8, 9, 16, 17)
# (rows, n_loc, ld): 16 001 x 66 is more than the 1 048 576 items of one pass of stk_flat_grid
SLABS = ((1, 1, 1), (7, 5, 6), (300, 33, 36), (16001, 65, 66))


def _spmm_matrix(rows, n_cols, rng):
    """Rectangular CSR with the row lengths 0, 1, 7, 8, 9, 16, 17 in turn and one row of 40."""
    lengths = np.array([SPMM_LENGTHS[i % len(SPMM_LENGTHS)] for i in range(rows)])
    lengths[rows // 2] = 40
    indptr = np.r_[0, np.cumsum(lengths)].astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(n_cols, k, replace=False)) for k in lengths]).astype(np.int32)
    return lengths, indptr, indices


def _row_sums(lengths, indptr, indices, vals, X):
    """sum_e vals[e][t] X[col(e)][t] per row in extended precision; vals is (nnz, n_loc)."""
    out = np.zeros((len(lengths), X.shape[1]), dtype=LD)
    for k in np.unique(lengths[lengths > 0]):
        rows = np.flatnonzero(lengths == k)
        e = indptr[rows][:, None] + np.arange(k)[None, :]
        out[rows] = (vals[e] * X[indices[e]]).sum(axis=1)
    return out


@pytest.mark.parametrize('rows,n_loc,ld', SLABS)
def test_csr_spmm(stk, rows, n_loc, ld):
    """y = alpha (ca A + cm_t M) x + beta z on a rectangular CSR whose rows cross the 8-wide
    clamped batch (`min(eb + u, e1 - 1)`: 7, 8, 9, 16, 17 and 40 entries) and are empty (the
    clamp would read entry e1 - 1 of the row BEFORE: never entered), with and without vals_m /
    cm, z apart and z == y (the form of `u_j -= P u_c`), beta = 0 on a NaN-filled y, padding
    zero; 16 001 x 66 takes a second pass of the capped grid."""
    lib, rng = stk.lib(), np.random.RandomState(rows)
    n_cols = max(45, (2 * rows) // 3)
    lengths, indptr, indices = _spmm_matrix(rows, n_cols, rng)
    nnz, k = len(indices), 40
    va, vm, ca, cm = rng.randn(nnz), rng.randn(nnz), 0.7, rng.randn(n_loc)
    X, Z = rng.randn(n_cols, n_loc), rng.randn(rows, n_loc)
    x, z0 = _filled((n_cols, ld)), _filled((rows, ld))
    x[:, :n_loc], z0[:, :n_loc] = _dev(X), _dev(Z)
    d = [_dev(a) for a in (indptr, indices, va, vm, cm)]
    Xl, Zl = X.astype(LD), Z.astype(LD)
    worst = 0.0
    for with_m in (False, True):
        a_part = (LD(ca) * va.astype(LD))[:, None] * np.ones(n_loc, dtype=LD)
        m_part = vm.astype(LD)[:, None] * cm.astype(LD)[None, :] if with_m else 0 * a_part
        s = _row_sums(lengths, indptr, indices, a_part + m_part, Xl)
        mag = _row_sums(lengths, indptr, indices, np.abs(a_part) + np.abs(m_part), np.abs(Xl))
        for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.5, -0.75)):
            want = LD(alpha) * s + LD(beta) * Zl
            bound = gamma(k + 4) * (abs(LD(alpha)) * mag + np.abs(LD(beta) * Zl))
            for in_place in (False, True):
                ybuf, y = _guarded(rows, ld)
                if in_place and beta != 0.0:
                    y.copy_(z0)
                z = None if beta == 0.0 else (y if in_place else z0)
                stk.check(lib.stk_csr_spmm(stk.stream(), rows, n_loc, ld, stk.ptr(d[0]), stk.ptr(d[1]), stk.ptr(d[2]),
                                           ca, stk.ptr(d[3]) if with_m else None, stk.ptr(d[4]) if with_m else None,
                                           stk.ptr(x), alpha, beta, None if z is None else z.data_ptr(), y.data_ptr()))
                assert _guards_intact(ybuf, rows)
                got = y.cpu().numpy()
                assert not got[:, n_loc:].any(), 'padding'
                worst = max(worst, _ratio(got[:, :n_loc], want, bound, (rows, with_m, alpha, beta, in_place)))
    y = _filled((rows, ld), SENTINEL)
    assert lib.stk_csr_spmm(stk.stream(), 0, n_loc, ld, stk.ptr(d[0]), stk.ptr(d[1]), stk.ptr(d[2]), ca, None, None,
                            stk.ptr(x), 1.0, 0.0, None, stk.ptr(y)) == 0
    assert np.all(y.cpu().numpy() == SENTINEL)  # rows = 0 is a no-op
    print('stk_csr_spmm %d x %d (ld %d): %.3f of the bound' % (rows, n_loc, ld, worst))


@pytest.mark.parametrize('M,n_loc,ld', SLABS)
def test_time_csr_apply(stk, M, n_loc, ld):
    """y = (A_t kron I) x (+ x): random time rows, empty ones among them, whose columns
    >= n_loc are rows of `recv` (0, 1 and 3 of them; NULL when there are none), add_identity 0
    and 1, padding zero, x == y refused.  The bound counts the identity among the k + 1 terms
    of the magnitude: without |x_t| there no float64 result can meet it once |x_t| exceeds the
    sum (printed as a figure: up to 6e4 of it on one MI355X for results correct to 0.58)."""
    lib, rng = stk.lib(), np.random.RandomState(M + n_loc)
    X = rng.randn(M, n_loc)
    x = _filled((M, ld))
    x[:, :n_loc] = _dev(X)
    worst, literal = 0.0, 0.0
    for n_recv in (0, 1, 3):
        counts = rng.randint(0, 5, size=n_loc)
        counts[rng.randint(n_loc)] = 0
        if n_recv:
            counts[-1] = max(counts[-1], n_recv)  # a row that reads every recv row
        t_cols = [np.sort(rng.choice(n_loc + n_recv, min(c, n_loc + n_recv), replace=False)) for c in counts]
        if n_recv:
            t_cols[-1] = np.unique(np.r_[t_cols[-1], n_loc + np.arange(n_recv)])
        t_indptr = np.r_[0, np.cumsum([len(c) for c in t_cols])].astype(np.int32)
        cols = np.concatenate(t_cols).astype(np.int32) if t_indptr[-1] else np.zeros(1, np.int32)
        vals = rng.randn(max(int(t_indptr[-1]), 1))
        R = rng.randn(n_recv, M)
        both = np.concatenate([X, R.T], axis=1).astype(LD)  # column c >= n_loc: recv row c - n_loc
        k = max(len(c) for c in t_cols)
        d = [_dev(a) for a in (t_indptr, cols, vals)]
        recv = _dev(R) if n_recv else None
        for add_identity in (0, 1):
            want, mag = np.zeros((M, n_loc), dtype=LD), np.zeros((M, n_loc), dtype=LD)
            for t in range(n_loc):
                c, v = t_cols[t], vals[t_indptr[t]:t_indptr[t + 1]].astype(LD)
                want[:, t] = both[:, c] @ v + (both[:, t] if add_identity else 0)
                mag[:, t] = np.abs(both[:, c]) @ np.abs(v) + (np.abs(both[:, t]) if add_identity else 0)
            ybuf, y = _guarded(M, ld)
            stk.check(lib.stk_time_csr_apply(stk.stream(), M, n_loc, ld, stk.ptr(d[0]), stk.ptr(d[1]), stk.ptr(d[2]),
                                             stk.ptr(x), stk.ptr(recv), add_identity, y.data_ptr()))
            assert _guards_intact(ybuf, M)
            got = y.cpu().numpy()
            assert not got[:, n_loc:].any(), 'padding'
            worst = max(worst, _ratio(got[:, :n_loc], want, gamma(k + 1) * mag, (M, n_recv, add_identity)))
            if add_identity:  # a figure, not a bound: the sum without the identity's own term
                err, own = np.abs(got[:, :n_loc].astype(LD) - want), gamma(k + 1) * (mag - np.abs(both[:, :n_loc]))
                literal = max(literal, float(np.max(err[own > 0] / own[own > 0])) if (own > 0).any() else 0.0)
    _refused(stk, lib.stk_time_csr_apply(stk.stream(), M, n_loc, ld, stk.ptr(d[0]), stk.ptr(d[1]), stk.ptr(d[2]),
                                         stk.ptr(x), stk.ptr(recv), 0, stk.ptr(x)), 'aliases')
    print('stk_time_csr_apply %d x %d (ld %d): %.3f of the bound (%.3g of it without |x_t|)' % (M, n_loc, ld, worst, literal))


@pytest.mark.parametrize('M', (1, 7, 300, 16001))
def test_time_dense_apply(stk, M):
    """y = (T kron I) x for rectangular dense T, ld_in != ld_out, padding zero; at M = 16 001
    the output slab of ld_out = 66 takes a second pass of the capped grid."""
    lib, rng = stk.lib(), np.random.RandomState(M)
    shapes = ((65, 2),) if M > 1000 else ((1, 1), (5, 9), (9, 5), (33, 33), (65, 2))
    worst = 0.0
    for n_in, n_out in shapes:
        ld_in, ld_out = n_in + 2, (66 if M > 1000 else n_out + 1)
        T, X = rng.randn(n_out, n_in), rng.randn(M, n_in)
        x = _filled((M, ld_in))
        x[:, :n_in] = _dev(X)
        t_dev = _dev(T)
        ybuf, y = _guarded(M, ld_out)
        stk.check(lib.stk_time_dense_apply(stk.stream(), M, n_in, ld_in, n_out, ld_out, stk.ptr(t_dev), stk.ptr(x),
                                           y.data_ptr()))
        assert _guards_intact(ybuf, M)
        got = y.cpu().numpy()
        assert not got[:, n_out:].any(), 'padding'
        want = X.astype(LD) @ T.astype(LD).T
        bound = gamma(n_in) * (np.abs(X).astype(LD) @ np.abs(T).astype(LD).T)
        worst = max(worst, _ratio(got[:, :n_out], want, bound, (M, n_in, n_out)))
    _refused(stk, lib.stk_time_dense_apply(stk.stream(), M, n_in, ld_in, n_out, ld_in, stk.ptr(t_dev), stk.ptr(x),
                                           stk.ptr(x)), 'aliased')
    print('stk_time_dense_apply M = %d: %.3f of the bound' % (M, worst))


@pytest.mark.parametrize('M,n_loc,ld', SLABS)
def test_slab_gather_and_scatter_columns(stk, M, n_loc, ld):
    """Time slices of a slab, bit for bit against NumPy: one column, a random subset and all
    columns; an odd n_cols under an even ld_y leaves a padding column, written as zero;
    gather then scatter restores the selected columns and leaves the others untouched."""
    lib, rng = stk.lib(), np.random.RandomState(M)
    X = rng.randn(M, n_loc)
    x = _filled((M, ld))
    x[:, :n_loc] = _dev(X)
    subsets = [np.array([rng.randint(n_loc)]), np.arange(n_loc)]
    if n_loc > 2:
        subsets.append(rng.permutation(n_loc)[:(n_loc // 2) | 1])  # odd count, any order
    for cols in subsets:
        n_cols = len(cols)
        ld_y = n_cols + (n_cols & 1) if M < 16001 else 66
        c_dev = _dev(cols.astype(np.int32))
        ybuf, y = _guarded(M, ld_y)
        stk.check(lib.stk_slab_gather_columns(stk.stream(), M, n_cols, stk.ptr(c_dev), stk.ptr(x), ld, y.data_ptr(),
                                              ld_y))
        assert _guards_intact(ybuf, M)
        got = y.cpu().numpy()
        assert np.array_equal(got[:, :n_cols], X[:, cols]) and not got[:, n_cols:].any(), (M, n_cols)
        bbuf, back = _guarded(M, ld)
        back.fill_(SENTINEL)
        stk.check(lib.stk_slab_scatter_columns(stk.stream(), M, n_cols, stk.ptr(c_dev), y.data_ptr(), ld_y,
                                               back.data_ptr(), ld))
        assert _guards_intact(bbuf, M)
        want = np.full((M, ld), SENTINEL)
        want[:, cols] = X[:, cols]
        assert np.array_equal(back.cpu().numpy(), want), (M, n_cols)
    _refused(stk, lib.stk_slab_gather_columns(stk.stream(), M, 1, stk.ptr(c_dev), stk.ptr(x), ld, stk.ptr(x), ld),
             'stk_slab_gather_columns')
    _refused(stk, lib.stk_slab_scatter_columns(stk.stream(), M, 1, stk.ptr(c_dev), stk.ptr(x), ld, stk.ptr(x), ld),
             'stk_slab_scatter_columns')


@pytest.mark.parametrize('n', (1, 3, 513))
def test_axpbyz_odd_tail(stk, n):
    """z = a x + b y on an odd count: the pairs go through the 16-byte body, the last element
    through the scalar tail, which gives -- bit for bit, with b = 0 (z = a x) and b != 0
    (fma(a, x, b y)) -- what the body gives for the same operands at an even index; stk_axpby
    (z == y) alike; a pointer 8 bytes off the 16-byte grid is refused."""
    lib, rng = stk.lib(), np.random.RandomState(n)
    X, Y, a = rng.randn(n), rng.randn(n), 1.0 / 3.0
    worst = 0.0
    for b in (0.0, -0.7):
        x, y = _dev(np.r_[X, SENTINEL]), _dev(np.r_[Y, SENTINEL])
        z = _filled((n + 1,), SENTINEL)
        stk.check(lib.stk_axpbyz(stk.stream(), n, a, stk.ptr(x), b, stk.ptr(y), stk.ptr(z)))
        got = z.cpu().numpy()
        assert got[n] == SENTINEL
        want = LD(a) * X.astype(LD) + LD(b) * Y.astype(LD)
        bound = gamma(2) * (np.abs(LD(a) * X.astype(LD)) + np.abs(LD(b) * Y.astype(LD)))
        worst = max(worst, _ratio(got[:n], want, bound, (n, b)))
        if b == 0.0:
            assert np.array_equal(got[:n], a * X)
        # the operands of the tail at index 0 of a pair: the body alone (n = 2)
        x2, y2 = _dev(np.array([X[-1], 1.0])), _dev(np.array([Y[-1], 1.0]))
        z2 = _filled((2,))
        stk.check(lib.stk_axpbyz(stk.stream(), 2, a, stk.ptr(x2), b, stk.ptr(y2), stk.ptr(z2)))
        assert z2.cpu().numpy()[0] == got[n - 1], (n, b)
        y_in_place = y.clone()
        stk.check(lib.stk_axpby(stk.stream(), n, a, stk.ptr(x), b, stk.ptr(y_in_place)))
        assert np.array_equal(y_in_place.cpu().numpy(), got)
    big = _filled((8,), 1.0)
    for args in ((big.data_ptr() + 8, big.data_ptr(), big.data_ptr()), (big.data_ptr(), big.data_ptr() + 8, big.data_ptr()),
                 (big.data_ptr(), big.data_ptr(), big.data_ptr() + 8)):
        _refused(stk, lib.stk_axpbyz(stk.stream(), 3, a, args[0], -0.7, args[1], args[2]), '16-byte aligned')
    print('stk_axpbyz n = %d: %.3f of the bound' % (n, worst))
