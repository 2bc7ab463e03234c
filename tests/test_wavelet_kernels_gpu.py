"""The two kernels behind stk_wavelet_apply (csrc/wavelet.hip) on their own, through the ABI:
every J, both directions, row counts around each kernel's tile height, every launch
condition, every entry of the matrix, the padding column, in place and twice.  Needs an
MI355X.

Reference and bound: tests/test_wavelet_reference_host.py -- the stencil in np.longdouble
and, level by level, e_j = |L_j| e_{j-1} + gamma_5 |L_j| (|y_{j-1}| + e_{j-1}); the check is
|y - y_ref| <= bound on EVERY entry (a zero bound admits no error), on signed input whose
time nodes are scaled over twelve decades.  Every test prints its largest error in units of
the bound, and the kernel that ran.

Which kernel runs is the rule of stk_wavelet_apply, restated here from the arguments (never
asked of the library): the register kernel (one wavefront owns 64 rows, all levels in
registers) for 1 <= J <= 7 with ld == N + 1 (N = 2^J + 1) and x, y both 16-byte aligned; the
generic LDS kernel (R = min(128, 4160 // N) rows per workgroup) otherwise.  The paths:

    register          J = 1 .. 7,  ld = N + 1, aligned
    generic by ld     J = 0 .. 11, ld = N, N + 3 (odd padding width), N + 4 (even)
    generic by align  J = 1 .. 7,  ld = N + 1, x / y / both 8 bytes off the 16-byte grid

each with M = 1, H - 1, H, H + 1, 2 H + 1 for the tile height H of the kernel that runs: a
lone ragged tile, an exact one, a full tile followed by a ragged one.

Buffers: every output slab is NaN-filled and lies between sentinel rows that are checked
after every call.  Padding: the generic kernel writes zeros whatever x holds there (x's
padding is NaN here); the register kernel moves whole rows, padding included, so y's padding
is zero if x's is, and NaN in x's padding changes no bit of the data columns."""
import numpy as np
import pytest
import torch

import test_wavelet_reference_host as ref

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 4, 7.25  # 4 rows: the slab behind them starts on the 16-byte grid for every ld
NAN = float('nan')
REGISTER_J = range(1, 8)
ALL_J = range(ref.J_MAX + 1)
TILE_ELEMS = 4160          # doubles of LDS the generic kernel stages per workgroup
DIRECTIONS = ((False, 'W  '), (True, 'W^T'))


@pytest.fixture(scope='module')
def stk():
    from source import _lib
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _lib.lib()
    return _lib


# ---- the launch rule, restated -------------------------------------------------------------
def kernel_of(J, ld, x_ptr, y_ptr):
    N = ref.n_nodes(J)
    return 'register' if (1 <= J <= 7 and ld == N + 1 and (x_ptr | y_ptr) & 15 == 0) else 'generic'


def tile_height(kernel, J):
    return 64 if kernel == 'register' else min(128, TILE_ELEMS // ref.n_nodes(J))


def row_counts(kernel, J):
    H = tile_height(kernel, J)
    return sorted({1, max(H - 1, 1), H, H + 1, 2 * H + 1})


# ---- buffers ---------------------------------------------------------------------------------
class _Slab:
    """An (M, ld) slab `off` doubles behind the 16-byte grid, inside a flat buffer of
    sentinels; the slab itself starts as NaN."""
    def __init__(self, M, ld, off=0, fill=NAN):
        self.start, self.count = GUARD * ld + off, M * ld
        self.flat = torch.full(((M + 2 * GUARD) * ld + 2,), SENTINEL, dtype=torch.float64, device='cuda')
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[self.start:self.start + self.count].view(M, ld)
        self.view.fill_(fill)
        assert self.view.data_ptr() % 16 == 8 * off

    def load(self, X, pad):
        from source import _lib
        N = X.shape[1]
        self.view[:, :N] = _lib.to_dev(np.array(X))  # a writable copy of a shared, read-only case
        self.view[:, N:] = pad

    def guards_intact(self):
        h = self.flat.cpu().numpy()
        return bool(np.all(h[:self.start] == SENTINEL) and np.all(h[self.start + self.count:] == SENTINEL))


def _apply(stk, J, transposed, X, ld, x_off=0, y_off=0, x_pad=NAN, in_place=False, calls=1):
    """stk_wavelet_apply on X (M, N) in a slab of leading dimension ld: (y as (M, ld) NumPy,
    the kernel that ran by the launch rule).  `calls` > 1 repeats the same call on the same
    buffers (out of place only)."""
    M, N = X.shape
    assert N == ref.n_nodes(J) and ld >= N and M >= 1  # the kernels' bounds: rows of ld >= N doubles
    y = _Slab(M, ld, y_off)
    x = y if in_place else _Slab(M, ld, x_off)
    x.load(X, x_pad)
    for _ in range(calls):
        stk.check(stk.lib().stk_wavelet_apply(stk.stream(), M, J, ld, int(transposed), x.view.data_ptr(),
                                              y.view.data_ptr()))
    torch.cuda.synchronize()
    assert y.guards_intact() and x.guards_intact(), (J, transposed, M, ld, x_off, y_off, 'sentinels')
    if not in_place:  # x is read only
        h = x.view.cpu().numpy()
        assert np.array_equal(h[:, :N], X), (J, transposed, M, ld, 'x was written')
    return y.view.cpu().numpy(), kernel_of(J, ld, x.view.data_ptr(), y.view.data_ptr())


def _line(path, kernel, J, tag, ld, x_off, y_off, Ms, worst):
    N = ref.n_nodes(J)
    return 'wavelet %-16s %-8s J=%-2d %s ld=N+%d x+%d y+%d M=%s: %.3f of the bound' % (
        path, kernel, J, tag, ld - N, 8 * x_off, 8 * y_off, ','.join(str(m) for m in Ms), worst)


# ---- 0. J = 7 first ---------------------------------------------------------------------------
def test_j7_transposed_is_the_first_register_launch(stk):
    """J = 7 is the one instantiation above 64 KiB of dynamic LDS (64 rows x 130 doubles =
    66 560 bytes): its launch sets hipFuncAttributeMaxDynamicSharedMemorySize first.  This is
    the first test of the file, so in a run of this file W^T at J = 7 is the first register
    launch of the process, then W; one full tile and a ragged one."""
    J, M = 7, 65
    N = ref.n_nodes(J)
    for transposed, tag in ((True, 'W^T'), (False, 'W  ')):
        X, want, bound = ref.case(J, M, transposed)
        y, kernel = _apply(stk, J, transposed, X, N + 1, x_pad=0.0)
        assert kernel == 'register'
        worst = ref.ratio(y[:, :N], want, bound, (J, transposed, 'cold start'))
        assert not y[:, N:].any()
        print(_line('register (first)', kernel, J, tag, N + 1, 0, 0, [M], worst))


# ---- 1. the launch paths at the row counts around the tile height ---------------------------
@pytest.mark.parametrize('J', REGISTER_J)
def test_register_path(stk, J):
    """ld = N + 1, aligned pointers: the register kernel.  x's padding zero: y within the
    bound and y's padding zero.  x's padding NaN: the data columns of y keep every bit -- the
    padding column rides along in the 16-byte copies and no data column reads it."""
    N = ref.n_nodes(J)
    for transposed, tag in DIRECTIONS:
        Ms, worst = row_counts('register', J), 0.0
        assert Ms == [1, 63, 64, 65, 129]
        for M in Ms:
            X, want, bound = ref.case(J, M, transposed)
            y, kernel = _apply(stk, J, transposed, X, N + 1, x_pad=0.0)
            assert kernel == 'register'
            worst = max(worst, ref.ratio(y[:, :N], want, bound, ('register', J, transposed, M)))
            assert not y[:, N:].any(), ('register', J, transposed, M, 'padding of y with padding of x zero')
            y_nan, _ = _apply(stk, J, transposed, X, N + 1, x_pad=NAN)
            assert np.array_equal(y_nan[:, :N], y[:, :N]), ('register', J, transposed, M, 'the padding leaks into the data')
        print(_line('register', kernel, J, tag, N + 1, 0, 0, Ms, worst))


def _generic_case(stk, path, J, transposed, tag, ld, x_off, y_off):
    """The generic kernel on one (J, direction, ld, alignment) at its five row counts, x's
    padding NaN: data within the bound, padding exactly zero."""
    N = ref.n_nodes(J)
    Ms, worst = row_counts('generic', J), 0.0
    for M in Ms:
        X, want, bound = ref.case(J, M, transposed)
        y, kernel = _apply(stk, J, transposed, X, ld, x_off, y_off, x_pad=NAN)
        assert kernel == 'generic', (path, J, ld, x_off, y_off)
        worst = max(worst, ref.ratio(y[:, :N], want, bound, (path, J, transposed, M, ld, x_off, y_off)))
        assert np.array_equal(y[:, N:], np.zeros((M, ld - N))), (path, J, transposed, M, ld, 'padding of y')
    print(_line(path, kernel, J, tag, ld, x_off, y_off, Ms, worst))
    return Ms


@pytest.mark.parametrize('J', ALL_J)
def test_generic_path_by_ld(stk, J):
    """ld = N (no padding), N + 3 and N + 4 (odd and even padding widths, NaN in x, zeroed in
    y): the generic kernel at every J it takes, M around R = min(128, 4160 // N)."""
    N = ref.n_nodes(J)
    H = min(128, 4160 // N)
    for transposed, tag in DIRECTIONS:
        for ld in (N, N + 3, N + 4):
            Ms = _generic_case(stk, 'generic by ld', J, transposed, tag, ld, 0, 0)
            assert Ms == sorted({1, max(H - 1, 1), H, H + 1, 2 * H + 1})
    assert {0: 128, 4: 128, 5: 126, 6: 64, 7: 32, 10: 4, 11: 2}.get(J, H) == H  # the rule, spelled out


@pytest.mark.parametrize('J', REGISTER_J)
def test_generic_path_by_alignment(stk, J):
    """ld = N + 1 as the register kernel wants it, but x, y or both 8 bytes off the 16-byte
    grid (its third entry condition): the generic kernel, which zeroes the padding column."""
    N = ref.n_nodes(J)
    for transposed, tag in DIRECTIONS:
        for x_off, y_off in ((1, 0), (0, 1), (1, 1)):
            _generic_case(stk, 'generic by align', J, transposed, tag, N + 1, x_off, y_off)


# ---- 2. every matrix entry -------------------------------------------------------------------
def _identity_paths(J):
    N = ref.n_nodes(J)
    paths = [('generic by ld', N, 0, 0), ('generic by ld', N + 3, 0, 0)]
    if J in REGISTER_J:
        paths += [('register', N + 1, 0, 0), ('generic by align', N + 1, 1, 0)]
    return paths


@pytest.mark.parametrize('J', ALL_J)
def test_every_matrix_entry(stk, J):
    """The kernel on the identity slab (M = N, row r the unit vector e_r) against the
    reference on the identity: each coefficient of each level at each node on its own, end
    nodes included; entries that are zero in W are zero bit for bit.  At J = 11 the slab is
    2049 x 2052 doubles."""
    N = ref.n_nodes(J)
    eye = np.eye(N)
    for transposed, tag in DIRECTIONS:
        want, bound = ref.identity_case(J, transposed)
        for path, ld, x_off, y_off in _identity_paths(J):
            y, kernel = _apply(stk, J, transposed, eye, ld, x_off, y_off, x_pad=0.0)
            assert kernel == ('register' if path == 'register' else 'generic')
            worst = ref.ratio(y[:, :N], want, bound, ('identity', path, J, transposed))
            assert np.array_equal(y[:, :N] != 0, np.asarray(want != 0)), ('identity', path, J, transposed, 'pattern')
            assert not y[:, N:].any()
            print(_line('identity/' + path.split()[-1], kernel, J, tag, ld, x_off, y_off, [N], worst))


# ---- 3. the same doubles ---------------------------------------------------------------------
@pytest.mark.parametrize('J', ALL_J)
def test_in_place_and_twice_give_the_same_doubles(stk, J):
    """y == x gives the bits of the out-of-place call, and a second call the bits of the
    first, on both kernels, over a full tile, a second full tile and a ragged one."""
    N = ref.n_nodes(J)
    for path, ld, x_off, y_off in _identity_paths(J):
        kernel = 'register' if path == 'register' else 'generic'
        M = 2 * tile_height(kernel, J) + 1
        for transposed, tag in DIRECTIONS:
            X, want, bound = ref.case(J, M, transposed)
            pad = 0.0 if kernel == 'register' else NAN
            y, ran = _apply(stk, J, transposed, X, ld, x_off, y_off, x_pad=pad)
            assert ran == kernel
            worst = ref.ratio(y[:, :N], want, bound, (path, J, transposed, M))
            twice, _ = _apply(stk, J, transposed, X, ld, x_off, y_off, x_pad=pad, calls=2)
            assert np.array_equal(twice, y), (path, J, transposed, 'second call')
            # in place both pointers are the slab's: aligned or 8 bytes off together
            off = y_off if path != 'generic by align' else 1
            same, ran = _apply(stk, J, transposed, X, ld, off, off, x_pad=pad, in_place=True)
            assert ran == kernel
            assert np.array_equal(same, y), (path, J, transposed, 'y == x')
            print(_line('same doubles', kernel, J, tag, ld, off, off, [M], worst))


# ---- 4. refusals -----------------------------------------------------------------------------
def test_refusals(stk):
    """Every argument stk_wavelet_apply is written to refuse: non-zero, a message that names
    the argument, and no kernel runs -- y keeps its bits."""
    lib = stk.lib()
    J, M = 3, 5
    N = ref.n_nodes(J)
    x, y = _Slab(M, N + 1, fill=1.0), _Slab(M, N + 1, fill=SENTINEL)
    px, py = x.view.data_ptr(), y.view.data_ptr()

    def refused(rc, *words):
        msg = lib.stk_last_error().decode()
        assert rc != 0 and 'stk_wavelet_apply' in msg and all(w in msg for w in words), (rc, msg, words)

    assert lib.stk_wavelet_apply(stk.stream(), M, J, N + 1, 0, px, py) == 0
    y.view.fill_(SENTINEL)
    refused(lib.stk_wavelet_apply(stk.stream(), M, -1, N + 1, 0, px, py), 'J=-1')
    refused(lib.stk_wavelet_apply(stk.stream(), M, 12, 4098, 0, px, py), 'J=12')
    refused(lib.stk_wavelet_apply(stk.stream(), 0, J, N + 1, 0, px, py), 'M=0')
    refused(lib.stk_wavelet_apply(stk.stream(), M, J, N - 1, 0, px, py), 'ld=%d' % (N - 1))
    refused(lib.stk_wavelet_apply(stk.stream(), M, J, N + 1, 0, None, py), 'x is')
    refused(lib.stk_wavelet_apply(stk.stream(), M, J, N + 1, 0, px, None), 'y is')
    torch.cuda.synchronize()
    assert np.all(y.flat.cpu().numpy() == SENTINEL)


# ---- 5. through the Python layer -------------------------------------------------------------
def _dd(N, M):
    from source.comm import Comm
    from source.mpi_vector import DofDistributionMPI
    return DofDistributionMPI(Comm(distributed=False), N, M)


@pytest.mark.parametrize('J', range(1, 9))
def test_kron_identity_operators(stk, J):
    """WaveletTransformKronIdentityMPI and its transpose on a one-rank KronVectorMPI of M =
    65 rows, as the drivers reach the kernel: a vector's ld is N + 1, the register kernel for
    J <= 7.  Three forms against the reference: the fused call; without it the all-to-all form
    (the same kernel on a slab of ld = N + 1); and the per-level composite, J applies of
    stk_time_csr_apply on I + split(j), whose bound is the same recurrence with 7 for 5
    (tests/test_wavelet_reference_host.py: gamma_{k+1} with k = 3, the stored 2^(j/2), the
    rounded s - 1)."""
    from source.mpi_vector import KronVectorMPI
    from source.wavelets import TransposedWaveletTransformKronIdentityMPI, WaveletTransformKronIdentityMPI
    M, N = 65, ref.n_nodes(J)
    dd = _dd(N, M)
    for transposed, tag, cls in ((False, 'W  ', WaveletTransformKronIdentityMPI),
                                 (True, 'W^T', TransposedWaveletTransformKronIdentityMPI)):
        op = cls(dd, J)
        X, want, bound = ref.case(J, M, transposed)
        vec = KronVectorMPI(dd, np.ascontiguousarray(X.T))
        assert vec.ld == N + 1 and np.array_equal(vec.buf.cpu().numpy()[:, :N], X)
        assert op._fused is not None and op.mode == 'transpose'
        figures = {}
        for form in ('fused', 'all-to-all', 'composite'):
            if form != 'fused':
                op._fused = None
            op.mode = 'composite' if form == 'composite' else 'transpose'
            out = op @ vec
            assert out is not vec and out.buf.data_ptr() != vec.buf.data_ptr()
            if form == 'fused':
                kernel = kernel_of(J, vec.ld, vec.buf.data_ptr(), out.buf.data_ptr())
                assert kernel == ('register' if J <= 7 else 'generic')
            y = out.buf.cpu().numpy()
            assert not y[:, N:].any(), (J, tag, form, 'padding')
            if form == 'composite':
                _, want_c, bound_c = ref.case(J, M, transposed, ref.COMPOSITE_COUNT)
                assert np.array_equal(want_c, want)
                figures[form] = ref.ratio(y[:, :N], want_c, bound_c, (J, tag, form))
            else:
                figures[form] = ref.ratio(y[:, :N], want, bound, (J, tag, form))
            assert np.array_equal(vec.buf.cpu().numpy()[:, :N], X)
        print('wavelet operators        %-8s J=%-2d %s M=%d: fused %.3f, all-to-all %.3f of the bound; composite %.3f of '
              'its bound (7 for 5)' % (kernel, J, tag, M, figures['fused'], figures['all-to-all'], figures['composite']))


@pytest.mark.parametrize('J', (6, 7, 8))
def test_level_ordered_operator(stk, J):
    """WaveletTransformOp(J, interleaved=False) beyond the J <= 5 of the g1 goldens, against
    the reference permuted to the level-ordered numbering; and interleaved=True.  Its device
    call passes ld = N: the generic kernel."""
    from source.wavelets import WaveletTransformOp
    N, M = ref.n_nodes(J), 37
    pos = ref.level_order(J)
    op = WaveletTransformOp(J, interleaved=False)
    assert np.array_equal(op._pos, pos)
    X = ref.signed_input(J, M, seed=1)  # (M, N): column r of the operator's argument is X[r]
    worst = {}
    Xi = np.empty_like(X)
    Xi[:, pos] = X                      # level-ordered coefficients at their nodes
    want, bound = ref.reference(J, Xi, False)
    worst['W'] = ref.ratio((op @ X.T).T, want, bound, (J, 'level-ordered W'))
    want, bound = ref.reference(J, X, True)
    worst['W^T'] = ref.ratio((op.T @ X.T).T, want[:, pos], bound[:, pos], (J, 'level-ordered W^T'))
    il = WaveletTransformOp(J, interleaved=True)
    worst['W il'] = ref.ratio((il @ X.T).T, *ref.reference(J, X, False), (J, 'interleaved W'))
    worst['W^T il'] = ref.ratio((il.T @ X.T).T, want, bound, (J, 'interleaved W^T'))
    assert kernel_of(J, N, 0, 0) == 'generic'
    print('wavelet level-ordered    generic  J=%-2d ld=N+0 M=%d: %s of the bound' % (
        J, M, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
