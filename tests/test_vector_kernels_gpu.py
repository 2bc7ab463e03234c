"""The vector layer (csrc/blas1.hip: stk_slab_dot, stk_dot, stk_axpbyz; csrc/slab.hip: the byte
movers) through the ABI alone, against tests/test_vector_reference_host.py.

Every output lies in a guarded flat buffer (`Flat`, or `Slab` of the multigrid tests), pre-filled
with NaN where the kernel must write and with a sentinel where it must not; inputs carry NaN in
the padding column of an odd n_loc and in what lies behind their data, BEHIND behind the pair.
The movers are compared BIT FOR BIT with the restatements, untouched entries included.
stk_slab_dot returns, bit for bit, the doubles of `ref.slab_dot_model` on data whose products are
exact -- on ld = pair, on a wider ld, and on a column range inside a wider slab with other data
on both sides (what KronVectorMPI.dot passes for test-space slabs) -- and stays inside
gamma_L(M) sum|x y| of the exact sum on general data; stk_dot inside gamma_L(n).

(The slab kernels read pairs, so every ld here is even: the wider forms are pair + 4 and
pair + 6 columns, pair = n_loc + (n_loc & 1); an odd ld is one of the refusals.)

Paths and the cases that reach them (worst |got - exact| / bound of the recorded MI355X run; the
bit-for-bit tests have no ratio):

    path                                                          cases                                  worst
    slab_dot_blocks_kernel, groups > 1 (G <= 128), dead groups    M 1 7 8 9 255 256 257 513 with         0.957 (M 1)
      in the last workgroup (n_blocks mod groups != 0)              n_loc 1 2 5 6 (M 513, n_loc 1:       0.683 (M 7, 8)
    G = 256 exactly (np = 32), one group                            32 groups for 3 blocks); n_loc 63 64 0.410 (M 9)
    G > 256: rounds of SD_ITEMS (np = 33 .. 128)                  n_loc 65; M 513 n_loc 255, 256         0.096 (M 255 .. 257)
    second column-range launch, np = 1 / 32 / 33                  M 513 n_loc 257 258 / 320 / 322        0.086 (M 513)
    M < SD_CLASSES, classes without rows; tail block              M 1, 7; M 9 255 257 513
    slab_dot_steps_kernel, b += 256 runs twice                    M 65793 n_loc 3                        0.003
    pointer inside a wider slab, n_own < ld - 1                   every shape, layout `range`
    refusals: odd ld, steps outside N, pointers off 16 bytes      test_slab_dot_refusals
    dot_partial_kernel: odd tail, one workgroup / several         n 1 3 511 513 / 524289 ...             0.567 (n 1), 0.251 (n 3)
    DOT_BLOCKS cap, 2 .. 4 products per accumulator               n 1048577, 3 * 2**20 + 5               0.0007 signed, 0.059 positive (n >= 524289)
    dot_final_kernel, two partials per thread                     n 524289 (1025 partials) and above
    refusals: misaligned x, y; null work, out, input              test_dot_refusals
    axpbyz_kernel, second grid-stride pass (b != 0 and b = 0)     n 2 * 1048576 + 3
    transpose_kernel, tile loop twice (8194 tiles)                (33, 131073), (131073, 33)
    zero_to opens a row tile without a source row                 rows 32, zero_to 33, 34
    halo_pack*_kernel, second grid-stride pass                    M 1048577
    strides (1, 1) (2, 2) (3, 1), ld = n_loc + 5, one side only   every M, n_loc of test_halo_pack
    halo_pack_records_kernel, t1 = t2 = 0 / (x0, x1, x0, x1)      n_loc 1 / 2
    extract_rows_kernel: repeated, descending t_idx; ld_out gap   [4, 2, 2, 0], [0, 0], [1, 0, 1]; ld_out = M + 3
    extract_rows / copy_block / outer, second grid-stride pass    M 1048577 / 1048577 items / 1048579

(Signed data: the errors of a long sum cancel, sum|x y| does not, so the ratios fall with the
length however sharp L is -- 1 / (L sqrt n) is what random roundings give.  On the positive data of
test_dot the bound is asserted to be below 1e-6 of the smallest single product.)
"""
import numpy as np
import pytest
import torch

import test_vector_reference_host as ref
from test_multigrid_kernels_gpu import BEHIND, NAN, SENTINEL, Slab, pair_cols, stk  # noqa: F401  (stk: the fixture)

pytestmark = pytest.mark.gpu

WORST = {}


def note(path, r, case):
    if r >= WORST.get(path, (-1.0, None))[0]:
        WORST[path] = (r, case)


def show(path):
    print('%-28s worst %.3f of the bound  %r' % ((path,) + WORST[path]))


class Flat:
    """n entries inside a buffer of sentinels, filled with `fill`; `off` entries behind the grid of
    the guard (64 bytes)."""
    def __init__(self, n, fill, dtype=torch.float64, off=0, sentinel=SENTINEL):
        self.n, self.g, self.sentinel = n, (16 if dtype == torch.int32 else 8) + off, sentinel
        self.flat = torch.full((self.g + n + 8,), sentinel, dtype=dtype, device='cuda')
        assert self.flat.data_ptr() % 64 == 0
        self.view = self.flat[self.g:self.g + n]
        self.view.fill_(fill)

    def load(self, a):
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(a).ravel()).cuda())
        return self

    @property
    def ptr(self):
        return self.flat.data_ptr() + self.g * self.flat.element_size()

    def host(self, what='buffer'):
        """The entries, after a look at the guards."""
        h = self.flat.cpu().numpy()
        assert np.all(h[:self.g] == self.sentinel) and np.all(h[self.g + self.n:] == self.sentinel), (what, 'guard')
        return h[self.g:self.g + self.n].copy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else a.dtype)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (what, '%d entries differ in some bit; the first: %r, got %r for %r'
                           % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def slab_guards(s, what):
    h = s.flat.cpu().numpy()
    assert np.all(h[:s.start] == SENTINEL) and np.all(h[s.start + s.count:] == SENTINEL), (what, 'guard')
    return h[s.start:s.start + s.count].reshape(s.rows, s.ld)


def refused(stk, rc, text=None):
    assert rc != 0, 'a call that must be refused was accepted'
    with pytest.raises(stk.StkError, match=text):
        stk.check(rc)


# ---- stk_slab_dot -------------------------------------------------------------------------------------
LAYOUTS = ('pair', 'wide', 'range')


def place(X, layout, seed=0):
    """X (M, n_loc) in a guarded slab -> (slab, pointer, ld, the slab's contents on the host)."""
    M, n_loc = X.shape
    pc = pair_cols(n_loc)
    if layout != 'range':
        s = Slab(M, pc + (4 if layout == 'wide' else 0)).load(X)
        return s, s.ptr, s.ld
    s = Slab(M, pc + 6)  # two columns of other data in front, the pair, four behind
    live = np.random.RandomState(seed).randn(M, s.ld) * 1e3
    live[:, 2:2 + n_loc] = X
    live[:, 2 + n_loc:2 + pc] = NAN  # the column right behind an odd n_loc
    s.view.copy_(torch.from_numpy(live).cuda())
    return s, s.ptr + 16, s.ld


def slab_dot(stk, M, n_loc, ld, px, py, N, t_begin, what):
    lib = stk.lib()
    work = Flat(int(lib.stk_slab_dot_work_size(M, n_loc)), NAN)
    out = Flat(N, NAN)
    stk.check(lib.stk_slab_dot(stk.stream(), M, n_loc, ld, px, py, work.ptr, N, t_begin, out.ptr))
    work.host(what)
    h = out.host(what)
    other = np.concatenate([h[:t_begin], h[t_begin + n_loc:]])
    assert np.all(other == 0.0) and not np.any(np.signbit(other)), (what, 'a foreign step is not +0.0')
    return h[t_begin:t_begin + n_loc]


def shapes_of(M):
    return [n for m, n in ref.SLAB_DOT_SHAPES if m == M]


SLAB_M = sorted({M for M, _ in ref.SLAB_DOT_SHAPES})


@pytest.mark.parametrize('M', SLAB_M)
def test_slab_dot_is_the_stated_summation_shape(stk, M):
    """Bit for bit the model, on three layouts and three positions in the N-vector, twice."""
    for n_loc in shapes_of(M):
        X, Y, want = ref.exact_product_data(M, n_loc)
        N = n_loc + 3
        for layout in LAYOUTS:
            (sx, px, ld), (sy, py, _) = place(X, layout, 1), place(Y, layout, 2)
            before = sx.flat.clone(), sy.flat.clone()
            for t_begin in (0, 1, N - n_loc):
                what = (M, n_loc, layout, t_begin)
                got = slab_dot(stk, M, n_loc, ld, px, py, N, t_begin, what)
                same(got, want, what)
                same(slab_dot(stk, M, n_loc, ld, px, py, N, t_begin, what), got, what + ('second call',))
            for s, b in zip((sx, sy), before):  # inputs are inputs
                assert torch.equal(s.flat.view(torch.int64), b.view(torch.int64)), (M, n_loc, layout, 'input written')


@pytest.mark.parametrize('M', SLAB_M)
def test_slab_dot_accuracy(stk, M):
    """General data with mixed exponents: inside gamma_L(M) sum|x y| of the exact sum."""
    path = 'stk_slab_dot M=%d' % M
    for n_loc in shapes_of(M):
        X, Y = ref.general_data(M, n_loc, 11)
        exact, lo, mag = ref.slab_dot_exact(X, Y)
        bound = ref.gamma(ref.slab_dot_roundings(M)) * mag
        first = None
        for layout in LAYOUTS:
            (sx, px, ld), (sy, py, _) = place(X, layout, 3), place(Y, layout, 4)
            got = slab_dot(stk, M, n_loc, ld, px, py, n_loc + 1, 1, (M, n_loc, layout))
            r = ref.ratio(got, exact, bound, lo)
            note(path, r, (n_loc, layout))
            assert r <= 1.0, (M, n_loc, layout, r)
            first = got if first is None else first
            same(got, first, (M, n_loc, layout, 'layouts differ'))
    show(path)


def test_slab_dot_refusals(stk):
    lib, M, n_loc = stk.lib(), 9, 3
    X, Y, _ = ref.exact_product_data(9, 5)
    (sx, px, ld), (sy, py, _) = place(X[:, :3], 'wide'), place(Y[:, :3], 'wide')
    work, out = Flat(int(lib.stk_slab_dot_work_size(M, n_loc)) + 2, NAN), Flat(5, NAN)
    call = lambda **k: lib.stk_slab_dot(stk.stream(), M, n_loc, k.get('ld', ld), k.get('x', px), k.get('y', py),
                                        k.get('work', work.ptr), k.get('N', 5), k.get('t_begin', 0), out.ptr)
    refused(stk, call(ld=ld - 1), 'ld must be even')
    refused(stk, call(ld=2), 'bad sizes')
    refused(stk, call(t_begin=3), 'steps')
    refused(stk, call(N=2), 'steps')
    refused(stk, call(t_begin=-1), 'steps')
    for k in ('x', 'y', 'work'):
        refused(stk, call(**{k: dict(x=px, y=py, work=work.ptr)[k] + 8}), '16-byte')
    refused(stk, call(work=None), 'null')
    torch.cuda.synchronize()
    assert np.all(np.isnan(out.host())) and np.all(np.isnan(work.host())), 'a refused call wrote'
    stk.check(call())


# ---- stk_dot, stk_axpbyz -------------------------------------------------------------------------------
@pytest.mark.parametrize('n', ref.DOT_SIZES)
def test_dot(stk, n):
    lib = stk.lib()
    assert lib.stk_dot_work_size() == ref.DOT_BLOCKS
    grid, L = ref.dot_grid(n), ref.dot_roundings(n)
    for kind, data in (('signed', ref.general_data), ('positive', ref.positive_data)):
        x, y = data(1, n, 5) if n else (np.zeros((1, 0)), np.zeros((1, 0)))
        dx, dy = Flat(n, NAN).load(x), Flat(n, NAN).load(y)
        exact, lo, mag = ref.dot_exact(x, y)
        got = []
        for rep in range(2):
            work, out = Flat(ref.DOT_BLOCKS, NAN), Flat(1, NAN)
            stk.check(lib.stk_dot(stk.stream(), n, dx.ptr if n else None, dy.ptr if n else None, work.ptr, out.ptr))
            w = work.host(n)
            assert np.all(np.isfinite(w[:grid])) and np.all(np.isnan(w[grid:])), (n, 'partials written: not exactly `grid`')
            got.append(out.host(n))
        same(got[0], got[1], (n, 'second call'))
        bound = ref.gamma(L) * mag
        r = ref.ratio(got[0], exact, bound, lo)
        print('stk_dot n=%d  L=%d  %s: %.4f of the bound' % (n, L, kind, r))
        assert r <= 1.0, (n, kind, r)
        if kind == 'positive' and n:
            assert bound < 1e-6 * np.abs(x * y).min(), (n, 'a dropped term would hide inside the bound')
        if n == 0:
            assert got[0][0] == 0.0 and not np.signbit(got[0][0])
        dx.host(), dy.host()


def test_dot_refusals(stk):
    lib = stk.lib()
    x, y = Flat(8, 1.0), Flat(8, 1.0)
    work, out = Flat(ref.DOT_BLOCKS, NAN), Flat(1, NAN)
    refused(stk, lib.stk_dot(stk.stream(), 6, x.ptr + 8, y.ptr, work.ptr, out.ptr), '16-byte')
    refused(stk, lib.stk_dot(stk.stream(), 6, x.ptr, y.ptr + 8, work.ptr, out.ptr), '16-byte')
    refused(stk, lib.stk_dot(stk.stream(), 6, x.ptr, y.ptr, None, out.ptr), 'null')
    refused(stk, lib.stk_dot(stk.stream(), 6, x.ptr, y.ptr, work.ptr, None), 'null')
    refused(stk, lib.stk_dot(stk.stream(), 6, None, y.ptr, work.ptr, out.ptr), 'null')
    torch.cuda.synchronize()
    assert np.all(np.isnan(out.host())) and np.all(np.isnan(work.host()))


def test_axpbyz_second_grid_stride_pass(stk):
    """n = 2 * 1048576 + 3: 4096 workgroups hold 1048576 pairs, the last pair and the odd tail come
    in the second pass.  Bit for bit fma(a, x, fl(b y)); b = 0 ignores y (NaN) and gives fl(a x)."""
    n = 2 * 1048576 + 3
    assert ref.flat_grid(n // 2 + 1) == ref.FLAT_CAP and n // 2 > ref.FLAT_CAP * 256
    a, x, b, y = ref.axpbyz_data(n)
    dx, dy = Flat(n, NAN).load(x), Flat(n, NAN).load(y)
    z = Flat(n, NAN)
    stk.check(stk.lib().stk_axpbyz(stk.stream(), n, a, dx.ptr, b, dy.ptr, z.ptr))
    same(z.host(), ref.axpbyz_ref(a, x, b, y), 'fma(a, x, b y)')
    z, nans = Flat(n, NAN), Flat(n, NAN)
    stk.check(stk.lib().stk_axpbyz(stk.stream(), n, a, dx.ptr, 0.0, nans.ptr, z.ptr))
    same(z.host(), a * x, 'a x')
    same(dx.host(), x, 'x'), same(dy.host(), y, 'y')


# ---- stk_transpose, upload, download ---------------------------------------------------------------------
def run_transpose(stk, rows, cols, zero_to, pad_src=3, pad_dst=2, seed=0):
    ld_src, ld_dst = cols + pad_src, max(rows, zero_to) + pad_dst
    data = np.random.RandomState(seed).randn(rows, cols)
    src = Slab(rows, ld_src)  # NaN behind the data
    src.view[:, :cols] = torch.from_numpy(data).cuda()
    dst = Slab(cols, ld_dst)
    dst.view.fill_(BEHIND)
    stk.check(stk.lib().stk_transpose(stk.stream(), rows, cols, src.ptr, ld_src, dst.ptr, ld_dst, zero_to))
    what = ('transpose', rows, cols, zero_to)
    want = ref.transpose_ref(slab_guards(src, what), rows, cols, np.full((cols, ld_dst), BEHIND), zero_to)
    same(slab_guards(dst, what), want, what)


@pytest.mark.parametrize('rows,cols', [(1, 1), (31, 33), (32, 32), (33, 31), (32, 64)])
def test_transpose(stk, rows, cols):
    for zero_to in (0, rows, rows + 1, rows + 2):
        run_transpose(stk, rows, cols, zero_to)
    run_transpose(stk, rows, cols, 0, pad_src=0, pad_dst=0)


@pytest.mark.parametrize('rows,cols,zero_to', [(33, 131073, 34), (131073, 33, 0)])
def test_transpose_runs_its_tile_loop_twice(stk, rows, cols, zero_to):
    tiles = -(-cols // 32) * -(-max(rows, zero_to) // 32)
    assert tiles == 8194 > 256 * 32
    run_transpose(stk, rows, cols, zero_to)


def test_transpose_refusals(stk):
    lib, a, b = stk.lib(), Flat(64, 1.0), Flat(64, NAN)
    refused(stk, lib.stk_transpose(stk.stream(), 4, 4, a.ptr, 4, a.ptr, 4, 0), 'bad arguments')
    refused(stk, lib.stk_transpose(stk.stream(), 4, 4, a.ptr, 4, b.ptr, 5, 6), 'leading')
    refused(stk, lib.stk_transpose(stk.stream(), 4, 4, a.ptr, 4, b.ptr, 3, 0), 'leading')
    refused(stk, lib.stk_transpose(stk.stream(), 4, 4, a.ptr, 3, b.ptr, 4, 0), 'leading')
    refused(stk, lib.stk_transpose(stk.stream(), 0, 4, a.ptr, 4, b.ptr, 4, 0), 'bad arguments')
    torch.cuda.synchronize()
    assert np.all(np.isnan(b.host()))


@pytest.mark.parametrize('M,n_loc', [(1, 1), (33, 32), (131073, 3)])
def test_slab_upload_download_round_trip(stk, M, n_loc):
    lib = stk.lib()
    X = np.random.RandomState(M).randn(n_loc, M)  # time-major on the host
    for ld in (pair_cols(n_loc), pair_cols(n_loc) + 2):
        s = Slab(M, ld)
        stk.check(lib.stk_slab_upload(stk.stream(), M, n_loc, ld, X.ctypes.data, s.ptr))
        h = slab_guards(s, ('upload', M, n_loc, ld))
        same(h[:, :n_loc], X.T, ('upload', M, n_loc, ld))
        assert np.all(h[:, n_loc:] == 0.0) and not np.any(np.signbit(h[:, n_loc:])), 'padding is not +0.0'
        s.view[:, n_loc:] = NAN  # the download must not read it
        back = np.full(16 + M * n_loc, SENTINEL)
        back[8:8 + M * n_loc] = NAN
        stk.check(lib.stk_slab_download(stk.stream(), M, n_loc, ld, s.ptr, back[8:].ctypes.data))
        assert np.all(back[:8] == SENTINEL) and np.all(back[8 + M * n_loc:] == SENTINEL)
        same(back[8:8 + M * n_loc].reshape(n_loc, M), X, ('download', M, n_loc, ld))


# ---- stk_halo_pack, stk_halo_pack_records ---------------------------------------------------------------
@pytest.mark.parametrize('n_loc', (1, 2, 3, 9))
@pytest.mark.parametrize('M', (1, 255, 256, 257, 1048577))
def test_halo_pack(stk, M, n_loc):
    lib = stk.lib()
    assert M <= 257 or M > ref.flat_grid(M) * 256  # the long case: second grid-stride pass
    for ld in (pair_cols(n_loc), n_loc + 5):
        X = np.random.RandomState(n_loc).randn(M, n_loc)
        x = Slab(M, ld).load(X)
        xh = slab_guards(x, 'x')
        rec_want = ref.records_ref(X, n_loc)
        if n_loc == 1:
            same(rec_want, np.repeat(X, 4, axis=1), '(a, a, a, a)')
        if n_loc == 2:
            same(rec_want, np.concatenate([X, X], axis=1), '(x0, x1, x0, x1)')
        for s_first, s_last in ((1, 1), (2, 2), (3, 1)):
            for use_first, use_last in ((1, 0), (0, 1), (1, 1)):
                what = (M, n_loc, ld, s_first, s_last, use_first, use_last)
                for records in (False, True):
                    first = Flat(M * s_first, BEHIND) if use_first else None
                    last = Flat(M * s_last, BEHIND) if use_last else None
                    args = (stk.stream(), M, n_loc, ld, x.ptr, first.ptr if first else None, s_first,
                            last.ptr if last else None, s_last)
                    if records:
                        rec = Flat(4 * M, NAN)
                        assert rec.ptr % 32 == 0
                        stk.check(lib.stk_halo_pack_records(*(args + (rec.ptr,))))
                        same(rec.host(what).reshape(M, 4), rec_want, what + ('records',))
                    else:
                        stk.check(lib.stk_halo_pack(*args))
                    f_want, l_want = ref.halo_pack_ref(xh, n_loc, np.full(M * s_first, BEHIND) if first else None,
                                                       s_first, np.full(M * s_last, BEHIND) if last else None, s_last)
                    if first:
                        same(first.host(what), f_want, what + ('first', records))
                    if last:
                        same(last.host(what), l_want, what + ('last', records))
        same(slab_guards(x, 'x'), xh, 'x written')


def test_halo_pack_refusals(stk):
    lib, M = stk.lib(), 5
    x = Slab(M, 4).load(np.ones((M, 3)))
    dst, rec = Flat(2 * M, NAN), Flat(4 * M + 4, NAN)
    st = stk.stream()
    refused(stk, lib.stk_halo_pack(st, M, 3, 4, x.ptr, None, 1, None, 1), 'no destination')
    refused(stk, lib.stk_halo_pack(st, M, 3, 4, x.ptr, dst.ptr, 0, None, 1), 'stride')
    refused(stk, lib.stk_halo_pack(st, M, 5, 4, x.ptr, dst.ptr, 1, None, 1), 'bad arguments')
    refused(stk, lib.stk_halo_pack_records(st, M, 3, 4, x.ptr, None, 1, None, 1, rec.ptr + 16), '32-byte')
    refused(stk, lib.stk_halo_pack_records(st, M, 3, 4, x.ptr, None, 1, None, 1, rec.ptr + 8), '32-byte')
    refused(stk, lib.stk_halo_pack_records(st, M, 3, 4, x.ptr, None, 1, None, 1, None), 'bad arguments')
    refused(stk, lib.stk_halo_pack_records(st, M, 3, 4, x.ptr, dst.ptr, 1, dst.ptr, 0, rec.ptr), 'stride')
    torch.cuda.synchronize()
    assert np.all(np.isnan(dst.host())) and np.all(np.isnan(rec.host()))
    stk.check(lib.stk_halo_pack_records(st, M, 3, 4, x.ptr, None, 1, None, 1, rec.ptr))  # no destination is fine here


# ---- stk_slab_extract_time_rows, stk_copy_block, stk_outer ------------------------------------------------
@pytest.mark.parametrize('M,n_loc,ld,t_idx', [(257, 5, 6, [3]), (257, 5, 10, [4, 2, 2, 0]), (1, 1, 2, [0, 0]),
                                              (1048577, 2, 2, [1, 0, 1])])
def test_extract_time_rows(stk, M, n_loc, ld, t_idx):
    X = np.random.RandomState(M % 1000).randn(M, n_loc)
    x = Slab(M, ld).load(X)
    xh = slab_guards(x, 'x')
    ld_out, n_rows = M + 3, len(t_idx)
    out = Flat(n_rows * ld_out, BEHIND)
    d_idx = stk.to_dev(np.array(t_idx, dtype=np.int32))
    stk.check(stk.lib().stk_slab_extract_time_rows(stk.stream(), M, n_rows, stk.ptr(d_idx), x.ptr, ld, out.ptr, ld_out))
    want = ref.extract_rows_ref(xh, t_idx, np.full((n_rows, ld_out), BEHIND))
    same(out.host().reshape(n_rows, ld_out), want, (M, t_idx))
    refused(stk, stk.lib().stk_slab_extract_time_rows(stk.stream(), M, n_rows, stk.ptr(d_idx), x.ptr, ld, out.ptr, M - 1),
            'bad arguments')


@pytest.mark.parametrize('rows,cols,ld_src,ld_dst', [(37, 5, 7, 9), (300, 1, 1, 4), (1048577, 1, 3, 2), (4099, 257, 257, 258)])
def test_copy_block(stk, rows, cols, ld_src, ld_dst):
    S = np.random.RandomState(cols).randn(rows, ld_src)
    src, dst = Flat(rows * ld_src, NAN).load(S), Flat(rows * ld_dst, BEHIND)
    stk.check(stk.lib().stk_copy_block(stk.stream(), rows, cols, src.ptr, ld_src, dst.ptr, ld_dst))
    same(dst.host().reshape(rows, ld_dst), ref.copy_block_ref(S, rows, cols, np.full((rows, ld_dst), BEHIND)),
         (rows, cols))
    same(src.host().reshape(rows, ld_src), S, 'src written')


def test_copy_block_of_nothing_and_refusals(stk):
    lib, st = stk.lib(), stk.stream()
    src, dst = Flat(12, 1.0), Flat(12, NAN)
    for rows, cols in ((0, 3), (4, 0), (0, 0)):
        assert lib.stk_copy_block(st, rows, cols, src.ptr, 3, dst.ptr, 3) == 0
        assert lib.stk_copy_block(st, rows, cols, None, 3, None, 3) == 0
    refused(stk, lib.stk_copy_block(st, 4, 3, src.ptr, 2, dst.ptr, 3), 'bad sizes')
    refused(stk, lib.stk_copy_block(st, 4, 3, src.ptr, 3, dst.ptr, 2), 'bad sizes')
    refused(stk, lib.stk_copy_block(st, 4, 3, None, 3, dst.ptr, 3), 'null')
    refused(stk, lib.stk_copy_block(st, -1, 3, src.ptr, 3, dst.ptr, 3), 'bad sizes')
    torch.cuda.synchronize()
    assert np.all(np.isnan(dst.host()))


@pytest.mark.parametrize('M,n_loc,ld', [(1, 1, 1), (257, 5, 5), (257, 5, 6), (257, 5, 9), (149797, 3, 7)])
def test_outer(stk, M, n_loc, ld):
    """Bit for bit u_t[t] * u_x[i]; every column from n_loc on of every row is +0.0 (all ld are written)."""
    rng = np.random.RandomState(M)
    u_t, u_x = rng.randn(n_loc), rng.randn(M)
    if M > 257:
        assert M * ld > ref.FLAT_CAP * 256
    dt, dx, y = Flat(n_loc, NAN).load(u_t), Flat(M, NAN).load(u_x), Flat(M * ld, NAN)
    stk.check(stk.lib().stk_outer(stk.stream(), M, n_loc, ld, dt.ptr, dx.ptr, y.ptr))
    same(y.host().reshape(M, ld), ref.outer_ref(u_t, u_x, ld), (M, n_loc, ld))
    refused(stk, stk.lib().stk_outer(stk.stream(), M, n_loc, n_loc - 1, dt.ptr, dx.ptr, y.ptr), 'bad arguments')
