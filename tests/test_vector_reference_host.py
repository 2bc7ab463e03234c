"""What tests/test_vector_kernels_gpu.py measures the vector layer with (csrc/blas1.hip: stk_dot,
stk_slab_dot, stk_axpbyz; csrc/slab.hip: stk_transpose, stk_slab_upload / stk_slab_download,
stk_halo_pack, stk_halo_pack_records, stk_slab_extract_time_rows, stk_copy_block, stk_outer), and a
check of that yardstick where there is no GPU.

a. `slab_dot_model(X, Y)`: the summation shape that the comment above slab_dot_blocks_kernel
   states, written from that comment and from block_sum, step by step in binary64:

     rows in blocks of 256; in a block, row i goes to class i mod 8; a class adds its products in
     increasing i with fused multiply-adds from zero; the 8 class sums are added pairwise (0+1,
     2+3, ...; pairs of pairs; ...); block b goes to partial b mod 256 in increasing b; the 256
     partials meet in block_sum: within 64 lanes v[l] += v[l + off] for off = 32, 16, ... 1, then
     the 4 wavefronts' values are added in increasing order onto 0.0.

   It takes (M, n_loc) data alone: no ld, no column range, no partition.  NumPy has no fma, so
   the data of the bit-for-bit tests (`exact_product_data`) has at most 25 significant bits per
   operand (odd or even integers below 2**25, times a power of two, signed): every product is
   exact in binary64 and fma(x, y, a) = fl(x y + a), which is what NumPy computes.  The partial
   sums still round (the exponents of one column spread over 2**20), so the order matters:

b. on every catalogue shape the model differs, in at least one step, from the plain left-to-right
   sum (M >= 4) and from each restatement with one thing wrong (`WRONG`, where the shape lets
   them differ); the data of a shape is drawn again from a fixed sequence of seeds until it does.

c. Bounds.  U = 2**-53, gamma_L = L U / (1 - L U): |got - exact| <= gamma_L sum|x_i y_i|, L the
   longest chain of roundings one product passes through.  Adding 0.0 is exact, so only additions
   with two live operands count.

   stk_slab_dot, `slab_dot_roundings(M)`, with nb = ceil(M / 256) row blocks:
     chain of a class     ceil(min(M, 256) / 8)  one rounding per fma, the first (onto 0.0) rounds
                                                 the product
     class tree           ceil(log2 min(M, 8))
     chain of a partial   ceil(nb / 256) - 1     the first block of a partial is added onto 0.0
     wavefront tree       ceil(log2 min(nb, 64))
     wavefronts           ceil(min(nb, 256) / 64) - 1
   stk_dot, `dot_roundings(n)`, with n2 = n // 2 pairs, grid = min(max(ceil((n // 2 + 1) / 256), 1),
   2048) workgroups of 256 threads, two accumulators per thread:
     chain of an acc.     ceil(n2 / (256 grid)) products, + 1 for the odd tail (thread 0, acc0); at
                          least 1 (the product rounds, contracted to an fma or not)
     acc0 + acc1          1 if n2 >= 1
     block_sum            ceil(log2 min(n2, 64)) + ceil(min(n2, 256) / 64) - 1   (live threads)
     dot_final_kernel     ceil(grid / 1024) - 1, then ceil(log2 min(grid, 64)) + ceil(min(grid, 1024) / 64) - 1
   The reference is exact: every product split into two doubles (Dekker), all of them summed by
   math.fsum and rounded once, and what that rounding left summed once more (`dot_exact`: hi + lo).
   On data with signs the errors of a long sum cancel and sum|x y| does not, so the ratios of the
   long sizes are small however sharp L is; `positive_data` (factors in [1, 2)) is there to show
   that the bound is still far below any single product: a dropped or doubled term leaves it.

d. Plain NumPy restatements of the byte movers as functions of their arguments and of the
   destination's contents before the call: what they return is the whole destination afterwards,
   the entries the kernel must not touch included.
"""
import math

import numpy as np
import pytest

U = 2.0 ** -53
SD_ROWS, SD_CLASSES, SD_PARTIALS, WAVE = 256, 8, 256, 64
DOT_BS, DOT_BLOCKS, FLAT_CAP = 256, 2048, 4096
WRONG = ('classes-mod-4', 'rows-128', 'class-tree-left-to-right', 'partials-128', 'wave-tree-up')

SLAB_DOT_SHAPES = ([(M, n) for M in (1, 7, 8, 9, 255, 256, 257, 513) for n in (1, 2, 5, 6, 63, 64, 65)]
                   + [(513, n) for n in (255, 256, 257, 258, 320, 322)] + [(65793, 3)])
DOT_SIZES = (0, 1, 2, 3, 511, 512, 513, 524289, 1048575, 1048576, 1048577, 3 * 2 ** 20 + 5)


def gamma(L):
    return L * U / (1.0 - L * U)


def _log2_up(k):
    return 0 if k <= 1 else int(k - 1).bit_length()


def _up(a, b):
    return -(-a // b)


# ---- a. the summation shape of stk_slab_dot ---------------------------------------------------------
def _block_sum(v, up=False):
    """block_sum of csrc/blas1.hip on v of shape (threads, ...): result of thread 0."""
    waves = []
    for w in range(v.shape[0] // WAVE):
        lane = v[w * WAVE:(w + 1) * WAVE].copy()
        offs = (1, 2, 4, 8, 16, 32) if up else (32, 16, 8, 4, 2, 1)
        for off in offs:
            if up:  # (a wrong tree: neighbours first)
                lane = lane[0::2] + lane[1::2]
            else:
                lane[:off] = lane[:off] + lane[off:2 * off]
        waves.append(lane[0])
    r = np.zeros_like(waves[0])
    for s in waves:
        r = r + s
    return r


def slab_dot_model(X, Y, wrong=None):
    """The n_loc doubles stk_slab_dot returns for X, Y of shape (M, n_loc) whose products are exact
    in binary64.  `wrong`: one of WRONG, a restatement with one thing different."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    M, n_loc = X.shape
    rows = 128 if wrong == 'rows-128' else SD_ROWS
    classes = 4 if wrong == 'classes-mod-4' else SD_CLASSES
    n_part = 128 if wrong == 'partials-128' else SD_PARTIALS
    nb, per = _up(M, rows), rows // classes
    prod = np.zeros((nb * rows, n_loc))
    prod[:M] = X * Y  # exact by the choice of the data; rows past M add +0.0, which changes nothing
    prod = prod.reshape(nb, per, classes, n_loc)  # row i of a block: step i // classes of class i % classes
    acc = np.zeros((nb, classes, n_loc))
    for k in range(per):
        acc = acc + prod[:, k]  # fma(x, y, a) = fl(x y + a)
    if wrong == 'class-tree-left-to-right':
        blk = np.zeros((nb, n_loc))
        for c in range(classes):
            blk = blk + acc[:, c]
    else:
        w = 1
        while w < classes:
            acc[:, 0::2 * w] = acc[:, 0::2 * w] + acc[:, w::2 * w]
            w *= 2
        blk = acc[:, 0]
    part = np.zeros((max(n_part, SD_PARTIALS), n_loc))
    for b0 in range(0, nb, n_part):  # block b to partial b mod 256, increasing b
        k = min(n_part, nb - b0)
        part[:k] = part[:k] + blk[b0:b0 + k]
    return _block_sum(part, up=wrong == 'wave-tree-up')


def left_to_right(X, Y):
    acc = np.zeros(X.shape[1])
    for i in range(X.shape[0]):
        acc = acc + X[i] * Y[i]
    return acc


def can_differ(M, wrong):
    """Whether the shape lets the wrong restatement (None: the left-to-right sum) differ at all."""
    nb = _up(M, SD_ROWS)
    return {None: M >= 4, 'classes-mod-4': M >= 5, 'rows-128': M >= 129, 'class-tree-left-to-right': M >= 4,
            'partials-128': nb >= 129, 'wave-tree-up': nb >= 3}[wrong]


def _draw(M, n_loc, seed):
    rng = np.random.RandomState(seed)

    def one():
        m = rng.randint(1, 2 ** 25, size=(M, n_loc)).astype(np.float64)
        s = np.where(rng.rand(M, n_loc) < 0.5, -1.0, 1.0)
        return s * m * 2.0 ** rng.randint(-10, 11, size=(M, n_loc))
    return one(), one()


_DATA = {}


def exact_product_data(M, n_loc):
    """(X, Y, model) of the shape: 25-bit operands with mixed exponents, drawn again until the
    model differs from every other order the shape lets it differ from (b)."""
    if (M, n_loc) not in _DATA:
        for seed in range(1000 * n_loc + M, 1000 * n_loc + M + 64):
            X, Y = _draw(M, n_loc, seed)
            want = slab_dot_model(X, Y)
            others = [left_to_right(X, Y)] if can_differ(M, None) else []
            others += [slab_dot_model(X, Y, w) for w in WRONG if can_differ(M, w)]
            if all(np.any(o != want) for o in others):
                break
        else:
            raise AssertionError('no seed tells the orders apart at %r' % ((M, n_loc),))
        for a in (X, Y, want):
            a.setflags(write=False)
        _DATA[M, n_loc] = (X, Y, want)
    return _DATA[M, n_loc]


def general_data(M, n_loc, seed):
    """randn with mixed exponents: what the accuracy tests run on."""
    rng = np.random.RandomState(seed)
    one = lambda: rng.randn(M, n_loc) * 2.0 ** rng.randint(-8, 9, size=(M, n_loc))
    return one(), one()


def positive_data(M, n_loc, seed):
    rng = np.random.RandomState(seed)
    return 1.0 + rng.rand(M, n_loc), 1.0 + rng.rand(M, n_loc)


# ---- c. bounds -----------------------------------------------------------------------------------------
def slab_dot_roundings(M):
    nb = _up(M, SD_ROWS)
    return (_up(min(M, SD_ROWS), SD_CLASSES) + _log2_up(min(M, SD_CLASSES)) + _up(nb, SD_PARTIALS) - 1
            + _log2_up(min(nb, WAVE)) + _up(min(nb, SD_PARTIALS), WAVE) - 1)


def flat_grid(items, block=256):
    return int(min(max(_up(items, block), 1), FLAT_CAP))


def dot_grid(n):
    return min(flat_grid(n // 2 + 1, DOT_BS), DOT_BLOCKS)


def dot_roundings(n):
    if n <= 0:
        return 0
    n2, grid = n // 2, dot_grid(n)
    L = max(_up(n2, DOT_BS * grid) + (n & 1), 1)
    if n2 >= 1:
        L += 1 + _log2_up(min(n2, WAVE)) + _up(min(n2, DOT_BS), WAVE) - 1
    L += _up(grid, 1024) - 1 + _log2_up(min(grid, WAVE)) + _up(min(grid, 1024), WAVE) - 1
    return L


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def two_product(x, y):
    """p + e = x y exactly (Dekker); no overflow or underflow at the magnitudes used here."""
    p = x * y
    xh, xl = _split(x)
    yh, yl = _split(y)
    return p, ((xh * yh - p) + xh * yl + xl * yh) + xl * yl


def dot_exact(x, y):
    """(hi, lo, sum |x_i y_i|) of two vectors: hi the exact sum of the products rounded once, lo what
    that rounding left (rounded once), so that hi + lo is the sum to 2**-106."""
    p, e = two_product(np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel())
    terms = np.concatenate([p, e]).tolist()
    hi = math.fsum(terms)
    return hi, math.fsum(terms + [-hi]), math.fsum(np.abs(p))


def slab_dot_exact(X, Y):
    cols = [dot_exact(X[:, t], Y[:, t]) for t in range(X.shape[1])]
    return tuple(np.array([c[k] for c in cols]) for k in range(3))


def ratio(got, want, bound, lo=0.0):
    """Largest |got - (want + lo)| / bound; a zero bound admits no error."""
    err = np.abs((np.asarray(got, dtype=np.float64) - want) - lo)  # got - want is exact: they are neighbours
    bound = np.asarray(bound, dtype=np.float64) * np.ones_like(err)
    assert np.all(np.isfinite(err)), 'a result is not finite'
    if np.any(err[bound == 0.0] != 0.0):
        return np.inf
    live = bound > 0.0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


# ---- d. the byte movers -----------------------------------------------------------------------------
def transpose_ref(src, rows, cols, dst, zero_to):
    """src (>= rows, ld_src), dst (>= cols, ld_dst) before the call -> dst after it."""
    out = np.array(dst, copy=True)
    out[:cols, :rows] = src[:rows, :cols].T
    if zero_to > rows:
        out[:cols, rows:zero_to] = 0.0
    return out


def halo_pack_ref(x, n_loc, first, s_first, last, s_last):
    """x (M, ld); first / last: flat destinations before the call (or None) -> after it."""
    M = x.shape[0]
    out = []
    for dst, s, col in ((first, s_first, 0), (last, s_last, n_loc - 1)):
        if dst is not None:
            dst = np.array(dst, copy=True)
            dst[np.arange(M) * s] = x[:, col]
        out.append(dst)
    return out


def records_ref(x, n_loc):
    """(M, 4): (x[j][0], x[j][1], x[j][n_loc-2], x[j][n_loc-1]); a slab of one step repeats its step
    (t1 = t2 = 0), one of two steps gives (x0, x1, x0, x1)."""
    t1, t2 = (1, n_loc - 2) if n_loc > 1 else (0, 0)
    return np.stack([x[:, 0], x[:, t1], x[:, t2], x[:, n_loc - 1]], axis=1)


def extract_rows_ref(x, t_idx, out):
    """out (n_rows, ld_out) before the call -> after it: out[k, j] = x[j, t_idx[k]], j < M."""
    res = np.array(out, copy=True)
    for k, t in enumerate(t_idx):
        res[k, :x.shape[0]] = x[:, t]
    return res


def copy_block_ref(src, rows, cols, dst):
    out = np.array(dst, copy=True)
    out[:rows, :cols] = src[:rows, :cols]
    return out


def outer_ref(u_t, u_x, ld):
    """The whole (M, ld) slab: the kernel writes every column, those from n_loc on as +0.0."""
    out = np.zeros((len(u_x), ld))
    out[:, :len(u_t)] = np.asarray(u_x)[:, None] * np.asarray(u_t)[None, :]
    return out


def axpbyz_ref(a, x, b, y):
    """fma(a, x, fl(b y)) in np.longdouble, rounded once; exact there when a x fits 64 bits beside b y."""
    by = (b * y).astype(np.longdouble)
    return (np.longdouble(a) * x.astype(np.longdouble) + by).astype(np.float64)


def axpbyz_data(n, seed=3):
    """a, x of 25 bits (a x exact in binary64) and exponents close enough for a x + fl(b y) to be
    exact in the 64 bits of np.longdouble: the reference rounds once, as the fma does."""
    rng = np.random.RandomState(seed)
    x = rng.randint(-2 ** 24, 2 ** 24, size=n).astype(np.float64) * 2.0 ** -20
    y = np.where(rng.rand(n) < 0.5, -1.0, 1.0) * (1.0 + rng.rand(n))
    return 1.0 + 2.0 ** -20, x, -0.7, y


# ---- the yardstick checks itself -----------------------------------------------------------------
@pytest.mark.parametrize('M', sorted({M for M, _ in SLAB_DOT_SHAPES}))
def test_the_data_tells_summation_orders_apart(M):
    """b: on every shape, the model is not the left-to-right sum and not any WRONG restatement
    (where the shape lets them differ), and it is a function of (M, n_loc) data alone."""
    for (m, n_loc) in SLAB_DOT_SHAPES:
        if m != M:
            continue
        X, Y, want = exact_product_data(M, n_loc)
        assert np.array_equal(want, slab_dot_model(X, Y))
        p, e = two_product(X, Y)
        assert not e.any(), 'a product is not exact'
        if can_differ(M, None):
            assert np.any(left_to_right(X, Y) != want), (M, n_loc)
        for w in WRONG:
            if can_differ(M, w):
                assert np.any(slab_dot_model(X, Y, w) != want), (M, n_loc, w)
            else:
                assert np.array_equal(slab_dot_model(X, Y, w), want), (M, n_loc, w, 'differs where it cannot')
        # columns do not see each other: the model of one column is that column of the model
        t = n_loc // 2
        assert slab_dot_model(X[:, t:t + 1], Y[:, t:t + 1])[0] == want[t]


def test_every_wrong_restatement_is_told_apart_somewhere():
    seen = {w: any(can_differ(M, w) for M, _ in SLAB_DOT_SHAPES) for w in WRONG}
    assert all(seen.values()), seen


def test_the_model_sits_inside_the_bound():
    """c: the model on the exact-product data, and on general data (where its products round once
    more than the kernel's fused ones: L + 1), against the exact sums."""
    worst = 0.0
    for M, n_loc in SLAB_DOT_SHAPES:
        X, Y, want = exact_product_data(M, n_loc)
        exact, lo, mag = slab_dot_exact(X, Y)
        r = ratio(want, exact, gamma(slab_dot_roundings(M)) * mag, lo)
        assert r <= 1.0, (M, n_loc, r)
        worst = max(worst, r)
        Xg, Yg = general_data(M, n_loc, 7)
        exact, lo, mag = slab_dot_exact(Xg, Yg)
        assert ratio(slab_dot_model(Xg, Yg), exact, gamma(slab_dot_roundings(M) + 1) * mag, lo) <= 1.0
    print('model / bound: %.3f' % worst)
    assert worst >= 0.01, 'the bound is too loose to notice a dropped term'


def test_the_counts_of_roundings():
    assert [slab_dot_roundings(M) for M in (1, 2, 7, 8, 9, 255, 256, 257, 513, 65793)] == \
        [1, 2, 4, 4, 5, 35, 35, 36, 37, 35 + 1 + 6 + 3]
    assert [dot_grid(n) for n in DOT_SIZES] == [1, 1, 1, 1, 1, 2, 2, 1025, 2048, 2048, 2048, 2048]
    assert [dot_roundings(n) for n in (0, 1, 2, 3)] == [0, 1, 2, 3]
    # 3 * 2**20 + 5: four products and the tail, acc0 + acc1, 6 + 3, one chained partial, 6 + 15
    assert dot_roundings(DOT_SIZES[-1]) == 5 + 1 + 9 + 1 + 21
    x, y = general_data(1, 4099, 1)
    exact, lo, mag = dot_exact(x, y)
    assert abs(lo) <= U * abs(exact)
    assert abs(float(np.dot(x.ravel().astype(np.longdouble), y.ravel().astype(np.longdouble))) - exact) \
        <= 4099 * 2.0 ** -63 * mag
    assert abs(exact - math.fsum((x * y).ravel())) <= 4099 * U * mag


def test_the_byte_mover_restatements():
    rng = np.random.RandomState(0)
    src = rng.rand(5, 9)
    dst = np.full((7, 8), 9.0)
    out = transpose_ref(src, 5, 7, dst, 7)
    assert np.array_equal(out[:, :5], src[:, :7].T) and np.all(out[:, 5:7] == 0.0) and np.all(out[:, 7] == 9.0)
    assert np.array_equal(transpose_ref(src, 5, 7, dst, 0)[:, 5:], dst[:, 5:])
    x = rng.rand(4, 6)
    f, l = halo_pack_ref(x, 3, np.full(12, 9.0), 3, None, 1)
    assert l is None and np.array_equal(f[::3], x[:, 0]) and np.all(np.delete(f, np.arange(4) * 3) == 9.0)
    assert np.array_equal(halo_pack_ref(x, 3, None, 1, np.zeros(4), 1)[1], x[:, 2])
    assert np.array_equal(records_ref(x, 1), np.repeat(x[:, :1], 4, axis=1))
    assert np.array_equal(records_ref(x, 2), x[:, [0, 1, 0, 1]])
    assert np.array_equal(records_ref(x, 5), x[:, [0, 1, 3, 4]])
    out = extract_rows_ref(x, [2, 2, 0], np.full((3, 6), 9.0))
    assert np.array_equal(out[:, :4], x[:, [2, 2, 0]].T) and np.all(out[:, 4:] == 9.0)
    out = copy_block_ref(x, 3, 2, np.full((4, 5), 9.0))
    assert np.array_equal(out[:3, :2], x[:3, :2]) and (out == 9.0).sum() == 20 - 6
    o = outer_ref([2.0, 3.0], [1.0, -1.0, 0.5], 4)
    assert np.array_equal(o[:, :2], np.outer([1.0, -1.0, 0.5], [2.0, 3.0])) and not o[:, 2:].any()
    a, xs, b, ys = axpbyz_data(1001)
    assert np.array_equal(axpbyz_ref(a, xs, b, ys), a * xs + b * ys)  # a x is exact: one rounding either way
    assert not two_product(np.full(1001, a), xs)[1].any()
