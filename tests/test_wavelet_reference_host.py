"""What tests/test_wavelet_kernels_gpu.py measures the fused wavelet kernels
(csrc/wavelet.hip, stk_wavelet_apply) with, and a check of that yardstick where there is no
GPU: the stencil form of oracle/wavelets.py (level_step, level_step_transposed) in
np.longdouble, vectorised over the stride-S nodes, together with a component-wise rounding
bound of a float64 evaluation of the same stencil.

Layout.  Time is the LAST axis, as in a device slab: x[..., t], t = 0 .. 2^J, interleaved
numbering.  Level j acts on the nodes k S, S = 2^(J-j), k = 0 .. 2^j, with s = 2^(j/2) (here
sqrt(longdouble(2))**j), reading pre-level values only:

    W    odd  k: y = 1/2 (x[k-1] + x[k+1]) + s x[k]
         even k: y = x[k] - 1/2 s (x[k-1] + x[k+1]);  end nodes: y = x[k] - s x[k+-1]
    W^T  even k: y = x[k] + 1/2 x[k-1] + 1/2 x[k+1]    (a missing neighbour dropped)
         odd  k: y = s (x[k] - cl x[k-1] - cr x[k+1]), c = 1 next to an end node, else 1/2

W runs j = 1 .. J, W^T runs j = J .. 1.  Nodes that are no multiple of S are not touched by
level j: value and error are carried over unchanged.

Bound.  U = 2^-53, gamma_n = n U / (1 - n U).  Write L_j for the stencil above on the level's
nodes and |L_j| for the same stencil with every coefficient replaced by its absolute value.
Every term c x of a row of L_j reaches the result through at most five factors (1 + d),
|d| <= U, in a float64 evaluation:

  * s as the kernel holds it is off by up to 2 U relatively: the register kernel multiplies
    the correctly rounded sqrt(2) (one U) by a power of two, the generic kernel calls the
    device's exp2(0.5 j), which may be one unit in the last place (2 U) off.          -> 2
  * the inner sum xl + xr of W, or the two subtractions of the odd node of W^T (x[k] and
    x[k-1] pass both, x[k+1] the second only).                                        -> 2
  * one multiplication by s and one final addition; the products by 1/2, by 1 and the
    product 1/2 s are exact.  No term meets all of these: the worst is
      W   even interior  xl, xr: s (2), xl + xr (1), the product (1), the subtraction (1) = 5
      W^T odd            x[k], x[k-1]: two subtractions (2), s (2), the product (1)      = 5
    (W odd: 4 on s x[k], 2 on the neighbours; W end nodes: 4; W^T even: 2).
  * a fused multiply-add only removes roundings.

So fl(L_j v) = L_j v + d with |d| <= gamma_5 |L_j| |v| entry by entry, whatever the order.
The kernel applies level j to its own rounded values v = y_{j-1} + err, |err| <= e_{j-1}, so

    e_j = |L_j| e_{j-1} + gamma_5 |L_j| (|y_{j-1}| + e_{j-1}),     e_0 = 0,

on the level's nodes, y_{j-1} being the exact (extended precision) values before level j.
The bound is derived, not measured: 5 is the count above.  The reference's own rounding
(2^-64 per operation) is three orders below U and is not part of it.  `count` replaces the 5
for another evaluation of the same stencil: the per-level composite of
WaveletTransformKronIdentityMPI runs each level through stk_time_csr_apply on I + split(j),
whose rows hold k = 3 entries; that kernel's bound (tests/test_lu_and_factor_kernels_gpu.py)
is gamma_{k+1} = gamma_4 of the sum of magnitudes, identity included, and the stored entries
add theirs: 2^(j/2) as a double (2 U, as above) and the rounding of the diagonal entry s - 1
(at most U |s - 1| <= U s; the magnitude |1| + |s - 1| is s because s > 1): 4 + 2 + 1 = 7.

A node that level j does not touch is copied, not computed: it takes no gamma_5 term from
that level (the recurrence read over all nodes, with identity rows in |L_j|, would add one
per level and be up to J times wider on the finest nodes; this one is never wider).

The float64 oracle sits inside the bound at every J = 0 .. 11, matrix form and stencil form
alike (0.2 to 0.66 of it for J >= 1, the larger figures where more nodes are drawn), and a
float64 stencil with one thing wrong -- an end coefficient halved, cl / cr at the wrong
neighbour, s through float32, the levels in the wrong order, a node reading a post-level
value -- leaves it."""
import functools

import numpy as np
import pytest

from test_lu_reference_host import LD, U, gamma  # noqa: F401  (U: re-exported to the GPU tests)

KERNEL_COUNT = 5             # the fused kernels: the derivation above
COMPOSITE_COUNT = (3 + 1) + 2 + 1  # per-level composite: gamma_{k+1}, k = 3; s stored; s - 1 rounded
J_MAX = 11                   # stk_wavelet_apply takes J = 0 .. 11
SQRT2 = np.sqrt(LD(2))


def n_nodes(J):
    return 2**J + 1


# ---- the stencil in extended precision ------------------------------------------------------
def _level(v, s, transposed, sign):
    """One level on its own nodes: v[..., k], k = 0 .. 2^j (a new array).  sign = -1: L_j;
    sign = +1: |L_j| (every coefficient replaced by its absolute value)."""
    out = v.copy()
    left, mid, right = v[..., 0:-1:2], v[..., 1::2], v[..., 2::2]  # around every odd node
    if not transposed:
        out[..., 1::2] = LD(0.5) * (left + right) + s * mid
        out[..., 2:-1:2] = v[..., 2:-1:2] + sign * (LD(0.5) * s) * (v[..., 1:-2:2] + v[..., 3::2])
        out[..., 0] = v[..., 0] + sign * s * v[..., 1]
        out[..., -1] = v[..., -1] + sign * s * v[..., -2]
    else:
        out[..., 0:-1:2] += LD(0.5) * mid
        out[..., 2::2] += LD(0.5) * mid
        cl = np.full(mid.shape[-1], LD(0.5))
        cr = cl.copy()
        cl[0] = cr[-1] = LD(1)
        out[..., 1::2] = s * (mid + sign * cl * left + sign * cr * right)
    return out


def reference(J, X, transposed, count=KERNEL_COUNT):
    """(y_ref, bound) of W x (W^T x) along the last axis of X, both np.longdouble."""
    y = np.array(X, dtype=LD)
    assert y.shape[-1] == n_nodes(J), (y.shape, J)
    e = np.zeros_like(y)
    g = gamma(count)
    for j in (range(J, 0, -1) if transposed else range(1, J + 1)):
        S, s = 2**(J - j), SQRT2**j
        v, ev = y[..., ::S], e[..., ::S]
        e_new = _level(ev, s, transposed, +1) + g * _level(np.abs(v) + ev, s, transposed, +1)
        y[..., ::S] = _level(v, s, transposed, -1)
        e[..., ::S] = e_new
    return y, e


def ratio(got, want, bound, what=()):
    """The largest |got - want| in units of the bound, every entry checked (a zero bound
    admits no error); asserts it is at most 1."""
    got = np.asarray(got)
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape)
    assert np.all(np.isfinite(got)), (what, 'not finite')
    err = np.abs(got.astype(LD) - want)
    assert np.all(err[bound == 0] == 0), (what, 'error where the bound is zero')
    pos = bound > 0
    worst = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
    assert worst <= 1.0, (what, worst)
    return worst


def unchecked_ratio(got, want, bound):
    """The same figure without the assertion (inf: an error where the bound is zero)."""
    err = np.abs(np.asarray(got).astype(LD) - want)
    if np.any(err[bound == 0] != 0) or not np.all(np.isfinite(got)):
        return float('inf')
    pos = bound > 0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


# ---- inputs, shared with the GPU tests ------------------------------------------------------
def signed_input(J, M, seed=0):
    """(M, 2^J + 1) float64: standard normal values, every time node scaled by its own power
    of ten over twelve decades and every row by one over six -- neighbours in time differ by
    orders of magnitude, so an error in a small entry does not hide behind a large one."""
    rng = np.random.RandomState(1000 * J + M + seed)
    N = n_nodes(J)
    return rng.randn(M, N) * 10.0**rng.uniform(-6, 6, size=N) * 10.0**rng.uniform(-3, 3, size=(M, 1))


@functools.lru_cache(maxsize=None)
def case(J, M, transposed, count=KERNEL_COUNT, seed=0):
    """(X, y_ref, bound) for signed_input(J, M): computed once, shared, left unchanged."""
    X = signed_input(J, M, seed)
    y, e = reference(J, X, transposed, count)
    for a in (X, y, e):
        a.setflags(write=False)
    return X, y, e


@functools.lru_cache(maxsize=None)
def identity_case(J, transposed):
    """(y_ref, bound) of the identity slab: row r is the unit vector e_r, so row r of the
    result is column r of W (W^T)."""
    y, e = reference(J, np.eye(n_nodes(J)), transposed)
    for a in (y, e):
        a.setflags(write=False)
    return y, e


def level_order(J):
    """Position in the interleaved numbering of the k-th level-ordered wavelet (the `_pos`
    rule of WaveletTransformOp): level 0 -> the two end nodes, level j -> the odd multiples
    of 2^(J-j)."""
    pos = [0, 2**J]
    for j in range(1, J + 1):
        S = 2**(J - j)
        pos += [(2 * m + 1) * S for m in range(2**(j - 1))]
    return np.array(pos)


# ---- a float64 stencil, node by node as the kernels walk it, with one thing wrong ------------
MUTATIONS = ('end-coefficient-halved', 'c-at-the-wrong-neighbour', 's-through-float32', 'levels-in-the-wrong-order',
             'reads-post-level-values')


def stencil_float64(J, X, transposed, wrong=None):
    """csrc/wavelet.hip's arithmetic in NumPy float64 (time on the last axis); `wrong` names
    one mutation."""
    y = np.array(X, dtype=np.float64)
    order = list(range(J, 0, -1) if transposed else range(1, J + 1))
    if wrong == 'levels-in-the-wrong-order':
        order.reverse()
    for j in order:
        S, n = 2**(J - j), 2**j
        s = 2.0**(j // 2) * (1.4142135623730951 if j & 1 else 1.0)
        if wrong == 's-through-float32':
            s = float(np.float32(s))
        end = 0.5 * s if wrong == 'end-coefficient-halved' else s
        src = y if wrong == 'reads-post-level-values' else y.copy()
        ks = list(range(n + 1))
        if wrong == 'reads-post-level-values':  # the odd nodes first, then the even ones in place
            ks = ks[1::2] + ks[0::2]
        for k in ks:
            xc = src[..., k * S].copy()
            xl = src[..., (k - 1) * S] if k > 0 else 0.0
            xr = src[..., (k + 1) * S] if k < n else 0.0
            if not transposed:
                if k & 1:
                    v = 0.5 * (xl + xr) + s * xc
                elif k == 0:
                    v = xc - end * xr
                elif k == n:
                    v = xc - end * xl
                else:
                    v = xc - 0.5 * s * (xl + xr)
            elif k & 1:
                cl = 1.0 if k - 1 == 0 else 0.5
                cr = 1.0 if k + 1 == n else 0.5
                if wrong == 'c-at-the-wrong-neighbour':
                    cl, cr = cr, cl
                v = s * (xc - cl * xl - cr * xr)
            else:
                v = xc + 0.5 * xl + 0.5 * xr
            y[..., k * S] = v
    return y


# ---- the yardstick on the host ---------------------------------------------------------------
@pytest.mark.parametrize('J', range(J_MAX + 1))
def test_float64_oracle_sits_inside_the_bound(J):
    """oracle.wavelets.apply / apply_transposed (sparse p, q) and apply_stencil /
    apply_transposed_stencil (the kernel's specification) in float64, and this file's
    node-by-node float64 stencil: every entry within the bound."""
    from oracle import wavelets as ow
    M = 5
    figures = []
    for transposed, forms in ((False, (ow.apply, ow.apply_stencil)),
                              (True, (ow.apply_transposed, ow.apply_transposed_stencil))):
        X, y, e = case(J, M, transposed)
        for form in forms:
            figures.append(ratio(form(J, X.T).T, y, e, (J, form.__name__)))
        figures.append(ratio(stencil_float64(J, X, transposed), y, e, (J, transposed, 'stencil_float64')))
        assert J == 0 or np.all(e > 0)
        assert J > 0 or (np.array_equal(y, X) and not e.any())  # J = 0: the identity, exactly
    print('J = %d: float64 oracle at most %.3f of the bound' % (J, max(figures)))


@pytest.mark.parametrize('J', range(9))
def test_identity_against_the_two_scale_matrix(J):
    """The reference applied to the identity is source.wavelets.WaveletTransformMat(J) --
    built independently from the two-scale relations, level-ordered columns -- after the
    permutation to the interleaved numbering; W^T of the identity is the transpose."""
    from source.wavelets import WaveletTransformMat
    T = WaveletTransformMat(J).toarray()
    pos = level_order(J)
    y, e = identity_case(J, False)  # y[r, t] = W[t, r]
    worst = ratio(T, y.T[:, pos], e.T[:, pos], (J, 'W'))
    y, e = identity_case(J, True)   # y[r, t] = W^T[t, r] = W[r, t]
    worst = max(worst, ratio(T, y[:, pos], e[:, pos], (J, 'W^T')))
    assert np.array_equal(T != 0, np.asarray(y[:, pos] != 0))  # the same pattern, zeros exact
    print('J = %d: two-scale matrix at most %.3f of the bound' % (J, worst))


@pytest.mark.parametrize('J', (1, 2, 5, 8))
def test_the_composite_count_holds_the_level_matrices(J):
    """The per-level composite in float64 on the host (I + split(j) as SciPy CSR, the
    identity added as the accumulator's start) within the bound of count 7, and -- the
    point of a separate count -- the level matrices' stored entries are what it assumes:
    0.5, s - 1 and -0.5 s / -s with s = 2**(j/2) as a double."""
    from source.wavelets import WaveletTransformOp
    op = WaveletTransformOp(J, interleaved=True)
    for transposed in (False, True):
        X, y, e = case(J, 9, transposed, COMPOSITE_COUNT)
        Y = X.T.copy()
        for j in (range(J, 0, -1) if transposed else range(1, J + 1)):
            split = op.split(j)
            Y = Y + (split.T.tocsr() if transposed else split) @ Y
            assert set(np.unique(np.abs(split.data))) <= {0.0, 0.5, 2**(j / 2) - 1, 0.5 * 2**(j / 2), 2**(j / 2)}
            assert np.diff(split.indptr).max() <= 3
        worst = ratio(Y.T, y, e, (J, transposed, 'composite'))
        assert np.all(e >= case(J, 9, transposed)[2])
    print('J = %d: host composite at most %.3f of its bound' % (J, worst))


def _applies(J, wrong, transposed):
    """Whether the mutation changes the stencil at all -- by construction, not by result: the
    end coefficient belongs to W; cl / cr belong to W^T and differ only where an odd node has
    one end neighbour and one interior one (J >= 2); an order of levels needs two of them.  s
    through float32 is exact on even levels (a power of two) and every J >= 1 has level 1."""
    if wrong == 'end-coefficient-halved':
        return not transposed
    if wrong == 'c-at-the-wrong-neighbour':
        return transposed and J >= 2
    if wrong == 'levels-in-the-wrong-order':
        return J >= 2
    return True


MUTANTS = [(J, wrong, transposed) for J in (1, 2, 3, 6) for wrong in MUTATIONS for transposed in (False, True)
           if _applies(J, wrong, transposed)]


MUTANT_IDS = ['J%d-%s-%s' % (J, wrong, 'WT' if transposed else 'W') for J, wrong, transposed in MUTANTS]


@pytest.mark.parametrize('J,wrong,transposed', MUTANTS, ids=MUTANT_IDS)
def test_the_bound_separates(J, wrong, transposed):
    """A float64 stencil with one thing wrong exceeds the bound, and the same stencil with
    nothing wrong does not: the bound cannot pass a wrong kernel."""
    X, y, e = case(J, 5, transposed)
    assert ratio(stencil_float64(J, X, transposed), y, e, (J, transposed)) <= 1.0
    bad = unchecked_ratio(stencil_float64(J, X, transposed, wrong), y, e)
    print('J = %d %s %s: %.3g of the bound' % (J, 'W^T' if transposed else 'W', wrong, bad))
    assert bad > 1.0, (J, wrong, transposed, bad)


def test_every_mutation_is_tried_in_a_direction():
    assert {w for _, w, _ in MUTANTS} == set(MUTATIONS)
