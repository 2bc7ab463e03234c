"""What tests/test_lu_and_factor_kernels_gpu.py measures the device LU solve with, and a
check of that yardstick where there is no GPU: triangular factors built by hand, the solve
Pr A Pc = L U written out in np.longdouble, the backward bound of a substitution, and a
model of the launch plan csrc/sptrsv.hip derives from a pair of factors.

Bound.  U = 2^-53, gamma_n = n U / (1 - n U).  A row with k entries (diagonal included)
computes (rhs - sum v x) (1 / d): every product passes at most ceil(k / 16) fused
multiply-adds and 4 additions of the shuffle tree, then one subtraction, the rounded
reciprocal and one multiplication, so the computed y solves (T + dT) y = c with
|dT| <= gamma_{k+6} |T| entry by entry, in any order of summation.  With c[perm_r[i]] =
b[i], z[perm_c[i]] = x[i], g_L = gamma_{k_L+6}, g_U = gamma_{k_U+6} (k_L, k_U the longest
rows) therefore

    |c - L U z| <= (g_L + g_U + g_L g_U) |L| |U| |z|        entry by entry,

residual and bound evaluated in extended precision.  The float64 substitution of this file
(NumPy, row by row) sits inside it -- 0.02-0.12 of the bound on the chain and comb cases --
and its largest forward error against the longdouble solution, e_host, is the yardstick
of the dense-top form on the device, which has no backward bound."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

U = 2.0**-53
LD = np.longdouble
WIDE = 64        # csrc/sptrsv.hip: a level with at least this many rows is a launch of its own
TOP_LEVELS = 16  # a dense top needs at least this many levels from the first narrow one on
N_RHS = 33       # columns of every right-hand side (the longest slab of the GPU tests)


def gamma(n):
    return LD(n) * LD(U) / (LD(1) - LD(n) * LD(U))


def test_extended_precision_is_extended():
    assert np.finfo(LD).eps < 2e-19


# ---- factors ----------------------------------------------------------------------------
class Factors:
    """L (unit lower, diagonal stored or not), U (upper with its diagonal) as CSR with sorted
    int32 columns, and SuperLU's two permutations (None: identity)."""
    def __init__(self, name, L, Um, perm_r=None, perm_c=None):
        self.name = name
        self.L, self.U = sp.csr_matrix(L, dtype=np.float64), sp.csr_matrix(Um, dtype=np.float64)
        for T in (self.L, self.U):
            T.sort_indices()
            T.indptr, T.indices = T.indptr.astype(np.int32), T.indices.astype(np.int32)
        self.n = self.L.shape[0]
        self.perm_r = None if perm_r is None else np.ascontiguousarray(perm_r, dtype=np.int32)
        self.perm_c = None if perm_c is None else np.ascontiguousarray(perm_c, dtype=np.int32)
        self.Ls = sp.csr_matrix(sp.tril(self.L, -1))  # the part below the diagonal
        self.Ls.sort_indices()
        self.k_L = int(np.diff(self.Ls.indptr).max()) + 1
        self.k_U = int(np.diff(self.U.indptr).max())

    def permuted(self, rng):
        """The same factors behind independent random perm_r, perm_c."""
        return Factors(self.name + '-perm', self.L, self.U, rng.permutation(self.n), rng.permutation(self.n))

    def rhs(self, n_rhs=N_RHS):
        return np.random.RandomState(self.n + 7 * n_rhs).randn(self.n, n_rhs)


def _assemble(n, rows, cols, vals):
    return sp.csr_matrix((np.asarray(vals, dtype=np.float64), (np.asarray(rows), np.asarray(cols))), shape=(n, n))


def _from_rows(n, l_rows, u_rows, explicit, rng, name):
    """l_rows[i] / u_rows[i]: the columns of row i off the diagonal.  Entries uniform in
    (-1/2, 1/2) / fan, U's diagonal in (1, 2): cond(L U) is a small constant."""
    r, c, v = [], [], []
    for i, cs in enumerate(l_rows):
        r += [i] * len(cs)
        c += list(cs)
        v += list(rng.uniform(-0.5, 0.5, len(cs)) / max(len(cs), 1))
    if explicit:
        r, c, v = r + list(range(n)), c + list(range(n)), v + [1.0] * n
    L = _assemble(n, r, c, v)
    r, c, v = list(range(n)), list(range(n)), list(1.0 + rng.rand(n))
    for i, cs in enumerate(u_rows):
        r += [i] * len(cs)
        c += list(cs)
        v += list(rng.uniform(-0.5, 0.5, len(cs)) / max(len(cs), 1))
    return Factors(name, L, _assemble(n, r, c, v))


def chain(n, explicit=True, seed=1):
    """L unit lower bidiagonal, U upper bidiagonal: n levels of one row."""
    rng = np.random.RandomState(seed + n)
    return _from_rows(n, [[i - 1] if i else [] for i in range(n)], [[i + 1] if i + 1 < n else [] for i in range(n)],
                      explicit, rng, 'chain-%d-%s' % (n, 'explicit' if explicit else 'implicit'))


def comb(n_leaf, n_chain, late_leaf=False, seed=2):
    """n_leaf rows without L entries, then a chain of n_chain rows that each read the row
    before and 5 random leaves; U's leaf rows read 3 rows of the chain, a chain row the next.
    late_leaf: the last leaf comes AFTER the chain, and the chain's last row reads it in U --
    U's rows of S then reach outside S (not closed)."""
    rng = np.random.RandomState(seed + 1000 * n_leaf + n_chain)
    n = n_leaf + n_chain
    first = n_leaf - 1 if late_leaf else n_leaf   # first chain row
    leaves = np.r_[np.arange(first), [n - 1]] if late_leaf else np.arange(n_leaf)
    chain_rows = np.arange(first, first + n_chain)
    l_rows, u_rows = [[] for _ in range(n)], [[] for _ in range(n)]
    for q, i in enumerate(chain_rows):
        below = leaves[leaves < i]
        l_rows[i] = sorted(([i - 1] if q else []) + list(rng.choice(below, min(5, len(below)), replace=False)))
        if q + 1 < n_chain:
            u_rows[i] = [i + 1]
    for i in leaves:
        above = chain_rows[chain_rows > i]
        u_rows[i] = sorted(rng.choice(above, min(3, len(above)), replace=False))
    if late_leaf:
        u_rows[chain_rows[-1]] = [n - 1]
    return _from_rows(n, l_rows, u_rows, True, rng,
                      'comb-%d-%d%s' % (n_leaf, n_chain, '-late-leaf' if late_leaf else ''))


ROW_LENGTHS = (0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 130, 300)


def row_lengths(ell, n=400, seed=3):
    """Row i of L has min(i, ell) entries: the row before it (so the rows are a chain of n
    levels) and random earlier ones; U the same, mirrored."""
    rng = np.random.RandomState(seed + ell)
    l_rows = []
    for i in range(n):
        k = min(i, ell)
        others = list(rng.choice(i - 1, k - 1, replace=False)) if k > 1 else []
        l_rows.append(sorted([i - 1] + others) if k else [])
    u_rows = [[n - 1 - j for j in l_rows[n - 1 - i]][::-1] for i in range(n)]
    return _from_rows(n, l_rows, u_rows, True, rng, 'rows-%d' % ell)


def grid_cap(n_half=4100, seed=4):
    """n_half rows without L entries, then n_half rows that each read 3 of them; U mirrored.
    Two levels of n_half rows in either factor."""
    rng = np.random.RandomState(seed)
    n = 2 * n_half
    l_rows = [[] for _ in range(n_half)] + [sorted(rng.choice(n_half, 3, replace=False)) for _ in range(n_half)]
    u_rows = [sorted(n_half + rng.choice(n_half, 3, replace=False)) for _ in range(n_half)] + [[] for _ in range(n_half)]
    return _from_rows(n, l_rows, u_rows, True, rng, 'grid-cap-%d' % n_half)


def from_superlu(name, lu):
    return Factors(name, lu.L, lu.U, lu.perm_r, lu.perm_c)


@functools.lru_cache(maxsize=None)
def superlu_random():
    """A random unsymmetric matrix through default splu, the reference's own call
    (linop.py:18-26): perm_r != perm_c, and U's rows of S reach outside S."""
    from scipy.sparse.linalg import splu
    mat = sp.random(300, 300, 0.02, random_state=np.random.RandomState(3)) + sp.diags(np.linspace(0.5, 1.5, 300))
    return from_superlu('superlu-random-300', splu(sp.csc_matrix(mat)))


def laplacian(m=31):
    """The five-point Laplacian on an m x m grid."""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(m, m))
    return sp.csr_matrix(sp.kron(sp.eye(m), T) + sp.kron(T, sp.eye(m)))


@functools.lru_cache(maxsize=None)
def superlu_laplacian():
    """The factors InvLinOp computes of the 31 x 31 Laplacian (SymmetricMode)."""
    from scipy.sparse.linalg import splu
    lu = splu(sp.csc_matrix(laplacian()), options={"SymmetricMode": True}, permc_spec="MMD_AT_PLUS_A")
    return from_superlu('superlu-laplacian-961', lu)


# ---- the launch plan csrc/sptrsv.hip derives ----------------------------------------------
def _depths(T, lower, take=None, deps=None):
    n = T.shape[0]
    depth = np.zeros(n, dtype=np.int64)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        if take is not None and not take[i]:
            continue
        c = T.indices[T.indptr[i]:T.indptr[i + 1]]
        c = c[c != i]
        if deps is not None:
            c = c[deps[c]]
        depth[i] = depth[c].max() + 1 if len(c) else 0
    return depth


def _level_rows(depth, take=None):
    d = depth if take is None else depth[take]
    return np.bincount(d) if len(d) else np.zeros(0, dtype=np.int64)


def _launches(level_rows):
    """A wide level is one launch, a run of narrow levels one."""
    count, in_run = 0, False
    for r in level_rows:
        if r >= WIDE:
            count, in_run = count + 1, False
        elif not in_run:
            count, in_run = count + 1, True
    return count


def plan_shape(f, block=None):
    """What stk_lu_info / stk_lu_top_rows report for these factors: levels of both solves,
    the rows of the dense top (empty: none) and the launches per solve, level by level
    (block None) or with the top in diagonal blocks of `block` rows."""
    dL, dU = _depths(f.Ls, True), _depths(f.U, False)
    lvL, lvU = _level_rows(dL), _level_rows(dU)
    d0 = 0
    while d0 < len(lvL) and lvL[d0] >= WIDE:
        d0 += 1
    in_top = dL >= d0
    closed = all(in_top[f.U.indices[f.U.indptr[i]:f.U.indptr[i + 1]]].all() for i in np.flatnonzero(in_top))
    top = np.flatnonzero(in_top) if (len(lvL) - d0 >= TOP_LEVELS and in_top.sum() >= 2 and closed) else np.zeros(0, int)
    shape = dict(levels_L=len(lvL), levels_U=len(lvU), d0=d0, closed=closed, top_rows=top.astype(np.int32),
                 n_top=len(top), widest=(int(lvL.max()), int(lvU.max())))
    if block is None or not len(top):
        shape['launches'] = _launches(lvL) + _launches(lvU)
    else:
        head = ~in_top
        nb = min(block, len(top))
        shape['launches'] = (_launches(_level_rows(dL, head)) + 1 +
                             _launches(_level_rows(_depths(f.U, False, head, head), head)) + 4 * -(-len(top) // nb))
    return shape


# ---- the solve in extended precision and in float64 ---------------------------------------
def _rows(T):
    return [(T.indices[T.indptr[i]:T.indptr[i + 1]], T.data[T.indptr[i]:T.indptr[i + 1]]) for i in range(T.shape[0])]


def _substitute(f, B, dtype):
    """x = Pc U^-1 L^-1 Pr b, row by row; float64 rounds the reciprocal like the device."""
    n = f.n
    c = np.empty(B.shape, dtype=dtype)
    c[np.arange(n) if f.perm_r is None else f.perm_r] = B
    y = np.zeros_like(c)
    for i, (cols, vals) in enumerate(_rows(f.Ls)):
        y[i] = c[i] - vals.astype(dtype) @ y[cols]
    z = np.zeros_like(c)
    rows = _rows(f.U)
    for i in range(n - 1, -1, -1):
        cols, vals = rows[i]
        off = cols != i
        z[i] = (y[i] - vals[off].astype(dtype) @ z[cols[off]]) * (dtype(1) / vals[~off].astype(dtype)[0])
    return z if f.perm_c is None else z[f.perm_c]


def solve_reference(f, B):
    return _substitute(f, B, LD)


def solve_float64(f, B):
    return _substitute(f, np.asarray(B, dtype=np.float64), np.float64)


def _product(T, X):
    """T X in extended precision: dense up to 1000 rows, row by row above."""
    if T.shape[0] <= 1000:
        return T.toarray().astype(LD) @ X
    out = np.zeros(X.shape, dtype=LD)
    for i, (cols, vals) in enumerate(_rows(T)):
        out[i] = vals.astype(LD) @ X[cols]
    return out


def residual_ratio(f, B, X):
    """The largest |c - L U z| in units of its bound; X is (n, k) float64."""
    assert X.shape == B.shape and np.all(np.isfinite(X)), f.name
    n = f.n
    Lu = sp.csr_matrix(f.Ls + sp.eye(n))
    c, z = np.empty(B.shape, dtype=LD), np.empty(B.shape, dtype=LD)
    c[np.arange(n) if f.perm_r is None else f.perm_r] = B
    z[np.arange(n) if f.perm_c is None else f.perm_c] = X
    res = np.abs(c - _product(Lu, _product(f.U, z)))
    g_L, g_U = gamma(f.k_L + 6), gamma(f.k_U + 6)
    bound = (g_L + g_U + g_L * g_U) * _product(abs(Lu), _product(abs(f.U), np.abs(z)))
    assert np.all(bound > 0), f.name  # every row of |L| |U| has its diagonal
    return float(np.max(res / bound))


def forward_error(X, X_ref):
    """The largest error against the extended-precision solution over the largest |x_ref|."""
    return float(np.max(np.abs(X.astype(LD) - X_ref)) / np.max(np.abs(X_ref)))


@functools.lru_cache(maxsize=None)
def host_yardstick(make, *args):
    """(factors, right-hand side, longdouble solution, e_host) of a builder's factors;
    `make` may also return the permuted form (args ending in 'perm')."""
    perm = bool(args) and args[-1] == 'perm'
    f = make(*(args[:-1] if perm else args))
    if perm:
        f = f.permuted(np.random.RandomState(f.n))
    B = f.rhs()
    X_ref = solve_reference(f, B)
    return f, B, X_ref, forward_error(solve_float64(f, B), X_ref)


# ---- the cases, shared with the GPU tests --------------------------------------------------
CHAINS = [(chain, n, explicit) for n in (1, 15, 16, 20) for explicit in (False, True)]
COMBS = [(comb, 64, 20), (comb, 63, 20), (comb, 64, 15), (comb, 64, 20, True)]
ROWS = [(row_lengths, ell) for ell in ROW_LENGTHS]
SUPERLU = [(superlu_random,), (superlu_laplacian,)]


def with_perms(cases):
    return [c + p for c in cases for p in ((), ('perm',))]


def case_id(case):
    return '-'.join([case[0].__name__] + [str(a) for a in case[1:]])


# ---- the checker on the host ---------------------------------------------------------------
@pytest.mark.parametrize('case', with_perms(CHAINS + COMBS + ROWS) + SUPERLU, ids=case_id)
def test_float64_substitution_sits_inside_the_bound(case):
    """The reference alone, through the checker the device is held to: a float64
    substitution on the host solves every case within the backward bound."""
    f, B, X_ref, e_host = host_yardstick(*case)
    ratio = residual_ratio(f, B, solve_float64(f, B))
    print('%s: residual %.3f of the bound, e_host %.2e' % (f.name, ratio, e_host))
    assert ratio <= 1.0, (f.name, ratio)
    assert residual_ratio(f, B, X_ref.astype(np.float64)) <= 1.0  # the rounded exact solution


def test_the_checker_rejects_a_wrong_solve():
    """One entry of L dropped, one right-hand side row taken from its neighbour, a result
    off by a few units in the last place of its largest entry: all outside the bound."""
    f, B, X_ref, _ = host_yardstick(comb, 64, 20, 'perm')
    X = solve_float64(f, B)
    assert residual_ratio(f, B, X) <= 1.0
    L = f.L.copy()
    L.data[L.indptr[70]] = 0.0
    assert residual_ratio(f, B, solve_float64(Factors('dropped', L, f.U, f.perm_r, f.perm_c), B)) > 1e3
    swapped = B.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert residual_ratio(f, B, solve_float64(f, swapped)) > 1e3
    off = X.copy()
    i, t = np.unravel_index(np.argmax(np.abs(off)), off.shape)
    off[i, t] *= 1.0 + 64 * (f.k_L + f.k_U + 12) * U
    assert residual_ratio(f, B, off) > 1.0


def test_plan_shapes_of_the_cases():
    """The launch plans the GPU tests expect, by construction (WIDE = 64 rows decide between
    a launch per level and one workgroup walking a run of levels; a dense top needs 16 levels
    from the first narrow one on, two rows, and a U closed over S)."""
    s = plan_shape(chain(1))
    assert (s['levels_L'], s['levels_U'], s['n_top'], s['launches']) == (1, 1, 0, 2)
    s = plan_shape(chain(15))
    assert (s['levels_L'], s['levels_U'], s['n_top'], s['launches']) == (15, 15, 0, 2)
    for n in (16, 20):
        for explicit in (False, True):
            s = plan_shape(chain(n, explicit), block=7)
            # the top is all rows and the head is empty: one launch for d_S, four per block
            assert (s['levels_L'], s['n_top'], s['d0']) == (n, n, 0)
            assert s['launches'] == 1 + 4 * -(-n // 7)
    s = plan_shape(comb(64, 20), block=20)
    assert (s['d0'], s['n_top'], s['levels_L'], s['launches']) == (1, 20, 21, 1 + 1 + 1 + 4)
    assert np.array_equal(s['top_rows'], np.arange(64, 84))
    s = plan_shape(comb(63, 20), block=83)
    assert (s['d0'], s['n_top'], s['levels_L']) == (0, 83, 21)
    s = plan_shape(comb(64, 15))
    assert (s['d0'], s['n_top'], s['levels_L'], s['closed']) == (1, 0, 16, True)  # 15 levels behind d0
    s = plan_shape(comb(64, 20, True))
    assert (s['d0'], s['n_top'], s['closed']) == (1, 0, False)
    for ell in ROW_LENGTHS:
        f = row_lengths(ell)
        s = plan_shape(f)
        counts = np.diff(f.Ls.indptr)
        assert np.array_equal(counts, np.minimum(np.arange(400), ell))
        assert np.array_equal(np.diff(f.U.indptr) - 1, counts[::-1])
        assert (s['levels_L'], s['n_top']) == ((400, 400) if ell else (1, 0))
    s = plan_shape(grid_cap())
    assert (s['levels_L'], s['levels_U'], s['n_top'], s['launches']) == (2, 2, 0, 4)
    assert s['widest'] == (4100, 4100) and 4100 * 65 > 4096 * 1024 // 16
    f = superlu_random()
    s = plan_shape(f)
    assert not np.array_equal(f.perm_r, f.perm_c) and s['n_top'] == 0 and not s['closed']
    s = plan_shape(superlu_laplacian())
    assert s['closed'] and s['n_top'] > 64 and s['d0'] > 0
