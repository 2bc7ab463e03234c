"""What tests/test_kron_kernels_gpu.py measures the Kronecker-sum kernels (csrc/kron_pack.hip,
csrc/kron_pack_multi.hip, csrc/kron_ell.hip) with, and a check of that yardstick where there
is no GPU.

The operation, restated in np.longdouble on (M, n_loc) slabs (one row per space dof, one
column per local time step):

    y = beta y + sum_k T_k-stencil( Z_k ),      Z_k = X_k x_k  (the space factor, column by column)
    y[i, t] += dia_k[t] Z_k[i, t] + sub_k[t] Z_k[i, t - 1] + sup_k[t] Z_k[i, t + 1]

T_k is given as tri (3, n_loc) = (sub, dia, sup), or None for the identity.  Z_k[:, -1] is the
space factor of the ghost row x_lo (step -1) and Z_k[:, n_loc] that of x_hi (step n_loc), zero
where the slab has no such neighbour: sub[0] and sup[n_loc - 1] multiply the ghost rows and
nothing else.  Every term reads one shared slab, or a slab of its own.

Bound.  U = 2^-53, gamma_k = k U / (1 - k U).  As in test_multigrid_reference_host.py: every
output entry is a sum of products, each of which passes through at most k roundings, so
|fl(op(v)) - op(v)| <= gamma_k |op| |v| entry by entry whatever the order of the sum, |op| the
operation with every coefficient replaced by its magnitude.  k is counted from the kernels'
own arithmetic (kron_pack.hip:272-279 and 310-327, the slot loop; :350-402, the time stencil
and the store; kron_ell.hip:191-225 and 242-282; kron_pack_multi.hip:190-198 and 213-252; the
boundary kernels kron_pack.hip:479-508, 559-599 and kron_ell.hip:403-434 repeat the same sums):

  * one fused multiply-add per slot that holds an entry of the row in term k's matrix; a
    padding slot, the slot of a column only the partner row of a pair has, and an entry that
    is zero in this matrix add fma(0, x, s) = s exactly                                 -> nnz_k(i)
  * a tridiagonal factor: the product dia * z and two fused multiply-adds (sub, sup), the
    product passing through both of them; none for an identity factor                   -> 3 or 0
  * the terms are added one after the other onto 0.0: the first addition is exact, so
    term 0 passes through n_terms - 1 additions and term k > 0 through n_terms - k      -> adds_k
  * fma(beta, y_old, .) for beta != 0: one more rounding of everything, one of beta y   -> b
    k(i, term) = nnz_k(i) + 3 [tri] + adds_k + b
    e = sum_k gamma_k(i, term) (|T_k| kron |X_k|) |x_k| + gamma_b |beta| |y_old|

The explicit-value form adds the terms in another order (kron_pack.hip:46-54): the count of a
term is at most the same.  The longdouble restatement rounds too: REF_ULPS * k * 2^-64 is added
to gamma_k (`g` of the multigrid file).  The count is derived, not measured; the check used
everywhere is |got - ref| <= bound on EVERY entry, and a zero bound admits no error (`ratio`).

Inputs are signed; neighbouring time columns are scaled by different powers of two (factors of
8 to 128 between neighbours, the two ghost rows further out still), so a value from the wrong
column or ghost side is far outside the bound.  So that the bound says something every
catalogue case satisfies, column by column, max(bound) <= 1e-10 max|ref| (PARITY): signed sums
can cancel, and the vectors of a case are drawn again from a fixed sequence of seeds, with the
right restatement alone, until they do not.

The launch rules of the three entry points are restated from the arguments (`pack_launch`,
`terms_launch`, `ell_launch`; the CU count is a parameter) and never asked of the library; the
catalogue `CASES` names the smallest shape that reaches each path, and
test_the_catalogue_sits_where_it_says asserts that it does.  The float64 oracle (oracle/kron.py)
and the stored goldens sit inside the bound; a restatement with one thing wrong (`WRONG`)
leaves it."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import csr_from, load_golden
from test_lu_reference_host import LD, U
from test_multigrid_reference_host import PARITY, bound_is_informative, g
from test_wavelet_reference_host import ratio, unchecked_ratio  # noqa: F401  (re-exported to the GPU tests)

BS = 512                     # threads per workgroup of the three persistent kernels
LDS_CAP = 64 * 1024          # kron_pack.hip:796, 801
PACK_K = {1: (5, 7, 9, 12, 16), 2: (8, 10, 12)}  # instantiated slot counts per rows_per_unit
ELL_K = (5, 7, 9, 12, 16)
ROW_SLOTS = {8: 5, 10: 7, 12: 9}  # a pair of K2 slots serves rows of at most this many entries (stk_pack_unit_slots)
N_LOC_MAX = 1020             # (n_loc + 1) / 2 + 2 <= 512 (kron_pack.hip:895, kron_ell.hip:571)
WRONG = ('t0-for-t0+1', 'sub-super-swapped', 'hi-for-lo', 'ghost-dropped-at-last-step', 'partner-row-values',
         'other-terms-slab', 'beta-dropped', 'padding-for-z[n_loc]')


# ---- launch rules, from the arguments alone -------------------------------------------------------
def _npf(R, K):
    npf = -(-R * K // BS)
    return 1 if npf <= 1 else (2 if npf <= 2 else 4)


def _walk(n_units, R, per_cu, lds, n_cu):
    """(ngroups, chunk, grid, groups walked by the busiest workgroup): kron_pack.hip:797-809,
    178-182 and 212.  Workgroup b serves XCD b & 7 and takes the groups xcd * chunk + (b >> 3),
    + grid / 8, ... below min((xcd + 1) * chunk, ngroups)."""
    ngroups = -(-n_units // R)
    chunk = -(-ngroups // 8)
    by_lds = 160 * 1024 // (lds + 256)
    if per_cu > by_lds:
        per_cu = by_lds if by_lds > 0 else 1
    per_xcd = max(1, min((n_cu // 8) * per_cu, chunk))
    walk = -(-min(chunk, ngroups) // per_xcd)
    return ngroups, chunk, per_xcd * 8, walk


def pack_launch(K, rp, nt, n_units, n_loc, ghost, any_tri, n_codes, explicit=False, multi=False, n_cu=256):
    """stk_kron_pack_apply (kron_pack.hip:784-809, 739, 862): the main kernel."""
    assert K in PACK_K[rp] and (n_loc + 1) // 2 + 2 <= BS
    P = (n_loc + 1) // 2
    W = P + (1 if ghost else 0)
    R = BS // W
    if R * K > 4 * BS:
        R = 4 * BS // K
    if explicit and R * K * rp * nt > 2 * BS:
        R = 2 * BS // (K * rp * nt)
    KS = (K + 3) & ~3

    def lds_of(R):
        values = R * K * rp * nt if explicit else n_codes * rp * nt
        return 8 * ((nt * R * rp * (n_loc + 3) if any_tri else 0) + values + nt * 3 * (n_loc + 2)) + \
            4 * (R * KS + R * rp + 4) + 32
    R0 = R
    while R > 1 and lds_of(R) > LDS_CAP:
        R -= 1
    lds = lds_of(R)
    ngroups, chunk, grid, walk = _walk(n_units, R, 2 if (K >= 12 or rp > 1) else 3, lds, n_cu)
    return dict(kernel='kron_pack_kernel', K=K, RP=rp, NT=nt, P=P, W=W, R=R, lds_cut=R < R0, NPF=_npf(R, K),
                GHOST=bool(ghost), DICT=not explicit, MULTI=bool(multi), any_tri=bool(any_tri), lds=lds,
                refused=lds > LDS_CAP, ngroups=ngroups, chunk=chunk, grid=grid, walk=walk, idle=BS - R * W,
                tail=n_units % R)


def terms_lanes(n_loc, nt, steps):
    """Lanes per slot row of the lane-group kernel (kron_pack_multi.hip:345-361): term 0 covers
    every pair of time steps, term k > 0 the pairs of its stated steps [b, e)."""
    P = (n_loc + 1) // 2
    lanes = []
    for k in range(nt):
        p0, p1 = 0, P
        if k > 0 and steps is not None and steps[k] is not None:
            b, e = max(steps[k][0], 0), min(steps[k][1], n_loc)
            p0 = b // 2
            p1 = (e + 1) // 2 if e > b else p0
        lanes.append(p1 - p0)
    return lanes


def terms_launch(K, rp, nt, n_units, n_loc, n_codes, steps=None, n_cu=256):
    """stk_kron_pack_apply_multi_steps with a lane group per term (kron_pack_multi.hip:282-304,
    366); None where a slot row needs more than 256 lanes (the turn form runs instead)."""
    W = sum(terms_lanes(n_loc, nt, steps))
    if BS // W < 2:
        return None
    R = BS // W
    if R * K > 4 * BS:
        R = 4 * BS // K
    KS = (K + 3) & ~3
    lds_of = lambda R: 8 * (nt * R * rp * (n_loc + 3) + n_codes * rp * nt + nt * 3 * (n_loc + 2)) + \
        4 * (R * KS + R * rp + 4) + 32
    R0 = R
    while R > 1 and lds_of(R) > LDS_CAP:
        R -= 1
    lds = lds_of(R)
    ngroups, chunk, grid, walk = _walk(n_units, R, 2, lds, n_cu)
    return dict(kernel='kron_pack_terms_kernel', K=K, RP=rp, NT=nt, P=(n_loc + 1) // 2, W=W, R=R, lds_cut=R < R0,
                NPF=_npf(R, K), lds=lds, refused=lds > LDS_CAP, ngroups=ngroups, chunk=chunk, grid=grid, walk=walk,
                idle=BS - R * W, tail=n_units % R)


def ell_launch(K, nt, M, n_loc, ld, any_tri, overflow=False, shared=True, wg_per_cu=0, force_wide=0, n_cu=256):
    """stk_kron_ell_apply (kron_ell.hip:317-337, 308-310, 519)."""
    assert K in ELL_K and (n_loc + 1) // 2 + 2 <= BS
    P = (n_loc + 1) // 2
    R = BS // P
    if R * K > 4 * BS:
        R = 4 * BS // K
    wide = bool(force_wide) or M * ld * 8 >= 1 << 32
    KS = (K + 3) & ~3
    lds = 8 * ((nt * R * (n_loc + 3) if any_tri else 0) + nt * R * KS) + 4 * (R * KS + R + 4) + \
        8 * nt * 3 * (n_loc + 2) + 32
    per_cu = wg_per_cu if wg_per_cu > 0 else (2 if K >= 12 else 3)
    ngroups, chunk, grid, walk = _walk(M, R, per_cu, lds, n_cu)
    return dict(kernel='kron_ell_kernel', K=K, NT=nt, P=P, W=P, R=R, NPF=_npf(R, K), SHARED_IN=bool(shared),
                GENERIC=bool(overflow) or wide, WIDE=wide, any_tri=bool(any_tri), lds=lds, ngroups=ngroups,
                chunk=chunk, grid=grid, walk=walk, idle=BS - R * P, tail=M % R)


def path_name(L):
    if L['kernel'] == 'kron_ell_kernel':
        head = 'kron_ell_kernel<NT=%d, %s, K=%d, NPF=%d%s%s>' % (
            L['NT'], 'shared x' if L['SHARED_IN'] else 'x per term', L['K'], L['NPF'],
            ', GENERIC' if L['GENERIC'] else '', ', WIDE' if L['WIDE'] else '')
    elif L['kernel'] == 'kron_pack_terms_kernel':
        head = 'kron_pack_terms_kernel<NT=%d, K=%d, NPF=%d, RP=%d>' % (L['NT'], L['K'], L['NPF'], L['RP'])
    else:
        head = 'kron_pack_kernel<NT=%d, K=%d, NPF=%d, %s, RP=%d, %s%s>' % (
            L['NT'], L['K'], L['NPF'], 'GHOST' if L['GHOST'] else 'no ghost', L['RP'],
            'DICT' if L['DICT'] else 'explicit', ', MULTI' if L['MULTI'] else '')
    return '%s W=%d R=%d%s groups=%d grid=%d walk=%d' % (head, L['W'], L['R'], ' (LDS cut)' if L.get('lds_cut') else '',
                                                         L['ngroups'], L['grid'], L['walk'])


# ---- matrices -------------------------------------------------------------------------------------
SINGLE_EVERY = 5  # in a synthetic pair pattern, unit u serves one row alone when u % 5 == 2


def pair_units(M):
    """How the slot rows (units) follow from M matrix rows.  One row per slot row: M units.  Row
    pairs, synthetic patterns: the rows are taken two at a time in processing order, except that
    every fifth unit (u % 5 == 2) takes one row alone (row_ids = -1 in the middle of the stream)
    and so does the last unit where one row is left (an odd remainder: -1 at its end)."""
    u = left = 0
    left = M
    while left > 0:
        left -= 1 if (u % SINGLE_EVERY == 2 or left == 1) else 2
        u += 1
    return u


class Space:
    """n_mats matrices on one union pattern, in matrix-row order: cols[M, width] (a row's entries
    first, ascending; then padding at the row's own column), vals[n_mats, M, width] (zero in the
    padding), cnt[M] entries per row; own[pos] = the row processed at position pos; units[u] =
    (row, partner or -1) in processing order where the pattern was made for pairs."""
    def __init__(self, cols, vals, cnt, own, units=None):
        self.cols, self.vals, self.cnt, self.own, self.units = cols, vals, cnt, own, units
        self.M, self.width = cols.shape
        self.n_mats = len(vals)
        self.partner = np.arange(self.M)
        if units is not None:
            for a, b in units:
                if b >= 0:
                    self.partner[a], self.partner[b] = b, a

    def nnz(self, m):
        return (self.vals[m] != 0.0).sum(axis=1)

    def csr(self, m):
        rows = np.repeat(np.arange(self.M), self.width)
        keep = self.vals[m].reshape(-1) != 0.0
        return sp.csr_matrix((self.vals[m].reshape(-1)[keep], (rows[keep], self.cols.reshape(-1)[keep])),
                             shape=(self.M, self.M))


def _palette(rng, n_mats):
    size = 3 if n_mats <= 2 else 2  # (keeps the dictionary of a pair of three matrices small)
    return [rng.uniform(0.25, 1.0, size) * rng.choice([-1.0, 1.0], size) for _ in range(n_mats)]


@functools.lru_cache(maxsize=None)
def synthetic(K1, M, n_mats, seed, extra=0):
    """Signed matrices with rows of 1..K1 entries (+ `extra` more in every seventh row: overflow
    rows of the plain form), values from a small palette (a dictionary exists), an entry now and
    then zero in one matrix only.  For K1 in 5, 7, 9 the rows come in units whose union of columns
    fits the pair kernel's slots (`pair_units`)."""
    rng = np.random.RandomState(1000 * K1 + 7 * M + seed)
    K2 = {v: k for k, v in ROW_SLOTS.items()}.get(K1)
    own = rng.permutation(M).astype(np.int32)
    width = K1 + extra
    cols = np.repeat(np.arange(M)[:, None], width, axis=1)
    cnt = np.zeros(M, dtype=np.int64)
    held = [None] * M
    units = None
    window = lambda pos, n: np.sort(rng.choice(M, size=min(n, M), replace=False)) if M <= 4 * n else \
        np.sort((max(0, min(pos - 2 * n, M - 4 * n)) + rng.choice(4 * n, size=n, replace=False)))
    if K2 is not None and not extra:
        units, pos, u = [], 0, 0
        while pos < M:
            if u % SINGLE_EVERY == 2 or pos == M - 1:
                a = int(own[pos])
                held[a] = window(pos, K1 if u == 2 else int(rng.randint(1, K1 + 1)))
                units.append((a, -1))
                pos += 1
            else:
                a, b = int(own[pos]), int(own[pos + 1])
                union = window(pos, int(rng.randint(K1, K2 + 1)) if u else K2)
                n = len(union)
                na = int(rng.randint(max(1, n - K1), min(K1, n) + 1)) if u else min(K1, n)
                in_a = np.zeros(n, dtype=bool)
                in_a[rng.choice(n, size=na, replace=False)] = True
                in_b = ~in_a
                spare = np.flatnonzero(in_a)
                more = min(len(spare), min(K1, n) - int(in_b.sum()))
                if more > 0:  # columns the two rows share
                    in_b[rng.choice(spare, size=int(rng.randint(0, more + 1)), replace=False)] = True
                if not in_b.any():
                    in_b[0] = True
                held[a], held[b] = union[in_a], union[in_b]
                units.append((a, b))
                pos += 2
            u += 1
        assert len(units) == pair_units(M)
    else:
        for pos in range(M):
            n = K1 if pos == 0 else int(rng.randint(1, K1 + 1))
            if extra and pos % 7 == 3:
                n = K1 + int(rng.randint(1, extra + 1))
            held[int(own[pos])] = window(pos, n)
    for i in range(M):
        cnt[i] = len(held[i])
        cols[i, :cnt[i]] = held[i]
    pal = _palette(rng, n_mats)
    mask = np.arange(width)[None, :] < cnt[:, None]
    vals = []
    for m in range(n_mats):
        v = np.where(mask, pal[m][rng.randint(len(pal[m]), size=(M, width))], 0.0)
        if m == 1:
            v = np.where(rng.rand(M, width) < 0.1, 0.0, v)
        vals.append(v)
    return Space(cols, vals, cnt, own, units)


def space_from_csr(mats, own=None):
    """The union pattern of SciPy matrices as a Space (the wrappers' own layout is built by them)."""
    mats = [sp.csr_matrix(m).copy() for m in mats]
    for m in mats:
        m.sum_duplicates()
        m.sort_indices()
    pattern = sp.csr_matrix(sum(abs(m) for m in mats) + sum(sp.csr_matrix((np.ones(m.nnz), m.indices, m.indptr),
                                                                             shape=m.shape) for m in mats))
    pattern.sort_indices()
    M = pattern.shape[0]
    cnt = np.diff(pattern.indptr).astype(np.int64)
    width = int(cnt.max())
    cols = np.repeat(np.arange(M)[:, None], width, axis=1)
    slot = np.arange(pattern.nnz) - np.repeat(pattern.indptr[:-1], cnt)
    rows = np.repeat(np.arange(M), cnt)
    cols[rows, slot] = pattern.indices
    vals = []
    for m in mats:
        v = np.zeros((M, width))
        v[rows, slot] = np.asarray(m[rows, pattern.indices]).reshape(-1)
        vals.append(v)
    return Space(cols, vals, cnt, np.arange(M, dtype=np.int32) if own is None else own)


# ---- the layouts the entry points stream (host arrays; the GPU tests upload them) -----------------
def ell_layout(space, K):
    """stk_ell_pattern: rows in processing order, entries beyond K in an overflow CSR by position."""
    own, M = space.own, space.M
    idx = np.repeat(own[:, None], K, axis=1).astype(np.int32)
    vals = [np.zeros((M, K)) for _ in range(space.n_mats)]
    n = min(K, space.width)
    idx[:, :n] = space.cols[own, :n]
    pad = np.arange(n)[None, :] >= space.cnt[own][:, None]
    idx[:, :n][pad] = np.repeat(own[:, None], n, axis=1)[pad]
    for m in range(space.n_mats):
        vals[m][:, :n] = space.vals[m][own, :n]
    out = dict(K=K, M=M, idx=idx, vals=vals, row_ids=own.astype(np.int32), ovf=None)
    over = np.maximum(space.cnt[own] - K, 0)
    if over.any():
        indptr = np.concatenate([[0], np.cumsum(over)]).astype(np.int32)
        sel = [(own[p], s) for p in range(M) for s in range(K, int(space.cnt[own[p]]))]
        r, s = np.array(sel).T
        out['ovf'] = dict(indptr=indptr, indices=space.cols[r, s].astype(np.int32),
                          vals=[space.vals[m][r, s].copy() for m in range(space.n_mats)])
    return out


def unit_layout(space, rp, K):
    """(ucols[U, K], uvals[n_mats, U, K, rp], urows[U, rp]): the union of a unit's columns in
    ascending order, a row's value where it has the column and +0.0 where not."""
    if rp == 1:
        assert space.width <= K
        own = space.own
        U_ = space.M
        ucols = np.repeat(own[:, None].astype(np.int64), K, axis=1)
        ucols[:, :space.width] = space.cols[own]
        uvals = np.zeros((space.n_mats, U_, K, 1))
        for m in range(space.n_mats):
            uvals[m, :, :space.width, 0] = space.vals[m][own]
        return ucols, uvals, own.astype(np.int32)[:, None].copy()
    assert space.units is not None and ROW_SLOTS[K] >= space.width
    U_ = len(space.units)
    ucols = np.zeros((U_, K), dtype=np.int64)
    uvals = np.zeros((space.n_mats, U_, K, 2))
    urows = np.full((U_, 2), -1, dtype=np.int32)
    for u, (a, b) in enumerate(space.units):
        rows = [a] + ([b] if b >= 0 else [])
        union = np.unique(np.concatenate([space.cols[r, :space.cnt[r]] for r in rows]))
        assert len(union) <= K
        ucols[u] = a
        ucols[u, :len(union)] = union
        for j, r in enumerate(rows):
            urows[u, j] = r
            at = np.searchsorted(union, space.cols[r, :space.cnt[r]])
            for m in range(space.n_mats):
                uvals[m, u, at, j] = space.vals[m][r, :space.cnt[r]]
    return ucols, uvals, urows


def dict_layout(space, rp, K, n_codes_min=0):
    """stk_pack_pattern with a dictionary: slot word = code << col_bits | column.  n_codes_min pads
    the dictionary with value tuples no slot names (they only take room in LDS)."""
    ucols, uvals, urows = unit_layout(space, rp, K)
    U_, nm = ucols.shape[0], space.n_mats
    tuples = np.ascontiguousarray(uvals.transpose(1, 2, 3, 0).reshape(U_ * K, rp * nm))  # [slot][row j][matrix]
    uniq, code = np.unique(tuples.view(np.int64), axis=0, return_inverse=True)
    uniq = uniq.view(np.float64)
    if len(uniq) < n_codes_min:
        uniq = np.vstack([uniq, 0.5 + np.arange((n_codes_min - len(uniq)) * rp * nm).reshape(-1, rp * nm)])
    col_bits = max(1, int(space.M - 1).bit_length())
    assert len(uniq) <= 1 << (32 - col_bits)
    slots = (code.reshape(-1).astype(np.uint32) << np.uint32(col_bits)) | ucols.reshape(-1).astype(np.uint32)
    table = np.ascontiguousarray(uniq.reshape(len(uniq), rp, nm).transpose(2, 0, 1))  # dict[m][code][j]
    return dict(K=K, M=space.M, rp=rp, n_units=U_, col_bits=col_bits, n_codes=len(uniq), n_mats=nm,
                slots=slots.reshape(U_, K), row_ids=urows, dict=table, vals=None)


def explicit_layout(space, K, mats):
    """stk_pack_pattern with explicit values of the call's matrices, in term order (pairs only)."""
    ucols, uvals, urows = unit_layout(space, 2, K)
    vals = np.ascontiguousarray(uvals[list(mats)].transpose(1, 2, 3, 0))  # [unit][slot][row j][term]
    return dict(K=K, M=space.M, rp=2, n_units=ucols.shape[0], col_bits=max(1, int(space.M - 1).bit_length()),
                n_codes=1, n_mats=len(mats), slots=ucols.astype(np.uint32), row_ids=urows, dict=None, vals=vals)


# ---- inputs ---------------------------------------------------------------------------------------
def column_scales(n_loc):
    """2^(5 t mod 8 - 4): neighbours differ by a factor of 8 or 32."""
    return 2.0**((5 * np.arange(n_loc)) % 8 - 4)


LO_SCALE, HI_SCALE, PAD_SCALE = 2.0**9, 2.0**-9, 2.0**6


def signed(rng, *shape):
    return rng.uniform(0.25, 1.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)


def time_factor(kind, n_loc, rng):
    """tri (3, n_loc) of a kind: 'full' signed entries everywhere (sub[0] and sup[n_loc - 1]
    included: they multiply the ghost rows or nothing), 'zeros' the same with entries struck out,
    'gt' the single entry (0, 0), 'last' the single entry (n_loc - 1, n_loc - 1); None: identity."""
    if kind == 'id':
        return None
    t = signed(rng, 3, n_loc) * 1.5
    if kind == 'zeros':
        t[rng.rand(3, n_loc) < 0.35] = 0.0
        t[1, n_loc // 2] = 0.0
    elif kind in ('gt', 'last'):
        keep = t[1, 0 if kind == 'gt' else n_loc - 1]
        t[:] = 0.0
        t[1, 0 if kind == 'gt' else n_loc - 1] = keep
    return t


class Case:
    """One call.  form: 'dict' (rp 1 or 2), 'explicit' (rp 2), 'ell'; multi: None, or 'lanes' /
    'turns' / 'steps' (inputs per term through stk_kron_pack_apply_multi[_steps]); K: the slot
    count of the form (K2 for pairs); tris: the kind of every term's time factor; lo / hi: ghost
    rows; extra: columns of ld behind the pair; codes: pads the dictionary; tune: tuning keys."""
    def __init__(self, name, form, K, M, n_loc, tris, rp=1, lo=False, hi=False, beta=0.0, extra=0, multi=None,
                 per_term=False, codes=0, tune=None, overflow=0, seed=0, tags=()):
        self.name, self.form, self.K, self.M, self.n_loc, self.tris, self.rp = name, form, K, M, n_loc, tuple(tris), rp
        self.lo, self.hi, self.beta, self.extra, self.multi = lo, hi, beta, extra, multi
        self.per_term = per_term or multi is not None
        self.codes, self.tune, self.overflow, self.seed, self.tags = codes, dict(tune or {}), overflow, seed, set(tags)
        self.nt = len(self.tris)
        self.ld = ((n_loc + 1) & ~1) + extra
        self.K1 = ROW_SLOTS[K] if rp == 2 else K
        assert not (self.multi and (lo or hi)) and (form != 'explicit' or rp == 2)

    def __repr__(self):
        return self.name

    @property
    def space(self):
        return synthetic(self.K1, self.M, self.nt, self.seed, self.overflow)

    @property
    def any_tri(self):
        return any(k != 'id' for k in self.tris)

    @property
    def n_units(self):
        return pair_units(self.M) if self.rp == 2 else self.M

    def steps(self):
        """The stated steps of the 'steps' form: what each factor reads (time_factor_steps)."""
        out = []
        for kind in self.tris:
            out.append({'gt': (0, 1), 'last': (self.n_loc - 1, self.n_loc)}.get(kind))
        return out

    def layout(self):
        """The arrays the entry point streams (built once per pattern)."""
        return _layout(self.form, self.K1, self.M, self.nt, self.seed, self.overflow, self.rp, self.K, self.codes)

    def n_codes(self):
        return self.layout()['n_codes'] if self.form == 'dict' else 1

    def launch(self, n_cu=256, n_codes=None):
        n_codes = self.n_codes() if n_codes is None else n_codes
        if self.form == 'ell':
            return ell_launch(self.K, self.nt, self.M, self.n_loc, self.ld, self.any_tri, bool(self.overflow),
                              not self.per_term, self.tune.get('ell_wg_per_cu', 0), self.tune.get('ell_force_wide', 0),
                              n_cu)
        if self.multi in ('lanes', 'steps'):
            L = terms_launch(self.K, self.rp, self.nt, self.n_units, self.n_loc, n_codes,
                             self.steps() if self.multi == 'steps' else None, n_cu)
            if L is not None:
                return L
        return pack_launch(self.K, self.rp, self.nt, self.n_units, self.n_loc, self.lo or self.hi, self.any_tri,
                           n_codes, self.form == 'explicit', self.multi is not None, n_cu)


@functools.lru_cache(maxsize=None)
def _layout(form, K1, M, nt, seed, overflow, rp, K, codes):
    space = synthetic(K1, M, nt, seed, overflow)
    if form == 'ell':
        return ell_layout(space, K)
    if form == 'explicit':
        return explicit_layout(space, K, tuple(range(nt)))
    return dict_layout(space, rp, K, codes)


class Data:
    pass


def draw(c, space, redraw):
    rng = np.random.RandomState(c.seed + 31 * c.n_loc + 1000 * redraw + 17 * c.nt)
    d = Data()
    M, n = space.M, c.n_loc
    d.tri = [time_factor(kind, n, rng) for kind in c.tris]
    n_in = c.nt if c.per_term else 1
    d.X = [signed(rng, M, n) * column_scales(n) * 2.0**(3 * s) for s in range(n_in)]
    d.lo = [signed(rng, M) * LO_SCALE if c.lo else None for _ in range(n_in)]
    d.hi = [signed(rng, M) * HI_SCALE if c.hi else None for _ in range(n_in)]
    d.Y0 = signed(rng, M, n) * column_scales(n)[::-1]
    d.pad = signed(rng, M) * PAD_SCALE  # what a wrong restatement finds in the padding column
    return d


def space_factor(space, m, rows, Xe):
    """(Z, |X_m| |x|, nnz) of the given rows: the row's entries against every column of Xe."""
    cols, vals = space.cols[rows], space.vals[m][rows].astype(LD)
    Z = np.zeros((len(rows), Xe.shape[1]), dtype=LD)
    A = np.zeros_like(Z)
    aXe = np.abs(Xe)
    for u in range(space.width):
        v = vals[:, u, None]
        Z += v * Xe[cols[:, u]]
        A += np.abs(v) * aXe[cols[:, u]]
    return Z, A, (space.vals[m][rows] != 0.0).sum(axis=1)


def reference(c, space, d, wrong=None, rows=None, mats=None):
    """(y, bound) of the given output rows (all of them by default), np.longdouble.  `wrong`: one
    thing restated wrongly; the bound is that of the right restatement (None with `wrong`)."""
    n, nt = c.n_loc, c.nt
    rows = np.arange(space.M) if rows is None else np.asarray(rows)
    mats = list(range(nt)) if mats is None else mats
    src = space.partner[rows] if wrong == 'partner-row-values' else rows
    beta = 0.0 if wrong == 'beta-dropped' else c.beta
    b = 1 if c.beta != 0.0 else 0
    y = LD(beta) * d.Y0[rows].astype(LD)
    e = g(b) * np.abs(LD(c.beta) * d.Y0[rows].astype(LD))
    for k in range(nt):
        s = k if c.per_term else 0
        if wrong == 'other-terms-slab':
            s = (k + 1) % nt
        Xe = np.zeros((space.M, n + 2), dtype=LD)
        Xe[:, 1:n + 1] = d.X[s]
        if d.lo[s] is not None:
            Xe[:, 0] = d.lo[s]
        if d.hi[s] is not None:
            Xe[:, n + 1] = d.hi[s]
        if wrong == 't0-for-t0+1':  # the lane's second step reads its first column
            Xe[:, 2:n + 1:2] = Xe[:, 1:n:2].copy()
        elif wrong == 'hi-for-lo':
            Xe[:, 0] = Xe[:, n + 1]
        elif wrong == 'ghost-dropped-at-last-step':
            Xe[:, n + 1] = 0
        elif wrong == 'padding-for-z[n_loc]':
            Xe[:, n + 1] = d.pad
        Z, A, nnz = space_factor(space, mats[k], src, Xe)
        adds = nt - 1 if k == 0 else nt - k
        tri = d.tri[k]
        if tri is None:
            v, a, kk = Z[:, 1:n + 1], A[:, 1:n + 1], nnz + adds + b
        else:
            sub, dia, sup = (tri[i].astype(LD) for i in ((2, 1, 0) if wrong == 'sub-super-swapped' else (0, 1, 2)))
            v = dia * Z[:, 1:n + 1] + sub * Z[:, 0:n] + sup * Z[:, 2:n + 2]
            a = np.abs(dia) * A[:, 1:n + 1] + np.abs(sub) * A[:, 0:n] + np.abs(sup) * A[:, 2:n + 2]
            kk = nnz + 3 + adds + b
        y = y + v
        e = e + g(kk)[:, None] * a
    return y, (None if wrong else e)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(space, data, y_ref, bound) of a catalogue case: computed once, shared, left unchanged."""
    c = CASES[name]
    space = c.space
    for redraw in range(16):
        d = draw(c, space, redraw)
        y, e = reference(c, space, d)
        if bound_is_informative(y, e):
            return space, d, y, e
    raise AssertionError(name)


def applies(wrong, c, d, space):
    """Does the mistake change the operation of this case at all?"""
    tri = [t for t in d.tri if t is not None]
    n = c.n_loc
    if wrong == 't0-for-t0+1':
        return n >= 2 and any(t is None or t[1, 1::2].any() or t[0, 2::2].any() or t[2, 0:n - 1:2].any() for t in d.tri)
    if wrong == 'sub-super-swapped':  # a step with a neighbour on either side and sub != sup
        return any(t[0, s] != t[2, s] and (s > 0 or c.lo or s < n - 1 or c.hi) for t in tri for s in range(n))
    if wrong == 'hi-for-lo':
        return c.lo and any(t[0, 0] != 0.0 for t in tri)
    if wrong == 'ghost-dropped-at-last-step':
        return c.hi and any(t[2, n - 1] != 0.0 for t in tri)
    if wrong == 'partner-row-values':
        return c.rp == 2 and bool(np.any(space.partner[:96] != np.arange(space.M)[:96]))
    if wrong == 'other-terms-slab':
        return c.per_term
    if wrong == 'beta-dropped':
        return c.beta != 0.0
    if wrong == 'padding-for-z[n_loc]':
        return n % 2 == 1 and any(t[2, n - 1] != 0.0 for t in tri)
    raise KeyError(wrong)


# ---- the catalogue --------------------------------------------------------------------------------
def n_locs_for(launch_of):
    """1, 2, 3, 4, 9 plus the shortest slabs that reach an NPF instance those do not (every
    instance some n_loc reaches is reached): the idiom of the multigrid file."""
    out = [1, 2, 3, 4, 9]
    seen = {launch_of(n)['NPF'] for n in out}
    for n in range(1, N_LOC_MAX + 1):
        L = launch_of(n)
        if not L.get('refused') and L['NPF'] not in seen:
            out.append(n)
            seen.add(L['NPF'])
    return out


def rows_for_walk(make, walk=3, n_cu=256):
    """The fewest matrix rows (in steps of 64) with which the busiest workgroup of `make(M)` walks
    `walk` groups on n_cu CUs."""
    M = 64  # (a dictionary of one code: the least LDS, the most workgroups, the most rows)
    while make(M).launch(n_cu, n_codes=1)['walk'] < walk:
        M += 64
    return M


def rows_for_units(units, rp):
    """The fewest matrix rows that make this many slot rows."""
    return units if rp == 1 else next(m for m in range(units, 2 * units + 1) if pair_units(m) == units)


TRI_ROUND = (('full', 'full', 'zeros'), ('zeros', 'id', 'full'), ('full', 'gt', 'id'), ('id', 'full', 'full'))
GHOST_ROUND = ((False, False), (True, False), (False, True), (True, True))
BETA_ROUND = (0.0, 1.0, -0.5)


def _build_catalogue():
    cases, count = {}, [0]

    def add(name, form, K, M, n_loc, nt=None, **kw):
        i = count[0]
        count[0] += 1
        rp = kw.get('rp', 1)
        tris = kw.pop('tris', None)
        if tris is None:
            nt = nt or 1 + i % 3
            tris = TRI_ROUND[i % 4][:nt] if nt < 3 else TRI_ROUND[i % 4]
        if 'lo' not in kw and form != 'ell-multi' and not kw.get('multi'):
            kw['lo'], kw['hi'] = GHOST_ROUND[(i // 3) % 4]
        kw.setdefault('beta', BETA_ROUND[(i // 2) % 3])
        kw.setdefault('extra', (0, 2)[(i // 5) % 2])
        if n_loc + kw['extra'] > N_LOC_MAX:
            kw['extra'] = 0
        kw.setdefault('seed', i)
        assert name not in cases, name
        cases[name] = Case(name, form, K, M, n_loc, tris, **kw)
        return cases[name]

    forms = [('dict', 1, K) for K in PACK_K[1]] + [('dict', 2, K) for K in PACK_K[2]] + \
        [('explicit', 2, K) for K in PACK_K[2]] + [('ell', 1, K) for K in ELL_K]
    # a. every instance: form x K x the slab lengths that reach its NPF instances, two groups and a row
    for form, rp, K in forms:
        for nt in (1, 2, 3):
            def launch_of(n, form=form, rp=rp, K=K, nt=nt):
                if form == 'ell':
                    return ell_launch(K, nt, 64, n, (n + 1) & ~1, True)
                return pack_launch(K, rp, nt, 64, n, False, True, 16, form == 'explicit')
            for n_loc in n_locs_for(launch_of) if nt == 2 else (1, 9):
                R = launch_of(n_loc)['R']
                units = 2 * R + 1
                kw = dict(lo=False, hi=False) if nt == 2 else {}  # (nt = 2: the shape the probe stated)
                add('%s%d-K%d-nt%d-n%d' % (form, rp, K, nt, n_loc), form, K, rows_for_units(units, rp), n_loc, nt=nt,
                    rp=rp, tags={'instance'}, **kw)
    # b. lane geometry
    for form, rp, K in (('dict', 1, 7), ('dict', 2, 10), ('ell', 1, 7)):
        for n_loc in (127, 128, 129):  # P = 64 | 64 | 65: with a ghost lane W = 65 and a row crosses a wavefront
            add('%s%d-wave-n%d' % (form, rp, n_loc), form, K, 41, n_loc, nt=2, rp=rp, lo=True, hi=n_loc != 128,
                tris=('full', 'zeros'), tags={'wavefront'})
        add('%s%d-R1-n513' % (form, rp), form, K, 19, 513, nt=1, rp=rp, tris=('full',), lo=False, hi=True, tags={'R1'})
        add('%s%d-longest' % (form, rp), form, K, 11, N_LOC_MAX, nt=1, rp=rp, tris=('full',), lo=True, hi=True,
            tags={'longest'})
    add('dict2-lds-cut', 'dict', 10, 700, 2, rp=2, tris=('full', 'zeros', 'full'), codes=400, lo=True, hi=True,
        tags={'lds-cut'})
    add('dict2-lds-cut-n1', 'dict', 8, 700, 1, rp=2, tris=('full', 'full', 'id'), codes=300, lo=False, hi=False,
        tags={'lds-cut'})
    # c. the group walk: ngroups 1, 7, 8, 9, 17 with the last group full, one row, or one row short
    for form, rp, K, multi in (('dict', 1, 7, None), ('dict', 2, 10, None), ('ell', 1, 5, None), ('dict', 1, 7, 'lanes'),
                               ('explicit', 2, 8, None)):
        probe = Case('probe', form, K, 64, 9, ('full', 'id'), rp=rp, multi=multi)
        R = probe.launch()['R']
        for ngroups in (1, 7, 8, 9, 17):
            for tail in (0, 1, R - 1):
                units = ngroups * R if tail == 0 else (ngroups - 1) * R + tail
                if units < 1:
                    continue
                add('%s%d%s-g%d-tail%d' % (form, rp, '-' + multi if multi else '', ngroups, tail), form, K,
                    rows_for_units(units, rp), 9, rp=rp, multi=multi, tris=('full', 'id'), lo=False, hi=False,
                    tags={'groups'})
    # d. three or more groups per workgroup, each persistent kernel, with and without ghost lanes, rows and pairs
    long_walks = (('dict', 1, 7, None, False, 341), ('dict', 1, 7, None, True, 339), ('dict', 2, 10, None, False, 341),
                  ('dict', 2, 10, None, True, 255), ('explicit', 2, 10, None, True, 341), ('dict', 1, 7, 'turns', False, 255),
                  ('dict', 1, 7, 'lanes', False, 255), ('dict', 2, 10, 'lanes', False, 255), ('ell', 1, 7, None, False, 341),
                  ('ell', 1, 7, None, True, 255))
    for form, rp, K, multi, ghost, n_loc in long_walks:
        tune = dict(ell_wg_per_cu=1) if form == 'ell' else {}
        kw = dict(rp=rp, multi=multi, tris=('full', 'zeros'), lo=ghost, hi=ghost, beta=0.0, extra=0, tune=tune)
        M = rows_for_walk(lambda M: Case('probe', form, K, M, n_loc, **kw))
        add('%s%d%s%s-walk' % (form, rp, '-' + multi if multi else '', '-ghost' if ghost else ''), form, K, M + 1,
            n_loc, tags={'walk'}, **kw)
    # e. ghosts: none / lo / hi / both at short slabs, an odd and an even longer one; identity terms with ghosts
    for form, rp, K in (('dict', 1, 5), ('dict', 2, 8), ('explicit', 2, 12), ('ell', 1, 9)):
        for n_loc in (1, 2, 3, 24, 25):
            for lo, hi in GHOST_ROUND:
                add('%s%d-ghost-n%d-%d%d' % (form, rp, n_loc, lo, hi), form, K, 70, n_loc, nt=2, rp=rp, lo=lo, hi=hi,
                    tris=('full', 'zeros'), tags={'ghost'})
        add('%s%d-identity-ghost' % (form, rp), form, K, 70, 9, rp=rp, lo=True, hi=True, tris=('id', 'id'),
            tags={'identity-ghost'})
    # f. inputs per term: lane groups, turns, stated steps ending on the first pair or the last pair of an odd slab
    for rp, K in ((1, 9), (2, 8)):
        for n_loc in (1, 2, 9, 24, 33):
            for multi in ('lanes', 'turns', 'steps'):
                tris = {1: ('id', 'gt'), 24: ('id', 'zeros', 'gt')}.get(n_loc, ('full', 'last', 'gt'))
                add('dict%d-%s-n%d' % (rp, multi, n_loc), 'dict', K, 150, n_loc, rp=rp, multi=multi, tris=tris,
                    tags={multi})
        add('dict%d-lanes-fallback-n400' % rp, 'dict', K, 9, 400, rp=rp, multi='lanes', tris=('id', 'full'),
            tags={'lanes-fallback'})
    for n_loc in (3, 24):
        add('ell-per-term-n%d' % n_loc, 'ell', 7, 90, n_loc, per_term=True, tris=('full', 'id', 'zeros'), lo=True,
            hi=True, tags={'ell-per-term'})
    # g. the plain form's other instances: overflow rows, 64-bit addressing
    for K in ELL_K:
        add('ell-overflow-K%d' % K, 'ell', K, 100, 9, nt=2, overflow=3, tags={'GENERIC'})
        add('ell-wide-K%d' % K, 'ell', K, 100, 10, nt=2, tune=dict(ell_force_wide=1), tags={'WIDE'})
    return cases


CASES = _build_catalogue()
MESH_FAMILIES = (('square', 2), ('square', 4), ('lshape', 3), ('cube', 2))  # P1 matrices, through the wrappers


def mesh_matrices(problem, J):
    from source.assembly import space_matrices
    from source.problem import problem_helper
    M_x, A_x = space_matrices(problem_helper(problem, J_space=J, J_time=2)[0])
    return [sp.csr_matrix(M_x), sp.csr_matrix(A_x), sp.csr_matrix(M_x + 0.3 * A_x)]


def banded_matrices():
    """The banded matrices of test_kron_pack_row_pairs: 5-entry rows and a 9-point stencil."""
    rng = np.random.RandomState(123)
    n = 23 * 17
    band = sp.diags([rng.choice([1.0, -2.0, 0.5], size=n - abs(o)) for o in (-17, -1, 0, 1, 17)],
                    (-17, -1, 0, 1, 17), format='csr')
    offs9 = (-18, -17, -16, -1, 0, 1, 16, 17, 18)
    nine = sp.diags([rng.choice([1.0, -2.0, 0.5, 3.0], size=n - abs(o)) for o in offs9], offs9, format='csr')
    return dict(band5=[band, sp.csr_matrix(band.T), sp.csr_matrix(band + band.T)],
                nine=[nine, sp.csr_matrix(nine.T), sp.csr_matrix(nine + 2.0 * nine.T)])


@functools.lru_cache(maxsize=None)
def wrapper_matrices(name):
    if name in ('band5', 'nine'):
        return banded_matrices()[name]
    return mesh_matrices(*name)


WRAPPER_FAMILIES = MESH_FAMILIES + ('band5', 'nine')


def wrapper_case(name, n_loc, nt, lo, hi, beta, tris, seed=0):
    """A Case-like object on the matrices of a family, for the EllMatrices / PackedEllMatrices
    wrappers: (case, space, data, y_ref, bound), the vectors drawn again until the bound is
    informative."""
    space = space_from_csr(wrapper_matrices(name)[:nt])
    K = next(k for k in ELL_K if k >= space.width)
    c = Case('%s-n%d' % (name, n_loc), 'ell', K, space.M, n_loc, tris, lo=lo, hi=hi, beta=beta, seed=seed)
    for redraw in range(16):
        d = draw(c, space, redraw)
        y, e = reference(c, space, d)
        if bound_is_informative(y, e):
            return c, space, d, y, e
    raise AssertionError(name)


# ---- host tests -----------------------------------------------------------------------------------
def test_the_layouts_hold_the_matrices():
    """Every layout, decoded, is the matrix it was made from (and pairs really share columns)."""
    for K1, M, extra in ((5, 37, 0), (7, 64, 0), (9, 11, 0), (12, 20, 0), (7, 40, 3)):
        space = synthetic(K1, M, 2, 1, extra)
        ell = ell_layout(space, K1)
        for m in range(2):
            A = sp.lil_matrix((M, M))
            for p in range(M):
                for s in range(K1):
                    A[ell['row_ids'][p], ell['idx'][p, s]] += ell['vals'][m][p, s]
                if ell['ovf'] is not None:
                    for q in range(ell['ovf']['indptr'][p], ell['ovf']['indptr'][p + 1]):
                        A[ell['row_ids'][p], ell['ovf']['indices'][q]] += ell['ovf']['vals'][m][q]
            assert abs(sp.csr_matrix(A) - space.csr(m)).nnz == 0
        if extra:
            assert ell['ovf'] is not None
            continue
        for rp in (1, 2) if K1 in ROW_SLOTS.values() else (1,):
            K = {v: k for k, v in ROW_SLOTS.items()}[K1] if rp == 2 else K1
            lay = dict_layout(space, rp, K)
            assert lay['n_units'] == (pair_units(M) if rp == 2 else M)
            mask = (1 << lay['col_bits']) - 1
            for m in range(2):
                A = sp.lil_matrix((M, M))
                for u in range(lay['n_units']):
                    for j in range(rp):
                        if lay['row_ids'][u, j] >= 0:
                            for s in range(K):
                                w = int(lay['slots'][u, s])
                                A[lay['row_ids'][u, j], w & mask] += lay['dict'][m, w >> lay['col_bits'], j]
                assert abs(sp.csr_matrix(A) - space.csr(m)).nnz == 0
            if rp == 2:
                assert sorted(int(r) for r in lay['row_ids'].reshape(-1) if r >= 0) == list(range(M))
                single = np.flatnonzero(lay['row_ids'][:, 1] < 0)
                assert len(single) and (M < 6 or single[0] == 2)
                ex = explicit_layout(space, K, (1, 0))
                assert np.array_equal(ex['vals'][..., 0], unit_layout(space, 2, K)[1][1])


def _tri_of(T):
    """(3, n) of a tridiagonal SciPy matrix."""
    T = sp.csr_matrix(T).toarray()
    n = T.shape[0]
    assert np.count_nonzero(T) == np.count_nonzero(np.triu(np.tril(T, 1), -1))
    tri = np.zeros((3, n))
    tri[1] = np.diag(T)
    tri[0, 1:] = np.diag(T, -1)
    tri[2, :-1] = np.diag(T, 1)
    return tri


@pytest.mark.parametrize('name', ('g3_square', 'g3_lshape', 'g3_square3', 'g3_cube'))
def test_the_oracle_and_the_goldens_lie_inside_the_bound(name):
    """oracle/kron.py in float64 and the stored results of the reference's Kronecker applies, entry
    by entry (they apply the time factor first: the same products in another order)."""
    from oracle import kron as okron
    gd = load_golden(name)
    mats = {k: csr_from(gd, k) for k in ('A_t', 'L_t', 'M_t', 'G_t', 'M_x', 'A_x')}
    X = np.asarray(gd['X'])  # (N, M), time-major
    n, M = X.shape
    space = space_from_csr([mats['M_x'], mats['A_x']])
    d = Data()
    d.X, d.lo, d.hi, d.Y0 = [np.ascontiguousarray(X.T)], [None], [None], np.zeros((M, n))
    LtT = sp.csr_matrix(mats['L_t'].T)
    worst = 0.0
    singles = [('AtMx', mats['A_t'], 0), ('MtAx', mats['M_t'], 1), ('LtAx', mats['L_t'], 1), ('LtTMx', LtT, 0),
               ('GtMx', mats['G_t'], 0)]
    for nm, T, m in singles:
        c = Case(nm, 'ell', 16, M, n, ('full',))
        d.tri = [_tri_of(T)]
        y, e = reference(c, space, d, mats=[m])
        worst = max(worst, ratio(np.asarray(gd['kron_' + nm]).T, y, e, (name, nm)))
        worst = max(worst, ratio(okron.tridiag_kron_mat(T, space.csr(m), X).T, y, e, (name, nm, 'oracle')))
    c = Case('metric', 'ell', 16, M, n, ('full', 'full'))
    d.tri = [_tri_of(mats['A_t']), _tri_of(mats['M_t'])]
    y, e = reference(c, space, d)
    worst = max(worst, ratio(np.asarray(gd['kron_metric']).T, y, e, (name, 'metric')))
    worst = max(worst, ratio(okron.sum_apply([(mats['A_t'], mats['M_x']), (mats['M_t'], mats['A_x'])], X).T, y, e,
                             (name, 'metric', 'oracle')))
    c = Case('ident', 'ell', 16, M, n, ('id',))
    d.tri = [None]
    y, e = reference(c, space, d, mats=[0])
    worst = max(worst, ratio(np.asarray(gd['ident_Mx']).T, y, e, (name, 'ident')))
    worst = max(worst, ratio(okron.identity_kron_mat(mats['M_x'], X).T, y, e, (name, 'ident', 'oracle')))
    print('%s: float64 oracle and goldens at %.3f of the bound' % (name, worst))


def test_the_oracle_lies_inside_the_bound_on_catalogue_cases():
    """The float64 oracle on the signed catalogue inputs, ghost rows included (the time factor as
    an n_loc x (n_loc + 2) matrix on the ghosted block).  beta = 0 and 1: NumPy has no fused
    beta * y + s, and a separate product would be a rounding the kernels do not make."""
    from oracle import kron as okron
    worst, seen = 0.0, 0
    for name, c in CASES.items():
        if c.beta not in (0.0, 1.0) or c.M > 200 or not c.tags & {'ghost', 'ell-per-term', 'lanes', 'GENERIC'}:
            continue
        seen += 1
        space, d, y, e = case_data(name)
        n = c.n_loc
        want = np.zeros((space.M, n))
        for k in range(c.nt):
            s = k if c.per_term else 0
            Xe = np.zeros((n + 2, space.M))
            Xe[1:n + 1] = d.X[s].T
            Xe[0] = 0.0 if d.lo[s] is None else d.lo[s]
            Xe[n + 1] = 0.0 if d.hi[s] is None else d.hi[s]
            T = np.zeros((n, n + 2))
            for t in range(n):
                T[t, t:t + 3] = (0.0, 1.0, 0.0) if d.tri[k] is None else d.tri[k][:, t]
            want = want + okron.tridiag_kron_mat(sp.csr_matrix(T), space.csr(k), Xe).T
        worst = max(worst, ratio(want + c.beta * d.Y0, y, e, name))
    assert seen >= 40
    print('float64 oracle on %d catalogue cases at %.3f of the bound' % (seen, worst))


def test_the_bound_is_informative_on_the_whole_catalogue():
    for name, c in CASES.items():
        space, d, y, e = case_data(name)
        assert np.all(np.isfinite(y.astype(np.float64))) and bound_is_informative(y, e), name
        # the right restatement, rounded to float64, is of course inside it
        assert unchecked_ratio(y.astype(np.float64), y, e + LD(U) * np.abs(y)) <= 1.0


def test_the_catalogue_sits_where_it_says():
    """Every path of the tables, from the restated rules alone (256 CUs)."""
    L = {name: c.launch() for name, c in CASES.items()}
    of = lambda tag: [n for n, c in CASES.items() if tag in c.tags]
    # a. every NPF instance a (form, K, n_terms) can reach is reached, and the explicit form reaches one only
    for form, rp, Ks in (('dict', 1, PACK_K[1]), ('dict', 2, PACK_K[2]), ('explicit', 2, PACK_K[2]), ('ell', 1, ELL_K)):
        for K in Ks:
            got = {L[n]['NPF'] for n in of('instance') if CASES[n].form == form and CASES[n].rp == rp and CASES[n].K == K}
            if form == 'ell':
                reach = {ell_launch(K, 2, 64, n, (n + 1) & ~1, True)['NPF'] for n in range(1, N_LOC_MAX + 1)}
            else:
                reach = {pack_launch(K, rp, 2, 64, n, False, True, 16, form == 'explicit')['NPF']
                         for n in range(1, N_LOC_MAX - 8)}
            assert got == reach == ({1} if form == 'explicit' else {1, 2, 4}), (form, rp, K, got, reach)
            assert {CASES[n].nt for n in of('instance') if CASES[n].form == form and CASES[n].K == K} == {1, 2, 3}
            assert {1, 2, 3, 4, 9} <= {CASES[n].n_loc for n in of('instance') if CASES[n].form == form and CASES[n].K == K}
    for n in of('instance'):
        assert L[n]['ngroups'] >= 2 and (CASES[n].nt != 2 or L[n]['ngroups'] == 3), n
    # b. lane geometry
    assert any(L[n]['idle'] > 0 and L[n]['R'] > 1 for n in CASES)  # lanes with r >= R
    for form in ('dict1', 'dict2'):
        assert [(L['%s-wave-n%d' % (form, n)]['P'], L['%s-wave-n%d' % (form, n)]['W']) for n in (127, 128, 129)] == \
            [(64, 65), (64, 65), (65, 66)]
    assert [L['ell1-wave-n%d' % n]['W'] for n in (127, 128, 129)] == [64, 64, 65]
    for n in of('R1'):
        assert L[n]['W'] > 256 and L[n]['R'] == 1, n
    for n in of('longest'):
        assert CASES[n].n_loc == N_LOC_MAX and (N_LOC_MAX + 2) // 2 + 2 > BS and not L[n].get('refused'), n
    # ... and the longest slab whose single slot row still fits 64 KiB of LDS (include/stk.h states these)
    longest = lambda nt, rp: max(n for n in range(1, N_LOC_MAX + 1)
                                 if not pack_launch(PACK_K[rp][1], rp, nt, 64, n, True, True, 16)['refused'])
    assert [longest(nt, rp) for rp in (1, 2) for nt in (1, 2, 3)] == [1020, 1016, 675, 1020, 809, 536]
    for n in of('lds-cut'):
        assert L[n]['lds_cut'] and L[n]['lds'] <= LDS_CAP and CASES[n].nt == 3 and CASES[n].rp == 2 and CASES[n].n_loc <= 2
    # c. the group walk
    for stem in ('dict1', 'dict2', 'ell1', 'dict1-lanes', 'explicit2'):
        seen = set()
        for n in of('groups'):
            if n.startswith(stem + '-g'):
                R, t = L[n]['R'], L[n]['tail']
                seen.add((L[n]['ngroups'], 0 if t == 0 else (1 if t == 1 else 'R-1')))
                assert t in (0, 1, R - 1), n
        want = {(gq, t) for gq in (1, 7, 8, 9, 17) for t in (0, 1, 'R-1')}
        assert seen >= want, (stem, want - seen)
    assert L['dict1-lanes-g9-tail1']['kernel'] == 'kron_pack_terms_kernel'
    # d. three groups and more per workgroup, on each persistent kernel
    walked = {(L[n]['kernel'], L[n].get('RP', 1), bool(L[n].get('GHOST')), bool(L[n].get('MULTI')), L[n].get('DICT', True))
              for n in of('walk') if L[n]['walk'] >= 3}
    assert len(of('walk')) == len([n for n in of('walk') if L[n]['walk'] >= 3])
    assert walked >= {('kron_pack_kernel', 1, False, False, True), ('kron_pack_kernel', 1, True, False, True),
                      ('kron_pack_kernel', 2, False, False, True), ('kron_pack_kernel', 2, True, False, True),
                      ('kron_pack_kernel', 2, True, False, False), ('kron_pack_kernel', 1, False, True, True),
                      ('kron_pack_terms_kernel', 1, False, False, True), ('kron_pack_terms_kernel', 2, False, False, True),
                      ('kron_ell_kernel', 1, False, False, True)}, walked
    for n in of('walk'):
        assert CASES[n].M * CASES[n].ld * 8 < 32 << 20 and L[n]['R'] >= 2, n
    # row pairs: units of one row in the middle and at the end, odd M
    pairs = [c for c in CASES.values() if c.rp == 2]
    assert any(c.M % 2 for c in pairs) and all(c.space.units[2][1] == -1 for c in pairs if c.M > 5)
    assert any(c.space.units[-1][1] == -1 for c in pairs)
    # e. ghosts and time factors
    for stem in ('dict1', 'dict2', 'explicit2', 'ell1'):
        for n_loc in (1, 2, 3, 24, 25):
            assert {(CASES[n].lo, CASES[n].hi) for n in of('ghost') if n.startswith('%s-ghost-n%d-' % (stem, n_loc))} == \
                set(GHOST_ROUND)
        n = stem + '-identity-ghost'
        assert not CASES[n].any_tri and (stem == 'ell1' or (L[n]['GHOST'] and not L[n]['any_tri']))
    kinds = {k for c in CASES.values() for k in c.tris}
    assert kinds == {'full', 'zeros', 'gt', 'last', 'id'}
    assert any(c.any_tri and not c.lo and not c.hi for c in CASES.values())  # sub[0] / sup[-1] without a neighbour
    assert {c.beta for c in CASES.values()} == set(BETA_ROUND)
    assert any(c.extra for c in CASES.values()) and any(c.n_loc % 2 and c.extra for c in CASES.values())
    # f. inputs per term
    for rp in (1, 2):
        for n_loc in (1, 2, 9, 24, 33):
            assert L['dict%d-lanes-n%d' % (rp, n_loc)]['kernel'] == 'kron_pack_terms_kernel'
            assert L['dict%d-steps-n%d' % (rp, n_loc)]['kernel'] == 'kron_pack_terms_kernel'
            T = L['dict%d-turns-n%d' % (rp, n_loc)]
            assert T['kernel'] == 'kron_pack_kernel' and T['MULTI'] and not T['GHOST']
        F = L['dict%d-lanes-fallback-n400' % rp]
        assert F['kernel'] == 'kron_pack_kernel' and F['MULTI']
    c = CASES['dict1-steps-n9']  # (full, last, gt): ranges that end on the last pair of an odd slab and on the first
    assert c.tris == ('full', 'last', 'gt') and c.steps() == [None, (8, 9), (0, 1)]
    assert terms_lanes(9, 3, c.steps()) == [5, 1, 1] and L['dict1-steps-n9']['W'] == 7 < L['dict1-lanes-n9']['W'] == 15
    # g. the plain form's instances
    for K in ELL_K:
        assert L['ell-overflow-K%d' % K]['GENERIC'] and not L['ell-overflow-K%d' % K]['WIDE']
        assert L['ell-wide-K%d' % K]['WIDE'] and CASES['ell-overflow-K%d' % K].space.cnt.max() > K
    assert not L['ell-per-term-n3']['SHARED_IN'] and L['ell1-ghost-n3-11']['SHARED_IN']
    # sizes: nothing needs more than a few tens of megabytes
    assert max(c.M * c.ld * 8 for c in CASES.values()) < 32 << 20
    assert len(WRONG) == 8


@pytest.mark.parametrize('wrong', WRONG)
def test_a_wrong_restatement_leaves_the_bound(wrong):
    """Each mistake is an argument of the reference; the right restatement is the yardstick.  On
    every catalogue case the mistake applies to (the rows of a long case: its first 96)."""
    hit = 0
    for name, c in CASES.items():
        space, d, y, e = case_data(name)
        if not applies(wrong, c, d, space):
            continue
        rows = np.arange(min(space.M, 96))
        bad, _ = reference(c, space, d, wrong=wrong, rows=rows)
        assert unchecked_ratio(bad.astype(np.float64), y[rows], e[rows]) > 1.0, (wrong, name)
        hit += 1
    assert hit >= 10, (wrong, hit)
    print('%s: leaves the bound on all %d cases it applies to' % (wrong, hit))
