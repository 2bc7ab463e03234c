"""The element-block kernels (needs an MI355X) on matrices that come from no mesh and at
the edges of their launch shapes: the fused forms stk_kron_pack_elem_apply / _t in every
slot-count instantiation, the time stages stk_elem_time_apply / _t and stk_elem_block_mix
through the ABI alone, ElementKronMatMPI with one to three non-symmetric terms, and
every refusal of the fused entry points.

Reference and bound.  The reference is the sum written out in np.longdouble.  With
U = 2^-53, K the longest row of the union pattern and n = K + 4 n_terms + 1, every
elementary product passes through at most K fused multiply-adds of the space sum, at
most 4 n_terms of the time stage and one for beta, so entry by entry

    |got - ref| <= n U / (1 - n U) ((sum_k |blk_k| kron |X_k|) |x| + |beta y0|).

The time stages alone have K = 0, the block mix n = 2.  Every test prints its largest
error in units of this bound; DESIGN.md 3.9 records the figures."""
import ctypes
import functools
import itertools
import threading

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

U = 2.0**-53
LD = np.longdouble
BETAS = (0.0, -0.75)
N_LOCS = (1, 2, 3, 8, 9, 33, 64, 65)
LDS_LIMIT = 64 * 1024
BS = 512  # lanes of a workgroup of the fused kernels


def _gamma(n):
    return LD(n) * LD(U) / (LD(1) - LD(n) * LD(U))


# ---- the reference ----------------------------------------------------------------------
def _padded_rows(mat):
    """(columns, values), both (M, K): the rows of a CSR matrix padded with zeros."""
    mat = sp.csr_matrix(mat)
    mat.sort_indices()
    counts = np.diff(mat.indptr)
    K, M = max(int(counts.max()), 1), mat.shape[0]
    cols, vals = np.zeros((M, K), dtype=np.int64), np.zeros((M, K))
    slot = np.arange(mat.nnz) - np.repeat(mat.indptr[:-1], counts)
    row = np.repeat(np.arange(M), counts)
    cols[row, slot], vals[row, slot] = mat.indices, mat.data
    return cols, vals


def _union_K(mats):
    """The longest row of the union pattern."""
    total = sum(abs(sp.csr_matrix(m)) for m in mats)
    return int(np.diff(sp.csr_matrix(total).indptr).max())


def _space_images(ells, X):
    """[X_k X] for a space-major (M, n) array, in extended precision."""
    Xl = np.asarray(X, dtype=LD)
    out = []
    for cols, vals in ells:
        z = np.zeros(Xl.shape, dtype=LD)
        for s in range(cols.shape[1]):
            z += vals[:, s].astype(LD)[:, None] * Xl[cols[:, s]]
        out.append(z)
    return out


def _time_forward(blocks, zs, first_node, n_el):
    """y_{e,a} = sum_k sum_b blk_k[e][a][b] z_k[node(e) + b]; zs[k] is (M, n_loc + 2), its
    columns the nodes -1 .. n_loc (the ghost rows at both ends)."""
    q0 = first_node + 1 + np.arange(n_el)
    y = np.zeros((zs[0].shape[0], 2 * n_el), dtype=LD)
    for blk, z in zip(blocks, zs):
        b = np.asarray(blk, dtype=LD)
        y[:, 0::2] += b[:, 0, 0] * z[:, q0] + b[:, 0, 1] * z[:, q0 + 1]
        y[:, 1::2] += b[:, 1, 0] * z[:, q0] + b[:, 1, 1] * z[:, q0 + 1]
    return y


def _time_transposed(blocks, ws, first_node, n_el, n_loc):
    """x_n = sum_k sum_{e, a} blk_k[e][a][n - e] w_k[e, a] on the local nodes; ws[k] is
    (M, 2 n_el).  Nodes without an element stay zero."""
    q0 = first_node + 1 + np.arange(n_el)
    x = np.zeros((ws[0].shape[0], max(n_loc, first_node + n_el + 1) + 2), dtype=LD)  # column q = node + 1
    for blk, w in zip(blocks, ws):
        b = np.asarray(blk, dtype=LD)
        x[:, q0] += b[:, 0, 0] * w[:, 0::2] + b[:, 1, 0] * w[:, 1::2]
        x[:, q0 + 1] += b[:, 0, 1] * w[:, 0::2] + b[:, 1, 1] * w[:, 1::2]
    return x[:, 1:n_loc + 1]


def _check(got, ref, mag, beta, y0, n, what):
    """got within the bound of ref + beta y0, entry by entry; returns the largest error
    in units of the bound."""
    assert np.all(np.isfinite(got)), what
    ref = ref if beta == 0.0 else ref + LD(beta) * y0.astype(LD)
    bound = _gamma(n) * (mag if beta == 0.0 else mag + np.abs(LD(beta) * y0.astype(LD)))
    err = np.abs(got.astype(LD) - ref)
    pos = bound > 0
    worst = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
    assert np.all(err <= bound), what + (worst,)
    return worst


def _ranges(n_loc):
    """(first_node, n_el) of the slabs the drivers produce, then a short range."""
    out = [(0, n_loc), (-1, n_loc), (-1, n_loc + 1)]
    if n_loc > 1:
        out.insert(0, (0, n_loc - 1))
    if n_loc >= 3:
        out.append((0, (n_loc - 1) // 2))
    return out


def _dev(a):
    from source import _lib
    return _lib.to_dev(a)


def _nan_like(shape):
    return torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')


# ---- 1. the fused kernels ---------------------------------------------------------------
def _palette_copies(base, rng, n_mats=3, symmetric=False):
    """n_mats matrices on the pattern of `base` with values from a palette of 2-5 numbers;
    the second and third leave entries out (never the diagonal), so the union pattern
    is more than every matrix's own."""
    base = sp.csr_matrix(base)
    base.sort_indices()
    palette = rng.randn(int(rng.randint(2, 6)))
    mats = []
    for k in range(n_mats):
        m = base.copy()
        m.data = palette[rng.randint(len(palette), size=m.nnz)]
        if k > 0:
            coo = m.tocoo()
            keep = (rng.rand(m.nnz) < 0.8) | (coo.row == coo.col)
            m = sp.csr_matrix((coo.data[keep], (coo.row[keep], coo.col[keep])), shape=m.shape)
        if symmetric:
            upper = sp.triu(m, 1)
            m = sp.csr_matrix(upper + upper.T + sp.diags(m.diagonal()))
        m.sort_indices()
        mats.append(m)
    return mats


def _random_pattern(K, M, rng):
    """sp.random + eye with every row cut to at most min(K, M) entries and one row filled
    to exactly that many."""
    kmax = min(K, M)
    base = sp.csr_matrix(sp.random(M, M, density=min(1.0, 0.7 * kmax / M), random_state=rng, format='csr') + sp.eye(M))
    rows = []
    for i in range(M):
        c = base.indices[base.indptr[i]:base.indptr[i + 1]]
        others = c[c != i]
        if len(others) > kmax - 1:
            others = rng.choice(others, kmax - 1, replace=False)
        rows.append(np.concatenate([[i], others]))
    full = int(rng.randint(M))
    rest = np.setdiff1d(np.arange(M), rows[full])
    rows[full] = np.concatenate([rows[full], rng.choice(rest, kmax - len(rows[full]), replace=False)])
    r = np.repeat(np.arange(M), [len(c) for c in rows])
    return sp.csr_matrix((np.ones(len(r)), (r, np.concatenate(rows))), shape=(M, M))


def _symmetric_band(offsets, n, rng):
    diags, offs = [], []
    for o in offsets:
        d = rng.choice([1.0, -2.0, 0.5], size=n - o)
        diags += [d] if o == 0 else [d, d]
        offs += [o] if o == 0 else [o, -o]
    return sp.diags(diags, offs, format='csr')


SLOTS_BELOW = {5: 0, 7: 5, 9: 7, 12: 9, 16: 12}
# name -> (slot count of single rows, slot count of row pairs or None, builder)
SINGLE = [('random', K, M) for K in (5, 7, 9, 12, 16) for M in (3, 17, 130, 257) if M > 3 or K == 5]
FAMILIES = (['random-K%d-M%d' % (K, M) for _, K, M in SINGLE] +
            ['symmetric-K7-M130', 'band5', 'p1-square', 'nine'])
FULL_PRODUCT = ('random-K5-', 'random-K16-')  # the other families: a seeded half of the slabs


class _Family:
    """Three matrices on one plan, its two packed forms and what the reference needs."""
    def __init__(self, name):
        from source.linop import EllMatrices, SpaceMatrix
        self.name = name
        rng = np.random.RandomState(sum(map(ord, name)))
        self.symmetric, self.pair_K, hints = False, None, None
        if name.startswith('random-'):
            K, M = int(name.split('-')[1][1:]), int(name.split('-')[2][1:])
            self.single_K = K
            self.mats = _palette_copies(_random_pattern(K, M, rng), rng)
            kmax = _union_K(self.mats)
            assert SLOTS_BELOW[K] < kmax <= K or (M == 3 and kmax == 3), (name, kmax)
        elif name == 'symmetric-K7-M130':
            self.single_K, self.symmetric = 7, True
            pat = _random_pattern(4, 130, rng)
            pat = sp.csr_matrix(pat + pat.T)
            # (a row of the symmetrised pattern may exceed 7: cut the pattern, not the test)
            counts = np.diff(pat.indptr)
            while counts.max() > 7:
                i = int(np.argmax(counts))
                j = [c for c in pat.indices[pat.indptr[i]:pat.indptr[i + 1]] if c != i][-1]
                pat = pat.tolil()
                pat[i, j] = pat[j, i] = 0
                pat = sp.csr_matrix(pat)
                pat.eliminate_zeros()
                counts = np.diff(pat.indptr)
            self.mats = _palette_copies(pat, rng, symmetric=True)
            assert 5 < _union_K(self.mats) <= 7
        elif name == 'band5':
            self.single_K, self.pair_K, self.symmetric = 5, 8, True
            a = _symmetric_band((0, 1, 17), 23 * 17, rng)
            b = _symmetric_band((0, 1, 17), 23 * 17, rng)
            self.mats = [a, b, sp.csr_matrix(a + 0.5 * b)]
        elif name == 'nine':
            self.single_K, self.pair_K, self.symmetric = 9, 12, True
            a = _symmetric_band((0, 1, 16, 17, 18), 23 * 17, rng)
            b = _symmetric_band((0, 1, 16, 17, 18), 23 * 17, rng)
            self.mats = [a, b, sp.csr_matrix(a + 0.5 * b)]
        else:
            from source.assembly import space_matrices
            from source.problem import problem_helper
            assert name == 'p1-square'
            self.single_K, self.pair_K, self.symmetric = 7, 10, True
            M_x, A_x = space_matrices(problem_helper('square', J_space=2, J_time=1)[0])
            self.mats = [M_x, A_x, sp.csr_matrix(M_x + 0.3 * A_x)]
            hints = [M_x]
        self.mats = [sp.csr_matrix(m) for m in self.mats]
        self.M = self.mats[0].shape[0]
        if self.symmetric:
            assert all((abs(m - m.T) > 0).nnz == 0 for m in self.mats)
        else:
            assert all((abs(m - m.T) > 0).nnz > 0 for m in self.mats)
        self.ell = EllMatrices(self.mats, hints or ())
        self.one = self.ell.packed_variant(1)
        assert self.one.ok and not self.one.explicit and self.one.rows_per_unit == 1, name
        assert self.one.pattern.K == self.single_K and self.one.n_mats == 3, (name, self.one.pattern.K)
        self.plans = [self.one]
        if self.pair_K is not None:
            two = self.ell.packed_variant(2)
            assert two.ok and not two.explicit and two.rows_per_unit == 2, (name, two.ok)
            assert two.pattern.K == self.pair_K, (name, two.pattern.K)
            rows = two.row_ids.cpu().numpy().reshape(-1, 2)
            assert self.M % 2 == 1 and (rows < 0).any(), 'an odd M leaves a slot row with one matrix row'
            self.plans.append(two)
        self.ells = [_padded_rows(m) for m in self.mats]
        self.abs_ells = [(c, np.abs(v)) for c, v in self.ells]
        self.space_ops = [SpaceMatrix(m) for m in self.mats]


@functools.lru_cache(maxsize=None)
def _family(name):
    return _Family(name)


def _launch_shape(pat, n_el, n_loc, transposed):
    """(W, R, groups, LDS bytes at R, LDS bytes at the R the lanes alone would give) of a
    fused launch, as csrc/kron_pack_elem.hip chooses them; the LDS count for one slot row
    is checked against the library's own where it is used."""
    K, RP = pat.K, pat.rows_per_unit
    P = (n_loc + 1) // 2
    W = max(n_el, P) if transposed else P + 1
    KS = (K + 3) & ~3
    SW = 2 * n_el + 2 if transposed else n_loc + 3

    def lds(R):
        return 8 * (2 * R * RP * SW + pat.n_codes * RP * 2 + 8 * n_el) + 4 * (R * KS + ((R * RP + 3) & ~3)) + 32

    R0 = BS // W
    if R0 * K > 4 * BS:
        R0 = 4 * BS // K
    R = R0
    while R > 1 and lds(R) > LDS_LIMIT:
        R -= 1
    return W, R, -(-pat.n_units // R), lds(R), lds(R0)


def _lds_bytes(pat, n_el, n_loc, transposed):
    from source import _lib
    return int(_lib.lib().stk_kron_pack_elem_lds_bytes(ctypes.byref(pat), n_el, n_loc, int(transposed)))


def _composed(fam, terms, blocks_dev, x, ghosts, n_el, n_loc, first_node, beta, out, transposed):
    """stk_ell_spmm per matrix on the slab and on the ghost pair, then the time stage: what
    ElementKronMatMPI.apply_buf composes, the space factors untransposed as in the fused form."""
    from source import _lib
    from source.mpi_kron import _ptr_array
    lib, ops = _lib.lib(), [fam.space_ops[k] for k in terms]
    if transposed:
        w = [op.apply(x, n_loc=2 * n_el) for op in ops]
        _lib.check(lib.stk_elem_time_apply_t(_lib.stream(), fam.M, n_el, n_loc, out.shape[1], first_node, len(ops),
                                             _ptr_array(w), _ptr_array(blocks_dev), beta, _lib.ptr(out)))
        return
    z = [op.apply(x, n_loc=n_loc) for op in ops]
    zg = [None if ghosts is None else op.apply(ghosts, n_loc=2) for op in ops]
    _lib.check(lib.stk_elem_time_apply(_lib.stream(), fam.M, n_el, n_loc, x.shape[1], first_node, len(ops),
                                       _ptr_array(z), _ptr_array(zg), _ptr_array(blocks_dev), beta, _lib.ptr(out)))


class _Slab:
    """Inputs, reference and magnitudes of one slab in one direction."""
    def __init__(self, fam, terms, n_loc, first_node, n_el, transposed, rng):
        M = fam.M
        self.args = (n_loc, first_node, n_el, transposed)
        self.ld = ld = n_loc + (n_loc & 1)
        self.blocks = [rng.randn(n_el, 2, 2) for _ in terms]
        self.blocks_dev = [_dev(b) for b in self.blocks]
        ells, abs_ells = [fam.ells[k] for k in terms], [fam.abs_ells[k] for k in terms]
        abs_blocks = [np.abs(b) for b in self.blocks]
        self.ghosts = None
        if transposed:
            Y = rng.randn(M, 2 * n_el)
            self.x = _dev(Y)
            self.ref = _time_transposed(self.blocks, _space_images(ells, Y), first_node, n_el, n_loc)
            self.mag = _time_transposed(abs_blocks, _space_images(abs_ells, np.abs(Y)), first_node, n_el, n_loc)
            self.n_out = n_loc
            self.out_shape = (M, ld)
            self.no_element = np.arange(n_loc) > first_node + n_el  # nodes behind a short range
        else:
            X = np.zeros((M, n_loc + 2))  # the nodes -1 .. n_loc
            X[:, 1:n_loc + 1] = rng.randn(M, n_loc)
            below, above = first_node < 0, first_node + n_el == n_loc
            if below or above:  # ghosts exactly where an element reaches them, NaN elsewhere
                gh = np.full((M, 2), np.nan)
                if below:
                    gh[:, 0] = X[:, 0] = rng.randn(M)
                if above:
                    gh[:, 1] = X[:, n_loc + 1] = rng.randn(M)
                self.ghosts = _dev(gh)
            xs = np.zeros((M, ld))
            xs[:, :n_loc] = X[:, 1:n_loc + 1]
            self.x = _dev(xs)
            self.ref = _time_forward(self.blocks, _space_images(ells, X), first_node, n_el)
            self.mag = _time_forward(abs_blocks, _space_images(abs_ells, np.abs(X)), first_node, n_el)
            self.n_out = 2 * n_el
            self.out_shape = (M, 2 * n_el)

    def start(self, beta, rng):
        """An output before the call: NaN everywhere for beta = 0, else random with a zero
        padding column."""
        if beta == 0.0:
            return np.full(self.out_shape, np.nan)
        y0 = rng.randn(*self.out_shape)
        y0[:, self.n_out:] = 0.0
        return y0


def _run_slab(fam, terms, n_loc, first_node, n_el, transposed, rng, plans=None, composed=True):
    """Both betas on one slab: every plan's fused form and the composed one against the
    reference, the padding column, nodes without an element, and all forms bit for bit."""
    slab = _Slab(fam, terms, n_loc, first_node, n_el, transposed, rng)
    n = _union_K([fam.mats[k] for k in terms]) + 4 * len(terms) + 1
    worst = 0.0
    for beta in BETAS:
        y0 = slab.start(beta, rng)
        results = []
        forms = [('fused', p) for p in (fam.plans if plans is None else plans)] + ([('composed', None)] if composed else [])
        for form, plan in forms:
            what = (fam.name, terms, n_loc, first_node, n_el, transposed, beta, form, plan and plan.rows_per_unit)
            y = _dev(y0)
            if plan is None:
                _composed(fam, terms, slab.blocks_dev, slab.x, slab.ghosts, n_el, n_loc, first_node, beta, y, transposed)
            else:
                plan.apply_elem(terms, slab.blocks_dev, slab.x, slab.ghosts, n_el, n_loc, slab.ld, first_node, beta, y,
                                transposed=transposed)
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            worst = max(worst, _check(got[:, :slab.n_out], slab.ref, slab.mag, beta, y0[:, :slab.n_out], n, what))
            assert np.all(got[:, slab.n_out:] == 0.0), what + ('padding column',)
            if transposed and slab.no_element.any():
                behind = got[:, :n_loc][:, slab.no_element]  # beta * old exactly, 0 for beta = 0
                want = np.zeros_like(behind) if beta == 0.0 else np.float64(beta) * y0[:, :n_loc][:, slab.no_element]
                assert np.array_equal(behind, want), what + ('nodes behind the last element',)
            results.append((what, got))
        for what, got in results[1:]:  # row pairs = single rows = the composed form
            assert np.array_equal(got, results[0][1]), (what, results[0][0])
    return worst


TERMS = ((2, 0), (0, 1))


def _slabs(name):
    all_slabs = [(n_loc, fn, n_el) for n_loc in N_LOCS for fn, n_el in _ranges(n_loc)]
    if name.startswith(FULL_PRODUCT):
        return all_slabs
    rng = np.random.RandomState(len(name))
    pick = rng.permutation(len(all_slabs))[:(len(all_slabs) + 1) // 2]
    return [all_slabs[i] for i in sorted(pick)]


@pytest.mark.parametrize('name', FAMILIES)
def test_fused_kernels_on_every_slab_shape(name):
    """stk_kron_pack_elem_apply / _t on one family of matrices: the slabs of 1 .. 65 nodes
    with the four element ranges of the drivers and a short one, both directions, beta = 0
    on NaN and beta = -0.75, terms on the matrices (2, 0) and (0, 1) of a plan of three;
    single rows, row pairs and the composed form give the same doubles."""
    fam = _family(name)
    rng = np.random.RandomState(5)
    worst, shapes = 0.0, set()
    for i, (n_loc, first_node, n_el) in enumerate(_slabs(name)):
        terms = TERMS[i % 2]
        for transposed in (False, True):
            worst = max(worst, _run_slab(fam, terms, n_loc, first_node, n_el, transposed, rng))
            for plan in fam.plans:
                W, R, groups, _, _ = _launch_shape(plan.pattern, n_el, n_loc, transposed)
                slots = R * plan.pattern.K  # prefetched words of a group: 1, 2 or 4 per lane
                shapes.add((plan.pattern.n_units % R != 0, groups < 8, 1 if slots <= BS else 2 if slots <= 2 * BS else 4))
    if fam.M in (3, 17):
        assert any(tail for tail, _, _ in shapes), 'a tail group'
        assert any(few for _, few, _ in shapes), 'fewer than 8 groups: empty XCD chunks'
    print('%s: prefetch depths %s, largest error in units of the bound: %.3f'
          % (name, sorted({d for _, _, d in shapes}), worst))


def test_every_instantiation_runs_in_both_directions():
    """The eight (rows per unit, K) instantiations, forward and transposed, each on a plan
    that really has that shape, at a slab with a tail group and at one with several
    groups."""
    want = {(1, K) for K in (5, 7, 9, 12, 16)} | {(2, K) for K in (8, 10, 12)}
    names = ['random-K%d-M17' % K for K in (5, 7, 9, 12, 16)] + ['band5', 'p1-square', 'nine']
    rng = np.random.RandomState(6)
    seen, worst = set(), 0.0
    for name in names:
        fam = _family(name)
        for plan in fam.plans:
            for transposed in (False, True):
                for n_loc, first_node, n_el in ((3, -1, 4), (64, 0, 64)):
                    worst = max(worst, _run_slab(fam, (2, 0), n_loc, first_node, n_el, transposed, rng, plans=[plan],
                                                 composed=False))
                seen.add((plan.pattern.rows_per_unit, plan.pattern.K, transposed))
    assert seen == {(rp, K, t) for rp, K in want for t in (False, True)}, sorted(seen)
    print('largest error in units of the bound: %.3f' % worst)


def _cu_count():
    from source import _lib
    n_cu = ctypes.c_int32()
    _lib.check(_lib.lib().stk_device_info(ctypes.byref(n_cu), None, None))
    return n_cu.value


class _Band2600(_Family):
    """The symmetric 5-band matrix on 2600 rows: single rows and row pairs both give more
    slot rows than three workgroups per CU take in one turn."""
    def __init__(self):
        from source.linop import EllMatrices, SpaceMatrix
        rng = np.random.RandomState(26)
        self.name, self.symmetric, self.single_K, self.pair_K = 'band5-M2600', True, 5, 8
        a, b = _symmetric_band((0, 1, 52), 2600, rng), _symmetric_band((0, 1, 52), 2600, rng)
        self.mats = [a, b, sp.csr_matrix(a + 0.5 * b)]
        self.M = 2600
        self.ell = EllMatrices(self.mats)
        self.one, two = self.ell.packed_variant(1), self.ell.packed_variant(2)
        assert self.one.ok and not self.one.explicit and (self.one.rows_per_unit, self.one.pattern.K) == (1, 5)
        assert two.ok and not two.explicit and (two.rows_per_unit, two.pattern.K) == (2, 8)
        self.plans = [self.one, two]
        self.ells = [_padded_rows(m) for m in self.mats]
        self.abs_ells = [(c, np.abs(v)) for c, v in self.ells]
        self.space_ops = [SpaceMatrix(m) for m in self.mats]


@pytest.mark.parametrize('transposed', [False, True])
def test_one_slot_row_per_group_and_many_groups_per_workgroup(transposed):
    """n_loc = 511: a slot row takes more than half a workgroup's lanes, R = 1, and with
    M = 2600 every workgroup walks several groups through the register prefetch.  Forward
    511 elements (W = 257); transposed 512 (W = n_el = 512 > P), which fits the LDS with
    single rows only -- the library says so for the row pairs."""
    fam = _Band2600()
    n_loc, first_node, n_el = (511, -1, 512) if transposed else (511, 0, 511)
    plans = []
    for plan in fam.plans:
        need = _lds_bytes(plan.pattern, n_el, n_loc, transposed)
        if transposed and plan.rows_per_unit == 2:
            assert need > LDS_LIMIT, need  # 4 sums per test-space column and 8 n_el block doubles
            continue
        W, R, groups, lds, _ = _launch_shape(plan.pattern, n_el, n_loc, transposed)
        assert need == lds <= LDS_LIMIT and R == 1 and 2 * W > BS, (W, R, lds, need)
        assert groups == plan.pattern.n_units > 3 * _cu_count(), (groups, _cu_count())
        plans.append(plan)
    assert len(plans) == (1 if transposed else 2)
    worst = _run_slab(fam, (2, 0), n_loc, first_node, n_el, transposed, np.random.RandomState(8), plans=plans)
    print('largest error in units of the bound: %.3f' % worst)


def _refused(call, out, words):
    """A call the library refuses: non-zero, the error names `words`, and the output is
    unchanged bit for bit."""
    from source import _lib
    before = out.clone()
    rc = call()
    message = _lib.lib().stk_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0, words
    for w in words:
        assert w in message, (w, message)
    assert torch.equal(out.view(torch.int64), before.view(torch.int64)), message


def _raw_call(plan, slab, n_el, n_loc, ld, first_node, transposed, out, n_terms=2, mats=(2, 0), pattern=None, x=None,
              ghosts='slab', y=None):
    """The fused entry point itself (no _lib.check), every argument replaceable."""
    from source import _lib
    lib = _lib.lib()
    terms = (_lib.KronPackTerm * 3)()
    for t, k in zip(terms, tuple(mats) + (0,) * 3):
        t.tri, t.mat = None, k
    blocks = slab.blocks_dev + [slab.blocks_dev[0]] * 3
    blk = (ctypes.c_void_p * 3)(*[_lib.ptr(b) for b in blocks[:3]])
    pat = ctypes.byref(plan.pattern if pattern is None else pattern)
    x = _lib.ptr(slab.x) if x is None else x
    y = _lib.ptr(out) if y is None else y
    if transposed:
        return lambda: lib.stk_kron_pack_elem_apply_t(_lib.stream(), pat, n_el, n_loc, ld, first_node, n_terms, terms,
                                                      blk, x, -0.75, y)
    gh = _lib.ptr(slab.ghosts) if isinstance(ghosts, str) else ghosts
    return lambda: lib.stk_kron_pack_elem_apply(_lib.stream(), pat, n_el, n_loc, ld, first_node, n_terms, terms, blk,
                                                x, gh, -0.75, y)


def test_slabs_at_the_end_of_the_lds_and_of_the_lanes():
    """Row pairs.  Forward at n_loc = 500: two slot rows per group, as the lanes allow,
    outgrow 64 KiB, so the launch lowers R to 1 (one row fits, by the library's count).
    Transposed at the longest slab the library still accepts (found by bisection), the
    next longer one is refused for its LDS, and 1023 nodes forward for their lanes --
    both without touching the output."""
    fam = _family('band5')
    plan = fam.plans[1]
    pat = plan.pattern
    rng = np.random.RandomState(9)
    n_loc, first_node, n_el = 500, -1, 501
    W, R, _, lds, lds_by_lanes = _launch_shape(pat, n_el, n_loc, False)
    assert BS // W == 2 and lds_by_lanes > LDS_LIMIT and R == 1, (W, R, lds_by_lanes)
    assert _lds_bytes(pat, n_el, n_loc, False) == lds <= LDS_LIMIT
    worst = _run_slab(fam, (0, 1), n_loc, first_node, n_el, False, rng, plans=[plan])
    # transposed, n_el = n_loc + 1: the largest n_el that fits
    fits = lambda m: 0 <= _lds_bytes(pat, m, m - 1, True) <= LDS_LIMIT
    lo, hi = 2, 513
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    n_el = lo
    assert _launch_shape(pat, n_el, n_el - 1, True)[3] == _lds_bytes(pat, n_el, n_el - 1, True)
    worst = max(worst, _run_slab(fam, (0, 1), n_el - 1, -1, n_el, True, rng, plans=[plan]))
    print('transposed: %d elements fit; largest error in units of the bound: %.3f' % (n_el, worst))
    # just beyond
    n_el, n_loc = n_el + 1, n_el
    slab = _Slab(fam, (0, 1), n_loc, -1, n_el, True, rng)
    out = torch.full((fam.M, n_loc + (n_loc & 1)), 7.5, dtype=torch.float64, device='cuda')
    _refused(_raw_call(plan, slab, n_el, n_loc, n_loc + (n_loc & 1), -1, True, out, mats=(0, 1)), out,
             ('stk_kron_pack_elem_apply_t', 'LDS'))
    n_loc = 1023
    slab = _Slab(fam, (0, 1), n_loc, 0, n_loc - 1, False, rng)
    out = torch.full((fam.M, 2 * (n_loc - 1)), 7.5, dtype=torch.float64, device='cuda')
    _refused(_raw_call(plan, slab, n_loc - 1, n_loc, n_loc + 1, 0, False, out, mats=(0, 1), ghosts=None), out,
             ('stk_kron_pack_elem_apply', 'lanes'))


# ---- 2. the time stages and the block mix alone -----------------------------------------
def _ptrs(tensors):
    from source.mpi_kron import _ptr_array
    return _ptr_array(tensors)


@pytest.mark.parametrize('n_terms', [1, 2, 3])
def test_time_stages_through_the_abi(n_terms):
    """stk_elem_time_apply / _t on random images z_k / w_k: M = 1, 7, 1000, 1 .. 65 nodes,
    the ranges of the drivers and a short one, leading dimensions 1, 2 and 5 beyond n_loc
    (columns the forward stage must not read: NaN; columns the transpose must write as
    zero), beta = 0 on NaN and -0.75."""
    from source import _lib
    lib = _lib.lib()
    rng = np.random.RandomState(20 + n_terms)
    n, worst = 4 * n_terms + 1, 0.0
    for M, n_loc, extra in itertools.product((1, 7, 1000), (1, 2, 3, 9, 64, 65), (1, 2, 5)):
        ld = n_loc + extra
        for first_node, n_el in _ranges(n_loc):
            blocks = [rng.randn(n_el, 2, 2) for _ in range(n_terms)]
            abs_blocks = [np.abs(b) for b in blocks]
            blocks_dev = [_dev(b) for b in blocks]
            # forward
            zs = [rng.randn(M, n_loc + 2) for _ in range(n_terms)]
            below, above = first_node < 0, first_node + n_el == n_loc
            z_dev, zg_dev = [], []
            for z in zs:
                slab = np.full((M, ld), np.nan)
                slab[:, :n_loc] = z[:, 1:n_loc + 1]
                z_dev.append(_dev(slab))
                gh = np.full((M, 2), np.nan)
                if below:
                    gh[:, 0] = z[:, 0]
                if above:
                    gh[:, 1] = z[:, n_loc + 1]
                zg_dev.append(_dev(gh))
            ref = _time_forward(blocks, [z.astype(LD) for z in zs], first_node, n_el)
            mag = _time_forward(abs_blocks, [np.abs(z).astype(LD) for z in zs], first_node, n_el)
            zg = _ptrs(zg_dev) if below or above else None  # a middle range passes NULL
            for beta in BETAS:
                y0 = np.full((M, 2 * n_el), np.nan) if beta == 0.0 else rng.randn(M, 2 * n_el)
                y = _dev(y0)
                _lib.check(lib.stk_elem_time_apply(_lib.stream(), M, n_el, n_loc, ld, first_node, n_terms, _ptrs(z_dev),
                                                   zg, _ptrs(blocks_dev), beta, _lib.ptr(y)))
                torch.cuda.synchronize()
                worst = max(worst, _check(y.cpu().numpy(), ref, mag, beta, y0, n,
                                          ('forward', M, n_loc, ld, first_node, n_el, beta)))
            if below or above:  # ... and the same call without the ghost images is refused
                y = torch.full((M, 2 * n_el), 7.5, dtype=torch.float64, device='cuda')
                _refused(lambda: lib.stk_elem_time_apply(_lib.stream(), M, n_el, n_loc, ld, first_node, n_terms,
                                                         _ptrs(z_dev), None, _ptrs(blocks_dev), 0.0, _lib.ptr(y)),
                         y, ('stk_elem_time_apply', 'ghost'))
            # transposed
            ws = [rng.randn(M, 2 * n_el) for _ in range(n_terms)]
            w_dev = [_dev(w) for w in ws]
            ref = _time_transposed(blocks, [w.astype(LD) for w in ws], first_node, n_el, n_loc)
            mag = _time_transposed(abs_blocks, [np.abs(w).astype(LD) for w in ws], first_node, n_el, n_loc)
            no_element = np.arange(n_loc) > first_node + n_el
            for beta in BETAS:
                x0 = np.full((M, ld), np.nan)
                if beta != 0.0:
                    x0[:, :n_loc] = rng.randn(M, n_loc)
                x = _dev(x0)
                _lib.check(lib.stk_elem_time_apply_t(_lib.stream(), M, n_el, n_loc, ld, first_node, n_terms,
                                                     _ptrs(w_dev), _ptrs(blocks_dev), beta, _lib.ptr(x)))
                torch.cuda.synchronize()
                got = x.cpu().numpy()
                what = ('transposed', M, n_loc, ld, first_node, n_el, beta)
                worst = max(worst, _check(got[:, :n_loc], ref, mag, beta, x0[:, :n_loc], n, what))
                assert np.all(got[:, n_loc:] == 0.0), what + ('columns from n_loc to ld',)
                if no_element.any():
                    behind = got[:, :n_loc][:, no_element]  # beta * old exactly, 0 for beta = 0
                    want = np.zeros_like(behind) if beta == 0.0 else np.float64(beta) * x0[:, :n_loc][:, no_element]
                    assert np.array_equal(behind, want), what + ('nodes behind the last element',)
    print('%d terms: largest error in units of the bound: %.3f' % (n_terms, worst))


def test_block_mix_out_of_place_and_in_place():
    """stk_elem_block_mix: y = x gives the doubles of the out-of-place call, within
    2 U / (1 - 2 U) |blk| |x| of the reference."""
    from source import _lib
    lib = _lib.lib()
    rng = np.random.RandomState(31)
    worst = 0.0
    for M, n_el in itertools.product((1, 1000), (1, 2, 33)):
        blk, X = rng.randn(n_el, 2, 2), rng.randn(M, 2 * n_el)
        b, Xl = blk.astype(LD), X.astype(LD)
        ref, mag = np.zeros(X.shape, dtype=LD), np.zeros(X.shape, dtype=LD)
        for a in (0, 1):
            ref[:, a::2] = b[:, a, 0] * Xl[:, 0::2] + b[:, a, 1] * Xl[:, 1::2]
            mag[:, a::2] = np.abs(b[:, a, 0]) * np.abs(Xl[:, 0::2]) + np.abs(b[:, a, 1]) * np.abs(Xl[:, 1::2])
        blk_dev, x, y = _dev(blk), _dev(X), _nan_like(X.shape)
        _lib.check(lib.stk_elem_block_mix(_lib.stream(), M, n_el, _lib.ptr(blk_dev), _lib.ptr(x), _lib.ptr(y)))
        assert torch.equal(x, _dev(X)), 'the input of the out-of-place call'
        _lib.check(lib.stk_elem_block_mix(_lib.stream(), M, n_el, _lib.ptr(blk_dev), _lib.ptr(x), _lib.ptr(x)))
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        assert np.array_equal(got, x.cpu().numpy()), (M, n_el)
        worst = max(worst, _check(got, ref, mag, 0.0, None, 2, ('block mix', M, n_el)))
    print('largest error in units of the bound: %.3f' % worst)


# ---- 3. ElementKronMatMPI beyond two symmetric terms --------------------------------------
_global_matrices = {}
_build_lock = threading.Lock()  # rank threads share the matrices: one builds their device forms


def _operator_matrices(n_terms, ranks):
    """(B, exact B, B^T, exact B^T) of n_terms non-symmetric random terms, M = 6, N = 5, on
    `ranks` ranks; computed once."""
    from thread_comm import run_ranks
    from source.comm import Comm
    from source.mpi_kron import ElementKronMatMPI
    from source.mpi_vector import DofDistributionMPI
    if (n_terms, ranks) not in _global_matrices:
        rng = np.random.RandomState(40)
        M, N = 6, 5
        mats = _palette_copies(_random_pattern(4, M, rng), rng)[:n_terms]
        blocks = [rng.randn(N - 1, 2, 2) for _ in range(n_terms)]

        def body(comm):
            dd = DofDistributionMPI(comm, N, M)
            out = []
            for transposed in (False, True):
                with _build_lock:
                    op = ElementKronMatMPI(dd, blocks, mats, transposed=transposed)
                    assert op.fused_plan() is None  # not two symmetric terms: composed
                    for space_op in op.space_ops:
                        space_op._ell_form()
                out += [op.as_global_matrix(), op.as_matrix()]
            return out

        got = run_ranks(ranks, body)[0] if ranks > 1 else body(Comm(distributed=False))
        _global_matrices[(n_terms, ranks)] = (got, mats, blocks)
    return _global_matrices[(n_terms, ranks)]


@pytest.mark.parametrize('ranks', [1, 3])
@pytest.mark.parametrize('n_terms', [1, 2, 3])
def test_operators_of_one_to_three_unsymmetric_terms(n_terms, ranks):
    """as_global_matrix against as_matrix column by column (a column is the image of a unit
    vector: the bound is that column of sum_k |T_k| kron |X_k|), forward and transposed --
    the transpose must be sum_k T_k^T kron X_k^T, space factors transposed too -- and the
    3-rank matrices equal the 1-rank ones bit for bit."""
    (B, exact, BT, exact_T), mats, blocks = _operator_matrices(n_terms, ranks)
    M, N = 6, 5
    total, mag, time_factors = 0.0, 0.0, []
    for blk, X in zip(blocks, mats):
        T = np.zeros((2 * (N - 1), N))
        for e in range(N - 1):
            T[2 * e:2 * e + 2, e:e + 2] = blk[e]
        time_factors.append(T)
        total = total + np.kron(T.astype(LD), X.toarray().astype(LD))
        mag = mag + np.kron(np.abs(T).astype(LD), np.abs(X.toarray()).astype(LD))
    # as_matrix is n_terms rounded products per entry; the other transpose is another matrix
    assert np.all(np.abs(exact.astype(LD) - total) <= _gamma(n_terms) * mag)
    other = sum(np.kron(T_k.T, X.toarray()) for T_k, X in zip(time_factors, mats))
    assert np.max(np.abs(other - exact_T)) > 1e-2, 'space factors that equal their transposes show nothing'
    worst = 0.0
    for got, ref, bound_mag, K in ((B, exact, mag, _union_K(mats)),
                                   (BT, exact_T, mag.T, _union_K([m.T for m in mats]))):
        assert got.shape == ref.shape
        bound = _gamma(K + 4 * n_terms + 1) * bound_mag
        err = np.abs(got.astype(LD) - ref)
        assert np.all(err <= bound), (n_terms, ranks, K, float(np.max(err[bound > 0] / bound[bound > 0])))
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    assert np.array_equal(exact_T, exact.T)
    if ranks > 1:
        one = _operator_matrices(n_terms, 1)[0]
        assert np.array_equal(B, one[0]) and np.array_equal(BT, one[2])
    print('%d terms, %d ranks: largest error in units of the bound: %.3f' % (n_terms, ranks, worst))


def test_two_symmetric_terms_of_that_size_run_fused():
    from source.comm import Comm
    from source.mpi_kron import ElementKronMatMPI
    from source.mpi_vector import DofDistributionMPI
    rng = np.random.RandomState(41)
    M, N = 6, 5
    pat = _random_pattern(3, M, rng)
    mats = _palette_copies(sp.csr_matrix(pat + pat.T), rng, symmetric=True)[:2]
    blocks = [rng.randn(N - 1, 2, 2) for _ in mats]
    dd = DofDistributionMPI(Comm(distributed=False), N, M)
    for transposed in (False, True):
        assert ElementKronMatMPI(dd, blocks, mats, transposed=transposed).fused_plan() is not None


# ---- 4. what the fused entry points refuse ------------------------------------------------
@pytest.mark.parametrize('transposed', [False, True])
def test_fused_entry_points_refuse(transposed):
    """Every argument the fused entry points are written to refuse: non-zero, the error
    names the function, no kernel runs and the output keeps its bits."""
    from source import _lib
    fam = _family('p1-square')
    plan = fam.one
    rng = np.random.RandomState(50)
    n_loc, first_node, n_el, ld = 9, -1, 10, 10
    slab = _Slab(fam, (2, 0), n_loc, first_node, n_el, transposed, rng)
    who = 'stk_kron_pack_elem_apply_t' if transposed else 'stk_kron_pack_elem_apply'
    out = torch.full((fam.M, ld if transposed else 2 * n_el), 7.5, dtype=torch.float64, device='cuda')
    call = functools.partial(_raw_call, plan, slab)
    # the call itself is good
    good = out.clone()
    assert _raw_call(plan, slab, n_el, n_loc, ld, first_node, transposed, good)() == 0
    torch.cuda.synchronize()
    assert not torch.equal(good, out)
    explicit = _lib.PackPattern.from_buffer_copy(plan.pattern)
    explicit.vals = _lib.ptr(plan.dict)
    spare_x = torch.zeros(slab.x.numel() + 2, dtype=torch.float64, device='cuda')
    spare_y = torch.full((out.numel() + 2,), 7.5, dtype=torch.float64, device='cuda')
    cases = {
        'one term': call(n_el, n_loc, ld, first_node, transposed, out, n_terms=1),
        'three terms': call(n_el, n_loc, ld, first_node, transposed, out, n_terms=3, mats=(2, 0, 1)),
        'explicit values': call(n_el, n_loc, ld, first_node, transposed, out, pattern=explicit),
        'odd ld': call(n_el, n_loc, 9, first_node, transposed, out),
        'ld < n_loc': call(n_el, n_loc, 8, first_node, transposed, out),
        'first_node = 1': call(n_el - 2, n_loc, ld, 1, transposed, out),
        'first_node + n_el > n_loc': call(n_el, n_loc, ld, 0, transposed, out),
        'x aliases y': call(n_el, n_loc, ld, first_node, transposed, out, x=_lib.ptr(out)),
        'x off by 8 bytes': call(n_el, n_loc, ld, first_node, transposed, out, x=_lib.ptr(spare_x) + 8),
        'mat >= n_mats': call(n_el, n_loc, ld, first_node, transposed, out, mats=(2, 3)),
    }
    if not transposed:
        cases['a ghost and no ghosts'] = call(n_el, n_loc, ld, first_node, transposed, out, ghosts=None)
    for name, refused in cases.items():
        _refused(refused, out, (who,))
    _refused(call(n_el, n_loc, ld, first_node, transposed, spare_y, y=_lib.ptr(spare_y) + 8), spare_y, (who,))
