"""What tests/test_multigrid_kernels_gpu.py measures the multigrid kernels (csrc/rows_ell.hip,
csrc/mg.hip, csrc/mg_coarse.hip) with, and a check of that yardstick where there is no GPU.

The three primitives are restated in np.longdouble; each carries a pair (value, entrywise
error bound) through the computation.  Vectors are (rows, T) arrays, one column per time
slice; slices never interact, so every column is a problem of its own.

    SPMM    y = alpha A(t) x + beta z,            a(t) = ca va + cm[t] vm
    GS      one sweep in dof order, row by row:   u_i = (f_i - sum_{j != i} a_ij u_j) / a_ii
            (diag_free = 1), or the reference's   u_i += (f_i - row_i u) / a_ii  (diag_free = 0)
    COARSE  u = Inv[kind[t]] f scale

On top of them MGM(j, u, f) and `vcycles` cycles from zero (reference multigrid.py:168-182,
oracle/multigrid.py:137-150), the restricted residual either as R (A u - f) or as
(R A) u - R f, level by level.

Data.  The level matrices, the Galerkin products, the products R A, the member matrices and
the dense inverses are DATA, taken as the plan holds them (`Hierarchy` forms them the way the
plan does: SciPy's `R @ A @ P`, rounding-noise entries dropped; the inverse is handed over by
the caller).  Only the operation on them is restated: the conditioning of an inverse or of a
Galerkin chain does not enter the bound.

Bound.  U = 2^-53, gamma_k = k U / (1 - k U).  A float64 evaluation of one output entry is a
sum of terms, each of which passes through at most k factors (1 + d), |d| <= U, so
|fl(op(v)) - op(v)| <= gamma_k |op| |v| entry by entry, whatever the order of the sum, where
|op| is the operation with every coefficient replaced by its magnitude.  The kernel applies
the operation to its own rounded inputs, |v^ - v| <= e_in, hence

    e_out = |op| e_in + gamma_k |op| (|v| + e_in).

k is counted from the kernels' own arithmetic (rows_ell.hip:194-223, mg_coarse.hip:96-133,
mg.hip:64-78, 92-95):

  * an entry a(t):  ca * va is one rounding (none for ca = 1), fma(cm, vm, .) one more   -> ka
    (relative to w = |ca va| + |cm vm|, which is |a(t)| unless the two parts cancel: the
    rounding terms carry w in place of |a(t)|, the diagonal of a sweep the factor w / |a_ii|)
  * the sum of a row: one fused multiply-add per slot that holds an entry (an appended
    or padding slot is fma(0, x, s) = s, exact)                                           -> nnz
  * SPMM: the product with alpha (exact for |alpha| = 1) and fma(beta, z, .)              -> 2
    k_SPMM = nnz + ka + [|alpha| != 1] + [beta != 0]
  * GS, diagonal-free rows: the diagonal a_ii(t) like any entry (ka), the reciprocal, the
    subtraction f - s and the product                                                     -> 3
    k_GS = (nnz - 1) + 2 ka + 3;  with the diagonal among the slots one slot and the
    final addition more: k_GS' = nnz + 2 ka + 4.  (The exact update does not depend on
    the old u_i, so e_in of u_i itself does not enter |op| e_in; its magnitude does
    enter the rounding term.)
  * COARSE: n_0 fused multiply-adds for the dense row, the product with scale (none for
    scale = 1)                                                                            -> n_0 + 1
  * with member matrices the entries are read, not computed: ka = 0.

The longdouble restatement rounds too: REF_ULPS * k * 2^-64 is added to gamma_k (the same
count with the unit roundoff of the 64-bit significand, twice over).  The count is derived,
not measured; the check used everywhere is |got - ref| <= bound on EVERY entry, and a zero
bound admits no error (`ratio`).

Inputs are signed; time slice t is scaled by a power of ten spread over twelve decades
across the columns, so a value that lands in the wrong column is far outside the bound.  So
that the bound says something, every catalogue case satisfies, column by column,
max(bound) <= 1e-10 max|u_ref| (the project's own per-operator parity figure): the mesh
matrices are M-matrix-like, the algebraic ones strictly diagonally dominant.  That is a
condition on the inputs, asserted below for the whole catalogue.

The float64 oracle (oracle.multigrid.Smoother, MultiGrid) and the stored goldens sit inside
the bound; a restatement with one thing wrong -- a slot's column from the neighbouring slice,
cm[t0] for t0 + 1, a group's rows swept too early, beta dropped, the neighbour's kind --
leaves it."""
import collections
import functools
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import csr_from, load_golden
from test_lu_reference_host import LD, U, gamma
from test_wavelet_reference_host import ratio, unchecked_ratio  # noqa: F401  (re-exported to the GPU tests)

REF_ULPS = 2
SLOTS = (2, 4, 5, 6, 7, 9, 12, 16, 20)  # instantiated slot counts of the row engine
PARITY = 1e-10                          # bound <= PARITY * max|u_ref| per column
WRONG = ('slot-from-neighbour-slice', 'cm-of-t0-for-t0+1', 'group-swept-too-early', 'beta-dropped',
         'kind-of-neighbour-slice')


def g(k):
    """gamma_k plus the restatement's own rounding, for a count or an array of counts."""
    k = np.asarray(k, dtype=LD)
    return k * LD(U) / (LD(1) - k * LD(U)) + LD(REF_ULPS) * k * LD(2)**-64


def test_gamma_is_the_shared_one():
    assert g(7) - gamma(7) == LD(REF_ULPS * 7) * LD(2)**-64 and np.finfo(LD).eps < 2e-19


# ---- matrices as padded rows ------------------------------------------------------------------
def _sorted_csr(m):
    m = sp.csr_matrix(m).copy()
    m.sum_duplicates()
    m.sort_indices()
    return m


class Rows:
    """A (and optionally M) on their union pattern, row by row in CSR order, padded to the
    longest row: idx[n, K], va / vm[n, K] (zero in the padding), nnz[n], dpos[n] = slot of the
    diagonal entry (-1: none)."""
    def __init__(self, A, M=None):
        A = _sorted_csr(A)
        n, m = A.shape
        if M is not None:
            M = _sorted_csr(M)
            pat = _sorted_csr(sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape) +
                              sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=A.shape))
        else:
            pat = A
        self.shape, self.indptr, self.indices = (n, m), pat.indptr.copy(), pat.indices.copy()
        self.nnz = np.diff(pat.indptr).astype(np.int64)
        K = self.K = max(int(self.nnz.max()) if n else 1, 1)
        row_of = np.repeat(np.arange(n), self.nnz)
        slot = np.arange(pat.nnz) - pat.indptr[row_of]
        key = row_of.astype(np.int64) * m + pat.indices

        self._key, self._row_of, self._slot = key, row_of, slot
        self.idx = np.zeros((n, K), dtype=np.int64)
        self.idx[row_of, slot] = pat.indices
        self.va = self.lay(A)
        self.vm = self.lay(M) if M is not None else None
        self.dpos = np.full(n, -1, dtype=np.int64)
        d = pat.indices == row_of
        self.dpos[row_of[d]] = slot[d]

    def lay(self, B, strict=True):
        """The entries of B at the slots of this pattern (zero where B has none); entries of B
        outside the pattern are an error, or ignored (strict = False: member matrices)."""
        B = _sorted_csr(B)
        out = np.zeros((self.shape[0], self.K))
        r = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr)).astype(np.int64)
        want = r * self.shape[1] + B.indices
        at = np.minimum(np.searchsorted(self._key, want), len(self._key) - 1)
        hit = self._key[at] == want
        assert not strict or hit.all()
        out[self._row_of[at[hit]], self._slot[at[hit]]] = B.data[hit]
        return out

    def values(self, ca, cm=None, wrong=None):
        """(Vals(v, w), ka): v[n, K, T or 1] the entries a(t) in longdouble, w = |ca va| + |cm vm| the
        magnitude their roundings are relative to (w = |v| unless the two parts cancel)."""
        v = LD(ca) * self.va.astype(LD)[:, :, None]
        w = np.abs(v)
        ka = int(ca != 1.0)
        if cm is not None:
            assert self.vm is not None
            c = np.array(cm, dtype=LD)
            if wrong == 'cm-of-t0-for-t0+1':
                c[1::2] = c[0:len(c) - 1:2]
            part = c[None, None, :] * self.vm.astype(LD)[:, :, None]
            v, w = v + part, w + np.abs(part)
            ka += 1
        return Vals(v, w), ka

    def member_values(self, members, kind):
        """Entries of matrix kind[t] itself on this pattern (zero where it has none): read, not
        computed (ka = 0)."""
        per_kind = {k: self.lay(members[k], strict=False) for k in set(int(q) for q in kind)}
        v = np.stack([per_kind[int(k)] for k in kind], axis=2).astype(LD)
        return Vals(v, np.abs(v)), 0


Vals = collections.namedtuple('Vals', 'v w')


def slot_count(width):
    """The row engine's slot count for a longest row of `width` entries (0: no ELL copy)."""
    return next((s for s in SLOTS if s >= max(int(width), 1)), 0)


# ---- the three primitives ---------------------------------------------------------------------
def spmm(rows, V, ka, x, alpha=1.0, beta=0.0, z=None, wrong=None):
    """(y, e) of y = alpha A(t) x + beta z for x = (value, bound), z = (value, bound) or None."""
    xv, xe = x
    G, Ge = xv[rows.idx], xe[rows.idx]
    if wrong == 'slot-from-neighbour-slice':
        r = int(np.argmax(rows.nnz))
        T = xv.shape[1]
        swap = np.arange(T) ^ 1
        swap[swap >= T] = T - 1
        G = G.copy()
        G[r, 0, :] = xv[rows.idx[r, 0], swap]
    V, W = V
    s, lin, mag = (V * G).sum(1), (np.abs(V) * Ge).sum(1), (W * (np.abs(G) + Ge)).sum(1)
    a, b = LD(alpha), LD(beta)
    k = rows.nnz + ka + int(abs(alpha) != 1.0) + int(beta != 0.0)
    y, e, m = a * s, abs(a) * lin, abs(a) * mag
    if beta != 0.0 and wrong != 'beta-dropped':
        zv, ze = z
        y, e, m = y + b * zv, e + abs(b) * ze, m + abs(b) * (np.abs(zv) + ze)
    return y, e + g(k)[:, None] * m


def dof_order(n, backward):
    """The sequential sweep: one row per step."""
    order = range(n - 1, -1, -1) if backward else range(n)
    return [np.array([i]) for i in order]


def depth_groups(rows, backward):
    """Rows by depth in the dependency DAG of the sweep in dof order (mg.hip:7-15): a row waits
    for its neighbours j < i (j > i backwards).  Rows of one group are independent, so sweeping
    group after group performs the sequential sweep's updates on the same operands."""
    n = rows.shape[0]
    depth = np.zeros(n, dtype=np.int64)
    for i in (range(n - 1, -1, -1) if backward else range(n)):
        c = rows.indices[rows.indptr[i]:rows.indptr[i + 1]]
        c = c[c > i] if backward else c[c < i]
        if len(c):
            depth[i] = depth[c].max() + 1
    return [np.flatnonzero(depth == d) for d in range(int(depth.max()) + 1 if n else 0)]


def gs_sweep(rows, V, ka, u, f, batches, diag_free):
    """One Gauss-Seidel sweep over `batches` (lists of rows, in order), in place on u = (value,
    bound): dof_order() is the definition, depth_groups() the same sweep with fewer steps."""
    uv, ue = u
    fv, fe = f
    K = rows.K
    for b in batches:
        Vb, Wb, ib, dp = V.v[b], V.w[b], rows.idx[b], rows.dpos[b]
        assert np.all(dp >= 0)
        off = (np.arange(K)[None, :] != dp[:, None])[:, :, None]
        Dv = Vb[np.arange(len(b)), dp]
        D = np.abs(Dv)
        # the diagonal as computed is off by gamma_ka w_ii, relative to |a_ii| that is rho times more
        rho = Wb[np.arange(len(b)), dp] / D
        G, Ge = uv[ib], ue[ib]
        lin = (np.where(off, np.abs(Vb), 0) * Ge).sum(1)
        if diag_free:
            s = (np.where(off, Vb, 0) * G).sum(1)
            mag = (np.where(off, Wb, 0) * (np.abs(G) + Ge)).sum(1)
            val = (fv[b] - s) / Dv
            k = (rows.nnz[b] - 1) + 2 * ka + 3
            err = (fe[b] + lin) / D + (g(k)[:, None] + g(ka) * (rho - 1)) * ((np.abs(fv[b]) + fe[b] + mag) / D)
        else:
            s = (Vb * G).sum(1)
            mag = (Wb * (np.abs(G) + Ge)).sum(1)
            val = uv[b] + (fv[b] - s) / Dv
            k = rows.nnz[b] + 2 * ka + 4
            err = (fe[b] + lin) / D + (g(k)[:, None] + g(ka) * (rho - 1)) * (
                np.abs(uv[b]) + ue[b] + (np.abs(fv[b]) + fe[b] + mag) / D)
        uv[b], ue[b] = val, err


def coarse_solve(inv, kind, f, scale=1.0, wrong=None):
    """(u, e) of u = Inv[kind[t]] f scale; inv[n_kinds, n0, n0], kind[T] or None (kind 0)."""
    fv, fe = f
    n0, T = fv.shape
    kind = np.zeros(T, dtype=np.int64) if kind is None else np.asarray(kind, dtype=np.int64).copy()
    if wrong == 'kind-of-neighbour-slice':
        swap = np.arange(T) ^ 1
        swap[swap >= T] = T - 1
        kind = kind[swap]
    A = np.asarray(inv, dtype=np.float64).astype(LD)[kind]  # [T, n0, n0]
    s = LD(scale)
    uv = s * np.einsum('tic,ct->it', A, fv)
    k = n0 + int(scale != 1.0)
    aA = np.abs(A)
    e = abs(s) * np.einsum('tic,ct->it', aA, fe) + g(k) * abs(s) * np.einsum('tic,ct->it', aA, np.abs(fv) + fe)
    return uv, e


def smooth(rows, V, ka, u, f, its, backward, diag_free, order='groups'):
    """`its` sweeps, the value and bound of u returned as new arrays."""
    u = (np.array(u[0], dtype=LD), np.array(u[1], dtype=LD))
    batches = depth_groups(rows, backward) if order == 'groups' else (
        dof_order(rows.shape[0], backward) if order == 'dof' else order)
    for _ in range(its):
        gs_sweep(rows, V, ka, u, f, batches, diag_free)
    return u


# ---- a hierarchy as the plan holds it ---------------------------------------------------------
def drop_roundoff(mat, rel=1e-14):
    mat = _sorted_csr(mat)
    if mat.nnz:
        mat.data[np.abs(mat.data) < rel * np.abs(mat.data).max()] = 0.0
        mat.eliminate_zeros()
    return mat


class Hierarchy:
    """Level matrices A_j (and M_j), transfers and products R A_j as stk_mg_create_from_csr forms
    them (mg_build.hip:526-546, 612-623): SciPy's `R @ A @ P`, rounding noise dropped.  Level J is
    the finest; P[j] prolongs level j to j + 1."""
    def __init__(self, A, M, P_mats, name=''):
        self.name = name
        self.J = J = len(P_mats)
        self.P = [_sorted_csr(P) for P in P_mats]
        self.R = [_sorted_csr(P.T.tocsr()) for P in self.P]
        self.A, self.M = [None] * (J + 1), [None] * (J + 1)
        self.A[J] = _sorted_csr(A)
        self.has_m = M is not None
        if self.has_m:
            self.M[J] = _sorted_csr(M)
        for j in range(J - 1, -1, -1):
            self.A[j] = drop_roundoff(self.R[j] @ self.A[j + 1] @ self.P[j])
            if self.has_m:
                self.M[j] = drop_roundoff(self.R[j] @ self.M[j + 1] @ self.P[j])
        self.n = [a.shape[0] for a in self.A]
        self.rows = [Rows(self.A[j], self.M[j]) for j in range(J + 1)]
        self.p_rows = [None] + [Rows(self.P[j - 1]) for j in range(1, J + 1)]
        self.r_rows = [None] + [Rows(self.R[j - 1]) for j in range(1, J + 1)]
        self.ra_rows = [None] + [
            Rows(drop_roundoff(self.R[j - 1] @ self.A[j]),
                 drop_roundoff(self.R[j - 1] @ self.M[j]) if self.has_m else None) for j in range(1, J + 1)
        ]
        self.groups = [None] + [(depth_groups(self.rows[j], False), depth_groups(self.rows[j], True))
                                for j in range(1, J + 1)]

    def dense0(self, ca=1.0, cm=None):
        """The level-0 matrix the plan inverts for kind 0 (cm None) or for a coefficient."""
        a0 = self.A[0].toarray()
        return a0 if cm is None else ca * a0 + cm * self.M[0].toarray()

    def member_chain(self, ca, cm):
        """Galerkin chain of the ASSEMBLED matrix cm M + ca A (reference heateq_mpi.py:97-98): the
        member matrices a family hands to the coarse end."""
        C = [None] * (self.J + 1)
        C[self.J] = _sorted_csr(cm * self.M[self.J] + ca * self.A[self.J])
        for j in range(self.J - 1, -1, -1):
            C[j] = drop_roundoff(self.R[j] @ C[j + 1] @ self.P[j])
        return C


def vcycles(H, F, inv, smoothsteps=2, n_cycles=1, ca=1.0, cm=None, kind=None, fused_restrict=lambda j: False,
            diag_free=lambda j: True, members=None, member_levels=0, order='groups', wrong=None):
    """(u, e) after `n_cycles` V-cycles from zero on the right-hand side F[n_J, T] (float64,
    exact).  fused_restrict(j): the restricted residual of level j as (R A) u - R f instead of
    R (A u - f).  members[k][j]: member matrices of kind k, used on levels 1..member_levels."""
    T = F.shape[1]
    zero = lambda n: (np.zeros((n, T), dtype=LD), np.zeros((n, T), dtype=LD))
    cache = {}

    def level_values(j):
        if j not in cache:
            if members is not None and cm is not None and 1 <= j <= member_levels:
                kk = np.asarray(kind).copy()
                if wrong == 'kind-of-neighbour-slice':
                    swap = np.arange(T) ^ 1
                    swap[swap >= T] = T - 1
                    kk = kk[swap]
                cache[j] = H.rows[j].member_values({k: members[k][j] for k in set(int(q) for q in kk)}, kk)
            else:
                cache[j] = H.rows[j].values(ca, cm, wrong)
        return cache[j]

    def batches(j, backward):
        if order == 'dof':
            return dof_order(H.n[j], backward)
        grp = list(H.groups[j][1 if backward else 0])
        if wrong == 'group-swept-too-early' and j == H.J and not backward and len(grp) > 1:
            grp[0], grp[1] = grp[1], grp[0]
        return grp

    def mgm(j, u, f):
        if j == 0:
            return coarse_solve(inv, kind if cm is not None else None, f,
                                1.0 if cm is not None else float(np.float64(1.0) / np.float64(ca)), wrong)
        V, ka = level_values(j)
        for _ in range(smoothsteps):
            gs_sweep(H.rows[j], V, ka, u, f, batches(j, False), diag_free(j))
        if fused_restrict(j):
            Vra, kra = H.ra_rows[j].values(ca, cm, wrong)
            d = spmm(H.r_rows[j], *H.r_rows[j].values(1.0), f)
            d = spmm(H.ra_rows[j], Vra, kra, u, 1.0, -1.0, d, wrong=wrong if j == H.J else None)
        else:
            r = spmm(H.rows[j], V, ka, u, 1.0, -1.0, f, wrong=wrong if j == H.J else None)
            d = spmm(H.r_rows[j], *H.r_rows[j].values(1.0), r)
        u_c = mgm(j - 1, zero(H.n[j - 1]), d)
        u = spmm(H.p_rows[j], *H.p_rows[j].values(1.0), u_c, -1.0, 1.0, u,
                 wrong=wrong if (wrong == 'beta-dropped' and j == H.J) else None)
        u = (u[0].copy(), u[1].copy())
        for _ in range(smoothsteps):
            gs_sweep(H.rows[j], V, ka, u, f, batches(j, True), diag_free(j))
        return u

    f = (np.asarray(F, dtype=np.float64).astype(LD), np.zeros(F.shape, dtype=LD))
    u = zero(H.n[H.J])
    for _ in range(n_cycles):
        u = mgm(H.J, u, f)
    return u


# ---- the launch rules, restated (mg.hip:462-471, mg_coarse.hip:651-662, 931-1051) ---------------
LDS_ARENA = 144 * 1024
COARSE_MAX_ROWS = 4096
CJOB_BYTES = 48


def plan_shape(H, smoothsteps, gs_key=1):
    """What the plan's construction decides, from the matrices alone: per level the slot counts of
    its ELL copies (0: none), the cut level Lc of the fused coarse end (-1: none), the arena rows,
    the number of jobs and the slot count KU of the uniform form (0: none)."""
    J = H.J
    lev = [None]
    for j in range(1, J + 1):
        w = int(H.rows[j].nnz.max())
        full_rows = gs_key == 0 or (gs_key == 2 and j == J)
        k = dict(a=slot_count(w), gs=slot_count(w if full_rows else w - 1), p=slot_count(H.p_rows[j].nnz.max()),
                 r=slot_count(H.r_rows[j].nnz.max()), ra=slot_count(H.ra_rows[j].nnz.max()))
        k['ell'] = all(k[q] for q in ('a', 'gs', 'p', 'r'))
        k['diag_free'] = not full_rows
        k['n_fwd'], k['n_bwd'] = len(H.groups[j][0]), len(H.groups[j][1])
        lev.append(k)
    Lc, arena = -1, 3 * H.n[0]
    for j in range(1, J):
        arena += 3 * H.n[j]
        if H.n[j] > COARSE_MAX_ROWS or arena * 8 > LDS_ARENA or not lev[j]['ell']:
            break
        Lc = j
    Lc = Lc if Lc >= 1 else -1
    out = dict(levels=lev, Lc=Lc, lds_rows=0, n_jobs=0, KU=0, has_m=H.has_m)
    if Lc >= 1:
        out['lds_rows'] = 3 * sum(H.n[:Lc + 1])
        out['n_jobs'] = 1 + sum(smoothsteps * (lev[j]['n_fwd'] + lev[j]['n_bwd']) + 3 + (1 if j >= 2 else 0)
                                for j in range(1, Lc + 1))
        kmax = max(max(lev[j][q] for q in ('a', 'gs', 'p', 'r')) for j in range(1, Lc + 1))
        out['KU'] = 8 if kmax <= 8 else (12 if kmax <= 12 else 0)
    return out


def coarse_path(shape, ld, with_cm, fuse_coarse=1, coarse_lds=1, uniform=1):
    """The kernel stk_coarse_plan_run launches for the coarse end, as a tuple:
    ('levels',) | ('global', has_m) | ('lds', has_m, pair) | ('uniform', KU, key2, has_m, pair, threads)."""
    if not fuse_coarse or shape['Lc'] < 1 or ld & 1:
        return ('levels',)
    rows = shape['lds_rows']
    if not coarse_lds or 8 * rows > LDS_ARENA:
        return ('global', bool(with_cm))
    pair = 16 * rows <= LDS_ARENA
    lds = (16 if pair else 8) * rows
    if uniform and shape['KU'] and (not with_cm or shape['has_m']):
        lds_u = lds + (0 if pair else 8 * (rows & 1)) + CJOB_BYTES * shape['n_jobs']
        if lds_u <= 160 * 1024 - 512:
            KU = shape['KU']
            key2 = (uniform == 2) if KU == 8 else None
            threads = 1024 if (KU == 8 and uniform != 2 and not with_cm and not pair) else 512
            return ('uniform', KU, key2, bool(with_cm), pair, threads)
    return ('lds', bool(with_cm), pair)


UNIFORM_SITES = {('uniform', KU, key2, has_m, pair, 1024 if (KU == 8 and not key2 and not has_m and not pair) else 512)
                 for KU, keys in ((8, (True, False)), (12, (None,))) for key2 in keys
                 for has_m in (False, True) for pair in (False, True)}
LDS_SITES = {('lds', has_m, pair) for has_m in (False, True) for pair in (False, True)}
GLOBAL_SITES = {('global', False), ('global', True)}


def rows_launch(n_loc, K):
    """(P, R, NPF) of stk_rows_ell_launch (rows_ell.hip:480-482, 406-412)."""
    P = (n_loc + 1) // 2
    R = 512 // P
    if R * K > 2048:
        R = 2048 // K
    npf = -(-R * K // 512)
    return P, R, 1 if npf <= 1 else (2 if npf <= 2 else 4)


# ---- inputs -----------------------------------------------------------------------------------
def column_scales(T):
    """Powers of ten spread over twelve decades across the columns (T = 1: one)."""
    return 10.0**(np.linspace(-6.0, 6.0, T) if T > 1 else np.zeros(1))


def signed_input(n, T, seed):
    rng = np.random.RandomState(seed)
    return (rng.uniform(0.25, 1.0, size=(n, T)) * rng.choice([-1.0, 1.0], size=(n, T))) * column_scales(T)


# Off-diagonal entries are negative and the diagonal only just dominates: the Galerkin products
# then stay weakly dominant too and the coarse levels carry a visible part of the result (with
# entries of random sign they cancel, the coarse matrices come out almost diagonal, and a wrong
# coarse solve changes the V-cycle by less than the bound).
DOMINANCE = 1.25  # diagonal over the sum of the row's other magnitudes


def shifted_matrix(n, shifts, seed, extra=None, boundary=0):
    """Strictly diagonally dominant, M-matrix-like, symmetric in its pattern but not in its values: row i couples to (i +- s) mod n for the
    given shifts -- few dependency groups however large n -- plus `extra` = {row: columns}, plus,
    for boundary = b > 0, i <-> i + 1 wherever the two lie in different ones of b contiguous
    aggregates (the level of b rows is then a chain, while this one stays shallow)."""
    rng = np.random.RandomState(seed)
    cols = [set() for _ in range(n)]
    for i in range(n):
        for s in shifts:
            cols[i].update(((i + s) % n, (i - s) % n))
        if boundary and i + 1 < n and (i * boundary) // n != ((i + 1) * boundary) // n:
            cols[i].add(i + 1)
            cols[i + 1].add(i)
    for i, cs in (extra or {}).items():
        for c in cs:  # (both ways: the sweeps' schedule takes a structurally symmetric pattern)
            cols[i].add(int(c))
            cols[int(c)].add(i)
    r, c, v = [], [], []
    for i in range(n):
        cs = sorted(cols[i] - {i})
        vals = -rng.uniform(0.25, 1.0, len(cs))
        r += [i] * (len(cs) + 1)
        c += cs + [i]
        v += list(vals) + [DOMINANCE * np.abs(vals).sum() + rng.uniform(0.1, 0.2)]
    return _sorted_csr(sp.csr_matrix((v, (r, c)), shape=(n, n)))


def aggregation(nf, nc, seed, second=7):
    """Aggregation-type prolongation: fine dof i belongs to the contiguous aggregate
    floor(i nc / nf) with weight 1; every `second`-th dof also to the next one, lightly."""
    rng = np.random.RandomState(seed)
    par = (np.arange(nf) * nc) // nf
    r, c, v = list(range(nf)), list(par), [1.0] * nf
    if second:
        for i in range(0, nf, second):
            if nc > 1:
                r.append(i)
                c.append(int((par[i] + 1) % nc))
                v.append(float(rng.uniform(0.05, 0.25)))
    return _sorted_csr(sp.csr_matrix((v, (r, c)), shape=(nf, nc)))


def mass_like(A, seed):
    """A second matrix on (nearly) the pattern of A: diagonally dominant, positive diagonal."""
    rng = np.random.RandomState(seed)
    A = _sorted_csr(A)
    M = A.copy()
    M.data = rng.uniform(0.05, 0.2, A.nnz) * rng.choice([-1.0, 1.0], A.nnz)
    M = sp.lil_matrix(M)
    M.setdiag(np.asarray(abs(sp.csr_matrix(M)).sum(axis=1)).ravel() + rng.uniform(0.5, 1.0, A.shape[0]))
    return _sorted_csr(M.tocsr())


# name: level sizes coarse -> fine and how the finest matrix is made.  Shifts n // 2 and n // 3 with
# pure aggregation keep every level at 7 slots or fewer (KU = 8); the shift n // 2 alone with a
# second parent for every 7th dof gives rows of 8 and 9 entries below the top (KU = 12).
KU12 = dict(shifts=(2,), second=7)
ALGEBRAIC = {
    # arena sum_{j <= Lc} n_j on each side of the double2 limit 3072 ...
    'arena-3072': dict(sizes=(32, 160, 640, 2240, 3400), family=True),
    'arena-3073': dict(sizes=(32, 160, 640, 2241, 3400), family=True),
    'arena-3073-ku12': dict(sizes=(32, 160, 640, 2241, 3400), family=True, **KU12),
    # ... and of the plan's own 144 KiB rule, 6144: the cut level drops by one
    'arena-6144': dict(sizes=(24, 120, 480, 1424, 4096, 4100)),
    'arena-6145': dict(sizes=(24, 120, 480, 1425, 4096, 4100)),
    # COARSE_MAX_ROWS
    'rows-4096': dict(sizes=(16, 80, 400, 1500, 4096, 4100), family=True),
    'rows-4097': dict(sizes=(16, 80, 400, 1500, 4097, 4100)),
    # enough jobs that the descriptors no longer fit beside the arena: levels 1 and 2 are chains
    'jobs-s1': dict(sizes=(12, 60, 300, 1200, 2800), chain_level=2, smoothsteps=1),
    'jobs-s3': dict(sizes=(12, 60, 300, 1200, 2800), chain_level=2, smoothsteps=3),
    # longest row of the fused levels: 7, 8, 9, 12, 13 entries
    'width-7': dict(sizes=(23, 90, 180), width=7, family=True),
    'width-8': dict(sizes=(23, 90, 180), width=8),
    'width-9': dict(sizes=(23, 90, 180), width=9),
    'width-12': dict(sizes=(23, 90, 180), width=12, family=True),
    'width-13': dict(sizes=(23, 90, 180), width=13),
    # a level with a row above 20 slots: no ELL copy there, the fused end stops below it
    'row-26': dict(sizes=(8, 20, 200, 300), wide_level_2=26),
    # nothing to fuse: no level between the ends, or one whose restriction has rows of 30 entries
    'two-level': dict(sizes=(5, 40)),
    'three-level': dict(sizes=(2, 60, 240)),
    # small and deep: three sweeps, two cycles
    'small-s3-v2': dict(sizes=(4, 17, 70, 150), smoothsteps=3, vcycles=2, family=True, **KU12),
}


@functools.lru_cache(maxsize=None)
def algebraic(name):
    """(A, M or None, P_mats, smoothsteps, vcycles) of a catalogue entry."""
    spec = ALGEBRAIC[name]
    sizes = spec['sizes']
    n, seed = sizes[-1], 1 + sorted(ALGEBRAIC).index(name)
    shifts = tuple(n // q for q in spec.get('shifts', (2, 3)))
    second = spec.get('second', 0)
    P_mats = [aggregation(b, a, seed + 10 * i, second=second) for i, (a, b) in enumerate(zip(sizes, sizes[1:]))]
    extra = {}
    if 'width' in spec:
        # level J-1 gets a row of exactly `width` entries: fine row 0 couples to one dof of each of
        # enough aggregates that its row of the Galerkin product does not reach yet
        base = Hierarchy(shifted_matrix(n, shifts, seed), None, P_mats)
        below = base.rows[base.J - 1]
        have = set(int(c) for c in base.A[base.J - 1][0].indices)
        # (the mirrored entry makes the partner's row one longer: row 0 stays the longest)
        want = [c for c in range(2, sizes[-2] - 2) if c not in have and below.nnz[c] + 1 < spec['width']]
        want = want[:spec['width'] - len(have)]
        assert len(want) == spec['width'] - len(have)
        extra = {0: [int(np.ceil(c * n / sizes[-2])) for c in want]}
    if 'wide_level_2' in spec:
        # level 2 of (n0, n1, n2, n3): row 0 with 26 more entries, inside three aggregates of level 1
        extra = {0: [int(np.ceil(c * n / sizes[2])) for c in range(10, 10 + spec['wide_level_2'])]}
    A = shifted_matrix(n, shifts, seed, extra, boundary=sizes[spec['chain_level']] if 'chain_level' in spec else 0)
    M = mass_like(A, seed + 5) if spec.get('family') else None
    return A, M, tuple(P_mats), spec.get('smoothsteps', 1), spec.get('vcycles', 1)


@functools.lru_cache(maxsize=None)
def algebraic_hierarchy(name):
    A, M, P_mats, _, _ = algebraic(name)
    return Hierarchy(A, M, list(P_mats), name)


@functools.lru_cache(maxsize=None)
def mesh_problem(problem, J_space):
    """(A_x, M_x, P_mats, coords) of a mesh problem of the package."""
    from source.assembly import prolongation_matrices, space_matrices
    from source.multigrid import MeshHierarchy
    from source.problem import problem_helper
    mesh = problem_helper(problem, J_space=J_space, J_time=2)[0]
    M_x, A_x = space_matrices(mesh)
    coords = np.ascontiguousarray(MeshHierarchy(mesh).coords, dtype=np.float64)
    return _sorted_csr(A_x), _sorted_csr(M_x), tuple(_sorted_csr(P) for P in prolongation_matrices(mesh)), coords


MESHES = (('square', 5), ('lshape', 4), ('cube', 2))


@functools.lru_cache(maxsize=None)
def mesh_hierarchy(problem, J_space, family=True):
    A, M, P_mats, _ = mesh_problem(problem, J_space)
    return Hierarchy(A, M if family else None, list(P_mats), '%s-%d' % (problem, J_space))


def chain_matrix(n=150, seed=3):
    """Tridiagonal: every row its own dependency group."""
    return shifted_matrix(n, (1,), seed)


def wide_group_matrix(n=600, seed=4):
    """i <-> i + n/2 only: two groups of n/2 rows each."""
    return shifted_matrix(n, (n // 2,), seed)


FAMILY_CA, FAMILY_CMS = 0.3, (1.0, 2.0, 4.0, 8.0)
T_MAX = 9  # columns of every V-cycle case; a shorter slab takes the first columns


def family_slices(T=T_MAX, scale=1.0):
    """(cms, cm[T], kind[T]): kind 1 + k is the coarse inverse of ca A_0 + cms[k] M_0.  Every slice
    has its own coefficient and the two slices of a pair never name the same kind; the last
    kind is named by no slice."""
    n = T + 1
    cms = np.array([FAMILY_CMS[t % len(FAMILY_CMS)] * (1.0 + t / 64.0) for t in range(n)]) * scale
    member = np.array([(4 * t) % T if T % 2 else t for t in range(T)])
    assert len(set(member)) == T
    return cms, cms[member], (member + 1).astype(np.int32)


def mesh_mass_scale(H):
    """P1 mass entries are h^2 times the stiffness entries: the family's coefficients are scaled
    so that both parts count (and the sum is diagonally dominant: the bound stays informative)."""
    return float(2.0**np.round(np.log2(0.3 * H.A[H.J].diagonal().mean() / H.M[H.J].diagonal().mean())))


def numpy_inverses(H, ca=1.0, cms=()):
    """The dense inverses a plan holds when numpy.linalg.inv is handed over: kind 0 = A_0, kind
    1 + k = ca A_0 + cms[k] M_0."""
    return np.stack([np.linalg.inv(H.dense0())] + [np.linalg.inv(H.dense0(ca, c)) for c in cms])


def case_hierarchy(kind_of, name):
    return algebraic_hierarchy(name) if kind_of == 'algebraic' else mesh_hierarchy(*name)


def case_family(kind_of, name):
    """(ca, cms, cm[T_MAX], kind[T_MAX]) of a catalogue family."""
    scale = 1.0 if kind_of == 'algebraic' else mesh_mass_scale(mesh_hierarchy(*name))
    return (FAMILY_CA,) + family_slices(T_MAX, scale)


@functools.lru_cache(maxsize=None)
def vcycle_case(kind_of, name, restrict, gs_key=1, with_cm=False, smoothsteps=None, n_cycles=None, wrong=None):
    """(F, u_ref, bound) of a catalogue hierarchy: kind_of 'algebraic' | 'mesh' (name = (problem, J)).
    restrict: 'two-step' (R (A u - f) on every level), 'fused' ((R A) u - R f on every level
    that has the product) or 'above-Lc' (fused above the coarse end, two steps inside it: what
    the job list runs).  The inverses are numpy.linalg.inv's of the plan's level-0 matrices,
    exactly what the GPU tests hand to the plan."""
    if kind_of == 'algebraic':
        H = algebraic_hierarchy(name)
        _, _, _, ss, vc = algebraic(name)
    else:
        H = mesh_hierarchy(*name)
        ss, vc = 2, 1
    ss = smoothsteps or ss
    vc = n_cycles or vc
    shape = plan_shape(H, ss, gs_key)
    F = signed_input(H.n[H.J], T_MAX, seed=zlib.crc32(str(name).encode()) % 1000 + 17)
    ca, cms, cm, kind = case_family(kind_of, name) if with_cm else (1.0, (), None, None)
    inv = numpy_inverses(H, ca, cms)
    fused = {'two-step': lambda j: False, 'fused': lambda j: shape['levels'][j]['ell'] and shape['levels'][j]['ra'] > 0,
             'above-Lc': lambda j: j > shape['Lc'] and shape['levels'][j]['ell'] and shape['levels'][j]['ra'] > 0}[restrict]
    u, e = vcycles(H, F, inv, ss, vc, ca, cm, kind, fused, lambda j: shape['levels'][j]['diag_free'], wrong=wrong)
    for a in (F, u, e):
        a.setflags(write=False)
    return F, u, e


def bound_is_informative(u, e):
    """max(bound) <= PARITY max|u_ref|, column by column."""
    return bool(np.all(e.max(axis=0) <= LD(PARITY) * np.abs(u).max(axis=0)))


# ---- smoother and member cases --------------------------------------------------------------------
SWEEP_MATRICES = ('square', 'lshape', 'cube', 'chain', 'wide-group')


@functools.lru_cache(maxsize=None)
def sweep_problem(name):
    """(H, A, M, P_mats, coords, slab lengths): the finest level of H is the matrix swept."""
    if name in ('chain', 'wide-group'):
        A = chain_matrix() if name == 'chain' else wide_group_matrix()
        M = mass_like(A, 21)
        P_mats = [aggregation(A.shape[0], A.shape[0] // 3, 5, second=0)]
        return Hierarchy(A, M, P_mats, name), A, M, P_mats, None, (1, 2, 3, 9, 17, 65)
    problem, J = {p: (p, j) for p, j in MESHES}[name]
    A, M, P_mats, coords = mesh_problem(problem, J)
    return mesh_hierarchy(problem, J), A, M, list(P_mats), coords, (1, 2, 3, 9, 17, 65)


@functools.lru_cache(maxsize=None)
def sweep_case(name, with_cm, backward, its, diag_free):
    """(U0, F, ca, cm, u_ref, bound) of `its` sweeps from the nonzero start U0."""
    H, A, M, P_mats, coords, n_locs = sweep_problem(name)
    n, T = H.n[H.J], max(n_locs)
    _, cm, _ = family_slices(T, mesh_mass_scale(H) if coords is not None else 1.0)
    ca = FAMILY_CA if with_cm else 1.0
    F, U0 = signed_input(n, T, 31), signed_input(n, T, 32)
    zero = np.zeros((n, T), dtype=LD)
    V, ka = H.rows[H.J].values(ca, cm if with_cm else None)
    u, e = smooth(H.rows[H.J], V, ka, (U0.astype(LD), zero), (F.astype(LD), zero), its, backward, diag_free)
    return U0, F, ca, (cm if with_cm else None), u, e


FAMILY_CASES = (('mesh', ('square', 5)), ('algebraic', 'rows-4096'))


@functools.lru_cache(maxsize=None)
def member_case(kind_of, name):
    """A family whose coarse end runs on member matrices: (F, members, u_ref, bound).  Member
    matrices are data to the plan.  The assembled chains differ from the combination of the two
    shared chains by a rounding; scaled by 1 + k / 100 they differ visibly, from it and from
    each other, so a slice that read the combination or its neighbour's member cannot pass."""
    H = case_hierarchy(kind_of, name)
    ss, vc = (2, 1) if kind_of == 'mesh' else algebraic(name)[3:]
    ca, cms, cm, kind = case_family(kind_of, name)
    shape = plan_shape(H, ss, 1)
    Lc = shape['Lc']
    members = {}
    for k in sorted(set(int(q) for q in kind)):
        members[k] = H.member_chain(ca, cms[k - 1])
        for C in members[k]:
            C.data *= 1.0 + k / 100.0
    F = vcycle_case(kind_of, name, 'two-step', 1, True)[0]
    fused = lambda j: j > Lc and shape['levels'][j]['ell'] and shape['levels'][j]['ra'] > 0
    u, e = vcycles(H, F, numpy_inverses(H, ca, cms), ss, vc, ca, cm, kind, fused, lambda j: True, members, Lc)
    return F, members, u, e


# ---- SPMM cases of the row engine -------------------------------------------------------------
N_LOCS = (1, 2, 3, 4, 9, 17, 18, 65, 66, 1023, 1024)


def n_locs_for(K):
    """The listed slab lengths, plus the shortest ones that reach an NPF instance the listed ones
    do not (every instance some n_loc <= 1024 reaches is reached)."""
    out = list(N_LOCS)
    seen = {rows_launch(n, K)[2] for n in out}
    for n in range(1, 1025):
        if rows_launch(n, K)[2] not in seen:
            out.append(n)
            seen.add(rows_launch(n, K)[2])
    return out


def row_counts(R):
    return sorted({1, max(R - 1, 1), R, R + 1, 8 * R + 1})


@functools.lru_cache(maxsize=None)
def ell_matrix(K, rows, seed):
    """A rectangular matrix in the ELL form itself: idx / va / vm[rows, K], between 1 and K entries
    per row (row 0 has K), padding slots at a valid column with value zero, and a permutation
    row_ids."""
    rng = np.random.RandomState(seed)
    cols = max(K, rows // 2) + 3
    nnz = rng.randint(1, K + 1, size=rows)
    nnz[0] = K
    idx = np.stack([rng.permutation(cols)[:K] for _ in range(rows)]).astype(np.int32)
    held = np.arange(K)[None, :] < nnz[:, None]
    sign = lambda: rng.choice([-1.0, 1.0], size=(rows, K))
    va = np.where(held, rng.uniform(0.25, 1.0, (rows, K)) * sign(), 0.0)
    vm = np.where(held, rng.uniform(0.25, 1.0, (rows, K)) * sign(), 0.0)
    return dict(K=K, rows=rows, cols=cols, nnz=nnz, idx=idx, va=va, vm=vm, row_ids=rng.permutation(rows).astype(np.int32))


class _EllRows:
    """Rows-like view of an ell_matrix for spmm(): output row row_ids[pos]."""
    def __init__(self, m):
        self.idx, self.nnz, self.K = m['idx'].astype(np.int64), m['nnz'].astype(np.int64), m['K']
        self.va, self.vm = m['va'], m['vm']

    values = Rows.values


def spmm_case(K, rows, n_loc, has_m, zmode, seed, wrong=None):
    """Inputs and (y_ref, bound), in OUTPUT row order, of one stk_ell_spmm call.  Signed sums
    cancel, and with one row and a thousand columns some column cancels badly: the vectors
    are drawn again (a fixed sequence of seeds) until every column keeps the bound informative
    -- a choice of input, made with the right restatement alone."""
    for attempt in range(16):
        c = _spmm_draw(K, rows, n_loc, has_m, zmode, seed, 1000 * attempt, None)
        if bound_is_informative(c['y'], c['e']):
            return c if wrong is None else _spmm_draw(K, rows, n_loc, has_m, zmode, seed, 1000 * attempt, wrong)
    raise AssertionError((K, rows, n_loc, has_m, zmode, seed))


def _spmm_draw(K, rows, n_loc, has_m, zmode, seed, redraw, wrong):
    m = ell_matrix(K, rows, seed)
    rng = np.random.RandomState(seed + 7 * n_loc)
    ca, alpha = float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.5, 1.5)) * (-1.0 if seed & 1 else 1.0)
    beta = 0.0 if zmode == 0 else -float(rng.uniform(0.5, 1.5))
    cm = (rng.uniform(0.5, 1.5, n_loc) * rng.choice([-1.0, 1.0], n_loc)) if has_m else None
    X, Z = signed_input(m['cols'], n_loc, seed + 1 + redraw), signed_input(rows, n_loc, seed + 2 + redraw)
    er = _EllRows(m)
    V, ka = er.values(ca, cm, wrong)
    zero = np.zeros(X.shape, dtype=LD)
    inv = np.argsort(m['row_ids'])  # position that produces output row i
    zpos = (Z.astype(LD)[m['row_ids']], np.zeros(Z.shape, dtype=LD)) if zmode else None
    y, e = spmm(er, V, ka, (X.astype(LD), zero), alpha, beta, zpos, wrong)
    return dict(m=m, ca=ca, alpha=alpha, beta=beta, cm=cm, X=X, Z=Z, y=y[inv], e=e[inv])


# ---- host tests ---------------------------------------------------------------------------------
G3 = ('g3_square', 'g3_lshape', 'g3_cube')
SMALL_ALGEBRAIC = ('small-s3-v2', 'width-12')


def _golden_hierarchy(name):
    gd = load_golden(name)
    P_mats = [csr_from(gd, 'P%d' % j) for j in range(int(gd['nP']))]
    return gd, csr_from(gd, 'A_x'), csr_from(gd, 'M_x'), P_mats


def _oracle_galerkin_as_data(H, omg):
    """The oracle forms the same chain with SciPy and keeps the rounding-noise entries; hand it
    the plan's matrices so that both sides run on one set of data."""
    from oracle.multigrid import Smoother
    omg.mats = [H.A[j] for j in range(H.J + 1)]
    omg.smoothers = [None] + [Smoother(H.A[j], omg.smoothsteps) for j in range(1, H.J + 1)]


@pytest.mark.parametrize('name', G3)
def test_reference_agrees_with_the_oracle_and_the_goldens(name):
    from oracle.multigrid import MultiGrid, Smoother
    gd, A, M, P_mats = _golden_hierarchy(name)
    H = Hierarchy(A, M, P_mats, name)
    b = np.asarray(gd['mg_b'], dtype=np.float64)
    F = b[:, None] * column_scales(3)[None, :]
    worst = 0.0
    # one smoother call: forward and backward, one and three sweeps, both row forms
    V, ka = H.rows[H.J].values(1.0)
    for backward in (False, True):
        for its in (1, 3):
            start = signed_input(H.n[H.J], 3, seed=5)
            zero = np.zeros(F.shape, dtype=LD)
            sm = Smoother(A, its)
            want = np.ascontiguousarray(start.T)
            (sm.PostSmooth if backward else sm.PreSmooth)(want, np.ascontiguousarray(F.T))
            for diag_free in (False, True):
                u, e = smooth(H.rows[H.J], V, ka, (start.astype(LD), zero), (F.astype(LD), zero), its, backward,
                              diag_free, order='dof')
                worst = max(worst, ratio(want.T, u, e, (name, backward, its, diag_free)))
                u2, e2 = smooth(H.rows[H.J], V, ka, (start.astype(LD), zero), (F.astype(LD), zero), its, backward,
                                diag_free, order='groups')
                assert np.array_equal(u, u2) and np.array_equal(e, e2)  # the groups ARE the dof-order sweep
    # whole V-cycles: the oracle on the plan's data, and the stored goldens
    # (the goldens come from the oracle's own chain, rounding-noise entries kept and SuperLU
    # on level 0: the same operation on data a few ulps away; they are compared on the
    # columns' scale with the project's parity figure, the oracle on equal data with the bound)
    for ss in (1, 3):
        for vc in (1, 2):
            omg = MultiGrid(A, P_mats, ss, vc)
            _oracle_galerkin_as_data(H, omg)
            inv = numpy_inverses(H)

            class _Dense:
                def solve(self, f, inv=inv[0]):
                    return inv @ f
            omg.coarse_solver = _Dense()
            want = omg.apply(np.ascontiguousarray(F.T)).T
            for order in ('dof', 'groups'):
                u, e = vcycles(H, F, inv, ss, vc, diag_free=lambda j: False, order=order)
                worst = max(worst, ratio(want, u, e, (name, ss, vc, order)))
                assert bound_is_informative(u, e)
            gold = np.asarray(gd['mg_Ax_s%d_v%d' % (ss, vc)])
            mid = F.shape[1] // 2  # the column scaled by one
            assert np.max(np.abs(gold - u[:, mid].astype(np.float64))) <= PARITY * np.max(np.abs(gold))
            for restrict in (lambda j: True,):  # the other arithmetic classes stay inside THEIR bound
                u3, e3 = vcycles(H, F, inv, ss, vc, fused_restrict=restrict)
                assert np.all(np.abs(u3 - u) <= e3 + e)
    # the family member 4 M + 0.3 A
    inv = numpy_inverses(H, 0.3, [4.0])
    cm, kind = np.full(3, 4.0), np.ones(3, dtype=np.int64)
    u, e = vcycles(H, F, inv, 3, 2, 0.3, cm, kind)
    gold = np.asarray(gd['mg_C2_s3_v2'])
    assert np.max(np.abs(gold - u[:, 1].astype(np.float64))) <= PARITY * np.max(np.abs(gold))
    omg = MultiGrid(sp.csr_matrix(4.0 * M + 0.3 * A), P_mats, 3, 2)
    want = omg.apply(np.ascontiguousarray(F.T)).T
    assert np.max(np.abs(want - u.astype(np.float64)) / np.abs(want).max(axis=0)) <= PARITY
    print('%s: float64 oracle at %.3f of the bound' % (name, worst))


@pytest.mark.parametrize('name', SMALL_ALGEBRAIC)
def test_reference_agrees_with_the_oracle_on_algebraic_hierarchies(name):
    from oracle.multigrid import MultiGrid
    A, M, P_mats, ss, vc = algebraic(name)
    H = algebraic_hierarchy(name)
    F = signed_input(H.n[H.J], 4, seed=9)
    inv = numpy_inverses(H)
    omg = MultiGrid(A, list(P_mats), ss, vc)
    _oracle_galerkin_as_data(H, omg)

    class _Dense:
        def solve(self, f):
            return inv[0] @ f
    omg.coarse_solver = _Dense()
    want = omg.apply(np.ascontiguousarray(F.T)).T
    u, e = vcycles(H, F, inv, ss, vc, diag_free=lambda j: False, order='dof')
    worst = ratio(want, u, e, name)
    u2, e2 = vcycles(H, F, inv, ss, vc, diag_free=lambda j: False, order='groups')
    assert np.array_equal(u, u2) and np.array_equal(e, e2)
    print('%s: float64 oracle at %.3f of the bound' % (name, worst))


def vcycle_catalogue():
    """Every (kind_of, name, restrict, gs_key, with_cm) reference the GPU tests compare with."""
    out = []
    for name in sorted(ALGEBRAIC):
        fam = bool(ALGEBRAIC[name].get('family'))
        for with_cm in ((False, True) if fam else (False,)):
            for restrict in ('two-step', 'above-Lc', 'fused'):
                out.append(('algebraic', name, restrict, 1, with_cm))
        out.append(('algebraic', name, 'two-step', 0, False))
    for mesh in MESHES:  # (families only: a stiffness matrix alone has an inverse of size h^-2, and
        # the worst-case bound, which sees no cancellation in A u - f, grows 14-fold per level)
        for restrict in ('two-step', 'above-Lc', 'fused'):
            out.append(('mesh', mesh, restrict, 1, True))
    return out


def test_the_bound_is_informative_on_the_whole_catalogue():
    for key in vcycle_catalogue():
        F, u, e = vcycle_case(*key)
        assert np.all(np.isfinite(u.astype(np.float64))) and bound_is_informative(u, e), key
    # the row-engine cases: every K, the extreme slab lengths and row counts
    for K in SLOTS:
        for n_loc in (1, 9, 66, 1024):
            R = rows_launch(n_loc, K)[1]
            for rows in row_counts(R):
                for has_m in (False, True):
                    c = spmm_case(K, rows, n_loc, has_m, 1 + (rows & 1), seed=K + rows)
                    assert bound_is_informative(c['y'], c['e']), (K, n_loc, rows, has_m)
    # the smoother cases and the families on member matrices
    for name in SWEEP_MATRICES:
        for with_cm in (False, True):
            for backward in (False, True):
                for its in (1, 3):
                    for diag_free in (False, True):
                        c = sweep_case(name, with_cm, backward, its, diag_free)
                        assert bound_is_informative(c[4], c[5]), (name, with_cm, backward, its, diag_free)
    for key in FAMILY_CASES:
        F, members, u, e = member_case(*key)
        assert bound_is_informative(u, e), key


def test_the_catalogue_sits_where_it_says():
    """The thresholds, from the restated rules alone."""
    shape = {name: plan_shape(algebraic_hierarchy(name), algebraic(name)[3]) for name in ALGEBRAIC}
    arena = lambda name: shape[name]['lds_rows'] // 3
    assert arena('arena-3072') == 3072 and coarse_path(shape['arena-3072'], 10, False)[4] is True
    assert arena('arena-3073') == 3073 and coarse_path(shape['arena-3073'], 10, False)[4] is False
    assert arena('arena-6144') == 6144
    assert shape['arena-6144']['Lc'] == 4 and shape['arena-6145']['Lc'] == 3 and arena('arena-6145') == 2049
    assert shape['rows-4096']['Lc'] == 4 and shape['rows-4097']['Lc'] == 3
    assert coarse_path(shape['jobs-s1'], 10, False)[0] == 'uniform'
    assert coarse_path(shape['jobs-s3'], 10, False)[0] == 'lds'
    assert shape['jobs-s3']['KU'] and shape['jobs-s3']['levels'][2]['n_fwd'] == 300
    for width, KU in ((7, 8), (8, 12), (9, 12), (12, 12), (13, 0)):
        s = shape['width-%d' % width]
        assert s['Lc'] == 1 and int(algebraic_hierarchy('width-%d' % width).rows[1].nnz.max()) == width
        assert s['KU'] == KU, (width, s['KU'])  # (8 entries are 9 slots in the plain copy: KU = 12)
    s = shape['row-26']
    assert not s['levels'][2]['ell'] and s['levels'][1]['ell'] and s['Lc'] == 1 and not s['levels'][3]['ell']
    assert shape['two-level']['Lc'] == -1 and shape['three-level']['Lc'] == -1
    # every kernel the launcher can select is selected by some catalogue case
    assert selected_paths() >= UNIFORM_SITES | LDS_SITES | GLOBAL_SITES, \
        (UNIFORM_SITES | LDS_SITES | GLOBAL_SITES) - selected_paths()
    assert ('uniform', 8, False, False, False, 1024) in selected_paths()
    for name in ALGEBRAIC:
        for n in algebraic_hierarchy(name).n:
            assert n <= 4100


FORMS = (('levels', dict(fuse_coarse=0)), ('global', dict(coarse_lds=0)), ('lds', dict(uniform=0)),
         ('uniform-512', dict(uniform=2)), ('uniform', dict(uniform=1)))


def selected_paths():
    """Every coarse kernel the V-cycle catalogue launches, by the restated rule (even ld)."""
    seen = set()
    for name in ALGEBRAIC:
        shape = plan_shape(algebraic_hierarchy(name), algebraic(name)[3])
        for with_cm in ((False, True) if ALGEBRAIC[name].get('family') else (False,)):
            for _, keys in FORMS:
                seen.add(coarse_path(shape, 10, with_cm, **keys))
    return seen


@pytest.mark.parametrize('wrong', WRONG)
def test_a_wrong_restatement_leaves_the_bound(wrong):
    """Each mistake is an argument of the reference; the right restatement is the yardstick."""
    if wrong in ('slot-from-neighbour-slice', 'cm-of-t0-for-t0+1', 'beta-dropped'):
        good = spmm_case(7, 40, 9, True, 1, seed=11)
        bad = spmm_case(7, 40, 9, True, 1, seed=11, wrong=wrong)
        assert unchecked_ratio(bad['y'].astype(np.float64), good['y'], good['e']) > 1.0
    key = ('algebraic', 'width-7', 'two-step', 1, True)
    F, u, e = vcycle_case(*key)
    Fb, ub, eb = vcycle_case(*key, wrong=wrong)
    assert np.array_equal(F, Fb)
    assert unchecked_ratio(ub.astype(np.float64), u, e) > 1.0, wrong
    # ... while the right restatement, rounded to float64, is of course inside it
    assert unchecked_ratio(u.astype(np.float64), u, e + LD(U) * np.abs(u)) <= 1.0
