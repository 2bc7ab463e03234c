"""Level transfer: a trial-space vector of a COARSER discretisation (J_time - a, J_space - s) as
the vector of this one that represents the same function -- P1 in space on the hierarchical
meshes (level l is a prefix of level l + 1), piecewise linear in time on the dyadic time meshes
(csrc/transfer.hip, include/stk.h "level transfer").  What nested iteration, warm starts and
|| u_h - P u_2h || are built from.

The rule, rounded term by term: a fine row with the parents (p, p) copies the coarse row p; any
other row is (A + B) * 0.5 of its two parents' values, 0.0 for a parent on the boundary; the
fine node k = (q << a) + rem is s(q) for rem == 0 and (1.0 - rem / 2^a) * s(q) + (rem / 2^a) *
s(q + 1) otherwise.  Time goes in ONE shot (a chain of half-steps rounds differently); several
space levels are chained with a = 0 on the coarse time mesh, and the last call, which writes the
big slab, carries all of the time refinement.

* ``parent_rows(mesh, level=None)``: the int32 table of one space level.
* ``check_nested(coarse_meshes, fine_meshes)``: (a, s) or ValueError; touches no GPU.
* ``TransferPlan(coarse_meshes, fine_meshes)``: the tables of the chain on the device, plus a.
* ``prolong_scan``: the thin call of stk_transfer_prolong.
* ``prolong_collective(plan, coarse_vec, fine_distr)``: every rank's coarse columns into one
  (M_c, N_c) buffer, one all-reduce, every rank prolongs into the columns it owns.

The adjoint P^T (include/stk.h "restriction") takes a FUNCTIONAL on the fine trial space -- a
right-hand side, a residual, E^T r of point data -- to the coarse one: (P^T f) . v = f . (P v).
A coarse row folds its own fine row (1.0) and its children (0.5) in ascending fine row, then
the stencil of 2^(a+1) - 1 fine nodes in ascending k with prolong's weights; every operation
rounded on its own, every sum of one fixed order (a gather over a transposed table).

* ``children_rows(table, M_coarse)``: the transposed table of one space level (host, no GPU).
* ``stencil_window(a, q_first, n_qc, n_fine)``: the fine columns a restriction reads.
* ``restrict_scan`` / ``restrict_time_scan``: the thin calls of stk_transfer_restrict(_time).
* ``restrict_window``: the chain of a TransferPlan downwards, on a window of columns.
* ``restrict_collective(plan, fine_vec, coarse_distr)``: the one-rank doubles on any number of
  ranks.  ``restrict_to(heat, coarse_heat, f)``: what both drivers' ``restrict_to`` do.

Scope: transfers of trial-space vectors between nested meshes of one coarsest mesh, time
ratios 2^a.  Injection, test-space vectors, a neighbour-only exchange of columns and other
time ratios are not served.
"""
import ctypes

import numpy as np

from . import _lib

MAX_A = _lib.STK_TRANSFER_MAX_A


def parent_rows(mesh, level=None):
    """(M_f, 2) int32: per free vertex of `level` of a hierarchical mesh (default: its last
    level, mesh.J), in free-dof order, the free-dof indices on level - 1 of what it
    interpolates -- (p, p) for a vertex that level - 1 has too, the two parents of a new one,
    -1 for a parent on the boundary.  Entry for entry the rows of
    ``assembly.prolongation_matrices(mesh)``: one entry 1.0, or at most two of 0.5."""
    level = mesh.J if level is None else int(level)
    if not 1 <= level <= mesh.J:
        raise ValueError('level %d has no coarser level in a mesh of levels 0..%d' % (level, mesh.J))
    nc, nf = int(mesh.nverts[level - 1]), int(mesh.nverts[level])
    free = ~np.asarray(mesh.boundary, dtype=bool)[:nf]
    coarse_row = np.where(free[:nc], np.cumsum(free[:nc]) - 1, -1)
    fine = np.flatnonzero(free)
    table = np.empty((len(fine), 2), dtype=np.int64)
    old = fine < nc
    table[old] = coarse_row[fine[old]][:, None]
    table[~old] = coarse_row[np.asarray(mesh.parents, dtype=np.int64)[fine[~old]]]
    assert nc - 1 < 2**31
    return np.ascontiguousarray(table, dtype=np.int32)


def identity_rows(M):
    """The table of a space level prolonged to itself: every row copies its own."""
    return np.ascontiguousarray(np.repeat(np.arange(M, dtype=np.int32)[:, None], 2, axis=1))


def time_levels(N_coarse, N_fine):
    """a with N_fine - 1 = 2^a (N_coarse - 1), 0 <= a <= MAX_A, or ValueError."""
    ec, ef = int(N_coarse) - 1, int(N_fine) - 1
    for a in range(MAX_A + 1):
        if ec >= 1 and ef == ec << a:
            return a
    raise ValueError('time meshes of %d and %d nodes: the finer one must have 2^a times the elements of the '
                     'coarser, 0 <= a <= %d' % (N_coarse, N_fine, MAX_A))


def check_nested(coarse_meshes, fine_meshes):
    """(a, s): the time levels and space levels between (mesh_space, mesh_time) of a coarse and
    of a fine discretisation, or ValueError where the coarse one is not nested in the fine one:
    its points, boundary flags and parents must be, array for array, the prefix of the fine
    mesh's, the level sizes a prefix of its level sizes, T the same and the time elements in the
    ratio 2^a.  Touches no GPU."""
    (xc, tc), (xf, tf) = coarse_meshes, fine_meshes
    if float(tc.T) != float(tf.T):
        raise ValueError('the time intervals differ: T = %r against %r' % (tc.T, tf.T))
    a = time_levels(tc.nv, tf.nv)
    s = xf.J - xc.J
    if s < 0 or list(xc.nverts) != list(xf.nverts[:xc.J + 1]):
        raise ValueError('the space meshes are not nested: levels of %s vertices against %s'
                         % (list(xc.nverts), list(xf.nverts)))
    n = xc.nv
    for name in ('points', 'boundary', 'parents'):
        mine, theirs = np.asarray(getattr(xc, name)), np.asarray(getattr(xf, name))[:n]
        if mine.shape != theirs.shape or not np.array_equal(mine, theirs):
            raise ValueError('the space meshes are not nested: the coarse %s are not the prefix of the fine ones'
                             % name)
    return a, s


def window(a, k_first, n_cols):
    """(q_first, q_last): the coarse columns that the fine columns [k_first, k_first + n_cols)
    read at `a` time levels, both inclusive -- q of the first, q of the last and q + 1 of the
    last only if its rem != 0.  The arithmetic of stk_transfer_prolong's refusal."""
    assert n_cols >= 1 and k_first >= 0 and 0 <= a <= MAX_A
    k_last = k_first + n_cols - 1
    return k_first >> a, (k_last >> a) + (1 if k_last & ((1 << a) - 1) else 0)


def stencil_window(a, q_first, n_qc, n_fine):
    """(k_lo, k_hi): the fine columns that the coarse columns [q_first, q_first + n_qc) read at
    `a` time levels on a fine mesh of `n_fine` nodes, both inclusive -- the stencil of q is
    ((q - 1) << a) + 1 .. ((q + 1) << a) - 1, clipped to [0, n_fine - 1].  The arithmetic of
    stk_transfer_restrict's refusal."""
    assert n_qc >= 1 and q_first >= 0 and 0 <= a <= MAX_A and (n_fine - 1) % (1 << a) == 0
    q_last = q_first + n_qc - 1
    assert q_last <= (n_fine - 1) >> a
    return max(0, ((q_first - 1) << a) + 1), min(n_fine - 1, ((q_last + 1) << a) - 1)


def children_rows(table, M_coarse):
    """(ptr (M_c + 1,) int64, entries int32) of stk_transfer_children: per coarse row its fine
    rows in ascending order, an entry being (fine row << 1) | (1 where the weight is 0.5).
    Host threads of libstk, no GPU; StkError where the table is refused."""
    table = np.ascontiguousarray(table, dtype=np.int32)
    assert table.ndim == 2 and table.shape[1] == 2, table.shape
    ptr = np.zeros(max(int(M_coarse), 0) + 1, dtype=np.int64)
    entries = np.zeros(2 * len(table) + 1, dtype=np.int32)
    _lib.check(_lib.lib().stk_transfer_children(len(table), int(M_coarse), table.ctypes.data, ptr.ctypes.data,
                                                entries.ctypes.data))
    return ptr, entries[:ptr[-1]].copy()


class _PlanHandle:
    """One stk_transfer_plan on the device of this process, destroyed with this object."""
    def __init__(self, table, M_coarse):
        import torch

        table = np.ascontiguousarray(table, dtype=np.int32)
        assert table.ndim == 2 and table.shape[1] == 2, table.shape
        self.M_fine, self.M_coarse = len(table), int(M_coarse)
        self._as_parameter_ = ctypes.c_void_p()
        self._lib = _lib.lib()  # kept here: __del__ may run at interpreter exit
        with torch.cuda.device(_lib.compute_device()):
            _lib.check(self._lib.stk_transfer_plan_create(self.M_fine, self.M_coarse, table.ctypes.data,
                                                          ctypes.byref(self._as_parameter_)))

    def __del__(self):
        if getattr(self, '_as_parameter_', None):
            self._lib.stk_transfer_plan_destroy(self._as_parameter_)
            self._as_parameter_ = None


class _RestrictHandle(_PlanHandle):
    """One stk_restrict_plan (the transposed table of a space level) on the device of this
    process, destroyed with this object."""
    def __init__(self, table, M_coarse):
        import torch

        table = np.ascontiguousarray(table, dtype=np.int32)
        assert table.ndim == 2 and table.shape[1] == 2, table.shape
        self.M_fine, self.M_coarse = len(table), int(M_coarse)
        self._as_parameter_ = ctypes.c_void_p()
        self._lib = _lib.lib()
        with torch.cuda.device(_lib.compute_device()):
            _lib.check(self._lib.stk_restrict_plan_create(self.M_fine, self.M_coarse, table.ctypes.data,
                                                          ctypes.byref(self._as_parameter_)))

    def __del__(self):
        if getattr(self, '_as_parameter_', None):
            self._lib.stk_restrict_plan_destroy(self._as_parameter_)
            self._as_parameter_ = None


class TransferPlan:
    """The chain of space levels from a coarse discretisation to a fine one, plus the time
    levels `a`: ``levels[j]`` maps the free rows of space level J_c + j to those of J_c + j + 1
    (one identity level where the space meshes are the same).  `coarse_meshes`, `fine_meshes`:
    (mesh_space, mesh_time) each; ValueError, before anything touches the GPU, where they are
    not nested (``check_nested``)."""
    def __init__(self, coarse_meshes, fine_meshes):
        self.a, self.s = check_nested(coarse_meshes, fine_meshes)
        (xc, tc), (xf, tf) = coarse_meshes, fine_meshes
        self.N_coarse, self.N_fine = int(tc.nv), int(tf.nv)
        free = ~np.asarray(xf.boundary, dtype=bool)
        sizes = [int(np.count_nonzero(free[:xf.nverts[l]])) for l in range(xc.J, xf.J + 1)]
        self.M_coarse, self.M_fine = sizes[0], sizes[-1]
        if self.s == 0:
            tables = [identity_rows(self.M_fine)]
            sizes = sizes * 2
        else:
            tables = [parent_rows(xf, l) for l in range(xc.J + 1, xf.J + 1)]
        self.levels = [_PlanHandle(t, m) for t, m in zip(tables, sizes[:-1])]
        self.sizes = sizes  # rows of the space levels, the coarsest first
        self._tables, self._transposed = tables, None

    def transposed(self):
        """The transposed levels (``transposed()[j]`` takes the rows of space level J_c + j + 1
        down to J_c + j), built and uploaded by the FIRST restriction: a run that only prolongs
        builds nothing of it.  None in place of an identity level (the time-only form needs no
        table)."""
        if self._transposed is None:
            self._transposed = [None if self.s == 0 else _RestrictHandle(t, m)
                                for t, m in zip(self._tables, self.sizes[:-1])]
            self._tables = None
        return self._transposed


def prolong_scan(plan, a, uc, ldc, qc_first, n_cc, out, ld, k_first, n_cols):
    """stk_transfer_prolong with one space level `plan` (a level of a TransferPlan): the fine
    columns [k_first, k_first + n_cols) into out[i * ld + c] from the coarse columns
    [qc_first, qc_first + n_cc) at uc[j * ldc + (q - qc_first)]; `uc`, `out`: device tensors
    or device addresses."""
    from .p1_plan import device_address
    _lib.check(_lib.lib().stk_transfer_prolong(_lib.stream(), plan, int(a), device_address(uc), int(ldc), int(qc_first),
                                               int(n_cc), device_address(out), int(ld), int(k_first), int(n_cols)))
    return out


def prolong_window(plan, full, ldc, n_cc, out, ld, k_first, n_cols):
    """The chain of `plan` (TransferPlan) on the coarse columns [0, n_cc) at full[j * ldc + q]
    into the fine columns [k_first, k_first + n_cols) of out[i * ld + c]: all levels but the
    last with a = 0, only on the coarse columns the last one reads; the last one carries the
    time refinement."""
    import torch
    if n_cols == 0 or plan.M_fine == 0:
        return out
    q0, q1 = window(plan.a, k_first, n_cols)
    src, src_ld, src_first, src_n = full, ldc, 0, n_cc
    for level in plan.levels[:-1]:
        n_w = q1 - q0 + 1
        mid = torch.empty((max(level.M_fine, 1), n_w), dtype=torch.float64, device=out.device)
        prolong_scan(level, 0, src, src_ld, src_first, src_n, mid, n_w, q0, n_w)
        src, src_ld, src_first, src_n = mid, n_w, q0, n_w
    return prolong_scan(plan.levels[-1], plan.a, src, src_ld, src_first, src_n, out, ld, k_first, n_cols)


def prolong_collective(plan, coarse_vec, fine_distr):
    """P u_c: the trial-space vector `coarse_vec` (KronVectorMPI of the coarse discretisation,
    on the communicator of `fine_distr`) as a new KronVectorMPI on `fine_distr`.  COLLECTIVE:
    every rank copies the coarse columns it owns into a zeroed (M_c, N_c) buffer, one
    all-reduce gives every rank all of it -- one non-zero contributor per entry (the idiom of
    ``sample_collective``; NaN and +-inf survive + 0.0) -- and every rank prolongs into the
    fine columns it owns.  An entry's operations do not depend on the columns that share its
    launch, so the doubles are the one-rank doubles whatever the number of ranks."""
    import torch

    from .mpi_vector import KronVectorMPI
    cd = coarse_vec.dofs_distr
    if (coarse_vec.N, coarse_vec.M) != (plan.N_coarse, plan.M_coarse):
        raise ValueError('a coarse vector of %d x %d; the plan takes %d x %d'
                         % (coarse_vec.N, coarse_vec.M, plan.N_coarse, plan.M_coarse))
    if (fine_distr.N, fine_distr.M) != (plan.N_fine, plan.M_fine):
        raise ValueError('a fine distribution of %d x %d; the plan gives %d x %d'
                         % (fine_distr.N, fine_distr.M, plan.N_fine, plan.M_fine))
    if cd.size != fine_distr.size or cd.rank != fine_distr.rank:
        raise ValueError('the coarse vector lives on %d ranks, the fine distribution on %d' % (cd.size, fine_distr.size))
    N_c = plan.N_coarse
    # (one row even where M_c = 0: the C ABI takes no null slab)
    full = torch.zeros((max(plan.M_coarse, 1), N_c), dtype=torch.float64, device=coarse_vec.buf.device)
    if plan.M_coarse and coarse_vec.n_loc:
        _lib.copy_block(coarse_vec.buf, plan.M_coarse, coarse_vec.n_loc, coarse_vec.ld, full, N_c,
                        dst_off=int(coarse_vec.t_begin))
    if cd.size > 1:
        cd.comm.allreduce_tensor_(full)
    out = KronVectorMPI(fine_distr)  # zeroed: the pad column of an odd n_loc stays 0
    prolong_window(plan, full, N_c, N_c, out.buf, out.ld, int(out.t_begin), out.n_loc)
    return out


def restrict_scan(level, a, f, ld, k_first, n_cols, n_fine, out, ldc, q_first, n_qc):
    """stk_transfer_restrict with one transposed space level `level` (of
    ``TransferPlan.transposed()``): the coarse columns [q_first, q_first + n_qc) into
    out[j * ldc + (q - q_first)] from the fine window [k_first, k_first + n_cols) at
    f[i * ld + (k - k_first)] of a fine time mesh of `n_fine` nodes; `f`, `out`: device tensors
    or device addresses."""
    from .p1_plan import device_address
    _lib.check(_lib.lib().stk_transfer_restrict(_lib.stream(), level, int(a), device_address(f), int(ld), int(k_first),
                                                int(n_cols), int(n_fine), device_address(out), int(ldc), int(q_first),
                                                int(n_qc)))
    return out


def restrict_time_scan(M, a, f, ld, k_first, n_cols, n_fine, out, ldc, q_first, n_qc):
    """stk_transfer_restrict_time: the time stage alone over `M` rows; no table."""
    from .p1_plan import device_address
    _lib.check(_lib.lib().stk_transfer_restrict_time(_lib.stream(), int(M), int(a), device_address(f), int(ld),
                                                     int(k_first), int(n_cols), int(n_fine), device_address(out),
                                                     int(ldc), int(q_first), int(n_qc)))
    return out


def _restrict_lower(plan, src, src_ld, out, ldc, q_first, n_qc, done):
    """The space levels below the `done` uppermost ones with a = 0 on the coarse columns
    [q_first, q_first + n_qc) held at src[i * src_ld + c]; the last one writes `out`.  With
    nothing left to do, `src` is copied to `out`."""
    import torch
    levels = plan.transposed()[:len(plan.levels) - done] if plan.s else []
    if not levels:
        _lib.copy_block(src, plan.M_coarse, n_qc, src_ld, out, ldc)
        return out
    N_c = plan.N_coarse
    for number, level in enumerate(reversed(levels)):
        last = number == len(levels) - 1
        dst = out if last else torch.empty((max(level.M_coarse, 1), n_qc), dtype=torch.float64, device=out.device)
        dst_ld = ldc if last else n_qc
        restrict_scan(level, 0, src, src_ld, q_first, n_qc, N_c, dst, dst_ld, q_first, n_qc)
        src, src_ld = dst, dst_ld
    return out


def restrict_window(plan, f, ld, k_first, n_cols, out, ldc, q_first, n_qc):
    """The chain of `plan` (TransferPlan) downwards: the coarse columns [q_first, q_first + n_qc)
    of out[j * ldc + c] from the fine window [k_first, k_first + n_cols) of f[i * ld + c].  The
    FIRST call acts on the fine slab and carries all of the time levels, so every later level
    works on coarse columns, with a = 0."""
    import torch
    if n_qc == 0 or plan.M_coarse == 0:
        return out
    if plan.s == 0:
        return restrict_time_scan(plan.M_fine, plan.a, f, ld, k_first, n_cols, plan.N_fine, out, ldc, q_first, n_qc)
    top = plan.transposed()[-1]
    if len(plan.levels) == 1:
        return restrict_scan(top, plan.a, f, ld, k_first, n_cols, plan.N_fine, out, ldc, q_first, n_qc)
    mid = torch.empty((max(top.M_coarse, 1), n_qc), dtype=torch.float64, device=out.device)
    restrict_scan(top, plan.a, f, ld, k_first, n_cols, plan.N_fine, mid, n_qc, q_first, n_qc)
    return _restrict_lower(plan, mid, n_qc, out, ldc, q_first, n_qc, 1)


def restrict_collective(plan, fine_vec, coarse_distr):
    """P^T f: the functional `fine_vec` (KronVectorMPI of the fine trial space, on the
    communicator of `coarse_distr`) as a new KronVectorMPI on `coarse_distr`.  COLLECTIVE.  On
    one rank: the fused call, then the remaining space levels.  On several: every rank applies
    the LAST space level with a = 0 to the fine columns it owns, into a zeroed (M_{L-1}, N_f)
    buffer at its column offset; one all-reduce gives every rank all of it (one non-zero
    contributor per entry: NaN and +-inf survive + 0.0); every rank runs the time-only form for
    the coarse columns it owns; the remaining levels follow with a = 0.  With a = 0 the time
    stage is an exact copy and with an identity table the space stage is, so the split route
    gives the doubles of the fused call: the one-rank doubles whatever the number of ranks."""
    import torch

    from .mpi_vector import KronVectorMPI
    fd = fine_vec.dofs_distr
    if (fine_vec.N, fine_vec.M) != (plan.N_fine, plan.M_fine):
        raise ValueError('a fine vector of %d x %d; the plan takes %d x %d'
                         % (fine_vec.N, fine_vec.M, plan.N_fine, plan.M_fine))
    if (coarse_distr.N, coarse_distr.M) != (plan.N_coarse, plan.M_coarse):
        raise ValueError('a coarse distribution of %d x %d; the plan gives %d x %d'
                         % (coarse_distr.N, coarse_distr.M, plan.N_coarse, plan.M_coarse))
    if fd.size != coarse_distr.size or fd.rank != coarse_distr.rank:
        raise ValueError('the fine vector lives on %d ranks, the coarse distribution on %d' % (fd.size, coarse_distr.size))
    out = KronVectorMPI(coarse_distr)  # zeroed: the pad column of an odd n_loc stays 0
    N_f = plan.N_fine
    if plan.M_coarse == 0 or plan.M_fine == 0:
        return out
    q_first, n_qc = int(out.t_begin), int(out.n_loc)
    if fd.size == 1:
        restrict_window(plan, fine_vec.buf, fine_vec.ld, 0, N_f, out.buf, out.ld, 0, plan.N_coarse)
        return out
    M_mid = plan.sizes[-2]  # the rows below the last space level (M_fine where s == 0)
    full = torch.zeros((max(M_mid, 1), N_f), dtype=torch.float64, device=fine_vec.buf.device)
    if fine_vec.n_loc and M_mid:
        t0, n = int(fine_vec.t_begin), int(fine_vec.n_loc)
        if plan.s == 0:
            _lib.copy_block(fine_vec.buf, plan.M_fine, n, fine_vec.ld, full, N_f, dst_off=t0)
        else:
            restrict_scan(plan.transposed()[-1], 0, fine_vec.buf, fine_vec.ld, t0, n, N_f,
                          full.data_ptr() + 8 * t0, N_f, t0, n)
    fd.comm.allreduce_tensor_(full)
    if n_qc == 0 or M_mid == 0:
        return out
    if len(plan.levels) == 1:
        restrict_time_scan(M_mid, plan.a, full, N_f, 0, N_f, N_f, out.buf, out.ld, q_first, n_qc)
        return out
    mid = torch.empty((M_mid, n_qc), dtype=torch.float64, device=full.device)
    restrict_time_scan(M_mid, plan.a, full, N_f, 0, N_f, N_f, mid, n_qc, q_first, n_qc)
    _restrict_lower(plan, mid, n_qc, out.buf, out.ld, q_first, n_qc, 1)
    return out


def _cached_plan(heat, coarse_heat, vector_of, vector, who):
    """(the TransferPlan of this pair of discretisations -- cached on `heat` per coarse (time
    elements, space levels), built on first use --, `vector` as a trial-space device vector of
    `vector_of`): the checks come before the GPU."""
    coarse_meshes, fine_meshes = coarse_heat._sample_meshes, heat._sample_meshes
    key = (int(coarse_meshes[1].N_el), int(coarse_meshes[0].J))
    cached = heat.transfer_plans.get(key)
    if cached is None or cached[1] is not coarse_meshes[0]:
        check_nested(coarse_meshes, fine_meshes)  # ValueError before an upload
        vector = vector_of._trial_vector(vector, who)
        cached = heat.transfer_plans[key] = (TransferPlan(coarse_meshes, fine_meshes), coarse_meshes[0])
    else:
        vector = vector_of._trial_vector(vector, who)
    return cached[0], vector


def restrict_to(heat, coarse_heat, f):
    """What both drivers' ``restrict_to`` do: the checks (before the GPU) and the plan cache of
    ``prolong_from``, then the collective."""
    plan, f = _cached_plan(heat, coarse_heat, heat, f, 'restrict_to()')
    return restrict_collective(plan, f, coarse_heat._adjoint_target(None)[0])


def prolong_from(heat, coarse_heat, u_coarse):
    """What both drivers' ``prolong_from`` do: the checks (before the GPU), the plan of this
    pair of discretisations -- cached on `heat` per coarse (time elements, space levels), built
    on first use --, the collective."""
    plan, u_coarse = _cached_plan(heat, coarse_heat, coarse_heat, u_coarse, 'prolong_from()')
    return prolong_collective(plan, u_coarse, heat._adjoint_target(None)[0])
