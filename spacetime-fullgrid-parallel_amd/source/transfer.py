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

Scope: prolongation of trial-space vectors between nested meshes of one coarsest mesh, time
ratios 2^a.  The adjoint P^T, injection and restriction, test-space vectors, a neighbour-only
exchange of coarse columns and other time ratios are not served.
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


def prolong_from(heat, coarse_heat, u_coarse):
    """What both drivers' ``prolong_from`` do: the checks (before the GPU), the plan of this
    pair of discretisations -- cached on `heat` per coarse (time elements, space levels), built
    on first use --, the collective."""
    coarse_meshes, fine_meshes = coarse_heat._sample_meshes, heat._sample_meshes
    key = (int(coarse_meshes[1].N_el), int(coarse_meshes[0].J))
    cached = heat.transfer_plans.get(key)
    if cached is None or cached[1] is not coarse_meshes[0]:
        check_nested(coarse_meshes, fine_meshes)  # ValueError before an upload
        u_coarse = coarse_heat._trial_vector(u_coarse, 'prolong_from()')
        cached = heat.transfer_plans[key] = (TransferPlan(coarse_meshes, fine_meshes), coarse_meshes[0])
    else:
        u_coarse = coarse_heat._trial_vector(u_coarse, 'prolong_from()')
    return prolong_collective(cached[0], u_coarse, heat._adjoint_target(None)[0])
