"""The multigrid kernels on their own, through the ABI: the row engine (csrc/rows_ell.hip), the
Gauss-Seidel sweeps and the V-cycle driver (csrc/mg.hip) and every form of the fused coarse end
(csrc/mg_coarse.hip), at the shapes where a launch rule changes.  Needs an MI355X.

Reference and bound: tests/test_multigrid_reference_host.py -- SPMM, one Gauss-Seidel sweep in
dof order and the dense coarse solve in np.longdouble, each with an entrywise bound derived
from the kernels' own arithmetic, composed to MGM and V-cycles.  The check is
|got - ref| <= bound on EVERY entry (a zero bound admits no error), on signed input whose time
slices are scaled over twelve decades.  Forms that the code says share an arithmetic must
agree bit for bit.  Every test prints the path that ran and its largest error in units of the
bound.

Which kernel runs is restated from the arguments and the plan's sizes (ref.rows_launch,
ref.plan_shape, ref.coarse_path: the rules of rows_ell.hip:480-482, mg.hip:462-471 and
mg_coarse.hip:931-1051), never asked of the library.

Buffers: every slab lies inside a flat buffer between sentinel rows, checked after every call;
outputs start as NaN; the padding column of an odd n_loc holds NaN in every INPUT (the kernels
read it with its pair and promise not to let it reach a data column), and the columns behind
the pair -- the slab as a column range of a wider one -- hold a second sentinel that must
survive.

Paths, the catalogue case (ref.ALGEBRAIC) that reaches each, and the largest error in units of
the derived bound, measured on an MI355X (n_loc = 1, 2, 3, 4, 9; M: with cm, -: without):

    form                        K / KU  PAIR    threads  reached by                                     worst
    rows_ell_kernel SPMM        2..20   -       512      test_row_engine[K]: NPF 1, 2, 4 for every K     0.88
    rows_ell_kernel GS          by plan -       512      test_sweeps, even ld: diag-free / full rows     0.75 / 0.34
    gs_group_kernel             CSR     -       256      test_sweeps, odd ld (bit-equal figures)         0.75 / 0.34
    level by level              by plan -       -        every hierarchy; two-level, three-level: alone  0.29
    level by level, flat CSR    -       -       256      row-26 (levels 2, 3), every odd ld              0.29
    mg_coarse_kernel<M>         2..20   pair    512      every fused hierarchy with mg_coarse_lds = 0    0.29
    mg_coarse_lds_kernel<M,P>   2..20   pair    512      arena-3072, width-*, small-s3-v2 (-, M)         0.25
                                        pair    512      jobs-s3 (2202 jobs: descriptors do not fit)     0.04
                                        single  512      arena-3073, -ku12, rows-4096 (-, M)             0.29
    mg_coarse_uniform_kernel    8       pair    512      arena-3072, width-7, small-s3-v2 (-, M; key 2)  0.25
                                8       single  512      rows-4096 (M; -, M with key 2), arena-6144      0.17
                                8       single  1024     arena-6144, rows-4096 (-, default key)          0.006
                                12      pair    512      width-8, -9, -12 (-, M), arena-6145, jobs-s1    0.16
                                12      single  512      arena-3073, arena-3073-ku12 (-, M)              0.29
    none (13 entries: 16 slots) -       pair    512      width-13: the levels' own copies                0.03
    member matrices             8       pair    512      test_families[square] (also key 2)              0.09
                                8       single  512      test_families[rows-4096] (also key 2)           0.19

(A row of 8 entries is 9 slots in the plain copy, so KU = 8 ends at 7 entries: width-7.)  Inside
an arithmetic class -- 'two-step' R (A u - f) everywhere, 'above-Lc' (R A) u - R f above the
fused end, 'fused' on every level -- all forms above agreed bit for bit; one figure per class.

Two rules the catalogue pins beside the arithmetic: on an even ld no call writes a column behind
the pair, also where a level has no ELL copies and the flat CSR kernels run (row-26, n_loc = 1,
ld = 6); and a call of stk_mg_set_member_matrices that is refused for a member without a diagonal
entry leaves members already in use as they were (test_families).  stk_mg_create_from_csr refuses
a pattern that is not structurally symmetric (test_unsymmetric_pattern_is_refused)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import test_multigrid_reference_host as ref

pytestmark = pytest.mark.gpu

MEASURED = {}  # largest error / bound per test of this run (printed; the docstring has a recorded run)

LD = ref.LD
GUARD, SENTINEL, BEHIND = 4, 7.25, -3.5  # 4 guard rows; BEHIND fills the columns behind the pair
NAN = float('nan')
DEFAULTS = dict(mg_strip_mb=250, mg_strip_width=2, mg_zero_start=1, mg_gs_diag_free=1, mg_fuse_restrict=1,
                mg_restrict_one_pass=1, mg_fuse_coarse=1, mg_coarse_lds=1, mg_coarse_uniform=1, rows_force_wide=0,
                # (the Kronecker-sum kernels' keys: tests/test_kron_kernels_gpu.py shares `tuning`)
                ell_wg_per_cu=0, ell_force_wide=0, pack_multi_lanes=1, pack_check_steps=0)


@pytest.fixture(scope='module')
def stk():
    from source import _lib
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    _lib.lib()
    return _lib


@contextlib.contextmanager
def tuning(stk, **keys):
    """Tuning keys for the block, the defaults restored whatever happens."""
    assert set(keys) <= set(DEFAULTS)
    try:
        for k, v in keys.items():
            stk.check(stk.lib().stk_set_tuning(k.encode(), v))
        yield
    finally:
        for k in keys:
            stk.check(stk.lib().stk_set_tuning(k.encode(), DEFAULTS[k]))


def pair_cols(n_loc):
    return (n_loc + 1) & ~1


# ---- buffers ---------------------------------------------------------------------------------
class Slab:
    """A (rows, ld) slab inside a flat buffer of sentinels, NaN-filled; `off` doubles behind the
    16-byte grid."""
    def __init__(self, rows, ld, off=0):
        self.rows, self.ld = rows, ld
        self.start, self.count = GUARD * ld + (GUARD * ld & 1) + off, rows * ld
        self.flat = torch.full((self.start + self.count + GUARD * ld + 2,), SENTINEL, dtype=torch.float64,
                               device='cuda')
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[self.start:self.start + self.count].view(rows, ld)
        self.view.fill_(NAN)
        assert self.view.data_ptr() % 16 == 8 * (off & 1)

    def load(self, X, pad=NAN):
        """Data columns, the padding column of an odd n_loc, and BEHIND in the rest."""
        n_loc = X.shape[1]
        self.n_loc = n_loc
        self.view[:, :n_loc] = torch.from_numpy(np.array(X, dtype=np.float64)).cuda()  # (a copy: cases are read-only)
        self.view[:, n_loc:pair_cols(n_loc)] = pad
        self.view[:, pair_cols(n_loc):] = BEHIND
        return self

    def as_output(self, n_loc):
        self.n_loc = n_loc
        self.view[:, min(pair_cols(n_loc), self.ld):] = BEHIND
        return self

    @property
    def ptr(self):
        return self.view.data_ptr()

    def data(self):
        return self.view[:, :self.n_loc].cpu().numpy()

    def check_frame(self, what, zero_pad=True, flat_output=False):
        """Guards intact, the columns behind the pair untouched, the padding column +0.0.
        flat_output: the output of a V-cycle on an odd ld, where the flat kernels write every
        column from n_loc on as +0.0 (stk_csr_spmm's rule: there are no pairs)."""
        h = self.flat.cpu().numpy()
        assert np.all(h[:self.start] == SENTINEL) and np.all(h[self.start + self.count:] == SENTINEL), (what, 'guard')
        v = h[self.start:self.start + self.count].reshape(self.rows, self.ld)
        if flat_output:
            pad = v[:, self.n_loc:]
            assert np.all(pad == 0.0) and not np.any(np.signbit(pad)), (what, 'padding of an odd ld is not +0.0')
            return
        assert np.all(v[:, min(pair_cols(self.n_loc), self.ld):] == BEHIND), (what, 'column behind the pair written')
        pad = v[:, self.n_loc:min(pair_cols(self.n_loc), self.ld)]
        if zero_pad and pad.size:
            assert np.all(pad == 0.0) and not np.any(np.signbit(pad)), (what, 'padding column is not +0.0')


def report(name, path, worst):
    MEASURED[name] = max(MEASURED.get(name, 0.0), worst)
    print('%-26s %.3f of the bound  %s' % (name, worst, path))


# ---- a. the row engine through stk_ell_spmm ----------------------------------------------------
def _ell_on_device(stk, m, has_m):
    dev = dict(idx=stk.to_dev(m['idx'].astype(np.int32)), va=stk.to_dev(m['va']),
               vm=stk.to_dev(m['vm']) if has_m else None, row_ids=stk.to_dev(m['row_ids']))
    struct = stk.EllRows(m['rows'], m['rows'], m['K'], stk.ptr(dev['idx']), stk.ptr(dev['va']), stk.ptr(dev['vm']),
                         stk.ptr(dev['row_ids']), None, None, 0)
    return struct, dev


def _spmm_call(stk, struct, c, n_loc, ld, zmode, x, cm_dev):
    """One call on fresh buffers: (y slab, z slab or None)."""
    rows = c['m']['rows']
    y = Slab(rows, ld)
    z = None
    if zmode == 2:
        y.load(c['Z'])
        z = y
    else:
        y.as_output(n_loc)
        if zmode == 1:
            z = Slab(rows, ld).load(c['Z'])
    rc = stk.lib().stk_ell_spmm(stk.stream(), ctypes.byref(struct), n_loc, ld, c['m']['cols'], c['ca'], stk.ptr(cm_dev),
                                x.ptr, c['alpha'], c['beta'], z.ptr if z is not None else None, y.ptr)
    stk.check(rc)
    return y, z


@pytest.mark.parametrize('K', ref.SLOTS)
def test_row_engine(stk, K):
    """rows_ell_kernel, MODE_SPMM: every slab length (all NPF instances this K reaches), row
    counts around R, ld as the pair and as a column range, z absent / separate / aliasing y,
    32- and 64-bit addressing, each case twice in a row (both walking directions)."""
    n_locs = ref.n_locs_for(K)
    reachable = {ref.rows_launch(n, K)[2] for n in range(1, 1025)}
    seen_npf, seen_combo, worst_by_npf, case_no = set(), set(), {}, 0
    for n_loc in n_locs:
        P, R, NPF = ref.rows_launch(n_loc, K)
        seen_npf.add(NPF)
        for rows in ref.row_counts(R):
            # ld, the form of z and the addressing go round with the (n_loc, rows) pair; both value
            # forms run on each, so all 36 combinations occur for every K
            extra, zmode, wide = (0, 2, 6)[case_no % 3], (case_no // 3) % 3, (case_no // 9) % 2
            case_no += 1
            if pair_cols(n_loc) + extra > 1024:
                extra = 0  # (no slab wider than 1024 columns)
            for has_m in (False, True):
                seen_combo.add((has_m, extra, zmode, wide))
                ld = pair_cols(n_loc) + extra
                c = ref.spmm_case(K, rows, n_loc, has_m, zmode, seed=K + rows)
                struct, keep = _ell_on_device(stk, c['m'], has_m)
                x = Slab(c['m']['cols'], ld).load(c['X'])
                cm_dev = stk.to_dev(c['cm']) if has_m else None
                what = (K, n_loc, rows, has_m, ld, zmode, wide)
                with tuning(stk, rows_force_wide=wide):
                    outs = [_spmm_call(stk, struct, c, n_loc, ld, zmode, x, cm_dev) for _ in range(2)]
                for y, z in outs:
                    y.check_frame(what)
                    if z is not None and z is not y:
                        z.check_frame(what, zero_pad=False)
                x.check_frame(what, zero_pad=False)
                got = outs[0][0].data()
                assert np.array_equal(got, outs[1][0].data()), (what, 'the two walking directions differ')
                w = ref.ratio(got, c['y'], c['e'], what)
                worst_by_npf[NPF] = max(worst_by_npf.get(NPF, 0.0), w)
    assert seen_npf == reachable, (K, seen_npf, reachable)  # every NPF instance this K can reach
    assert len(seen_combo) == 36, (K, len(seen_combo))
    for NPF, w in sorted(worst_by_npf.items()):
        report('row engine K=%d' % K, 'rows_ell_kernel<SPMM, %d, NPF=%d, vm 0/1, wide 0/1>' % (K, NPF), w)


def test_every_npf_instance_is_reached_by_some_k():
    assert {ref.rows_launch(n, K)[2] for K in ref.SLOTS for n in ref.n_locs_for(K)} == {1, 2, 4}


def test_row_engine_refusals(stk):
    """n_loc = 1025, an odd ld, a pointer 8 bytes off the 16-byte grid, cm without vm: each is
    refused on the host with a message, and no byte of the output changes."""
    K, rows = 5, 40
    lib = stk.lib()
    for what, n_loc, extra, y_off, x_off, with_cm, has_vm in (
            ('n_loc too large', 1025, 0, 0, 0, False, True), ('ld must be even', 9, 1, 0, 0, False, True),
            ('16-byte aligned', 9, 0, 1, 0, False, True), ('16-byte aligned', 9, 0, 0, 1, False, True),
            ('no vm', 9, 0, 0, 0, True, False)):
        c = ref.spmm_case(K, rows, min(n_loc, 1024), True, 0, seed=3)
        struct, keep = _ell_on_device(stk, c['m'], has_vm)
        ld = pair_cols(n_loc) + extra
        x = Slab(c['m']['cols'], ld, off=x_off)
        x.view.fill_(0.5)
        y = Slab(rows, ld, off=y_off)
        before = y.flat.clone()
        cm_dev = stk.to_dev(np.ones(n_loc)) if with_cm else None
        rc = lib.stk_ell_spmm(stk.stream(), ctypes.byref(struct), n_loc, ld, c['m']['cols'], 1.0, stk.ptr(cm_dev),
                              x.ptr, 1.0, 0.0, None, y.ptr)
        torch.cuda.synchronize()
        assert rc != 0, what
        assert what.encode() in lib.stk_last_error(), (what, lib.stk_last_error())
        assert torch.equal(before.view(torch.int64), y.flat.view(torch.int64)), what  # NaN bits included


# ---- plans -------------------------------------------------------------------------------------
def _host(stk, m):
    m = ref._sorted_csr(m)
    arrs = (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.astype(np.float64))
    return stk.CsrHost(m.shape[0], m.shape[1], arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data), arrs


class Plan:
    """stk_mg_create_from_csr on host CSR; the dense inverses are handed over (numpy.linalg.inv
    of the plan's own level-0 matrices, which are checked against the reference's data on the
    way), so that both sides hold the same inverse bit for bit."""
    def __init__(self, stk, H, A, M, P_mats, smoothsteps, vcycles, ca=1.0, cms=(), coords=None, max_ld=16, gs_key=1):
        self.stk, self.H = stk, H
        lib = stk.lib()
        want = [H.dense0()] + [H.dense0(ca, c) for c in cms]
        self.inv = ref.numpy_inverses(H, ca, cms)
        calls, problems = [], []

        def inverse(n0, a_ptr, inv_ptr, user):
            k = len(calls)
            a = np.ctypeslib.as_array(a_ptr, shape=(n0, n0))
            calls.append(k)
            # kind 0 is the Galerkin chain itself: bit for bit the reference's data; the others
            # are ca A_0 + cm M_0, which the host compiler may contract into one rounding
            if not (np.array_equal(a, want[k]) if k == 0 else np.allclose(a, want[k], rtol=4e-16, atol=0.0)):
                problems.append(k)
            np.ctypeslib.as_array(inv_ptr, shape=(n0, n0))[...] = self.inv[k]
            return 0

        INV = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int32, ctypes.POINTER(ctypes.c_double),
                               ctypes.POINTER(ctypes.c_double), ctypes.c_void_p)
        hook = INV(inverse)
        a_h, keep_a = _host(stk, A)
        m_h, keep_m = _host(stk, M) if M is not None else (None, None)
        Ps = [_host(stk, P) for P in P_mats]
        P_arr = (stk.CsrHost * len(Ps))(*[p[0] for p in Ps])
        cms_h = np.ascontiguousarray(cms, dtype=np.float64)
        self.handle = ctypes.c_void_p()
        stk.check(lib.stk_mg_set_coarse_inverse(ctypes.cast(hook, ctypes.c_void_p), None))
        try:
            with tuning(stk, mg_gs_diag_free=gs_key):
                stk.check(lib.stk_mg_create_from_csr(
                    len(P_mats) + 1, ctypes.byref(a_h), ctypes.byref(m_h) if M is not None else None, P_arr,
                    coords.ctypes.data if coords is not None else None, coords.shape[1] if coords is not None else 2,
                    smoothsteps, vcycles, ca, len(cms_h), cms_h.ctypes.data if len(cms_h) else None, max_ld,
                    ctypes.byref(self.handle)))
        finally:
            stk.check(lib.stk_mg_set_coarse_inverse(None, None))
        assert len(calls) == 1 + len(cms) and not problems, (H.name, calls, problems)

    def apply(self, F, n_loc, ld, ca=1.0, cm=None, kind=None):
        """One stk_mg_apply on fresh buffers (u NaN on entry): the output columns."""
        stk = self.stk
        f = Slab(F.shape[0], ld).load(F[:, :n_loc])
        u = Slab(F.shape[0], ld).as_output(n_loc)
        cm_d = stk.to_dev(np.ascontiguousarray(cm[:n_loc])) if cm is not None else None
        kind_d = stk.to_dev(np.ascontiguousarray(kind[:n_loc], dtype=np.int32)) if kind is not None else None
        stk.check(stk.lib().stk_mg_apply(self.handle, stk.stream(), n_loc, ld, ca, stk.ptr(cm_d), stk.ptr(kind_d),
                                         f.ptr, u.ptr))
        torch.cuda.synchronize()
        what = (self.H.name, n_loc, ld)
        f.check_frame(what, zero_pad=False)
        u.check_frame(what, flat_output=bool(ld & 1))
        return u.data()

    def smooth(self, level, U0, F, n_loc, ld, ca, cm, its, backward):
        stk = self.stk
        f = Slab(F.shape[0], ld).load(F[:, :n_loc])
        u = Slab(F.shape[0], ld).load(U0[:, :n_loc])
        cm_d = stk.to_dev(np.ascontiguousarray(cm[:n_loc])) if cm is not None else None
        stk.check(stk.lib().stk_mg_smooth(self.handle, stk.stream(), level, n_loc, ld, ca, stk.ptr(cm_d), its,
                                          int(backward), f.ptr, u.ptr))
        torch.cuda.synchronize()
        what = (self.H.name, 'smooth', n_loc, ld)
        f.check_frame(what, zero_pad=False)
        u.check_frame(what, zero_pad=not (ld & 1))
        return u.data()

    def destroy(self):
        if self.handle:
            self.stk.check(self.stk.lib().stk_mg_destroy(self.handle))
            self.handle = None


# ---- b. Gauss-Seidel sweeps through stk_mg_smooth --------------------------------------------
@pytest.mark.parametrize('name', ref.SWEEP_MATRICES)
def test_sweeps(stk, name):
    """Forward and backward, one and three sweeps from a nonzero start, rows with and without
    their diagonal among the slots (plan key mg_gs_diag_free 0, 1, 2), with and without cm, on
    the ELL engine (even ld, also as a column range) and the flat kernel (odd ld), strip by
    strip and level-wide: against the sequential sweep in dof order."""
    H, A, M, P_mats, coords, n_locs = ref.sweep_problem(name)
    J, T = H.J, max(n_locs)
    lib = stk.lib()
    plans = {key: Plan(stk, H, A, M, P_mats, 1, 1, ref.FAMILY_CA, (), coords, max_ld=T + 7, gs_key=key) for key in (0, 1, 2)}
    worst, strip_runs = {}, {True: 0, False: 0}
    try:
        for with_cm in (False, True):
            for backward in (False, True):
                for its in (1, 3):
                    want = {df: ref.sweep_case(name, with_cm, backward, its, df) for df in (False, True)}
                    U0, F, ca, cm = want[True][:4]
                    for n_loc in n_locs:
                        for ld, engine in ((pair_cols(n_loc), 'ell'), (pair_cols(n_loc) + 4, 'ell'),
                                           (n_loc | 1, 'flat')):
                            got = {}
                            for key in (0, 1, 2):
                                what = (name, with_cm, backward, its, n_loc, ld, key)
                                with tuning(stk, mg_strip_mb=0):
                                    got[key] = plans[key].smooth(J, U0, F, n_loc, ld, ca, cm, its, backward)
                                u, e = want[key == 1][4:]
                                w = ref.ratio(got[key], u[:, :n_loc], e[:, :n_loc], what)
                                path = ('rows_ell_kernel<GS>' if engine == 'ell' else 'gs_group_kernel') + \
                                    (' diag-free' if key == 1 else ' full rows')
                                worst[path] = max(worst.get(path, 0.0), w)
                                if engine == 'ell':
                                    # thin strips: the same updates in another order of launches
                                    stk.check(lib.stk_mg_set_option(plans[key].handle, b'strip_pct', 1))
                                    stk.check(lib.stk_set_tuning(b'mg_strips_used', 0))
                                    with tuning(stk, mg_strip_mb=1, mg_strip_width=0):
                                        strips = plans[key].smooth(J, U0, F, n_loc, ld, ca, cm, its, backward)
                                    assert np.array_equal(strips, got[key]), (what, 'strip-wise differs')
                                    ran = lib.stk_set_tuning(b'mg_strips_used', 1) == 0
                                    strip_runs[ran] += 1
                                    # The meshes have bands enough for two strips whatever the slab.  A matrix
                                    # without coordinates has breadth-first bands or none: the chain gets strips
                                    # in 216 of its 288 calls, the wide group (two bands at most) in none -- there
                                    # this comparison is of two level-wide runs and says nothing (printed below).
                                    assert ran or name in ('chain', 'wide-group'), (what, 'no strip ran')
                            # key 2 keeps the finest level's rows whole, like key 0
                            assert np.array_equal(got[2], got[0]), (name, with_cm, backward, its, n_loc, ld)
    finally:
        stk.check(lib.stk_set_tuning(b'mg_strips_used', 0))
        for p in plans.values():
            p.destroy()
    for path, w in sorted(worst.items()):
        report('sweeps %s' % name, path, w)
    print('sweeps %-19s strips ran in %d of %d strip-wise calls' % (name, strip_runs[True], sum(strip_runs.values())))


# ---- c. whole V-cycles on every coarse form ----------------------------------------------------
N_LOCS = (1, 2, 3, 4, 9)
FORM_KEYS = dict(fuse_coarse='mg_fuse_coarse', coarse_lds='mg_coarse_lds', uniform='mg_coarse_uniform')


def path_name(path):
    """('uniform', 8, False, True, False, 512) -> 'uniform<8,M,single,512>'."""
    if path[0] == 'uniform':
        return 'uniform<%d,%s,%s,%d>%s' % (path[1], 'M' if path[3] else '-', 'pair' if path[4] else 'single', path[5],
                                            ' key 2' if path[2] else '')
    if path[0] == 'lds':
        return 'lds<%s,%s>' % ('M' if path[1] else '-', 'pair' if path[2] else 'single')
    return 'global<%s>' % ('M' if path[1] else '-') if path[0] == 'global' else 'levels'


def _forms_agree(plan, F, n_loc, ld, ca, cm, kind, shape, with_cm, restrict_key, seen):
    """Runs the five forms of the coarse end under one setting of mg_fuse_restrict; returns
    {class: result} for the arithmetic classes that occur, after asserting that the forms
    inside a class agree bit for bit."""
    stk = plan.stk
    out = {}
    for form, keys in ref.FORMS:
        path = ref.coarse_path(shape, ld, with_cm, **keys)
        seen.add(path)
        # with the fused restricted residual the levels of the coarse end take it too when
        # they run one by one; the job lists form R (A u - f) there
        cls = 'two-step' if not restrict_key else ('fused' if path == ('levels',) else 'above-Lc')
        with tuning(stk, mg_fuse_restrict=restrict_key, **{FORM_KEYS[k]: v for k, v in keys.items()}):
            got = plan.apply(F, n_loc, ld, ca, cm, kind)
            if form == 'uniform':
                with tuning(stk, mg_zero_start=0):
                    assert np.array_equal(plan.apply(F, n_loc, ld, ca, cm, kind), got), (form, 'mg_zero_start')
                for one_pass in (0, 2):
                    with tuning(stk, mg_restrict_one_pass=one_pass):
                        assert np.array_equal(plan.apply(F, n_loc, ld, ca, cm, kind), got), (form, 'one pass', one_pass)
        if cls in out:
            assert np.array_equal(got, out[cls][0]), (plan.H.name, n_loc, ld, form, path, 'differs from', out[cls][1])
            out[cls][1].add(path_name(path))
        else:
            out[cls] = (got, {path_name(path)})
    return {cls: (got, ' = '.join(sorted(paths))) for cls, (got, paths) in out.items()}


@pytest.mark.parametrize('name', sorted(ref.ALGEBRAIC))
def test_vcycles(stk, name):
    """stk_mg_apply on an algebraic hierarchy whose sizes sit at a threshold: level by level, the
    global job list, the LDS job list on the levels' own copies and on the uniform copies (512
    threads, default), with mg_zero_start, mg_fuse_restrict and mg_restrict_one_pass either way;
    rows with and without the diagonal among the slots; ld as the pair, as a column range and
    odd; with and without per-slice coefficients where the catalogue entry is a family."""
    A, M, P_mats, ss, vc = ref.algebraic(name)
    H = ref.algebraic_hierarchy(name)
    family = M is not None
    ca_f, cms, cm_f, kind_f = ref.case_family('algebraic', name)
    shapes = {key: ref.plan_shape(H, ss, key) for key in (0, 1)}
    plans = {1: Plan(stk, H, A, M, list(P_mats), ss, vc, ca_f, cms if family else (), None, 16, 1),
             0: Plan(stk, H, A, None, list(P_mats), ss, vc, 1.0, (), None, 16, 0)}
    worst, seen = {}, set()
    try:
        assert stk.lib().stk_mg_coarse_levels(plans[1].handle) == \
            (shapes[1]['Lc'] if shapes[1]['Lc'] >= 1 and shapes[1]['KU'] and family else 0)
        for with_cm in ((False, True) if family else (False,)):
            ca, cm, kind = (ca_f, cm_f, kind_f) if with_cm else (1.0, None, None)
            for n_loc in N_LOCS:
                for ld in (pair_cols(n_loc), pair_cols(n_loc) + 4):
                    for restrict_key in (0, 1):
                        F = ref.vcycle_case('algebraic', name, 'two-step', 1, with_cm)[0]
                        res = _forms_agree(plans[1], F, n_loc, ld, ca, cm, kind, shapes[1], with_cm, restrict_key, seen)
                        for cls, (got, path) in res.items():
                            _, u, e = ref.vcycle_case('algebraic', name, cls, 1, with_cm)
                            w = ref.ratio(got, u[:, :n_loc], e[:, :n_loc], (name, with_cm, n_loc, ld, cls, path))
                            label = '%s: %s' % (cls, path)
                            worst[label] = max(worst.get(label, 0.0), w)
                # an odd ld: the flat kernels, level by level, whatever the keys
                ld = n_loc | 1
                F = ref.vcycle_case('algebraic', name, 'two-step', 1, with_cm)[0]
                got = plans[1].apply(F, n_loc, ld, ca, cm, kind)
                assert ref.coarse_path(shapes[1], ld, with_cm) == ('levels',)
                _, u, e = ref.vcycle_case('algebraic', name, 'two-step', 1, with_cm)
                w = ref.ratio(got, u[:, :n_loc], e[:, :n_loc], (name, with_cm, n_loc, ld, 'odd ld'))
                worst['two-step odd ld'] = max(worst.get('two-step odd ld', 0.0), w)
        # rows with their diagonal among the slots (plan key 0), the reference's forms everywhere
        F, u, e = ref.vcycle_case('algebraic', name, 'two-step', 0, False)
        for n_loc in N_LOCS:
            res = _forms_agree(plans[0], F, n_loc, pair_cols(n_loc), 1.0, None, None, shapes[0], False, 0, seen)
            (got, path), = res.values()
            w = ref.ratio(got, u[:, :n_loc], e[:, :n_loc], (name, 'full rows', n_loc, path))
            worst['two-step full rows'] = max(worst.get('two-step full rows', 0.0), w)
    finally:
        for p in plans.values():
            p.destroy()
    expected = {ref.coarse_path(shapes[1], 10, with_cm, **keys) for with_cm in ((False, True) if family else (False,))
                for _, keys in ref.FORMS}
    assert expected <= seen, expected - seen
    for label, w in sorted(worst.items()):
        report('vcycles %s' % name, label, w)


def test_every_coarse_kernel_is_selected_by_the_catalogue():
    """The twelve selections of launch_uniform, the four mg_coarse_lds_kernel and the two
    mg_coarse_kernel instantiations, by the restated rule over the cases test_vcycles runs
    (which asserts, case by case, that it ran each of them)."""
    sel = ref.selected_paths()
    assert ref.UNIFORM_SITES <= sel and len(ref.UNIFORM_SITES) == 12, ref.UNIFORM_SITES - sel
    assert ref.LDS_SITES <= sel and ref.GLOBAL_SITES <= sel and ('levels',) in sel
    assert ('uniform', 8, False, False, False, 1024) in sel


# ---- d. families: cm, kind and member matrices --------------------------------------------------
def _set_members(stk, plan, level, mats):
    """mats[k]: CSR or None (a NULL indptr) per kind."""
    n_kinds = len(mats)
    ptrs = [(ctypes.c_void_p * n_kinds)() for _ in range(3)]
    keep = []
    for k, C in enumerate(mats):
        if C is None:
            continue
        C = ref._sorted_csr(C)
        arrs = (C.indptr.astype(np.int32), C.indices.astype(np.int32), C.data.astype(np.float64))
        keep.append(arrs)
        for which in range(3):
            ptrs[which][k] = arrs[which].ctypes.data
    return stk.lib().stk_mg_set_member_matrices(plan.handle, level, n_kinds, *ptrs)


@pytest.mark.parametrize('kind_of,name', ref.FAMILY_CASES)
def test_families(stk, kind_of, name):
    """Per-slice coefficients, a different kind on the two slices of a pair, and the members' own
    matrices on the levels of the fused coarse end (kinds no slice names given as NULL): on the
    square and on an algebraic hierarchy whose arena takes the single-step form."""
    H = ref.case_hierarchy(kind_of, name)
    if kind_of == 'mesh':
        A, M, P_mats, coords = ref.mesh_problem(*name)
        ss, vc = 2, 1
    else:
        A, M, P_mats, ss, vc = ref.algebraic(name)
        coords = None
    ca, cms, cm, kind = ref.case_family(kind_of, name)
    shape = ref.plan_shape(H, ss, 1)
    Lc = shape['Lc']
    assert Lc >= 1 and shape['KU'] and (kind_of == 'mesh' or not ref.coarse_path(shape, 10, True)[4])
    plan = Plan(stk, H, A, M, list(P_mats), ss, vc, ca, cms, coords, 16, 1)
    lib = stk.lib()
    worst, seen = {}, set()
    try:
        assert lib.stk_mg_coarse_levels(plan.handle) == Lc
        F = ref.vcycle_case(kind_of, name, 'two-step', 1, True)[0]
        # without member matrices: every level runs on ca A_l + cm[t] M_l
        for n_loc in (1, 2, 3, 9):
            ld = pair_cols(n_loc)
            for restrict_key in (0, 1):
                for cls, (got, path) in _forms_agree(plan, F, n_loc, ld, ca, cm, kind, shape, True, restrict_key,
                                                     seen).items():
                    _, u, e = ref.vcycle_case(kind_of, name, cls, 1, True)
                    w = ref.ratio(got, u[:, :n_loc], e[:, :n_loc], (name, n_loc, cls, path))
                    label = 'combination %s: %s' % (cls, path)
                    worst[label] = max(worst.get(label, 0.0), w)
        # a member without a diagonal entry is refused before anything is in use ...
        named = sorted(set(int(k) for k in kind))
        _, chains, u, e = ref.member_case(kind_of, name)
        broken = chains[named[0]][1].tolil()
        broken[0, 0] = 0.0
        broken = ref._sorted_csr(broken.tocsr())
        broken.eliminate_zeros()
        n_kinds = 1 + len(cms)

        def mats(level, first=None):
            return [(first if (k == named[0] and first is not None) else chains[k][level]) if k in named else None
                    for k in range(n_kinds)]

        before = plan.apply(F, 9, 10, ca, cm, kind)
        assert _set_members(stk, plan, 1, mats(1, broken)) != 0 and b'diagonal' in lib.stk_last_error()
        assert np.array_equal(plan.apply(F, 9, 10, ca, cm, kind), before)
        for level in range(1, Lc + 1):
            stk.check(_set_members(stk, plan, level, mats(level)))
        results = {}
        for n_loc in (1, 2, 3, 9):
            ld = pair_cols(n_loc)
            for uniform in (1, 2):
                path = ref.coarse_path(shape, ld, True, uniform=uniform)
                assert path[0] == 'uniform'
                with tuning(stk, mg_coarse_uniform=uniform):
                    got = plan.apply(F, n_loc, ld, ca, cm, kind)
                results.setdefault(n_loc, got)
                assert np.array_equal(got, results[n_loc]), (name, n_loc, uniform)
                w = ref.ratio(got, u[:, :n_loc], e[:, :n_loc], (name, 'members', n_loc, path))
                label = 'members: %s' % path_name(path)
                worst[label] = max(worst.get(label, 0.0), w)
        assert not np.array_equal(results[9], before)  # the members' own matrices did run
        # ... and once the members are in use: the refused call changes nothing
        assert _set_members(stk, plan, 1, mats(1, broken)) != 0 and b'diagonal' in lib.stk_last_error()
        assert np.array_equal(plan.apply(F, 9, 10, ca, cm, kind), results[9]), 'a refused call changed the plan'
    finally:
        plan.destroy()
    for label, w in sorted(worst.items()):
        report('families %s' % (name if kind_of == 'algebraic' else name[0]), label, w)


def test_unsymmetric_pattern_is_refused(stk):
    """The sweeps' schedule takes a structurally symmetric pattern (include/stk.h): one entry
    without its mirror image is refused at plan creation, with a message that names it."""
    A, M, P_mats, ss, vc = ref.algebraic('two-level')
    A = A.tolil()
    assert A[3, 11] == 0.0 and A[11, 3] == 0.0
    A[3, 11] = -0.125
    A = ref._sorted_csr(A.tocsr())
    a_h, keep_a = _host(stk, A)
    Ps = [_host(stk, P) for P in P_mats]
    P_arr = (stk.CsrHost * len(Ps))(*[p[0] for p in Ps])
    handle = ctypes.c_void_p()
    rc = stk.lib().stk_mg_create_from_csr(len(P_mats) + 1, ctypes.byref(a_h), None, P_arr, None, 2, ss, vc, 1.0, 0, None,
                                          16, ctypes.byref(handle))
    assert rc != 0 and not handle.value
    assert b'structurally symmetric' in stk.lib().stk_last_error() and b'(3, 11)' in stk.lib().stk_last_error()
