"""The Kronecker-sum kernels (csrc/kron_pack.hip, csrc/kron_pack_multi.hip, csrc/kron_ell.hip)
against the np.longdouble restatement of tests/test_kron_reference_host.py, entry by entry:
|got - ref| <= bound, the bound derived there from the kernels' own arithmetic, on signed inputs
whose neighbouring time columns differ by powers of two.

Every catalogue case runs through the ABI on layouts built in NumPy (`dict_layout`,
`explicit_layout`, `ell_layout`), the P1 and banded matrices through the EllMatrices /
PackedEllMatrices wrappers.  x, every per-term slab, y, the ghost buffer, the received rows and
the halo records each lie inside guarded flat buffers (`Slab` of the multigrid tests); y starts
as NaN where beta = 0, the padding column of an odd n_loc is NaN in every input, the columns
behind the pair hold a second sentinel, and after every call the guards must be intact, the
columns behind the pair untouched and the padding column of y +0.0.

Forms that share an arithmetic must agree BIT FOR BIT on this data:

  * one row per slot row = row pairs = plain ELL (dictionary patterns); the explicit-value form
    adds its terms in its own order and is held to the bound only
  * ghost lanes in one pass = pass without ghosts + stk_kron_pack_ghost_apply = the same with
    stk_halo_pack_records + stk_kron_pack_boundary_apply; stk_kron_ell_apply = its local part +
    stk_kron_ell_ghost_apply
  * every slab of a time axis cut in 2, 3 and 8 = the columns of the one-slab apply
  * inputs per term: lane groups = turns = stated steps
  * a workgroup that walks three groups and more = the same apply done as several short applies
    over ranges of slot rows (one group per workgroup each); the plain form = itself with
    another ell_wg_per_cu

The launch of every case is restated from its arguments and the device's CU count
(`Case.launch`), printed, and for the long walks asserted to be three groups or more.

Paths and the catalogue cases that reach them (M: matrix rows; worst |got - ref| / bound of
the recorded MI355X run, 256 CUs):

    path                                                       catalogue cases                          worst
    kron_pack_kernel, one row per slot row, K 5 7 9 12 16,     dict1-K*-nt{1,2,3}-n* (NPF 1, 2, 4),     0.928
      no ghost / GHOST, 1-3 terms                              dict1-ghost-n{1,2,3,24,25}-{00,10,01,11}
    kron_pack_kernel, row pairs, K 8 10 12                     dict2-K*-nt*-n*, dict2-ghost-*           0.928
    kron_pack_kernel, explicit values (NPF = 1 only)           explicit2-K*-nt*-n*, explicit2-ghost-*   0.928
    kron_pack_kernel, MULTI (turns)                            dict{1,2}-turns-n{1,2,9,24,33},          0.709
                                                               dict{1,2}-lanes-fallback-n400
    kron_pack_terms_kernel (lane groups, stated steps)         dict{1,2}-{lanes,steps}-n{1,2,9,24,33}   0.722
    kron_ell_kernel, K 5 7 9 12 16, shared x / x per term      ell1-K*-nt*-n*, ell1-ghost-*,            0.928
                                                               ell-per-term-n{3,24}
    kron_ell_kernel, GENERIC (overflow rows) / WIDE            ell-overflow-K*, ell-wide-K*             0.531
    any_tri = 0 with GHOST                                     *-identity-ghost                         0.726
    W = 65 / 66, a row crossing a wavefront (n_loc 127-129)    *-wave-n{127,128,129}                    0.455
    R = 1 (W > 256); n_loc = 1020                              *-R1-n513; *-longest                     0.645
    the LDS loop shortens R (3 terms, pairs, n_loc <= 2)       dict2-lds-cut, dict2-lds-cut-n1          0.341
    ngroups 1 7 8 9 17, n_units mod R = 0, 1, R - 1            *-g{1,7,8,9,17}-tail{0,1,R-1}            0.681
    3 groups per workgroup (768 / 512 / 256 workgroups)        dict1-walk, dict1-ghost-walk, dict2-walk, 0.649
                                                               dict2-ghost-walk, explicit2-ghost-walk,
                                                               dict1-turns-walk, dict{1,2}-lanes-walk,
                                                               ell1-walk, ell1-ghost-walk
    time axis cut in 2, 3, 8                                   *-ghost-n{24,25}-00                      0.477
    the wrappers, P1 and banded matrices                       square 2 and 4, lshape 3, cube 2,        0.977
                                                               band5, nine, lshape_jitter 2

(One-entry rows of the P1 matrices' boundary dofs make a single rounding against a bound of one
rounding: ratios near 1 are expected there.)
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import test_kron_reference_host as ref
from test_multigrid_kernels_gpu import NAN, Slab, pair_cols, stk, tuning  # noqa: F401  (stk: the fixture)

pytestmark = pytest.mark.gpu

PATHS = {}  # kernel instance -> (worst error / bound, the case that gave it) of this run


@pytest.fixture(scope='module')
def n_cu(stk):
    cu, wave, hbm = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    stk.check(stk.lib().stk_device_info(ctypes.byref(cu), ctypes.byref(wave), ctypes.byref(hbm)))
    assert cu.value >= 8
    return cu.value


def note(L, worst, name):
    key = ref.path_name(L).split(' W=')[0]
    if worst >= PATHS.get(key, (-1.0, ''))[0]:
        PATHS[key] = (worst, name)


def show(title):
    for key in sorted(PATHS):
        print('%-92s %.3f of the bound  (%s)' % (key, PATHS[key][0], PATHS[key][1]))
    print('-- %s' % title)
    PATHS.clear()


# ---- patterns and buffers on the device ------------------------------------------------------------
class PackDev:
    """stk_pack_pattern of a layout, or of the slot rows [u0, u1) of it: the rectangular matrix of
    the rows they serve (M = their number; the columns, and so col_bits, stay)."""
    def __init__(self, stk, lay, units=None, K=None):
        u0, u1 = units or (0, lay['n_units'])
        M = int((lay['row_ids'][u0:u1] >= 0).sum())
        up = lambda a: None if a is None else stk.to_dev(np.ascontiguousarray(a))
        self.keep = (up(lay['slots'][u0:u1].view(np.int32)), up(lay['row_ids'][u0:u1]), up(lay['dict']),
                     up(None if lay['vals'] is None else lay['vals'][u0:u1]))
        self.pat = stk.PackPattern(M, K or lay['K'], lay['col_bits'], lay['n_codes'], lay['n_mats'], lay['rp'],
                                   u1 - u0, *[stk.ptr(t) for t in self.keep])
        self.lay = lay


class EllDev:
    def __init__(self, stk, lay, K=None):
        ovf = lay['ovf']
        self.idx, self.row_ids = stk.to_dev(lay['idx']), stk.to_dev(lay['row_ids'])
        self.vals = [stk.to_dev(v) for v in lay['vals']]
        self.ovf = None if ovf is None else (stk.to_dev(ovf['indptr']), stk.to_dev(ovf['indices']),
                                             [stk.to_dev(v) for v in ovf['vals']])
        self.pat = stk.EllPattern(lay['M'], K or lay['K'], stk.ptr(self.idx), stk.ptr(self.row_ids),
                                  stk.ptr(self.ovf[0]) if ovf else None, stk.ptr(self.ovf[1]) if ovf else None)


class Buffers:
    """The inputs of a case in guarded buffers; outputs are made per call."""
    def __init__(self, stk, c, space, d):
        self.stk, self.c, self.d, self.M = stk, c, d, space.M
        M, ld = space.M, c.ld
        self.x = [Slab(M, ld).load(X) for X in d.X]
        col = lambda v: None if v is None else Slab(M, 1).load(v[:, None])
        self.lo, self.hi = [col(v) for v in d.lo], [col(v) for v in d.hi]
        self.gh = None
        if d.lo[0] is not None or d.hi[0] is not None:
            self.gh = Slab(M, 2).load(np.stack([np.zeros(M) if v is None else v for v in (d.lo[0], d.hi[0])], axis=1))
        self.tri = [None if t is None else stk.to_dev(t) for t in d.tri]
        self.rec = None

    def out(self, beta):
        y = Slab(self.M, self.c.ld)
        return y.load(self.d.Y0) if beta != 0.0 else y.as_output(self.c.n_loc)

    def records(self):
        """stk_halo_pack_records of the shared slab, into a guarded buffer."""
        if self.rec is None:
            self.rec = Slab(self.M, 4)
            self.rec.n_loc = 4
            self.stk.check(self.stk.lib().stk_halo_pack_records(self.stk.stream(), self.M, self.c.n_loc, self.c.ld,
                                                                self.x[0].ptr, None, 1, None, 1, self.rec.ptr))
        return self.rec

    def check_inputs(self, what):
        for s_ in self.x + [v for v in self.lo + self.hi + [self.gh, self.rec] if v is not None]:
            s_.check_frame(what, zero_pad=False)


def pack_terms(stk, B, mats=None):
    terms = (stk.KronPackTerm * len(B.tri))()
    for k, t in enumerate(terms):
        t.tri, t.mat = stk.ptr(B.tri[k]), (k if mats is None else mats[k])
    return terms


def call_pack(stk, P, B, beta, ghosts=True, y=None, x=None):
    c = B.c
    y = B.out(beta) if y is None else y
    gh = B.gh.ptr if (ghosts and B.gh is not None) else None
    stk.check(stk.lib().stk_kron_pack_apply(stk.stream(), ctypes.byref(P.pat), c.n_loc, c.ld, c.nt, pack_terms(stk, B),
                                            (x or B.x[0]).ptr, gh, beta, y.ptr))
    return y


def call_pack_ghost(stk, P, B, y):
    c = B.c
    stk.check(stk.lib().stk_kron_pack_ghost_apply(
        stk.stream(), ctypes.byref(P.pat), c.n_loc, c.ld, c.nt, pack_terms(stk, B), B.x[0].ptr,
        B.lo[0].ptr if B.lo[0] is not None else None, B.hi[0].ptr if B.hi[0] is not None else None, y.ptr))
    return y


def call_pack_boundary(stk, P, B, y):
    c = B.c
    stk.check(stk.lib().stk_kron_pack_boundary_apply(
        stk.stream(), ctypes.byref(P.pat), c.n_loc, c.ld, c.nt, pack_terms(stk, B), B.records().ptr, B.gh.ptr,
        int(B.lo[0] is not None), int(B.hi[0] is not None), y.ptr))
    return y


def call_multi(stk, P, B, beta, form, y=None):
    c = B.c
    y = B.out(beta) if y is None else y
    xs = (ctypes.c_void_p * c.nt)(*[s_.ptr for s_ in B.x])
    t0 = t1 = None
    if form == 'steps':
        rng = [(0, c.n_loc) if s_ is None else s_ for s_ in c.steps()]
        t0 = (ctypes.c_int32 * c.nt)(*[a for a, _ in rng])
        t1 = (ctypes.c_int32 * c.nt)(*[b for _, b in rng])
    with tuning(stk, pack_multi_lanes=0 if form == 'turns' else 2, pack_check_steps=1):
        stk.check(stk.lib().stk_kron_pack_apply_multi_steps(stk.stream(), ctypes.byref(P.pat), c.n_loc, c.ld, c.nt,
                                                            pack_terms(stk, B), xs, t0, t1, beta, y.ptr))
    return y


def ell_terms(stk, E, B, ghosts):
    c = B.c
    terms = (stk.KronEllTerm * c.nt)()
    for k, t in enumerate(terms):
        s_ = k if c.per_term else 0
        t.tri, t.ell_vals = stk.ptr(B.tri[k]), stk.ptr(E.vals[k])
        t.ovf_vals = stk.ptr(E.ovf[2][k]) if E.ovf else None
        t.x = B.x[s_].ptr
        t.x_lo = B.lo[s_].ptr if (ghosts and B.lo[s_] is not None) else None
        t.x_hi = B.hi[s_].ptr if (ghosts and B.hi[s_] is not None) else None
    return terms


def call_ell(stk, E, B, beta, ghosts=True, y=None, **keys):
    c = B.c
    y = B.out(beta) if y is None else y
    with tuning(stk, **keys):
        stk.check(stk.lib().stk_kron_ell_apply(stk.stream(), ctypes.byref(E.pat), c.n_loc, c.ld, c.nt,
                                               ell_terms(stk, E, B, ghosts), beta, y.ptr))
    return y


def call_ell_ghost(stk, E, B, y):
    c = B.c
    stk.check(stk.lib().stk_kron_ell_ghost_apply(stk.stream(), ctypes.byref(E.pat), c.n_loc, c.ld, c.nt,
                                                 ell_terms(stk, E, B, True), y.ptr))
    return y


def same_bits(a, b, what):
    assert torch.equal(a.view.view(torch.int64), b.view.view(torch.int64)), (what, 'differs in some bit')


def layouts(c):
    """Every form the matrices of the case have: {label: (layout, Case of that form)}."""
    K1, out = c.K1, {}
    as_form = lambda form, rp, K: _variant(c, form, rp, K)
    if K1 in ref.ELL_K:
        out['ell'] = as_form('ell', 1, K1)
    if not c.overflow:
        out['dict1'] = as_form('dict', 1, K1)
        if c.space.units is not None:
            K2 = {v: k for k, v in ref.ROW_SLOTS.items()}[K1]
            out['dict2'] = as_form('dict', 2, K2)
            out['explicit'] = as_form('explicit', 2, K2)
    return out


def _variant(c, form, rp, K):
    v = copy.copy(c)
    v.form, v.rp, v.K = form, rp, K
    if form != 'ell':
        v.tune = {}
    return v


# ---- the catalogue -----------------------------------------------------------------------------------
def group_of(c):
    tag = sorted(c.tags)[0]
    if tag == 'instance':
        return 'instance-%s%d-K%d' % (c.form, c.rp, c.K)
    return '%s-%s%d' % (tag, c.form, c.rp) if tag in ('groups', 'ghost') else tag


GROUPS = sorted({group_of(c) for c in ref.CASES.values() if 'walk' not in c.tags})
WALKS = sorted(n for n, c in ref.CASES.items() if 'walk' in c.tags)


def run_case(stk, name, n_cu):
    """The case in every form its matrices have: each inside the bound on every entry, the forms of
    one arithmetic equal bit for bit, every buffer's frame intact.  Returns {label: y Slab}."""
    c = ref.CASES[name]
    space, d, yref, e = ref.case_data(name)
    B = Buffers(stk, c, space, d)
    forms = layouts(c)
    own = {('dict', 1): 'dict1', ('dict', 2): 'dict2', ('explicit', 2): 'explicit', ('ell', 1): 'ell'}[(c.form, c.rp)]
    assert own in forms
    outs = {}
    if c.multi is not None:
        P = PackDev(stk, c.layout())
        for form in ('lanes', 'turns', 'steps'):
            v = copy.copy(c)
            v.multi = form
            outs[form] = (call_multi(stk, P, B, c.beta, form), v.launch(n_cu))
        if 'ell' in forms:
            v = forms['ell']
            outs['ell'] = (call_ell(stk, EllDev(stk, v.layout()), B, c.beta), v.launch(n_cu))
        exact = ('lanes', 'turns', 'steps')
    else:
        dev = {}
        for label, v in forms.items():
            if c.per_term and label != 'ell':
                continue  # (inputs per term with ghost rows: the plain form only)
            if label == 'ell':
                dev[label] = EllDev(stk, v.layout())
                outs[label] = (call_ell(stk, dev[label], B, c.beta, **v.tune), v.launch(n_cu))
            else:
                dev[label] = PackDev(stk, v.layout())
                outs[label] = (call_pack(stk, dev[label], B, c.beta), v.launch(n_cu))
        exact = tuple(k for k in outs if k != 'explicit')
    for label, (y, L) in outs.items():
        y.check_frame((name, label))
        note(L, ref.ratio(y.data(), yref, e, (name, label)), name)
    for label in exact[1:]:
        same_bits(outs[exact[0]][0], outs[label][0], (name, exact[0], label))
    # the overlapped forms of a slab with neighbours (beta = 0: they overwrite)
    if (c.lo or c.hi) and c.multi is None:
        if c.beta != 0.0 and space.M <= 1000:
            y0ref, e0 = ref.reference(_zero_beta(c), space, d)
        for label, (y, L) in list(outs.items()):
            one = y if c.beta == 0.0 else (call_ell(stk, dev[label], B, 0.0, **forms[label].tune) if label == 'ell'
                                           else call_pack(stk, dev[label], B, 0.0))
            if c.beta != 0.0 and space.M <= 1000:
                one.check_frame((name, label, 'beta = 0'))
                note(L, ref.ratio(one.data(), y0ref, e0, (name, label, 'beta = 0')), name)
            if label == 'ell':
                two = call_ell_ghost(stk, dev[label], B, call_ell(stk, dev[label], B, 0.0, ghosts=False, **forms[label].tune))
                parts = [two]
            else:
                two = call_pack_ghost(stk, dev[label], B, call_pack(stk, dev[label], B, 0.0, ghosts=False))
                three = call_pack_boundary(stk, dev[label], B, call_pack(stk, dev[label], B, 0.0, ghosts=False))
                parts = [two, three]
            for q, part in enumerate(parts):
                part.check_frame((name, label, 'split', q))
                same_bits(one, part, (name, label, 'pass + boundary steps', q))
    B.check_inputs(name)
    return {k: v[0] for k, v in outs.items()}, B, forms


def _zero_beta(c):
    c0 = copy.copy(c)
    c0.beta = 0.0
    return c0


@pytest.mark.parametrize('group', GROUPS)
def test_catalogue(stk, n_cu, group):
    names = [n for n, c in ref.CASES.items() if 'walk' not in c.tags and group_of(c) == group]
    assert names
    for name in names:
        run_case(stk, name, n_cu)
    show('%s: %d cases' % (group, len(names)))


@pytest.mark.parametrize('name', WALKS)
def test_long_walks(stk, n_cu, name):
    """A workgroup that walks three and more groups (prefetch in registers, republished through
    LDS behind one barrier) against the same apply in pieces that give every workgroup one group."""
    c = ref.CASES[name]
    L = c.launch(n_cu)
    assert L['walk'] >= 3, (name, n_cu, L)  # recomputed for this device
    outs, B, forms = run_case(stk, name, n_cu)
    print('%s: %s' % (name, ref.path_name(L)))
    if c.form == 'ell':
        for wg in (0, 2):
            v = copy.copy(c)
            v.tune = dict(c.tune, ell_wg_per_cu=wg)
            assert v.launch(n_cu)['walk'] < L['walk']
            y = call_ell(stk, EllDev(stk, c.layout()), B, c.beta, **v.tune)
            same_bits(outs['ell'], y, (name, 'ell_wg_per_cu', wg))
    else:
        lay = c.layout()
        piece = L['R'] * L['grid'] // 2
        y = B.out(c.beta)
        for u0 in range(0, lay['n_units'], piece):
            u1 = min(u0 + piece, lay['n_units'])
            if L['kernel'] == 'kron_pack_terms_kernel':
                Ls = ref.terms_launch(c.K, c.rp, c.nt, u1 - u0, c.n_loc, lay['n_codes'], None, n_cu)
            else:
                Ls = ref.pack_launch(c.K, c.rp, c.nt, u1 - u0, c.n_loc, c.lo or c.hi, c.any_tri, lay['n_codes'],
                                     c.form == 'explicit', c.multi is not None, n_cu)
            assert Ls['walk'] == 1 and Ls['R'] == L['R'], (name, Ls)
            P = PackDev(stk, lay, (u0, u1))
            if c.multi is not None:
                call_multi(stk, P, B, c.beta, c.multi, y=y)
            else:
                call_pack(stk, P, B, c.beta, y=y)
        y.check_frame((name, 'pieces'))
        own = c.multi or {('dict', 1): 'dict1', ('dict', 2): 'dict2', ('explicit', 2): 'explicit'}[(c.form, c.rp)]
        same_bits(outs[own], y, (name, 'one apply against %d short ones' % -(-lay['n_units'] // piece)))
    show(name)


# ---- a cut time axis ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('dict1-ghost-n24-00', 'dict2-ghost-n25-00', 'explicit2-ghost-n25-00', 'ell1-ghost-n24-00'))
def test_every_slab_of_a_cut_time_axis_equals_the_one_slab_apply(stk, n_cu, name):
    """2, 3 and 8 cuts: each slab with its neighbours' columns as ghost rows and its part of the
    time factors, through every form, bit for bit the columns of the whole."""
    whole_c = ref.CASES[name]
    assert not whole_c.lo and not whole_c.hi
    space, d, yref, e = ref.case_data(name)
    whole, _, forms = run_case(stk, name, n_cu)
    n = whole_c.n_loc
    for cuts in (2, 3, 8):
        edges = [len(a) for a in np.array_split(np.arange(n), cuts)]
        a = 0
        for width in edges:
            b = a + width
            c = copy.copy(whole_c)
            c.n_loc, c.lo, c.hi, c.ld = width, a > 0, b < n, pair_cols(width) + whole_c.extra
            ds = ref.Data()
            ds.X, ds.Y0 = [d.X[0][:, a:b]], d.Y0[:, a:b]
            ds.lo, ds.hi = [d.X[0][:, a - 1] if a > 0 else None], [d.X[0][:, b] if b < n else None]
            ds.tri = [None if t is None else np.ascontiguousarray(t[:, a:b]) for t in d.tri]
            B = Buffers(stk, c, space, ds)
            for label, v in forms.items():
                vs = copy.copy(c)
                vs.form, vs.rp, vs.K = v.form, v.rp, v.K
                if label == 'ell':
                    y = call_ell(stk, EllDev(stk, vs.layout()), B, c.beta)
                else:
                    y = call_pack(stk, PackDev(stk, vs.layout()), B, c.beta)
                y.check_frame((name, cuts, a, label))
                note(vs.launch(n_cu), ref.ratio(y.data(), yref[:, a:b], e[:, a:b], (name, cuts, a, label)), name)
                assert np.array_equal(y.data().view(np.int64), whole[label].data()[:, a:b].view(np.int64)), \
                    (name, cuts, a, label)
            B.check_inputs((name, cuts, a))
            a = b
    show('%s cut in 2, 3 and 8' % name)


# ---- the wrappers ------------------------------------------------------------------------------------
WRAPPED = ref.WRAPPER_FAMILIES + (('lshape_jitter', 2),)


@pytest.mark.parametrize('family', WRAPPED, ids=str)
def test_wrappers(stk, n_cu, family):
    """EllMatrices / PackedEllMatrices on the P1 matrices of small meshes and on banded matrices:
    apply, apply_local + apply_ghost, the packed forms with one row and with pairs, their
    apply_ghost and apply_boundary, apply_multi -- on guarded buffers, against the bound."""
    from source.linop import EllMatrices, time_factor_steps
    mats_all = ref.wrapper_matrices(family)
    explicit = family == ('lshape_jitter', 2)
    i = WRAPPED.index(family)
    for j, n_loc in enumerate((1, 2, 3, 9, 24, 65)):
        nt = 1 + (i + j) % 3
        lo, hi = ref.GHOST_ROUND[(i + j) % 4]
        beta = ref.BETA_ROUND[j % 3]
        c, space, d, yref, e = ref.wrapper_case(family, n_loc, nt, lo, hi, beta, ref.TRI_ROUND[(i + j) % 4][:nt], seed=j)
        ell = EllMatrices(mats_all[:nt], [mats_all[0]])
        assert ell.K == c.K and ell.M == space.M
        B = Buffers(stk, c, space, d)
        what = (family, n_loc, nt)
        ld = c.ld
        y_ell = B.out(beta)
        ell.apply([(B.tri[k], k, B.x[0].view, B.lo[0] and B.lo[0].view, B.hi[0] and B.hi[0].view) for k in range(nt)],
                  n_loc, ld, beta, y_ell.view)
        y_ell.check_frame(what)
        note(ref.ell_launch(ell.K, nt, ell.M, n_loc, ld, c.any_tri, ell.ovf_indptr is not None, n_cu=n_cu),
             ref.ratio(y_ell.data(), yref, e, what), str(what))
        packs = []
        for rp in (1, 2):
            p = ell.packed_variant(rp)
            if explicit:  # values that do not repeat: no dictionary, pairs with explicit values
                assert (rp == 1 and not p.ok) or (p.ok and p.explicit and p.rows_per_unit == 2), what
            elif ell.K > 9:  # (no pair kernel for rows of more than 9 entries: the one-row form again)
                assert p.ok and p.rows_per_unit == 1, (what, rp)
            else:
                assert p.ok and p.rows_per_unit == rp, (what, rp)
            if p.ok and p not in packs:
                packs.append(p)
        specs = [(B.tri[k], k) for k in range(nt)]
        for p in packs:
            y = B.out(beta)
            p.apply(specs, B.x[0].view, B.gh and B.gh.view, n_loc, ld, beta, y.view)
            y.check_frame((what, p.rows_per_unit))
            L = ref.pack_launch(p.K, p.rows_per_unit, nt, p.n_units, n_loc, lo or hi, c.any_tri, p.n_codes, p.explicit,
                                n_cu=n_cu)
            note(L, ref.ratio(y.data(), yref, e, (what, p.rows_per_unit)), str(what))
            if not p.explicit:
                same_bits(y_ell, y, (what, 'plain and packed', p.rows_per_unit))
            if (lo or hi) and beta == 0.0:
                two = B.out(0.0)
                p.apply(specs, B.x[0].view, None, n_loc, ld, 0.0, two.view)
                p.apply_ghost(specs, B.x[0].view, B.lo[0] and B.lo[0].view, B.hi[0] and B.hi[0].view, n_loc, ld, two.view)
                three = B.out(0.0)
                p.apply(specs, B.x[0].view, None, n_loc, ld, 0.0, three.view)
                p.apply_boundary(specs, B.records().view, B.gh.view, lo, hi, n_loc, ld, three.view)
                for part in (two, three):
                    part.check_frame((what, 'split'))
                    same_bits(y, part, (what, 'pass + boundary steps', p.rows_per_unit))
        if (lo or hi) and beta == 0.0:
            two = B.out(0.0)
            full = [(B.tri[k], k, B.x[0].view, B.lo[0] and B.lo[0].view, B.hi[0] and B.hi[0].view) for k in range(nt)]
            ell.apply_local(full, n_loc, ld, 0.0, two.view)
            ell.apply_ghost(full, n_loc, ld, two.view)
            two.check_frame((what, 'local + ghost'))
            same_bits(y_ell, two, (what, 'local + ghost'))
        B.check_inputs(what)
        # inputs per term (no ghost rows), the three forms through apply_multi
        if nt >= 2 and not explicit:
            cm, space, dm, ymref, em = ref.wrapper_case(family, n_loc, nt, False, False, beta, ('id', 'gt', 'zeros')[:nt],
                                                        seed=j)
            cm.per_term = True
            for redraw in range(16):
                dm = ref.draw(cm, space, redraw)
                ymref, em = ref.reference(cm, space, dm)
                if ref.bound_is_informative(ymref, em):
                    break
            Bm = Buffers(stk, cm, space, dm)
            steps = [time_factor_steps(t) for t in dm.tri]
            for p in packs:
                got = []
                for form in ('lanes', 'turns', 'steps'):
                    y = Bm.out(beta)
                    with tuning(stk, pack_multi_lanes=0 if form == 'turns' else 2, pack_check_steps=1):
                        p.apply_multi([(Bm.tri[k], k, Bm.x[k].view) for k in range(nt)], n_loc, ld, beta, y.view,
                                      steps=steps if form == 'steps' else None)
                    y.check_frame((what, form))
                    L = ref.terms_launch(p.K, p.rows_per_unit, nt, p.n_units, n_loc, p.n_codes,
                                         steps if form == 'steps' else None, n_cu) if form != 'turns' else None
                    L = L or ref.pack_launch(p.K, p.rows_per_unit, nt, p.n_units, n_loc, False, True, p.n_codes,
                                             multi=True, n_cu=n_cu)
                    note(L, ref.ratio(y.data(), ymref, em, (what, form)), str(what))
                    got.append(y)
                same_bits(got[0], got[1], (what, 'lanes and turns'))
                same_bits(got[0], got[2], (what, 'lanes and stated steps'))
            Bm.check_inputs((what, 'per term'))
    show('wrappers on %s' % (family,))


# ---- refusals ----------------------------------------------------------------------------------------
def test_refusals(stk):
    """An odd ld, x == y, a slab 8 bytes off the 16-byte grid, n_loc one above the limit, a K
    without an instantiation, a slot row that does not fit the LDS: each refused on the host by
    its message, no byte of y changed."""
    lib = stk.lib()
    c = ref.CASES['dict1-ghost-n24-00']
    space, d, _, _ = ref.case_data(c.name)
    forms = layouts(c)
    assert (ref.N_LOC_MAX + 2) // 2 + 2 == ref.BS + 1
    table = (('ld must be even', dict(ld=c.ld + 1)), ('aliases', dict(alias=True)), ('16-byte aligned', dict(x_off=1)),
             ('16-byte aligned', dict(y_off=1)), ('n_loc=%d too large' % (ref.N_LOC_MAX + 1), dict(n_loc=ref.N_LOC_MAX + 1)),
             ('is not one of', dict(K=6)), ('is not one of 8, 10, 12 (row pairs)', dict(K=9, rp=2)),
             ('bytes of LDS per workgroup', dict(n_loc=900, rp=2)))  # (two terms in pairs: 809 steps at the most)
    for entry in ('pack', 'ell', 'multi'):
        for message, how in table:
            if how.get('rp') == 2 and entry != 'pack':
                continue
            n_loc = how.get('n_loc', c.n_loc)
            ld = how.get('ld', pair_cols(n_loc))
            x = Slab(space.M, ld, off=how.get('x_off', 0))
            x.view.fill_(0.5)
            y = x if how.get('alias') else Slab(space.M, ld, off=how.get('y_off', 0))
            before = y.flat.clone()
            tri = stk.to_dev(np.ones((3, n_loc)))
            if entry == 'ell':
                E = EllDev(stk, forms['ell'].layout(), K=how.get('K'))
                terms = (stk.KronEllTerm * 2)()
                for k, t in enumerate(terms):
                    t.tri, t.ell_vals, t.x = stk.ptr(tri), stk.ptr(E.vals[k]), x.ptr
                rc = lib.stk_kron_ell_apply(stk.stream(), ctypes.byref(E.pat), n_loc, ld, 2, terms, 0.0, y.ptr)
            else:
                P = PackDev(stk, forms['dict2' if how.get('rp') == 2 else 'dict1'].layout(), K=how.get('K'))
                terms = (stk.KronPackTerm * 2)()
                for k, t in enumerate(terms):
                    t.tri, t.mat = stk.ptr(tri), k
                if entry == 'pack':
                    rc = lib.stk_kron_pack_apply(stk.stream(), ctypes.byref(P.pat), n_loc, ld, 2, terms, x.ptr, None, 0.0,
                                                 y.ptr)
                else:
                    xs = (ctypes.c_void_p * 2)(x.ptr, x.ptr)
                    with tuning(stk, pack_multi_lanes=2):
                        rc = lib.stk_kron_pack_apply_multi(stk.stream(), ctypes.byref(P.pat), n_loc, ld, 2, terms, xs, 0.0,
                                                           y.ptr)
            torch.cuda.synchronize()
            assert rc != 0, (entry, message)
            said = lib.stk_last_error().decode()
            if entry == 'multi':  # (its own wording of two of them)
                message = {'aliases': 'aliasing the output', 'is not one of': 'has no instantiation'}.get(message, message)
            assert message in said, (entry, message, said)
            assert torch.equal(before.view(torch.int64), y.flat.view(torch.int64)), (entry, message)  # NaN bits included
