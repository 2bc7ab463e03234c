"""The plan builders on the device (csrc/ell_build.hip: stk_csr_galerkin, stk_ell_from_csr,
stk_gs_depth_step) through the ABI and through their Python callers, on the catalogue of
tests/test_plan_builders_reference_host.py.  Everything is bit for bit: the Galerkin products are
SciPy's sorted `(R @ A) @ P`, the ELL copies the per-row loop's arrays, the depths the longest-path
recurrence.  Every output lies in a guarded flat buffer (`Flat` of the vector tests) pre-filled with
a sentinel; what a kernel must not write -- the slots of a product row from row_counts[i] on, the
whole row and the count of a row that overflows -- must still hold it.

Paths and the catalogue cases that reach them:

    path                                                         cases
    galerkin_kernel, "exact zero is not emitted", in R A and     cancel-nc{64,65,129}, cancel-ra-nc*
      in (R A) P; unsorted rows                                    (every case stores its rows shuffled)
    every sum in SciPy's order, separately rounded               roundings-nc*, roundings-ra-nc*
    nt == CAP: 64 columns fit, the 65th reports CAP + 1          ra-64; ra-65, ra-70 (-> 65, not 70)
    ncol == CAP in (R A) P                                       rap-64; rap-65
    ncol > cap_out reports ncol                                  rap-cap{1,16,32}-fits / -over
    touched columns past cap through a sum that cancels          excess-cancels-in-rap (17), -in-ra (21)
    empty rows of R, of A, of P; a second and third workgroup,   empty-nc*, empty-ra-nc*; nc 65, 129
      dead threads in the last
    the host fall-back of galerkin_product                       every overflowing case, and cap 64 > 16 / 32
    ell_from_csr_kernel: rows of 0 entries, no diagonal,         ell_cases(): order x pad_col x grp x strip_diag
      unsorted; pad_col 0 / 3 / first kept column or the row;      x vm x (K = longest, K one short)
      K one short -> overflow = the longest kept row
    second grid-stride pass (n_pos = 1048577, K = 2)             long_ell_matrix()
    EllRowsMatrix.check() on a Gauss-Seidel copy of a matrix     test_ell_rows_matrix_reports_a_missing_diagonal
      without a diagonal
    gs_depth_kernel: depth 299; star; rows without entries;      chain-300; star; empty-rows; unsymmetric;
      n = 1, 255, 256, 257; second grid-stride pass               n1, n1-empty, n255 .. n257; short-chains-1048577

Recorded MI355X run: every case bit for bit (there are no tolerances here, so no ratios).  Before
ell_build.hip was built without contraction, empty-nc129 -- the first case in order with values that
are not small integers -- had 206 entries a few ulps off SciPy: the kernel's multiply and add were
one fused instruction.
"""
import numpy as np
import pytest
import torch

import test_plan_builders_reference_host as ref
from test_multigrid_kernels_gpu import BEHIND, NAN, stk  # noqa: F401  (stk: the fixture)
from test_vector_kernels_gpu import Flat, refused, same

pytestmark = pytest.mark.gpu

I32 = torch.int32
IFILL, IGUARD = -7, -9  # what an int32 output holds before the call; its guards


def ints(n, fill=IFILL):
    return Flat(n, fill, I32, sentinel=IGUARD)


def upload(stk, m):
    return [stk.to_dev(np.asarray(m.indptr, dtype=np.int32)), stk.to_dev(np.asarray(m.indices, dtype=np.int32)),
            stk.to_dev(np.asarray(m.data, dtype=np.float64))]


# ---- stk_csr_galerkin -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ref.GALERKIN))
def test_galerkin(stk, name):
    from source import multigrid as mgm
    R, A, P, cap = ref.GALERKIN[name]
    nc = R.shape[0]
    want = ref.galerkin_ref(R, A, P)
    over = ref.galerkin_overflow_rows(R, A, P, cap)
    keep = upload(stk, R) + upload(stk, A) + (upload(stk, P) if P is not None else [None] * 3)
    counts, idx, val, flag = ints(nc), ints(nc * cap), Flat(nc * cap, BEHIND), ints(1, 0)
    stk.check(stk.lib().stk_csr_galerkin(stk.stream(), nc, *[stk.ptr(t) for t in keep], cap, counts.ptr, idx.ptr,
                                         val.ptr, flag.ptr))
    assert flag.host()[0] == ref.galerkin_overflow(R, A, P, cap) == ref.OVERFLOWS.get(name, 0), (name, flag.host())
    e_counts, e_idx, e_val = np.full(nc, IFILL, np.int32), np.full((nc, cap), IFILL, np.int32), np.full((nc, cap), BEHIND)
    for i in np.flatnonzero(over == 0):  # rows that fit: SciPy's; the others: untouched
        a, b = want.indptr[i], want.indptr[i + 1]
        e_counts[i], e_idx[i, :b - a], e_val[i, :b - a] = b - a, want.indices[a:b], want.data[a:b]
    same(counts.host(), e_counts, (name, 'row_counts'))
    same(idx.host().reshape(nc, cap), e_idx, (name, 'columns'))
    same(val.host().reshape(nc, cap), e_val, (name, 'values'))
    if not over.any():
        assert e_counts.sum() == want.nnz
    # the caller: SciPy's matrix whether the kernel holds the rows or the host takes over
    got = mgm.galerkin_product(R, A, P)
    inner = 16 if P is not None else 32
    assert got.has_sorted_indices and got.shape == want.shape
    same(got.indptr.astype(np.int64), want.indptr.astype(np.int64), (name, 'galerkin_product', 'indptr'))
    same(got.indices.astype(np.int64), want.indices.astype(np.int64), (name, 'galerkin_product', 'indices'))
    same(got.data, want.data, (name, 'galerkin_product', 'data', 'host' if ref.galerkin_overflow(R, A, P, inner) else 'device'))


def test_galerkin_product_takes_both_ways():
    ways = {bool(ref.galerkin_overflow(R, A, P, 16 if P is not None else 32)) for R, A, P, _ in ref.GALERKIN.values()}
    assert ways == {False, True}


def test_galerkin_refusals(stk):
    R, A, P, _ = ref.GALERKIN['roundings-nc64']
    nc = R.shape[0]
    dR, dA, dP = upload(stk, R), upload(stk, A), upload(stk, P)
    counts, idx, val, flag = ints(nc), ints(nc * 64), Flat(nc * 64, BEHIND), ints(1, 0)
    p = stk.ptr

    def call(cap, P3, **k):
        return stk.lib().stk_csr_galerkin(stk.stream(), k.get('nc', nc), *[p(t) for t in dR + dA + P3], cap, counts.ptr,
                                          idx.ptr, val.ptr, k.get('flag', flag.ptr))
    refused(stk, call(0, dP), 'cap=0')
    refused(stk, call(65, dP), 'cap=65')
    refused(stk, call(-1, dP), 'cap')
    for gone in range(3):
        part = [None if k == gone else t for k, t in enumerate(dP)]
        refused(stk, call(16, part), 'whole or not at all')
    refused(stk, call(16, [dP[0], None, None]), 'whole or not at all')
    refused(stk, call(16, dP, nc=0), 'null pointer')
    refused(stk, call(16, dP, flag=None), 'null pointer')
    torch.cuda.synchronize()
    assert np.all(counts.host() == IFILL) and np.all(idx.host() == IFILL) and np.all(val.host() == BEHIND)
    assert flag.host()[0] == 0
    stk.check(call(64, dP))
    assert flag.host()[0] == 0 and counts.host().sum() == ref.galerkin_ref(R, A, P).nnz


# ---- stk_ell_from_csr -------------------------------------------------------------------------------------
def run_ell(stk, dev, n_pos, kw, with_dia=True):
    d_ptr, d_idx, d_va, d_vm, d_grp = dev
    K, vm = kw['K'], kw['vm'] is not None
    out = dict(idx=ints(n_pos * K), va=Flat(n_pos * K, NAN), vm=Flat(n_pos * K, NAN) if vm else None,
               dia_a=Flat(n_pos, NAN) if with_dia else None, dia_m=Flat(n_pos, NAN) if with_dia and vm else None,
               overflow=ints(1, 0))
    d_order = None if kw['order'] is None else stk.to_dev(np.asarray(kw['order'], dtype=np.int32))
    ptr = lambda f: None if f is None else f.ptr
    stk.check(stk.lib().stk_ell_from_csr(
        stk.stream(), n_pos, K, stk.ptr(d_order), stk.ptr(d_ptr), stk.ptr(d_idx), stk.ptr(d_va),
        stk.ptr(d_vm) if vm else None, int(kw['strip_diag']), stk.ptr(d_grp) if kw['grp'] is not None else None,
        int(kw['pad_col']), ptr(out['idx']), ptr(out['va']), ptr(out['vm']), ptr(out['dia_a']), ptr(out['dia_m']),
        out['overflow'].ptr))
    return {k: None if f is None else f.host(k) for k, f in out.items()}


@pytest.mark.parametrize('full_diagonal', (False, True))
def test_ell_from_csr(stk, full_diagonal):
    indptr, indices, va, vm, grp = ref.ell_matrix(full_diagonal)
    dev = [stk.to_dev(a) for a in (indptr, indices, va, vm, grp)]
    n = len(indptr) - 1
    shorts = 0
    for name, kw in ref.ell_cases(full_diagonal):
        want = ref.ell_loop(indptr, indices, va, **kw)
        n_pos, K, fits = len(want['fits']), kw['K'], want['fits']
        got = run_ell(stk, dev, n_pos, kw)
        assert got['overflow'][0] == want['overflow'], (name, 'overflow is not the longest kept row')
        shorts += want['overflow'] > 0
        assert fits.any()
        for key in ('idx', 'va', 'vm'):
            assert (got[key] is None) == (want[key] is None)
            if want[key] is not None:
                same(got[key].reshape(n_pos, K)[fits], want[key][fits], (name, key))
        same(got['dia_a'], want['dia_a'], (name, 'dia_a'))
        if want['dia_m'] is not None:
            same(got['dia_m'], want['dia_m'], (name, 'dia_m'))
    assert shorts > 20
    # dia_a / dia_m may be NULL; n_pos = 0 returns 0 and touches nothing
    name, kw = ref.ell_cases(full_diagonal)[0]
    got = run_ell(stk, dev, n, kw, with_dia=False)
    same(got['idx'].reshape(n, kw['K']), ref.ell_loop(indptr, indices, va, **kw)['idx'], 'no dia arrays')
    got = run_ell(stk, dev, 0, kw)
    assert got['overflow'][0] == 0 and got['idx'].size == 0


def test_ell_from_csr_refusals(stk):
    indptr, indices, va, vm, grp = ref.ell_matrix(True)
    d_ptr, d_idx, d_va, d_vm, _ = [stk.to_dev(a) for a in (indptr, indices, va, vm, grp)]
    n, K = len(indptr) - 1, 9
    idx, o_va, o_vm, flag = ints(n * K), Flat(n * K, NAN), Flat(n * K, NAN), ints(1, 0)
    p = stk.ptr

    def call(vm_in, vm_out, K=K, n_pos=n, flag_ptr=flag.ptr):
        return stk.lib().stk_ell_from_csr(stk.stream(), n_pos, K, None, p(d_ptr), p(d_idx), p(d_va), vm_in, 0, None, 0,
                                          idx.ptr, o_va.ptr, vm_out, None, None, flag_ptr)
    refused(stk, call(p(d_vm), None), 'go together')
    refused(stk, call(None, o_vm.ptr), 'go together')
    refused(stk, call(None, None, K=0), 'bad arguments')
    refused(stk, call(None, None, n_pos=-1), 'bad arguments')
    refused(stk, call(None, None, flag_ptr=None), 'bad arguments')
    assert call(None, None, n_pos=0) == 0
    torch.cuda.synchronize()
    assert np.all(idx.host() == IFILL) and np.all(np.isnan(o_va.host())) and np.all(np.isnan(o_vm.host()))
    assert flag.host()[0] == 0


def test_ell_from_csr_second_grid_stride_pass(stk):
    from source.linop import EllRowsMatrix
    indptr, indices, va = ref.long_ell_matrix()
    n = len(indptr) - 1
    assert n == 1048577 > 4096 * 256
    dev = [stk.to_dev(a) for a in (indptr, indices, va)] + [None, None]
    got = run_ell(stk, dev, n, dict(order=None, K=2, strip_diag=0, grp=None, pad_col=-1, vm=None))
    host = EllRowsMatrix.__new__(EllRowsMatrix)  # (vouched for by the per-row loop in the host file)
    host._build_with_numpy(indptr, indices, va, None, np.arange(n), 2, False, -1, True, None)
    assert got['overflow'][0] == 0
    same(got['idx'].reshape(n, 2), host.idx.cpu().numpy(), 'idx')
    same(got['va'].reshape(n, 2), host.va.cpu().numpy(), 'va')
    same(got['dia_a'], host.dia_a.cpu().numpy(), 'dia_a')


@pytest.mark.parametrize('full_diagonal', (False, True))
def test_ell_rows_matrix_is_the_numpy_builder(stk, full_diagonal):
    """The wrapper sizes K itself (the next instantiated slot count): its device copy, array by array,
    against _build_with_numpy and the per-row loop."""
    from source.linop import EllRowsMatrix
    indptr, indices, va, vm, grp = ref.ell_matrix(full_diagonal)
    n = len(indptr) - 1
    forms = [dict(), dict(pad_col=3), dict(earlier_group=grp, pad_col=-1)]
    if full_diagonal:
        forms += [dict(diag=True), dict(dia_values=True), dict(dia_values=True, earlier_group=grp, pad_col=-1)]
    for oname, order in ref.ell_orders(n).items():
        for kw in forms:
            for use_vm in (vm, None):
                dev = EllRowsMatrix(indptr, indices, va, use_vm, order, **kw)
                assert dev.ok
                dev.check()
                want_dia = kw.get('diag', False) or kw.get('dia_values') is not None
                loop = ref.ell_loop(indptr, indices, va, use_vm, order, dev.K, int(kw.get('diag', False)),
                                    kw.get('earlier_group'), kw.get('pad_col', 0))
                assert loop['overflow'] == 0
                host = EllRowsMatrix.__new__(EllRowsMatrix)
                host._build_with_numpy(indptr, indices, va, use_vm,
                                       np.arange(n) if order is None else order.astype(np.int64), dev.K,
                                       kw.get('diag', False), kw.get('pad_col', 0), want_dia, kw.get('earlier_group'))
                for key in ('idx', 'va', 'vm', 'dia_a', 'dia_m'):
                    a, b = getattr(dev, key), getattr(host, key)
                    assert (a is None) == (b is None), (oname, kw.keys(), key)
                    if a is not None:
                        same(a.cpu().numpy(), b.cpu().numpy(), (oname, list(kw), key, 'numpy builder'))
                        same(a.cpu().numpy(), loop[key].astype(a.cpu().numpy().dtype), (oname, list(kw), key, 'loop'))


def test_ell_rows_matrix_reports_a_missing_diagonal(stk):
    """A Gauss-Seidel copy counts on a diagonal entry in every row: row 2 has five entries and none on
    the diagonal, K is sized for four, and check() says so (overflow = 5, the longest kept row)."""
    from source.linop import EllRowsMatrix
    m = ref.csr_rows([[(0, 2.0), (1, 1.0)], [(1, 2.0), (0, 1.0)], [(5, 1.0), (0, 1.0), (1, 1.0), (3, 1.0), (4, 1.0)],
                      [(3, 2.0)], [(4, 2.0), (3, 1.0)], [(5, 2.0)]], 6)
    copy = EllRowsMatrix(m.indptr, m.indices, m.data, diag=True)
    assert copy.ok and copy.K == 4
    with pytest.raises(stk.StkError, match='a row has 5 entries for 4 slots'):
        copy.check()
    with pytest.raises(stk.StkError, match='5 entries'):
        EllRowsMatrix.check_all([copy])
    loop = ref.ell_loop(m.indptr, m.indices, m.data, None, None, 4, 1, None, 0)
    fits = loop['fits']
    assert fits.tolist() == [True, True, False, True, True, True] and loop['overflow'] == 5
    same(copy.idx.cpu().numpy()[fits], loop['idx'][fits], 'rows that fit')
    same(copy.va.cpu().numpy()[fits], loop['va'][fits], 'rows that fit')
    same(copy.dia_a.cpu().numpy(), loop['dia_a'], 'diagonal (0.0 where there is none)')


# ---- stk_gs_depth_step --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.DEPTH)
def test_depth_relaxation(stk, name):
    from source import multigrid as mgm
    ip, ix = ref.depth_case(name)
    n = len(ip) - 1
    d_ip, d_ix = stk.to_dev(ip), stk.to_dev(ix if len(ix) else np.zeros(1, np.int32))
    for backward in (False, True):
        want = ref.depth_want(name, backward)
        # the caller
        ptr, rows = mgm.gauss_seidel_schedule(ip, ix, backward, on_device=(d_ip, d_ix))
        p2, r2 = mgm._groups_by_depth(want.astype(np.int64), n, backward)
        same(ptr, p2, (name, backward, 'group pointers')), same(rows, r2, (name, backward, 'rows'))
        # the ABI, step by step: every relaxation is the restated one, `changed` is 0 at the fixed point alone
        depth = [ints(n, 0), ints(n)]
        host, steps = np.zeros(n, dtype=np.int32), 0
        while True:
            changed = ints(1, 0)
            src, dst = depth[steps & 1], depth[1 - (steps & 1)]
            stk.check(stk.lib().stk_gs_depth_step(stk.stream(), n, stk.ptr(d_ip), stk.ptr(d_ix), int(backward), src.ptr,
                                                  dst.ptr, changed.ptr))
            new = ref.depth_step_ref(ip, ix, backward, host)
            same(dst.host(), new, (name, backward, steps))
            same(src.host(), host, (name, backward, steps, 'depth_in written'))
            moved = not np.array_equal(new, host)
            assert changed.host()[0] == int(moved), (name, backward, steps)
            if not moved:
                break
            host, steps = new, steps + 1
            assert steps <= n
        same(host, want, (name, backward))
        assert steps == want.max()
        if name == 'chain-300':
            assert steps == 299  # and the 300th reported no change


def test_depth_step_refusals(stk):
    ip, ix = ref.depth_case('n255')
    d_ip, d_ix, d, changed = stk.to_dev(ip), stk.to_dev(ix), ints(255, 0), ints(1, 0)
    p = stk.ptr
    refused(stk, stk.lib().stk_gs_depth_step(stk.stream(), 255, p(d_ip), p(d_ix), 0, d.ptr, d.ptr, changed.ptr),
            'bad arguments')
    refused(stk, stk.lib().stk_gs_depth_step(stk.stream(), 0, p(d_ip), p(d_ix), 0, d.ptr, d.ptr + 4, changed.ptr),
            'bad arguments')
    refused(stk, stk.lib().stk_gs_depth_step(stk.stream(), 255, p(d_ip), p(d_ix), 0, d.ptr, None, changed.ptr),
            'bad arguments')
    torch.cuda.synchronize()
    assert not d.host().any() and changed.host()[0] == 0
