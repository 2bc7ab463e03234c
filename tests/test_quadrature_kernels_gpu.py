"""The load and error-norm kernels on their own (csrc/load_dev.hip, csrc/err_norms.hip, the shared
kernels of csrc/p1_mesh.h) against the NumPy restatement of tests/test_quadrature_reference_host.py,
EQUAL DOUBLES at every launch form and past every grid cap.  Needs an MI355X.

Every comparison is ref.same_bits: np.array_equal, NaN-aware, and the same sign wherever the value
is no NaN.  There is no tolerance in this file.  After every call the inputs are checked intact
(f, gf and the rows keep their bits; of a slab everything outside the written pair), and a padding
column full of NaN never comes in.  Which paths a call takes is restated from its sizes
(ref.paths), never asked of the library; test_every_path_was_reached prints the table and fails if
a row is missing.

The large meshes are ref.grid_mesh (incidence at most 8), built once per module.

Measured on the MI355X: the whole file (39 tests) takes 3.8 s, the slowest test 0.34 s
(test_load_and_points_at_the_tile_edges[square0], which also brings the library up); the
2 105 352-cell case takes 0.27 s, the 1 051 250-cell one 0.17 s.  The table of that run:

    path                                                 first reached by
    volume<2>                                            square0
    volume<3>                                            cube1
    volume<2> second trip                                grid1026x1026f
    shares<2> full tile                                  square4
    shares<2> tail tile                                  square0
    shares<3> full tile                                  cube1
    shares<3> tail tile                                  cube1
    shares<2> second trip                                grid513x512
    shares<2> nq = 16, n_k = 16                          square0
    shares<3> nq = 16, n_k = 16                          cube1
    gather                                               square0
    gather second trip                                   grid1026x1026f
    points<2>                                            square0
    points<3>                                            cube1
    points<2> second trip                                grid188x175
    geometry<2>                                          square0
    geometry<3>                                          cube1
    geometry<2> second trip                              grid725x725
    err_cells<2, grad> full tile                         square4
    err_cells<2, grad> tail tile                         square0
    err_cells<2, plain> full tile                        square4
    err_cells<2, plain> tail tile                        square0
    err_cells<3, grad> full tile                         cube1
    err_cells<3, grad> tail tile                         cube1
    err_cells<3, plain> full tile                        cube1
    err_cells<3, plain> tail tile                        cube1
    err_cells<2, grad> second trip                       grid725x725
    err_cells<2, grad> nq = 16, n_k = 16                 square0
    err_cells<3, grad> nq = 16, n_k = 16                 cube1
    err_finish LDS only                                  square0
    err_finish 1 global step, absent partners            first 65537 cells of grid257x256
    err_finish 1 global step, every partner present      first 131072 cells of grid257x256
    err_finish 2 global steps, absent partners           first 131073 cells of grid257x256
    err_finish 5 global steps, absent partners           grid725x725

(cube1 has 384 cells, a full tile and a tail; the first 65 793 cells are 258 tiles, one step with
two partners.)
"""
import functools
import types

import numpy as np
import pytest
import torch

import test_quadrature_reference_host as ref

pytestmark = pytest.mark.gpu

REACHED = {}  # path -> the first case that reached it
NQ, NK = (1, 3, 6, 11, 16), (1, 4, 16)


def note(case, call, d, nc, n_free, nq, n_k, with_grad=False):
    for path in ref.paths(call, d, nc, n_free, nq, n_k, with_grad):
        REACHED.setdefault(path, case)


# ---- meshes, built once -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name.startswith('first'):
        return ref.first_cells(_mesh('square4'), int(name[5:]))
    if name.startswith('grid'):  # grid<nx>x<ny>[f]: f = every vertex a free dof
        nx, ny = name[4:].rstrip('f').split('x')
        return ref.grid_mesh(int(nx), int(ny), seed=int(nx), all_free=name.endswith('f'))
    problem = name.rstrip('0123456789')
    return ref._mesh(problem, int(name[len(problem):]))


SMALL = ['square0', 'square1', 'square4', 'lshape_jitter3', 'cube1', 'cube2', 'first255', 'first256', 'first257', 'first513']
STAGES = 'grid257x256'  # 131 584 cells: the meshes of the finish stages are its first cells


@functools.lru_cache(maxsize=None)
def _load_plan(name, permuted=False):
    from source.assembly import DeviceLoadPlan
    mesh = _mesh(name)
    M = len(ref.free_rows(mesh)[0])
    order = np.random.RandomState(M).permutation(M) if permuted else None
    return DeviceLoadPlan(mesh, max_k=16, row_order=order)


@functools.lru_cache(maxsize=None)
def _err_plan(name):
    from source.error_norms import ErrorPlan
    return ErrorPlan(_mesh(name), None)


def _dev(a):
    from source import _lib
    return torch.from_numpy(np.ascontiguousarray(a)).to(_lib.compute_device())


def _bits_kept(tensor, before):
    return torch.equal(tensor.view(torch.int64), before.view(torch.int64))


# ---- the load --------------------------------------------------------------------------------------------------
def _columns(plan, mesh, case, qw, ql, f, coef, old, e_local, accumulate, pair=None):
    """One stk_load_columns call into a copy of the slab `old` against the restatement; f and
    everything outside the pair keep their bits.  Returns the pair the restatement gives."""
    d, nc = mesh.cells.shape[1] - 1, len(mesh.cells)
    n_k, nq = f.shape[0], f.shape[2]
    pair = ref.load_pair(mesh, qw, ql, f, coef) if pair is None else pair
    want = old.copy()
    cols = slice(2 * e_local, 2 * e_local + 2)
    with np.errstate(all='ignore'):
        want[:, cols] = old[:, cols] + pair if accumulate else pair
    f_d, buf = _dev(f), _dev(old)
    f_before = f_d.clone()
    plan.columns(f_d, coef, buf, e_local, accumulate=accumulate, qw=qw, ql=ql)
    got = buf.cpu().numpy()
    assert ref.same_bits(got, want), (case, 'nq', nq, 'n_k', n_k, 'ld', old.shape[1], 'e', e_local, accumulate)
    assert _bits_kept(f_d, f_before), (case, 'f was written')
    note(case, 'load_plan', d, nc, plan.n_free, nq, n_k)
    note(case, 'load', d, nc, plan.n_free, nq, n_k)
    return pair


def _slab(rng, M, ld, e_local, accumulate):
    """randn with NaN in every pair that is not written -- and in the written one too unless it is
    read (accumulate): no padding may come in, and an overwritten pair's old bits do not matter."""
    old = np.full((M, ld), np.nan)
    if accumulate:
        old[:, 2 * e_local:2 * e_local + 2] = rng.randn(M, 2)
    return old


@pytest.mark.parametrize('name', SMALL)
def test_load_and_points_at_the_tile_edges(name):
    """nq in {1, 3, 6, 11, 16} x n_k in {1, 4, 16} on a plan made for 16 time points, random
    rules, random f and coefficients of mixed sign: the pair and the quadrature points are the
    restatement's doubles.  nq = n_k = 16 is the 32 KiB tile."""
    mesh, plan = _mesh(name), _load_plan(name)
    d, nc, M = plan.d, plan.nc, plan.n_free
    rng = np.random.RandomState(nc + 7 * d)
    for nq in NQ:
        qw, ql = ref.random_rule(rng, nq, d)
        got = plan.points(ql).cpu().numpy()
        assert got.shape == (d, nc, nq) and ref.same_bits(got, ref.quadrature_points(mesh.points, mesh.cells, ql)), (name, nq)
        note(name, 'points', d, nc, M, nq, 1)
        for n_k in NK:
            f, coef = rng.randn(n_k, nc, nq), rng.randn(n_k, 2)
            accumulate = (nq + n_k) % 2 == 0
            pair = _columns(plan, mesh, name, qw, ql, f, coef, _slab(rng, M, 4, 1, accumulate), 1, accumulate)
            assert not np.isnan(pair).any()


@pytest.mark.parametrize('name', ['lshape_jitter3', 'cube1', 'first257'])
def test_load_slab_forms(name):
    """ld = 2 (the pair is the whole slab) and ld = 2 n_el + 2 for n_el = 1, 3, 8; the pair first,
    in the middle, last; accumulate on and off; an ascending and a permuted row order: one pair,
    every placement."""
    mesh = _mesh(name)
    plans = {'ascending': _load_plan(name), 'permuted': _load_plan(name, True)}
    d, nc, M = plans['ascending'].d, plans['ascending'].nc, plans['ascending'].n_free
    rng = np.random.RandomState(nc)
    nq, n_k = (6, 4) if d == 2 else (11, 4)
    qw, ql = ref.random_rule(rng, nq, d)
    f, coef = rng.randn(n_k, nc, nq), rng.randn(n_k, 2)
    pair = ref.load_pair(mesh, qw, ql, f, coef)
    forms = [(2, 0)] + [(2 * n_el + 2, e) for n_el in (1, 3, 8) for e in sorted({0, n_el // 2, n_el - 1})]
    for ld, e in forms:
        for accumulate in (False, True):
            old = _slab(rng, M, ld, e, accumulate)
            for order, plan in plans.items():
                _columns(plan, mesh, '%s ld=%d e=%d %s' % (name, ld, e, order), qw, ql, f, coef, old, e, accumulate, pair=pair)


@pytest.mark.parametrize('name', ['first513', 'cube1'])
def test_load_after_a_call_with_more_time_points(name):
    """n_k = 16 and then n_k = 1 on one plan: the shares of the time points 1 .. 15 are still in
    the workspace, and the second result is that of a fresh plan."""
    from source.assembly import DeviceLoadPlan
    mesh, plan = _mesh(name), _load_plan(name)
    d, nc, M = plan.d, plan.nc, plan.n_free
    rng = np.random.RandomState(3)
    qw, ql = ref.random_rule(rng, 6, d)
    _columns(plan, mesh, name, qw, ql, rng.randn(16, nc, 6), rng.randn(16, 2), _slab(rng, M, 2, 0, False), 0, False)
    f, coef = rng.randn(1, nc, 6), rng.randn(1, 2)
    pair = _columns(plan, mesh, name + ' after n_k = 16', qw, ql, f, coef, _slab(rng, M, 2, 0, False), 0, False)
    fresh = DeviceLoadPlan(mesh, max_k=1)
    buf = torch.zeros((M, 2), dtype=torch.float64, device='cuda')
    fresh.columns(_dev(f), coef, buf, 0, qw=qw, ql=ql)
    assert ref.same_bits(buf.cpu().numpy(), pair)


def test_load_nan_and_inf_stay_in_the_rows_of_their_cells():
    """first 513 cells of square 4: NaN in f of cell 255 (the last lane of tile 0), +inf and -inf
    at two points of cell 256 (the first lane of the next tile), +inf and -inf at two time points
    of cell 512 (the only cell of the tail tile).  Every one of them ends as NaN, and exactly the
    rows of the free vertices of those three cells are NaN -- which the restatement says by
    itself."""
    name = 'first513'
    mesh, plan = _mesh(name), _load_plan(name)
    nc, M = plan.nc, plan.n_free
    rng = np.random.RandomState(5)
    qw, ql = ref.random_rule(rng, 3, 2)
    f, coef = rng.randn(2, nc, 3), rng.rand(2, 2) + 0.5
    f[0, 255, :] = np.nan
    f[0, 256, 0], f[0, 256, 1] = np.inf, -np.inf
    f[0, 512, 0], f[1, 512, 0] = np.inf, -np.inf
    pair = _columns(plan, mesh, name + ' NaN and inf in f', qw, ql, f, coef, _slab(rng, M, 4, 0, False), 0, False)
    _, row_of = ref.free_rows(mesh)
    rows = row_of[mesh.cells[[255, 256, 512]].reshape(-1)]
    touched = np.zeros(M, dtype=bool)
    touched[rows[rows >= 0]] = True
    assert touched.sum() >= 3 and not touched.all()
    assert np.array_equal(np.isnan(pair[:, 0]), touched) and np.array_equal(np.isnan(pair[:, 1]), touched)
    assert np.isfinite(pair[~touched]).all()


def test_load_shares_second_trip():
    """525 312 cells, 2052 tiles: above the 2048 workgroups per time point of the shares grid."""
    name = 'grid513x512'
    mesh, plan = _mesh(name), _load_plan(name)
    assert plan.nc == 524288 + 2 * 512
    rng = np.random.RandomState(11)
    qw, ql = ref.random_rule(rng, 1, 2)
    f, coef = rng.randn(2, plan.nc, 1), rng.randn(2, 2)
    _columns(plan, mesh, name, qw, ql, f, coef, _slab(rng, plan.n_free, 2, 0, True), 0, True)


def test_load_gather_and_volume_second_trips():
    """2 105 352 cells and 1 054 729 vertices, every one a free dof: the second trips of
    load_volume_kernel and of load_gather_kernel (and of the shares); nq = 1, n_k = 1, ld = 2."""
    name = 'grid1026x1026f'
    mesh, plan = _mesh(name), _load_plan(name)
    assert plan.nc == 2105352 and plan.n_free == 1054729
    rng = np.random.RandomState(12)
    qw, ql = ref.random_rule(rng, 1, 2)
    f, coef = rng.randn(1, plan.nc, 1), rng.randn(1, 2)
    _columns(plan, mesh, name, qw, ql, f, coef, _slab(rng, plan.n_free, 2, 0, False), 0, False)


def test_points_second_trip():
    """65 800 cells x 16 points = 1 052 800 lanes: the second trip of p1_points_kernel, where
    idx / nq runs past the first 4096 workgroups."""
    name = 'grid188x175'
    mesh, plan = _mesh(name), _load_plan(name)
    assert plan.nc == 65800
    ql = ref.random_rule(np.random.RandomState(13), 16, 2)[1]
    got = plan.points(ql).cpu().numpy()
    assert ref.same_bits(got, ref.quadrature_points(mesh.points, mesh.cells, ql))
    note(name, 'points', 2, plan.nc, plan.n_free, 16, 1)


# ---- the error norms ----------------------------------------------------------------------------------------------
def _element(plan, mesh, case, qw, ql, w_lo, w_hi, c, f, gf, lo, hi, forms=((1, 1),), want=None):
    """stk_err_element against the restatement; lo / hi (n_free,) rows.  forms: pairs of row
    strides -- 1 = a contiguous copy, anything else = a column of a slab of that leading dimension
    whose other columns are NaN.  f, gf and the rows keep their bits."""
    d, nc, M = plan.d, plan.nc, plan.n_free
    n_k, nq = f.shape[0], f.shape[2]
    if want is None:
        want = ref.err_element(mesh, qw, ql, w_lo, w_hi, c, f, gf, lo, hi)
    f_d, gf_d = _dev(f), None if gf is None else _dev(gf)
    f_before, gf_before = f_d.clone(), None if gf is None else gf_d.clone()
    for s_lo, s_hi in forms:
        rows = []
        for values, stride, col in ((lo, s_lo, 1), (hi, s_hi, 2)):
            if stride == 1:
                t = _dev(values)
                rows.append((t, t.data_ptr(), t.clone()))
            else:
                slab = np.full((M, stride), np.nan)
                slab[:, col] = values
                t = _dev(slab)
                rows.append((t, t.data_ptr() + 8 * col, t.clone()))
        out = torch.full((4,), -7.0, dtype=torch.float64, device=f_d.device)
        plan.element(f_d, gf_d, w_lo, w_hi, c, rows[0][1], s_lo, rows[1][1], s_hi, out, qw=qw, ql=ql)
        got = out.cpu().numpy()
        assert ref.same_bits(got, want), (case, 'nq', nq, 'n_k', n_k, gf is not None, (s_lo, s_hi), got, want)
        assert _bits_kept(f_d, f_before) and (gf is None or _bits_kept(gf_d, gf_before)), (case, 'f or gf was written')
        assert all(_bits_kept(t, before) for t, _, before in rows), (case, 'the rows were written')
    note(case, 'err_plan', d, nc, M, nq, n_k)
    note(case, 'err', d, nc, M, nq, n_k, gf is not None)
    return want


def _err_data(rng, plan, nq, n_k, grad=True):
    d, nc, M = plan.d, plan.nc, plan.n_free
    qw, ql = ref.random_rule(rng, nq, d)
    w_lo, w_hi, c = rng.rand(n_k), rng.rand(n_k), rng.rand(n_k) + 0.1
    f = rng.randn(n_k, nc, nq)
    gf = rng.randn(n_k, d, nc, nq) if grad else None
    return qw, ql, w_lo, w_hi, c, f, gf, rng.randn(M), rng.randn(M)


@pytest.mark.parametrize('name', SMALL)
def test_err_at_the_tile_edges(name):
    """Five (nq, n_k) pairs that name every value, with and without gf: the four doubles of the
    restatement.  Without gf entries 1 and 3 are 0.0."""
    mesh, plan = _mesh(name), _err_plan(name)
    rng = np.random.RandomState(plan.nc + 1)
    for nq, n_k in ((1, 16), (3, 1), (6, 4), (11, 4), (16, 16)):
        qw, ql, w_lo, w_hi, c, f, gf, lo, hi = _err_data(rng, plan, nq, n_k)
        want = _element(plan, mesh, name, qw, ql, w_lo, w_hi, c, f, gf, lo, hi)
        assert np.all(want > 0.0)
        plain = _element(plan, mesh, name, qw, ql, w_lo, w_hi, c, f, None, lo, hi)
        assert plain[0] == want[0] and plain[2] == want[2] and plain[1] == 0.0 and plain[3] == 0.0


@pytest.mark.parametrize('nc', [65536, 65537, 65793, 131072, 131073])
def test_err_finish_stages(nc):
    """256 tiles: the finish in LDS alone.  257: one in-place step in global memory with one
    partner.  258 (257 full tiles and a tail of one cell): one step, two partners.  512: one full
    step.  513: two steps.  nq = 3, n_k = 2, with and without gf."""
    mesh = ref.first_cells(_mesh(STAGES), nc)
    from source.error_norms import ErrorPlan
    plan = ErrorPlan(mesh, None)
    rng = np.random.RandomState(nc)
    qw, ql, w_lo, w_hi, c, f, gf, lo, hi = _err_data(rng, plan, 3, 2)
    case = 'first %d cells of %s' % (nc, STAGES)
    want = _element(plan, mesh, case, qw, ql, w_lo, w_hi, c, f, gf, lo, hi)
    plain = _element(plan, mesh, case, qw, ql, w_lo, w_hi, c, f, None, lo, hi)
    assert np.all(want > 0.0) and plain[0] == want[0] and plain[2] == want[2] and plain[1] == 0.0 and plain[3] == 0.0
    # the plan's partials were added in place: a second call starts from its own
    again = _element(plan, mesh, case, qw, ql, w_lo, w_hi, c, f, gf, lo, hi, want=want)
    assert again is want


def test_err_second_trip():
    """1 051 250 cells, 4107 tiles: the second trip of err_cells_kernel and of p1_geometry_kernel,
    and five global steps of the finish; nq = 1, n_k = 1, with gf."""
    name = 'grid725x725'
    mesh, plan = _mesh(name), _err_plan(name)
    assert plan.nc == 1051250
    qw, ql, w_lo, w_hi, c, f, gf, lo, hi = _err_data(np.random.RandomState(14), plan, 1, 1)
    _element(plan, mesh, name, qw, ql, w_lo, w_hi, c, f, gf, lo, hi)


@pytest.mark.parametrize('name', ['first513', 'cube2'])
def test_err_corners(name):
    """nq = 16, n_k = 16 with gf; the rows contiguous and as columns of a slab whose other columns
    are NaN, strides (1, ld), (ld, 1), (ld, ld); and two calls in a row on one plan and stream,
    not synchronised in between, each with its own answer (the plan's partials are reused)."""
    mesh, plan = _mesh(name), _err_plan(name)
    rng = np.random.RandomState(15)
    a = _err_data(rng, plan, 16, 16)
    want_a = _element(plan, mesh, name, *a, forms=((1, 1), (1, 6), (5, 1), (4, 4)))
    b = _err_data(rng, plan, 3, 2)
    want_b = ref.err_element(mesh, *b)
    dev = [[None if x is None else _dev(x) for x in (args[5], args[6], args[7], args[8])] for args in (a, b)]
    outs = [torch.full((4,), -7.0, dtype=torch.float64, device='cuda') for _ in range(2)]
    for args, (f_d, gf_d, lo_d, hi_d), out in zip((a, b), dev, outs):
        plan.element(f_d, gf_d, args[2], args[3], args[4], lo_d.data_ptr(), 1, hi_d.data_ptr(), 1, out, qw=args[0], ql=args[1])
    assert ref.same_bits(outs[0].cpu().numpy(), want_a) and ref.same_bits(outs[1].cpu().numpy(), want_b)
    assert not ref.same_bits(want_a, want_b)


def test_err_a_tile_of_boundary_only_cells():
    """first 513 cells of square 4 with every vertex of the cells 256 .. 511 put on the boundary:
    tile 1 reads no row at all, its cells give the norm of f."""
    base = _mesh('first513')
    boundary = np.asarray(base.boundary, dtype=bool).copy()
    boundary[base.cells[256:512].reshape(-1)] = True
    mesh = types.SimpleNamespace(points=base.points, cells=base.cells, boundary=boundary, nv=base.nv)
    _, row_of = ref.free_rows(mesh)
    assert (row_of[mesh.cells[256:512]] < 0).all() and (row_of[mesh.cells[:256]] >= 0).any()
    from source.error_norms import ErrorPlan
    plan = ErrorPlan(mesh, None)
    qw, ql, w_lo, w_hi, c, f, gf, lo, hi = _err_data(np.random.RandomState(16), plan, 6, 4)
    want = _element(plan, mesh, 'first513, tile 1 on the boundary', qw, ql, w_lo, w_hi, c, f, gf, lo, hi, forms=((1, 1), (3, 3)))
    assert want[0] != want[2] and want[1] != want[3]
    # the boundary-only tile alone: err = ref, in the same doubles
    per_cell = ref.err_cells(mesh, qw, ql, w_lo, w_hi, c, f, gf, lo, hi)
    assert ref.same_bits(per_cell[0, 256:512], per_cell[2, 256:512]) and ref.same_bits(per_cell[1, 256:512], per_cell[3, 256:512])


# ---- the paths ---------------------------------------------------------------------------------------------------------
def test_every_path_was_reached():
    for path in ref.EXPECTED_PATHS:
        print('%-52s %s' % (path, REACHED.get(path, '-- NOT REACHED --')))
    missing = [p for p in ref.EXPECTED_PATHS if p not in REACHED]
    assert not missing, missing
    assert sorted(REACHED) == sorted(ref.EXPECTED_PATHS), sorted(set(REACHED) - set(ref.EXPECTED_PATHS))
    _load_plan.cache_clear(), _err_plan.cache_clear(), _mesh.cache_clear()
