"""The forward sampling kernels on their own, through the ABI (csrc/sample.hip: stk_sample_locate,
stk_sample_eval, stk_sample_pairs, stk_sample_grad_coeffs), bit for bit against the NumPy
restatement of include/stk.h in tests/test_sample_reference_host.py, at every launch form.  Needs
an MI355X.

Every call goes through ctypes on a stream of its own (never the default one).  Every device array
-- x, cell, lam, t, the slab, out -- lies inside a flat buffer between sentinels that must survive
the call; out starts as a sentinel of its own, and the rows and columns beyond n_p and beyond the
requested fields must keep it; the padding columns of a slab (ld > n_loc) hold NaN.  Every
comparison is ref.same_bits: np.array_equal(..., equal_nan=True) and the sign of every zero.  No
tolerances.

Which kernel a call reaches is restated from its arguments (ref.launch_plan for the launches of
stk_sample_eval, `!(ld & 1) && !(addr & 15)` for the two pairs kernels, 4096 workgroups for the
capped grids), never asked of the library.  test_every_path_was_reached prints the table and
fails if a row is missing.

The table of a run on an MI355X (66 tests; the whole file took 6.4 s, the slowest test 1.4 s --
test_locate[lshape_jitter 3], nearly all of it the NumPy model of 9000 points in 1536 cells,
computed once and shared):

    path                                                 first reached by
    locate<2>                                            square 1
    locate<3>                                            cube 1
    grad_coeffs<2>                                       square 1
    grad_coeffs<3>                                       cube 1
    eval<2> 1 launch                                     shuffled2d: 1 columns, n_p=1 ld=300 ld_out=1
    eval<2> 2 launches                                   shuffled2d: 97 columns, n_p=1 ld=301 ld_out=1
    eval<2> 4 launches                                   shuffled2d: 300 columns, n_p=1 ld=303 ld_out=1
    eval<3> 1 launch                                     tetfan: 1 columns, n_p=1 ld=300 ld_out=1
    eval<3> 2 launches                                   tetfan: 97 columns, n_p=1 ld=301 ld_out=1
    eval<3> 4 launches                                   tetfan: 300 columns, n_p=1 ld=303 ld_out=1
    eval<2> launch of 0 columns                          shuffled2d: (-1, -1) at the boundary, n_p=63 ld=303 ld_out=63
    eval<3> launch of 0 columns                          tetfan: (-1, -1) at the boundary, n_p=63 ld=303 ld_out=63
    pairs<2, wide>                                       shuffled2d
    pairs<2, narrow>                                     shuffled2d N=2 h = 1 / (N - 1), misaligned, even ld, fields=1
    pairs<3, wide>                                       tetfan
    pairs<3, narrow>                                     shuffled3d N=2 h = 1 / (N - 1), misaligned, even ld, fields=1
    pairs<2, wide> both columns, c0 even: 16-byte loads  shuffled2d N=2 h = 1 / (N - 1), aligned, even ld, fields=7
    pairs<2, wide> both columns, c0 odd: per point       shuffled2d N=3 h = 1 / (N - 1), aligned, even ld, fields=7
    pairs<3, wide> both columns, c0 even: 16-byte loads  shuffled3d N=2 h = 1 / (N - 1), aligned, even ld, fields=7
    pairs<3, wide> both columns, c0 odd: per point       shuffled3d N=3 h = 1 / (N - 1), aligned, even ld, fields=7
    pairs<2> only have0                                  shuffled2d N=9 rank 0 of 2: columns 0..3, aligned, even ld
    pairs<2> only have1                                  shuffled2d N=9 rank 1 of 2: columns 4..8, misaligned, even ld
    pairs<3> only have0                                  shuffled3d N=9 rank 0 of 2: columns 0..3, aligned, even ld
    pairs<3> only have1                                  shuffled3d N=9 rank 1 of 2: columns 4..8, misaligned, even ld
    locate<2> second trip                                n_p = 1048833
    grad_coeffs<2> second trip                           n_p = 1048833
    eval<2> second trip                                  n_p = 262209
    pairs<2, wide> second trip                           n_p = 1048833

(Launches of 3 come with the 192- and 193-column calls.  Placements of a slab: an aligned base
with an even ld selects the wide kernel; the same slab 8 bytes further on, and an odd ld, the
narrow one.)
"""
import ctypes

import numpy as np
import pytest
import torch

import test_sample_reference_host as ref
from test_multigrid_kernels_gpu import NAN, SENTINEL, Slab, stk  # noqa: F401  (stk: the fixture)

pytestmark = pytest.mark.gpu

GUARD = 16  # items before and behind a flat array
INT_SENTINEL = -777777
OUT_START = -77.5  # what out holds before a call
REACHED = {}  # path -> the first case that reached it
EXPECTED = (['locate<%d>' % d for d in (2, 3)] + ['grad_coeffs<%d>' % d for d in (2, 3)]
            + ['eval<%d> %d launch%s' % (d, n, 'es' if n > 1 else '') for d in (2, 3) for n in (1, 2, 4)]
            + ['eval<%d> launch of 0 columns' % d for d in (2, 3)]
            + ['pairs<%d, %s>' % (d, w) for d in (2, 3) for w in ('wide', 'narrow')]
            + ['pairs<%d, wide> both columns, c0 %s' % (d, w) for d in (2, 3) for w in ('even: 16-byte loads', 'odd: per point')]
            + ['pairs<%d> only %s' % (d, w) for d in (2, 3) for w in ('have0', 'have1')]
            + ['%s second trip' % k for k in ('locate<2>', 'grad_coeffs<2>', 'eval<2>', 'pairs<2, wide>')])


def note(path, case):
    REACHED.setdefault(path, case)


@pytest.fixture(scope='module')
def side():
    return torch.cuda.Stream()


@pytest.fixture(autouse=True)
def on_the_side_stream(stk, side):
    """The whole test, uploads included, on one non-default stream."""
    with torch.cuda.stream(side):
        assert stk.stream() != 0 and stk.stream() == side.cuda_stream
        yield
    side.synchronize()


# ---- buffers -------------------------------------------------------------------------------------
class Flat:
    """A flat device array between GUARD sentinels on either side."""
    def __init__(self, data=None, n=None, dtype=np.float64, fill=None):
        if data is not None:
            data = np.ascontiguousarray(data, dtype=dtype).reshape(-1)
            n = len(data)
        self.sentinel = SENTINEL if np.dtype(dtype).kind == 'f' else INT_SENTINEL
        tdtype = {np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32}[np.dtype(dtype)]
        self.flat = torch.full((n + 2 * GUARD,), self.sentinel, dtype=tdtype, device='cuda')
        self.view = self.flat[GUARD:GUARD + n]
        if data is not None:
            self.view.copy_(torch.from_numpy(data.copy()))
        elif fill is not None:
            self.view.fill_(fill)

    @classmethod
    def of(cls, tensor):
        """Around a device tensor that is already there (the tiled arrays of the second trips)."""
        self = cls(n=tensor.numel(), dtype=np.float64 if tensor.dtype == torch.float64 else np.int32)
        self.view.copy_(tensor.reshape(-1))
        return self

    @property
    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        return self.view.cpu().numpy()

    def check(self, what):
        assert bool((self.flat[:GUARD] == self.sentinel).all()) and bool((self.flat[-GUARD:] == self.sentinel).all()), (
            what, 'guard')


def slab_buffer(U, ld, off=0):
    """The (M, n_loc) nodal values in a Slab of leading dimension ld, NaN in its padding columns."""
    s = Slab(U.shape[0], ld, off)
    s.n_loc = U.shape[1]
    s.view[:, :s.n_loc] = torch.from_numpy(np.array(U)).cuda()
    return s


def out_buffer(rows, ld_out):
    o = Slab(rows, ld_out)
    o.view.fill_(OUT_START)
    return o


def frame_intact(s, what):
    assert bool((s.flat[:s.start] == SENTINEL).all()) and bool((s.flat[s.start + s.count:] == SENTINEL).all()), (what, 'guard')


def result(o, n_rows, n_p, what):
    """The (n_rows, n_p) block of an out buffer; the guards, the columns beyond n_p and the rows
    beyond n_rows must be as they were."""
    frame_intact(o, what)
    h = o.view.cpu().numpy()
    assert np.all(h[:, n_p:] == OUT_START), (what, 'a column beyond n_p was written')
    assert np.all(h[n_rows:] == OUT_START), (what, 'a row beyond the requested ones was written')
    return h[:n_rows, :n_p]


# ---- plans and calls ---------------------------------------------------------------------------------
class Plan:
    def __init__(self, stk, mesh):
        self.stk, self.mesh, self.handle = stk, mesh, ctypes.c_void_p()
        with torch.cuda.device(stk.compute_device()):
            stk.check(stk.lib().stk_sample_plan_create(mesh.d, mesh.nv, mesh.nc, mesh.points.ctypes.data,
                                                       mesh.cells.ctypes.data, mesh.n_free, mesh.free.ctypes.data,
                                                       ctypes.byref(self.handle)))

    def close(self):
        if self.handle:
            self.stk.lib().stk_sample_plan_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    __del__ = close


_plans = {}


def plan_of(stk, name):
    if name not in _plans:
        _plans[name] = Plan(stk, ref.catalogue()[name])
    return _plans[name]


def locate(stk, plan, x, what):
    """(cell, lam) of the points x (n, d), guards checked."""
    n, d = x.shape
    xb = Flat(np.ascontiguousarray(x.T))
    cell, lam = Flat(n=n, dtype=np.int32, fill=INT_SENTINEL + 1), Flat(n=n * (d + 1), fill=OUT_START)
    stk.check(stk.lib().stk_sample_locate(stk.stream(), plan.handle, n, xb.ptr, cell.ptr, lam.ptr))
    for b in (xb, cell, lam):
        b.check(what)
    assert ref.same_bits(xb.get(), x.T.reshape(-1))
    note('locate<%d>' % d, what)
    return cell.get(), lam.get().reshape(n, d + 1)


def grad_coeffs(stk, plan, cell, what):
    n, d = len(cell), plan.mesh.d
    cb, out = Flat(cell, dtype=np.int32), Flat(n=d * n * (d + 1), fill=OUT_START)
    stk.check(stk.lib().stk_sample_grad_coeffs(stk.stream(), plan.handle, n, cb.ptr, out.ptr))
    cb.check(what), out.check(what)
    note('grad_coeffs<%d>' % d, what)
    return out.get().reshape(d, n, d + 1)


def evaluate(stk, plan, cell, lam, slab, columns, weights, ld_out, what, out=None, first_row=0, lam_ptr=None):
    """One stk_sample_eval: cell, lam Flat buffers (or lam_ptr, a device address), slab a Slab,
    the requests host arrays.  Returns the out buffer (not looked at: `result` does that)."""
    n_p = cell.view.numel()
    columns = np.ascontiguousarray(columns, dtype=np.int32).reshape(-1, 2)
    weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, 2)
    n_k = len(columns)
    if out is None:
        out = out_buffer(n_k + 1, ld_out)
    stk.check(stk.lib().stk_sample_eval(stk.stream(), plan.handle, n_p, cell.ptr, lam.ptr if lam_ptr is None else lam_ptr,
                                        plan.mesh.n_free, slab.n_loc, slab.ld, slab.ptr, n_k, columns.ctypes.data,
                                        weights.ctypes.data, ld_out, out.ptr + 8 * first_row * ld_out))
    launches = ref.launch_plan(columns, slab.n_loc)
    if n_k > 1 or first_row == 0:
        note('eval<%d> %d launch%s' % (plan.mesh.d, len(launches), 'es' if len(launches) > 1 else ''), what)
    if any(l[2] == 0 for l in launches):
        note('eval<%d> launch of 0 columns' % plan.mesh.d, what)
    return out


def is_wide(slab):
    return not (slab.ld & 1) and not (slab.ptr & 15)


def pairs(stk, plan, cell, lam, t, h, N, t_begin, slab, fields, ld_out, what):
    n_p, d = cell.view.numel(), plan.mesh.d
    n_rows = ref.pair_rows(d, fields)
    out = out_buffer(n_rows + 1, ld_out)
    stk.check(stk.lib().stk_sample_pairs(stk.stream(), plan.handle, n_p, cell.ptr, lam.ptr, t.ptr, h, N, t_begin,
                                         plan.mesh.n_free, slab.n_loc, slab.ld, slab.ptr, fields, ld_out, out.ptr))
    note('pairs<%d, %s>' % (d, 'wide' if is_wide(slab) else 'narrow'), what)
    return out


def inputs_intact(what, *buffers):
    for b in buffers:
        frame_intact(b, what) if isinstance(b, Slab) else b.check(what)


# ---- stk_sample_locate ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.MESH_NAMES)
def test_locate(stk, name):
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    x = ref.all_points_of(name)
    want_cell, want_lam = ref.located(name)
    all_cell, all_lam, _ = ref.located_all_cells(name)
    cell, lam = locate(stk, plan, x, name)
    assert cell.dtype == np.int32 and np.array_equal(cell, want_cell)
    assert ref.same_bits(lam, want_lam)
    inside = all_cell >= 0
    assert np.array_equal(cell[inside], all_cell[inside]) and ref.same_bits(lam[inside], all_lam[inside])
    for n in (1, 63, 64, 65, 255, 256, 257):
        c, l = locate(stk, plan, x[:n], '%s n_p=%d' % (name, n))
        assert np.array_equal(c, want_cell[:n]) and ref.same_bits(l, want_lam[:n]), n
    print('%-16s %5d points, %5d inside, %d with an empty bin' % (name, len(x), (cell >= 0).sum(), np.isnan(lam).all(axis=1).sum()))
    assert mesh.nc > 0


def test_nothing_to_do(stk):
    """n_p = 0 with null pointers: every entry point returns 0 and launches nothing."""
    for name in ('square 1', 'cube 1'):
        plan, lib = plan_of(stk, name), stk.lib()
        M = plan.mesh.n_free
        assert lib.stk_sample_locate(stk.stream(), plan.handle, 0, None, None, None) == 0
        assert lib.stk_sample_grad_coeffs(stk.stream(), plan.handle, 0, None, None) == 0
        assert lib.stk_sample_eval(stk.stream(), plan.handle, 0, None, None, M, 1, 1, None, 0, None, None, 0, None) == 0
        assert lib.stk_sample_pairs(stk.stream(), plan.handle, 0, None, None, None, 0.5, 3, 0, M, 3, 3, None, 7, 0, None) == 0


BLOCK = 4099  # the tiled block of the second trips: no multiple of a workgroup, a wavefront or a tile
FLAT_N = ref.FLAT_CAP * ref.BS + 257  # one lane per point: the capped grid goes round once more
TILE_N = ref.TP * ref.FLAT_CAP + 65  # one eval tile per 64 points: the tile loop goes round once more


def tiled(block, n):
    """A device tensor: the rows of `block` (host) repeated up to n rows."""
    b = torch.from_numpy(np.ascontiguousarray(block)).cuda()
    reps = -(-n // len(b))
    return b.repeat((reps,) + (1,) * (b.dim() - 1))[:n].contiguous()


def copies_equal_the_first(got, block_rows):
    """got: device tensor whose leading axis is the point; every later copy of the block equals
    the first, as bit patterns."""
    bits = got.view(torch.int64) if got.dtype == torch.float64 else got
    whole = (len(bits) // block_rows) * block_rows
    first = bits[:block_rows]
    assert bool((bits[:whole].reshape((-1, block_rows) + tuple(bits.shape[1:])) == first).all())
    assert bool((bits[whole:] == first[:len(bits) - whole]).all())


def second_trip_block(name):
    """BLOCK catalogue points of a mesh (the catalogue from its end: the random points and some
    of every other kind), with their model location."""
    x = ref.all_points_of(name)
    idx = np.arange(len(x))[::-1][:BLOCK] if len(x) >= BLOCK else np.resize(np.arange(len(x)), BLOCK)
    cell, lam = ref.located(name)
    return x[idx], cell[idx], lam[idx]


def test_locate_second_trip(stk):
    """n_p = 4096 * 256 + 257 on `square 1`: lanes of the capped grid take a second point."""
    name = 'square 1'
    plan = plan_of(stk, name)
    xb, want_cell, want_lam = second_trip_block(name)
    x = Flat.of(tiled(xb, FLAT_N).t().contiguous())  # [d][n_p]
    cell, lam = Flat(n=FLAT_N, dtype=np.int32, fill=INT_SENTINEL + 1), Flat(n=3 * FLAT_N, fill=OUT_START)
    stk.check(stk.lib().stk_sample_locate(stk.stream(), plan.handle, FLAT_N, x.ptr, cell.ptr, lam.ptr))
    inputs_intact('second trip', x, cell, lam)
    assert np.array_equal(cell.view[:BLOCK].cpu().numpy(), want_cell)
    assert ref.same_bits(lam.view[:3 * BLOCK].cpu().numpy().reshape(BLOCK, 3), want_lam)
    copies_equal_the_first(cell.view, BLOCK)
    copies_equal_the_first(lam.view.view(FLAT_N, 3), BLOCK)
    note('locate<2> second trip', 'n_p = %d' % FLAT_N)


# ---- stk_sample_grad_coeffs ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ref.MESH_NAMES)
def test_grad_coeffs(stk, name):
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    cell = np.concatenate([ref.located(name)[0], [-1, mesh.nc, mesh.nc + 5], np.arange(mesh.nc)]).astype(np.int32)
    got = grad_coeffs(stk, plan, cell, name)
    want = ref.grad_coeffs_model(mesh, cell)
    assert ref.same_bits(got, want)
    n = len(cell) - mesh.nc
    assert np.isnan(got[:, n - 3:n]).all() and np.isnan(got[:, cell < 0]).all()
    negative = mesh.signed_measures() < 0
    print('%-16s %5d cells asked, %d of the mesh have det < 0' % (name, len(cell), negative.sum()))
    for n in (1, 255, 256, 257):
        assert ref.same_bits(grad_coeffs(stk, plan, cell[-n:], name), want[:, -n:])


def test_grad_coeffs_second_trip(stk):
    name = 'square 1'
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    block = np.resize(np.concatenate([ref.located(name)[0], [-1, mesh.nc, mesh.nc + 5]]), BLOCK).astype(np.int32)
    cell = Flat.of(tiled(block, FLAT_N))
    out = Flat(n=2 * FLAT_N * 3, fill=OUT_START)
    stk.check(stk.lib().stk_sample_grad_coeffs(stk.stream(), plan.handle, FLAT_N, cell.ptr, out.ptr))
    inputs_intact('second trip', cell, out)
    got = out.view.view(2, FLAT_N, 3)
    assert ref.same_bits(got[:, :BLOCK].cpu().numpy(), ref.grad_coeffs_model(mesh, block))
    for j in range(2):
        copies_equal_the_first(got[j], BLOCK)
    note('grad_coeffs<2> second trip', 'n_p = %d' % FLAT_N)


# ---- stk_sample_eval --------------------------------------------------------------------------------------------
EVAL_MESHES = ('shuffled2d', 'tetfan')
N_LOC = 300


def eval_points(name, n_p=65):
    """(cell, lam) of n_p catalogue points: vertices and midpoints from the front, random points
    (some outside: cell = -1) from the end, and two cells set to nc."""
    mesh = ref.catalogue()[name]
    cell, lam = ref.located(name)
    idx = np.concatenate([np.arange(0, 4 * 40, 4), np.arange(len(cell) - (n_p - 40), len(cell))])[:n_p]
    cell, lam = cell[idx].copy(), lam[idx].copy()
    cell[[5, 44]] = mesh.nc
    assert (cell < 0).any() and ((cell >= 0) & (cell < mesh.nc)).sum() > n_p // 2
    return cell, lam


def ascending(n):
    """Requests (c, c + 1) that name n distinct columns; one column: (0, 0)."""
    return [(c, c + 1) for c in range(n - 1)] if n > 1 else [(0, 0)]


def eval_sequences():
    full = ascending(96)  # 96 columns in use
    seq = {'%d columns' % n: ascending(n) for n in (1, 2, 95, 96, 97, 98, 192, 193, 300)}
    seq['95 used, two fresh'] = ascending(95) + [(200, 201), (201, 94)]
    seq['96 used, one fresh'] = full + [(95, 96), (3, 150)]
    seq['96 used, one fresh beside an old one'] = full + [(3, 150), (150, 3)]
    seq['reversed pairs'] = [(c + 1, c) for c in range(97)]
    seq['the same column twice'] = [(c, c) for c in range(100)]
    seq['columns of the launch before'] = full + [(96, 97), (0, 1), (5, 2), (95, 0), (97, 96)]
    seq['(-1, c) at the boundary'] = full + [(-1, 200), (200, 7), (-1, 7)]
    seq['(c, -1) at the boundary'] = full + [(200, -1), (7, 200), (7, -1)]
    seq['(-1, -1) at the boundary'] = full + [(-1, -1), (200, 201), (-1, -1)]
    seq['all (-1, -1)'] = [(-1, -1)] * 5
    return seq


@pytest.mark.parametrize('name', EVAL_MESHES)
def test_eval_launches(stk, name):
    """Every request sequence, with n_p, ld and ld_out going round; every call against the model,
    and every call of more than one launch against the same requests served one per call."""
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    cell_h, lam_h = eval_points(name)
    U = ref.slab_of(mesh.n_free, N_LOC, 41)
    slabs = [slab_buffer(U, ld) for ld in (N_LOC, N_LOC + 1, N_LOC + 3)]
    rs = np.random.RandomState(42)
    seen = set()
    for i, (label, columns) in enumerate(eval_sequences().items()):
        n_p, slab = (1, 63, 64, 65)[i % 4], slabs[i % 3]
        ld_out = n_p + 3 * ((i // 2) % 2)
        columns = np.array(columns, dtype=np.int32)
        weights = rs.randn(len(columns), 2)
        cell, lam = Flat(cell_h[:n_p], dtype=np.int32), Flat(lam_h[:n_p])
        what = '%s: %s, n_p=%d ld=%d ld_out=%d' % (name, label, n_p, slab.ld, ld_out)
        out = evaluate(stk, plan, cell, lam, slab, columns, weights, ld_out, what)
        got = result(out, len(columns), n_p, what)
        inputs_intact(what, cell, lam, slab)
        want = ref.eval_model(mesh, cell_h[:n_p], lam_h[:n_p], U, columns, weights)
        assert ref.same_bits(got, want), what
        launches = ref.launch_plan(columns, N_LOC)
        seen |= {l[2] for l in launches}
        if len(launches) > 1:
            single = out_buffer(len(columns) + 1, ld_out)
            for k in range(len(columns)):
                evaluate(stk, plan, cell, lam, slab, columns[k], weights[k], ld_out, what, out=single, first_row=k)
            assert ref.same_bits(result(single, len(columns), n_p, what), got), what
        if label == 'all (-1, -1)':
            ok = (cell_h[:n_p] >= 0) & (cell_h[:n_p] < mesh.nc)
            assert np.all(got[:, ok] == 0.0) and not np.signbit(got[:, ok]).any() and np.isnan(got[:, ~ok]).all()
        print('%-60s launches (k0, requests, columns): %s' % (what, launches))
    assert {0, 1, 2, 95, 96} <= seen and any(n % 2 == 0 and n > 2 for n in seen)


@pytest.mark.parametrize('name', EVAL_MESHES)
def test_eval_shapes(stk, name):
    """The 300-column call (4 launches) at every n_p, ld and ld_out."""
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    cell_h, lam_h = eval_points(name)
    U = ref.slab_of(mesh.n_free, N_LOC, 43)
    columns = np.array(ascending(N_LOC), dtype=np.int32)
    weights = np.random.RandomState(44).randn(len(columns), 2)
    assert len(ref.launch_plan(columns, N_LOC)) == 4
    for ld in (N_LOC, N_LOC + 1, N_LOC + 3):
        slab = slab_buffer(U, ld)
        for n_p in (1, 63, 64, 65):
            cell, lam = Flat(cell_h[:n_p], dtype=np.int32), Flat(lam_h[:n_p])
            want = ref.eval_model(mesh, cell_h[:n_p], lam_h[:n_p], U, columns, weights)
            for ld_out in (n_p, n_p + 3):
                what = '%s: n_p=%d ld=%d ld_out=%d' % (name, n_p, ld, ld_out)
                out = evaluate(stk, plan, cell, lam, slab, columns, weights, ld_out, what)
                assert ref.same_bits(result(out, len(columns), n_p, what), want), what
                inputs_intact(what, cell, lam, slab)


def test_eval_second_trip(stk):
    """n_p = 64 * 4096 + 65: workgroups of the capped grid take a second tile."""
    name = 'shuffled2d'
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    _, cell_b, lam_b = second_trip_block(name)
    cell_b = cell_b.copy()
    cell_b[[7, 1000]] = mesh.nc
    U = ref.slab_of(mesh.n_free, 5, 45)
    slab = slab_buffer(U, 6)
    columns, weights = np.array([(0, 1), (4, 3), (2, -1)], dtype=np.int32), np.random.RandomState(46).randn(3, 2)
    cell, lam = Flat.of(tiled(cell_b, TILE_N)), Flat.of(tiled(lam_b, TILE_N))
    out = evaluate(stk, plan, cell, lam, slab, columns, weights, TILE_N, 'second trip')
    inputs_intact('second trip', cell, lam, slab, out)
    assert bool((out.view[3] == OUT_START).all())
    got = out.view[:3]
    assert ref.same_bits(got[:, :BLOCK].cpu().numpy(), ref.eval_model(mesh, cell_b, lam_b, U, columns, weights))
    for k in range(3):
        copies_equal_the_first(got[k].contiguous(), BLOCK)
    note('eval<2> second trip', 'n_p = %d' % TILE_N)


@pytest.mark.parametrize('name', EVAL_MESHES)
def test_eval_plan_reuse(stk, side, name):
    """Small, large, small, large on one plan and one stream with no host synchronisation between
    the calls (the request tables grow under the second call): each output is that call's on a
    fresh plan."""
    mesh = ref.catalogue()[name]
    cell_h, lam_h = eval_points(name)
    n_p = len(cell_h)
    U = ref.slab_of(mesh.n_free, N_LOC, 47)
    slab = slab_buffer(U, N_LOC + 1)
    rs = np.random.RandomState(48)
    small = (np.array([(7, 8), (299, -1)], dtype=np.int32), rs.randn(2, 2))
    large = (np.array(ascending(N_LOC), dtype=np.int32), rs.randn(N_LOC - 1, 2))
    cell, lam = Flat(cell_h, dtype=np.int32), Flat(lam_h)
    side.synchronize()
    plan = Plan(stk, mesh)
    outs = [evaluate(stk, plan, cell, lam, slab, c, w, n_p, 'reuse') for c, w in (small, large, small, large)]
    side.synchronize()
    got = [result(o, len(c), n_p, 'reuse') for o, (c, w) in zip(outs, (small, large, small, large))]
    plan.close()
    for g, (c, w) in zip(got, (small, large, small, large)):
        fresh = Plan(stk, mesh)
        alone = result(evaluate(stk, fresh, cell, lam, slab, c, w, n_p, 'alone'), len(c), n_p, 'alone')
        side.synchronize()
        fresh.close()
        assert ref.same_bits(g, alone)
        assert ref.same_bits(g, ref.eval_model(mesh, cell_h, lam_h, U, c, w))
    inputs_intact('reuse', cell, lam, slab)


def pair_points(name, n_p, stride=13):
    """(cell, lam) of n_p catalogue points, one in `stride` through the whole catalogue, and one
    cell set to nc."""
    mesh = ref.catalogue()[name]
    cell, lam = ref.located(name)
    idx = (np.arange(n_p) * stride) % len(cell)
    cell, lam = cell[idx].copy(), lam[idx].copy()
    cell[n_p // 2] = mesh.nc
    return cell, lam


@pytest.mark.parametrize('name', EVAL_MESHES)
def test_eval_with_the_gradient_coefficients_as_lam(stk, name):
    """Row j of stk_sample_grad_coeffs as `lam`: the block of grad_j -- the model's, and on its
    diagonal what stk_sample_pairs gives for the pairs (h a power of two)."""
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    N, d = 9, mesh.d
    h = 1.0 / (N - 1)
    t_h = ref.times_of(N, h, 49)[:-5]
    t_h = t_h[(t_h >= 0.0) & (t_h <= float(N - 1) * h)]
    n_p = len(t_h)
    cell_h, lam_h = pair_points(name, n_p, stride=5)
    U = ref.slab_of(mesh.n_free, N, 50)
    slab = slab_buffer(U, N + 1)
    cell, lam, t = Flat(cell_h, dtype=np.int32), Flat(lam_h), Flat(t_h)
    G = Flat(n=d * n_p * (d + 1), fill=OUT_START)
    stk.check(stk.lib().stk_sample_grad_coeffs(stk.stream(), plan.handle, n_p, cell.ptr, G.ptr))
    G_model = ref.grad_coeffs_model(mesh, cell_h)
    assert ref.same_bits(G.get().reshape(d, n_p, d + 1), G_model)
    columns, weights = ref.requests_of_times(t_h, h, N, 0, N)
    from_pairs = result(pairs(stk, plan, cell, lam, t, h, N, 0, slab, 4, n_p, name), d, n_p, name)
    assert ref.same_bits(from_pairs, ref.pairs_model(mesh, cell_h, lam_h, t_h, h, N, 0, U, 4))
    for j in range(d):
        out = evaluate(stk, plan, cell, None, slab, columns, weights, n_p, name, lam_ptr=G.ptr + 8 * j * n_p * (d + 1))
        block = result(out, n_p, n_p, name)
        assert ref.same_bits(block, ref.eval_model(mesh, cell_h, G_model[j], U, columns, weights))
        assert ref.same_bits(block[np.arange(n_p), np.arange(n_p)], from_pairs[j])
    inputs_intact(name, cell, lam, t, G, slab)
    assert 0 < np.isnan(from_pairs[0]).sum() < n_p


# ---- stk_sample_pairs -----------------------------------------------------------------------------------------------
PAIR_MESHES = ('shuffled2d', 'shuffled3d')


def rows_of_mask(d, fields):
    """The rows of the fields = 7 result that a mask asks for, in their order."""
    return [0] * (fields & 1) + [1] * (fields >> 1 & 1) + list(range(2, 2 + d)) * (fields >> 2 & 1)


def placements(U, n_loc):
    """(label, Slab): an aligned base with an even ld, that slab 8 bytes further on, an odd ld."""
    even, odd = n_loc + 2 - (n_loc & 1), n_loc + 1 - (n_loc & 1)
    return [('aligned, even ld', slab_buffer(U, even)), ('misaligned, even ld', slab_buffer(U, even, off=1)),
            ('odd ld', slab_buffer(U, odd))]


def note_brackets(d, t, h, N, t_begin, n_loc, valid, wide, what):
    ef, _, _ = ref.time_bracket(np.where(valid, t, 0.0), h, N)
    c0 = ef.astype(np.int64) - t_begin
    have0, have1 = valid & (c0 >= 0) & (c0 < n_loc), valid & (c0 + 1 >= 0) & (c0 + 1 < n_loc)
    if (have0 & ~have1).any():
        note('pairs<%d> only have0' % d, what)
    if (have1 & ~have0).any():
        note('pairs<%d> only have1' % d, what)
    if wide and (have0 & have1 & (c0 % 2 == 0)).any():
        note('pairs<%d, wide> both columns, c0 even: 16-byte loads' % d, what)
    if wide and (have0 & have1 & (c0 % 2 == 1)).any():
        note('pairs<%d, wide> both columns, c0 odd: per point' % d, what)


@pytest.mark.parametrize('spacing', ('h = 1 / (N - 1)', 'h = 0.1'))
@pytest.mark.parametrize('N', (2, 3, 9, 130))
@pytest.mark.parametrize('name', PAIR_MESHES)
def test_pairs(stk, name, N, spacing):
    """Every mask at the three slab placements: the same bits, the model's."""
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    d = mesh.d
    h = 0.1 if spacing == 'h = 0.1' else 1.0 / (N - 1)
    t_h = ref.times_of(N, h, 51 + N)
    n_p = len(t_h)
    cell_h, lam_h = pair_points(name, n_p)
    U = ref.slab_of(mesh.n_free, N, 52 + N)
    want = ref.pairs_model(mesh, cell_h, lam_h, t_h, h, N, 0, U, 7)
    valid = ~np.isnan(want[0])
    assert np.array_equal(np.isnan(want), np.isnan(want[:1]).repeat(2 + d, axis=0)) and 5 <= (~valid).sum() < n_p // 2
    cell, lam, t = Flat(cell_h, dtype=np.int32), Flat(lam_h), Flat(t_h)
    chosen = set()
    for label, slab in placements(U, N):
        wide = is_wide(slab)
        chosen.add(wide)
        print('%s N=%d %s: %-20s ld=%d, base %% 16 = %d -> %s' % (name, N, spacing, label, slab.ld, slab.ptr % 16,
                                                                    'wide' if wide else 'narrow'))
        for fields in range(1, 8):
            what = '%s N=%d %s, %s, fields=%d' % (name, N, spacing, label, fields)
            ld_out = n_p + 3 * (fields & 1)
            out = pairs(stk, plan, cell, lam, t, h, N, 0, slab, fields, ld_out, what)
            got = result(out, ref.pair_rows(d, fields), n_p, what)
            assert ref.same_bits(got, want[rows_of_mask(d, fields)]), what
        note_brackets(d, t_h, h, N, 0, N, valid, wide, what)
        inputs_intact(label, cell, lam, t, slab)
    assert chosen == {True, False}


@pytest.mark.parametrize('size', (2, 3, 8))
@pytest.mark.parametrize('N', (9, 130))
@pytest.mark.parametrize('name', PAIR_MESHES)
def test_pairs_on_rank_windows(stk, name, N, size):
    """The time axis cut by stk_partition: every rank's out is the model's for its window, and
    the ranks' outs added in rank order are the one-rank doubles."""
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    d = mesh.d
    h = 1.0 / (N - 1) if size != 3 else 0.1
    t_h = ref.times_of(N, h, 53 + N)
    n_p = len(t_h)
    cell_h, lam_h = pair_points(name, n_p, stride=17)
    U = ref.slab_of(mesh.n_free, N, 54 + N)
    one = ref.pairs_model(mesh, cell_h, lam_h, t_h, h, N, 0, U, 7)
    valid = ~np.isnan(one[0])
    cell, lam, t = Flat(cell_h, dtype=np.int32), Flat(lam_h), Flat(t_h)
    whole = result(pairs(stk, plan, cell, lam, t, h, N, 0, slab_buffer(U, N + 1 + (N & 1)), 7, n_p, name), 2 + d, n_p, name)
    assert ref.same_bits(whole, one)
    total, begins = np.zeros_like(one), []
    for rank in range(size):
        tb, te = ctypes.c_int32(), ctypes.c_int32()
        stk.check(stk.lib().stk_partition(N, size, rank, ctypes.byref(tb), ctypes.byref(te), None, None))
        tb, n_loc = tb.value, te.value - tb.value
        begins.append(tb)
        label, slab = placements(U[:, tb:tb + n_loc], n_loc)[rank % 3 if n_loc > 1 else 0]
        what = '%s N=%d rank %d of %d: columns %d..%d, %s' % (name, N, rank, size, tb, tb + n_loc - 1, label)
        got = result(pairs(stk, plan, cell, lam, t, h, N, tb, slab, 7, n_p, what), 2 + d, n_p, what)
        assert ref.same_bits(got, ref.pairs_model(mesh, cell_h, lam_h, t_h, h, N, tb, U[:, tb:tb + n_loc], 7)), what
        note_brackets(d, t_h, h, N, tb, n_loc, valid, is_wide(slab), what)
        inputs_intact(what, cell, lam, t, slab)
        total += got
    assert begins[0] == 0 and sorted(begins) == begins
    print('%s N=%d on %d ranks: t_begin = %s' % (name, N, size, begins))
    assert np.array_equal(total, one, equal_nan=True) and np.array_equal(total[:, valid], whole[:, valid])


@pytest.mark.parametrize('name', PAIR_MESHES)
def test_pairs_short_and_full_workgroups(stk, name):
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    N, h, d = 130, 0.1, mesh.d
    t_h = ref.times_of(N, h, 55)
    cell_h, lam_h = pair_points(name, len(t_h), stride=11)
    U = ref.slab_of(mesh.n_free, N, 56)
    want = ref.pairs_model(mesh, cell_h, lam_h, t_h, h, N, 0, U, 7)
    for label, slab in placements(U, N)[::2]:
        for n_p in (1, 255, 256, 257):
            cell, lam, t = Flat(cell_h[-n_p:], dtype=np.int32), Flat(lam_h[-n_p:]), Flat(t_h[-n_p:])
            what = '%s %s n_p=%d' % (name, label, n_p)
            got = result(pairs(stk, plan, cell, lam, t, h, N, 0, slab, 7, n_p + 3, what), 2 + d, n_p, what)
            assert ref.same_bits(got, want[:, -n_p:]), what
            inputs_intact(what, cell, lam, t, slab)


def test_pairs_second_trip(stk):
    name = 'shuffled2d'
    mesh, plan = ref.catalogue()[name], plan_of(stk, name)
    N, h = 9, 0.125
    _, cell_b, lam_b = second_trip_block(name)
    t_b = np.resize(ref.times_of(N, h, 57), BLOCK)
    U = ref.slab_of(mesh.n_free, N, 58)
    slab = slab_buffer(U, N + 1)
    assert is_wide(slab)
    cell, lam, t = Flat.of(tiled(cell_b, FLAT_N)), Flat.of(tiled(lam_b, FLAT_N)), Flat.of(tiled(t_b, FLAT_N))
    out = pairs(stk, plan, cell, lam, t, h, N, 0, slab, 7, FLAT_N, 'second trip')
    inputs_intact('second trip', cell, lam, t, slab, out)
    assert bool((out.view[4] == OUT_START).all())
    got = out.view[:4]
    assert ref.same_bits(got[:, :BLOCK].cpu().numpy(), ref.pairs_model(mesh, cell_b, lam_b, t_b, h, N, 0, U, 7))
    for k in range(4):
        copies_equal_the_first(got[k].contiguous(), BLOCK)
    note('pairs<2, wide> second trip', 'n_p = %d' % FLAT_N)


# ---- the paths ---------------------------------------------------------------------------------------------------------
def test_every_path_was_reached(stk):
    for path in EXPECTED:
        print('%-52s %s' % (path, REACHED.get(path, '-- NOT REACHED --')))
    missing = [p for p in EXPECTED if p not in REACHED]
    assert not missing, missing
    for plan in _plans.values():
        plan.close()
    _plans.clear()
