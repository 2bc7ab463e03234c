"""What tests/test_sample_kernels_gpu.py holds the forward sampling kernels to (csrc/sample.hip:
stk_sample_locate, stk_sample_eval, stk_sample_pairs, stk_sample_grad_coeffs), and the checks of
that yardstick that need no GPU.

a. THE RESTATEMENT.  `locate_model`, `locate_all_cells`, `eval_model`, `pairs_model` and
   `grad_coeffs_model` restate the four entry points in NumPy binary64 from the text of
   include/stk.h ("sampling the trial space"), not from the kernels: every product, quotient and
   sum is one NumPy operation, in the header's order (NumPy contracts nothing).  `grid_model`
   restates the bucket grid from the same text and must equal what libstk's host code builds
   (source.sampling.bucket_grid), list for list.  `launch_plan` restates "launches of at most 96
   distinct columns": which consecutive requests share a launch.

   Comparisons are `same_bits`: equal as 64-bit patterns, every NaN equal to every NaN.  That is
   np.array_equal(..., equal_nan=True) and the sign of every zero.

b. `WRONG`: restatements with one thing wrong each.  Every one must differ from the model in at
   least one output double or cell index on the catalogue; the slab and the times are drawn again
   from a fixed sequence of seeds until it does.

c. THE MESH CATALOGUE (`catalogue()`), built from seeds: the project's `square 1`,
   `lshape_jitter 3`, `cube 1`; `shuffled2d` / `shuffled3d` (the latter two renumbered, permuted,
   about half the cells with det < 0, the free vertices in a random order); `fan` (40 triangles
   round one vertex, orientation alternating); `graded` (sizes 1 .. 2^-20 towards a corner);
   `sliver` (aspect ratio 1e6); `degenerate` (a zero-area cell, a cell listed twice); `tetfan`
   (tetrahedra round one edge); and `ledge`, whose one interior edge lies one ulp below a bin
   boundary: the only place where the widening of the bins decides an answer.

d. THE POINT CATALOGUE (`points_of`): vertices, edge midpoints, centroids, dyadic combinations on
   shared edges and faces, points on the faces of the bounding box, at lo - widen and hi + widen
   and one ulp beyond, on the bin boundaries and one ulp to either side, -0.0, +-inf, NaN and a
   denormal in one coordinate and in all, 1000 seeded random points in the box enlarged by 5 %.
   `Mesh.designed` (appended by `all_points_of`): the few points placed by hand ON a threshold
   (min l_a = -1e-12 exactly, and just beyond it; one ulp beyond the ledge).

   The cross-check of the bin search against the search over all cells leaves out NO point.  The
   statement beside it -- no point has its np.longdouble best minimum inside (-2e-12, -5e-13) --
   holds for every seeded point except those that were PUT at the threshold: the designed points
   and the points at lo - widen / hi + widen (`placed_at_the_threshold`), which lie 1e-12 extent
   outside the box and so have min l_a = -1e-12 next to any cell as high as the mesh (`graded`,
   `degenerate`, `ledge`).  The test counts and prints them.

e. The yardstick's own tests are at the end."""
import functools

import numpy as np
import pytest

from test_sampling_host import edges_of, mesh_of

INSIDE = -1e-12
MAX_COLS = 96  # distinct columns of one launch of stk_sample_eval (include/stk.h)
FLAT_CAP, BS, TP = 4096, 256, 64  # the capped grids: 4096 workgroups of 256 lanes; 64 points per eval tile
NAN = float('nan')


def same_bits(a, b):
    """Equal shapes and equal doubles bit for bit (so +0.0 != -0.0), any NaN equal to any NaN;
    integer arrays: equal values."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


# ---- c. the meshes -------------------------------------------------------------------------------
class Mesh:
    """points (nv, d), cells (nc, d + 1) int64, free (n_free,) int64 = the vertex of every slab
    row; row_of (nv,) = the slab row of a vertex, -1 on the boundary."""
    def __init__(self, name, points, cells, free, well_shaped=True, designed=None):
        self.name, self.well_shaped = name, well_shaped
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        self.cells = np.ascontiguousarray(cells, dtype=np.int64)
        self.free = np.ascontiguousarray(free, dtype=np.int64)
        self.nv, self.d = self.points.shape
        self.nc = len(self.cells)
        self.n_free = len(self.free)
        assert len(set(self.free.tolist())) == self.n_free and self.cells.max() < self.nv
        self.row_of = np.full(self.nv, -1, dtype=np.int64)
        self.row_of[self.free] = np.arange(self.n_free)
        self.designed = np.zeros((0, self.d)) if designed is None else np.array(designed, dtype=np.float64)
        for a in (self.points, self.cells, self.free, self.row_of, self.designed):
            a.setflags(write=False)

    def signed_measures(self):
        V = self.points[self.cells]
        return np.linalg.det(V[:, 1:] - V[:, :1])


def _project(problem, J):
    from source.assembly import free_dofs
    m = mesh_of(problem, J)
    return Mesh('%s %d' % (problem, J), m.points, m.cells, free_dofs(m))


def _shuffled(name, base, seed):
    rs = np.random.RandomState(seed)
    perm = rs.permutation(base.nv)  # the new number of vertex v
    pts = np.empty_like(base.points)
    pts[perm] = base.points
    cells = perm[base.cells][rs.permutation(base.nc)]
    for t in range(base.nc):
        c = np.roll(cells[t], rs.randint(base.d + 1))
        if rs.rand() < 0.5:
            c[[-2, -1]] = c[[-1, -2]]
        cells[t] = c
    return Mesh(name, pts, cells, perm[base.free][rs.permutation(base.n_free)])


def _fan(seed=21, n=40):
    rs = np.random.RandomState(seed)
    ang = 2.0 * np.pi * np.arange(n) / n
    rad = 1.0 + 0.3 * rs.rand(n)
    pts = np.concatenate([[[0.13, -0.07]], np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)])
    cells = [(0, 1 + k, 1 + (k + 1) % n) if k % 2 == 0 else (0, 1 + (k + 1) % n, 1 + k) for k in range(n)]
    return Mesh('fan', pts, cells, [5, 0, 11, 2, 38])


def _graded(levels=20):
    a = [(2.0 ** -k, 0.0) for k in range(levels + 1)]
    b = [(0.0, 2.0 ** -k) for k in range(levels + 1)]
    A, B = lambda k: 1 + k, lambda k: 2 + levels + k
    cells = []
    for k in range(levels):
        cells += [(A(k), A(k + 1), B(k + 1)), (A(k), B(k + 1), B(k))]
    cells.append((0, A(levels), B(levels)))
    return Mesh('graded', [(0.0, 0.0)] + a + b, cells, [A(1), B(1), A(10), B(levels), 0], well_shaped=False)


def _sliver(seed=22, n=4):
    rs = np.random.RandomState(seed)
    bottom = [(float(i), 0.0) for i in range(n + 1)]
    top = [(i + (0.1 * rs.rand() if 0 < i < n else 0.0), 1e-6) for i in range(n + 1)]
    cells = []
    for i in range(n):
        cells += [(i, i + 1, n + 1 + i), (i + 1, n + 2 + i, n + 1 + i)]
    return Mesh('sliver', bottom + top, cells, [1, n + 3, 3], well_shaped=False)


DEGENERATE_ZERO, DEGENERATE_TWICE = 1, (3, 9)  # the zero-area cell; the cell listed twice (lower, upper index)


def _degenerate():
    """A 2 x 2 grid of squares cut in two; cell 1 is the collinear bottom row, cell 9 repeats
    cell 3.  Cell 0 = ((0, 0), (.5, 0), (.5, .5)) has l2 = 2 y exactly: the designed point
    (0.3, -5e-13) has min l_a = l2 = -1e-12, the threshold itself."""
    pts = [(0.5 * i, 0.5 * j) for j in range(3) for i in range(3)]
    v = lambda i, j: 3 * j + i
    cells = []
    for j in range(2):
        for i in range(2):
            cells += [(v(i, j), v(i + 1, j), v(i + 1, j + 1)), (v(i, j), v(i + 1, j + 1), v(i, j + 1))]
    cells.insert(DEGENERATE_ZERO, (0, 1, 2))
    cells.append(cells[DEGENERATE_TWICE[0]])
    assert len(cells) - 1 == DEGENERATE_TWICE[1]
    return Mesh('degenerate', pts, cells, [4, 1, 7], well_shaped=False, designed=[(0.3, -5e-13), (0.3, -0.5000000001e-12)])


def _bin_axis(x, lo, inv_w, nb):
    """bin of x along one axis: floor((x - lo) * inv_width), clamped to 0 .. nb - 1; NaN: bin 0."""
    with np.errstate(invalid='ignore'):
        t = np.floor((x - lo) * inv_w)
        return np.where(t >= 0.0, np.minimum(t, nb - 1.0), 0.0).astype(np.int64)


def _ledge():
    """Two triangles over [0, xe] x [0, 1] and a small one in the far corner (the bounding box is
    the unit square, 3 cells: 2 bins per axis).  xe is the largest double of bin 0 along x, so the
    point (xb, 0.3), xb the next double, lies in bin 1, one ulp outside the two triangles --
    inside by the -1e-12 rule -- and finds them there only because the lists widen the cells."""
    widen = 1e-12
    lo, inv_w, nb = 0.0 - widen, 2.0 / ((1.0 - 0.0) + 2.0 * widen), 2
    xb = 0.5
    while _bin_axis(xb, lo, inv_w, nb) == 1:
        xb = np.nextafter(xb, -np.inf)
    while _bin_axis(xb, lo, inv_w, nb) == 0:
        xb = np.nextafter(xb, np.inf)
    xe = np.nextafter(xb, -np.inf)
    assert _bin_axis(xe, lo, inv_w, nb) == 0 and _bin_axis(xb, lo, inv_w, nb) == 1 and abs(xb - 0.5) < 1e-10
    pts = [(0.0, 0.0), (xe, 0.0), (xe, 1.0), (0.0, 1.0), (0.9, 0.9), (1.0, 0.9), (1.0, 1.0)]
    return Mesh('ledge', pts, [(0, 1, 2), (0, 2, 3), (4, 5, 6)], [2, 0, 5], well_shaped=False, designed=[(xb, 0.3)])


def _tetfan(seed=23, n=12):
    rs = np.random.RandomState(seed)
    ang = 2.0 * np.pi * np.arange(n) / n
    rad = 1.0 + 0.2 * rs.rand(n)
    ring = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.5 + 0.2 * (rs.rand(n) - 0.5)], axis=1)
    pts = np.concatenate([[[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], ring])
    cells = [(0, 1, 2 + k, 2 + (k + 1) % n) if k % 2 == 0 else (0, 1, 2 + (k + 1) % n, 2 + k) for k in range(n)]
    return Mesh('tetfan', pts, cells, [1, 4, 0, 9, 13])


@functools.lru_cache(maxsize=None)
def catalogue():
    base2, base3 = _project('lshape_jitter', 3), _project('cube', 1)
    meshes = [_project('square', 1), base2, base3, _shuffled('shuffled2d', base2, 31), _shuffled('shuffled3d', base3, 32),
              _fan(), _graded(), _sliver(), _degenerate(), _tetfan(), _ledge()]
    return {m.name: m for m in meshes}


MESH_NAMES = ('square 1', 'lshape_jitter 3', 'cube 1', 'shuffled2d', 'shuffled3d', 'fan', 'graded', 'sliver', 'degenerate',
              'tetfan', 'ledge')
WELL_SHAPED = ('square 1', 'lshape_jitter 3', 'cube 1', 'shuffled2d', 'shuffled3d', 'fan', 'tetfan')
EXACT_AT_VERTICES = ('square 1', 'lshape_jitter 3', 'cube 1', 'shuffled2d', 'shuffled3d', 'fan')  # see test_eval_model_...


# ---- the bucket grid -------------------------------------------------------------------------------
def grid_model(mesh, wrong=None):
    """The bucket grid by the text of include/stk.h, as the dict of source.sampling.bucket_grid."""
    pts, cells, d, nc = mesh.points, mesh.cells, mesh.d, mesh.nc
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    extent = (hi - lo).max()
    widen = 1e-12 * extent
    nb = max(1, int(np.floor(float(nc) ** (1.0 / d) + 0.5)))
    lo_s, inv_w = lo - widen, nb / ((hi - lo) + 2.0 * widen)
    corners = pts[cells]
    grow = 0.0 if wrong == 'bins-unwidened' else widen
    first = np.stack([_bin_axis(corners[:, :, k].min(axis=1) - grow, lo_s[k], inv_w[k], nb) for k in range(d)], axis=1)
    last = np.stack([_bin_axis(corners[:, :, k].max(axis=1) + grow, lo_s[k], inv_w[k], nb) for k in range(d)], axis=1)
    member = np.zeros((nb,) * d + (nc,), dtype=bool)  # [iz][iy][ix][cell]
    for t in range(nc):
        member[tuple(slice(first[t, k], last[t, k] + 1) for k in reversed(range(d))) + (t,)] = True
    member = member.reshape(-1, nc)
    bins_of, cells_of = np.nonzero(member)  # row-major: the cells of a bin ascending
    bin_ptr = np.concatenate([[0], np.cumsum(member.sum(axis=1))]).astype(np.int32)
    return {'bins': np.full(d, nb, dtype=np.int32), 'lo': lo_s, 'inv_width': inv_w, 'widen': widen, 'bin_ptr': bin_ptr,
            'bin_cells': cells_of.astype(np.int32)}


@functools.lru_cache(maxsize=None)
def grid_of(name):
    """The grid libstk's host code builds for a catalogue mesh (no GPU is touched)."""
    from source.sampling import bucket_grid
    return bucket_grid(catalogue()[name])


def _members(mesh, grid):
    ptr = grid['bin_ptr'].astype(np.int64)
    member = np.zeros((len(ptr) - 1, mesh.nc), dtype=bool)
    member[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), grid['bin_cells']] = True
    return member


def bins_of_points(grid, x):
    """The flat bin index of every point: (iz bins[1] + iy) bins[0] + ix."""
    d = x.shape[1]
    flat = np.zeros(len(x), dtype=np.int64)
    for k in reversed(range(d)):
        flat = flat * int(grid['bins'][k]) + _bin_axis(x[:, k], grid['lo'][k], grid['inv_width'][k], int(grid['bins'][k]))
    return flat


# ---- a. the restatement ------------------------------------------------------------------------------
def _cross(a, b):
    return [a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
            a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]]


def _edges(V):
    p0 = V[:, 0]
    return p0, [V[:, r + 1] - p0 for r in range(V.shape[2])]


def _fused(a, b, c):
    """a b + c with the product not rounded to binary64 on its own: an emulation of one fused
    multiply-add (the product in np.longdouble)."""
    return (np.asarray(a, np.longdouble) * np.asarray(b, np.longdouble) + np.asarray(c, np.longdouble)).astype(np.float64)


def barycentric(V, x, wrong=None):
    """l [n][nc][d + 1] of the points x (n, d) in the cells with vertices V (nc, d + 1, d), in the
    dtype of V: e_r = p_r - p0, q = x - p0;  triangles l1 = (q x e2) / (e1 x e2), l2 = (e1 x q) /
    (e1 x e2), a x b = a0 b1 - a1 b0;  tetrahedra l_r = q . c_r / det with c = (e2 x e3, e3 x e1,
    e1 x e2), det = e1 . c_1, dot products from the left;  l0 = ((1 - l1) - l2) [- l3]."""
    d = x.shape[1]
    one = V.dtype.type(1.0)
    p0, e = _edges(V)
    q = x.astype(V.dtype)[:, None, :] - p0[None, :, :]
    q = [q[..., k] for k in range(d)]
    with np.errstate(all='ignore'):
        if d == 2:
            e1, e2 = e
            det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            if wrong == 'one-product-fused':
                n1 = _fused(q[0], e2[:, 1], -(q[1] * e2[:, 0]))
            else:
                n1 = q[0] * e2[:, 1] - q[1] * e2[:, 0]
            l = [n1 / det, (e1[:, 0] * q[1] - e1[:, 1] * q[0]) / det]
        else:
            c = [_cross(e[1], e[2]), _cross(e[2], e[0]), _cross(e[0], e[1])]
            det = (e[0][:, 0] * c[0][0] + e[0][:, 1] * c[0][1]) + e[0][:, 2] * c[0][2]
            l = []
            for r in range(3):
                if wrong == 'one-product-fused' and r == 0:
                    two = _fused(q[1], c[r][1], q[0] * c[r][0])
                else:
                    two = q[0] * c[r][0] + q[1] * c[r][1]
                l.append((two + q[2] * c[r][2]) / det)
        if wrong == 'l0-grouped':
            l0 = one - (l[0] + l[1]) if d == 2 else one - ((l[0] + l[1]) + l[2])
        else:
            l0 = (one - l[0]) - l[1]
            if d == 3:
                l0 = l0 - l[2]
    return np.stack([l0] + l, axis=2)


def _locate(mesh, x, member_of_point, wrong=None, dtype=np.float64, chunk=512):
    """(cell, lam, best) over the allowed candidates: a candidate with a NaN coordinate is skipped,
    the largest min_a l_a wins, strict `>` from -inf in ascending order (the lowest index on a
    tie; a candidate whose minimum is -inf never wins); cell = -1 where best < -1e-12; lam is the
    winner's also outside, NaN without a winner."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    V = mesh.points[mesh.cells].astype(dtype)
    cell, lam, best = np.empty(n, np.int32), np.empty((n, d + 1), dtype), np.empty(n, dtype)
    for a in range(0, n, chunk):
        s = slice(a, min(a + chunk, n))
        l = barycentric(V, x[s], wrong)
        with np.errstate(invalid='ignore'):
            ok = ~np.isnan(l).any(axis=2)
            if member_of_point is not None:
                ok &= member_of_point(s)
            m = np.where(ok, np.where(ok[:, :, None], l, 0.0).min(axis=2), -np.inf)
        if wrong == 'tie-to-highest':
            win = mesh.nc - 1 - np.argmax(m[:, ::-1], axis=1)
        else:
            win = np.argmax(m, axis=1)  # the first of equal maxima
        rows = np.arange(len(win))
        b = m[rows, win]
        found = b > -np.inf
        inside = b > INSIDE if wrong == 'inside-strict' else b >= INSIDE
        cell[s] = np.where(found & inside, win, -1)
        lam[s] = np.where(found[:, None], l[rows, win], np.nan)
        best[s] = b
    return cell, lam, best


def locate_model(mesh, grid, x, wrong=None):
    """(cell [n_p] int32, lam [n_p][d + 1]) as stk_sample_locate writes them: the candidates are the
    cells of the point's bin."""
    x = np.asarray(x, dtype=np.float64)
    member, flat = _members(mesh, grid), bins_of_points(grid, x)
    cell, lam, _ = _locate(mesh, x, lambda s: member[flat[s]], wrong)
    return cell, lam


def locate_all_cells(mesh, x, wrong=None, dtype=np.float64):
    """(cell, lam, best minimum): the same arithmetic over ALL cells, no grid."""
    return _locate(mesh, x, None, wrong, dtype)


def grad_coeffs_model(mesh, cell, wrong=None):
    """out [d][n_p][d + 1] of stk_sample_grad_coeffs: out[j][p][a] = d_j l_a of cell[p], NaN for
    cell < 0 and cell >= nc."""
    cell = np.asarray(cell, dtype=np.int64)
    d = mesh.d
    ok = (cell >= 0) & (cell < mesh.nc)
    _, e = _edges(mesh.points[mesh.cells[np.where(ok, cell, 0)]])
    with np.errstate(all='ignore'):
        if d == 2:
            e1, e2 = e
            det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            g = [[e2[:, 1] / det, (-e2[:, 0]) / det], [(-e1[:, 1]) / det, e1[:, 0] / det]]
        else:
            c = [_cross(e[1], e[2]), _cross(e[2], e[0]), _cross(e[0], e[1])]
            det = (e[0][:, 0] * c[0][0] + e[0][:, 1] * c[0][1]) + e[0][:, 2] * c[0][2]
            g = [[c[r][j] / det for j in range(3)] for r in range(3)]
        out = np.empty((d, len(cell), d + 1))
        for j in range(d):
            if wrong == 'grad-l0-negated-sum':
                s = g[0][j] + g[1][j]
                g0 = -(s + g[2][j]) if d == 3 else -s
            else:
                g0 = (0.0 - g[0][j]) - g[1][j]
                if d == 3:
                    g0 = g0 - g[2][j]
            out[j, :, 0] = g0
            for r in range(d):
                out[j, :, r + 1] = g[r][j]
    out[:, ~ok, :] = np.nan
    return out


def spatial_sums(mesh, cell, k, slab, wrong=None):
    """S(k, c) [n_p][n_loc] = ((k_0 u[v_0][c] + k_1 u[v_1][c]) + k_2 u[v_2][c]) [+ k_3 u[v_3][c]] for
    every column of slab (M, n_loc); a boundary vertex has the value 0.  Rows of cells out of
    range are those of cell 0 (the callers overwrite them)."""
    cell = np.asarray(cell, dtype=np.int64)
    ok = (cell >= 0) & (cell < mesh.nc)
    rows = mesh.row_of[mesh.cells[np.where(ok, cell, 0)]]  # (n_p, d + 1)
    u = np.where((rows >= 0)[:, :, None], slab[np.maximum(rows, 0)], 0.0)  # (n_p, d + 1, n_loc)
    with np.errstate(all='ignore'):
        terms = k[:, :, None] * u
        order = range(mesh.d, -1, -1) if wrong == 'S-from-the-right' else range(mesh.d + 1)
        total = None
        for a in order:
            total = terms[:, a] if total is None else total + terms[:, a]
    return total


def eval_model(mesh, cell, lam, slab, columns, weights, wrong=None):
    """out [n_k][n_p] of stk_sample_eval for slab (M, n_loc) (the valid columns), columns (n_k, 2)
    (-1 = absent) and weights (n_k, 2): p_0 + p_1, p_a = w_a S(lam, c_a), an absent term exactly
    0.0; NaN for cell < 0 and cell >= nc."""
    cell = np.asarray(cell, dtype=np.int64)
    columns, weights = np.asarray(columns).reshape(-1, 2), np.asarray(weights, dtype=np.float64).reshape(-1, 2)
    S = spatial_sums(mesh, cell, np.asarray(lam, dtype=np.float64), slab, wrong)
    out = np.empty((len(columns), len(cell)))
    a, b = (1, 0) if wrong == 'weights-swapped' else (0, 1)
    with np.errstate(all='ignore'):
        for k, (c0, c1) in enumerate(columns):
            p0 = weights[k, a] * S[:, c0] if c0 >= 0 else 0.0
            p1 = weights[k, b] * S[:, c1] if c1 >= 0 else 0.0
            out[k] = p0 + p1
    out[:, (cell < 0) | (cell >= mesh.nc)] = np.nan
    return out


def time_bracket(t, h, N, wrong=None):
    """(ef, w0, w1): e = min(floor(t / h), N - 2) as a double, s = t / h - e, (w0, w1) = (1 - s, s)."""
    with np.errstate(all='ignore'):
        x = np.asarray(t, dtype=np.float64) / h
        ef = np.rint(x) if wrong == 'bracket-rounds' else np.floor(x)
        if wrong != 'bracket-unclamped':
            ef = np.minimum(ef, float(N - 2))
        s = x - ef
        return ef, 1.0 - s, s


def requests_of_times(t, h, N, t_begin, n_loc):
    """(columns (n_k, 2) int32, weights (n_k, 2)) of times in [0, (N - 1) h] on a rank that holds
    the nodes t_begin .. t_begin + n_loc - 1: what stk_sample_eval takes."""
    ef, w0, w1 = time_bracket(t, h, N)
    c0 = ef.astype(np.int64) - t_begin
    cols = np.stack([c0, c0 + 1], axis=1)
    cols[(cols < 0) | (cols >= n_loc)] = -1
    return np.ascontiguousarray(cols, dtype=np.int32), np.ascontiguousarray(np.stack([w0, w1], axis=1))


def pair_rows(d, fields):
    return (fields & 1) + (fields >> 1 & 1) + (fields >> 2 & 1) * d


def pairs_model(mesh, cell, lam, t, h, N, t_begin, slab, fields, wrong=None):
    """out [n_rows][n_p] of stk_sample_pairs for slab (M, n_loc): the requested rows in the order
    u, dt, grad_0 .. grad_(d-1); NaN where cell < 0, cell >= nc, t is NaN or outside [0, (N - 1) h]."""
    cell, t = np.asarray(cell, dtype=np.int64), np.asarray(t, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    n_p, n_loc, d = len(cell), slab.shape[1], mesh.d
    with np.errstate(invalid='ignore'):
        valid = (cell >= 0) & (cell < mesh.nc) & (t >= 0.0) & (t <= float(N - 1) * h)
    ef, w0, w1 = time_bracket(np.where(valid, t, 0.0), h, N, wrong)
    if wrong == 'weights-swapped':
        w0, w1 = w1, w0
    c0 = ef.astype(np.int64) - t_begin
    c1 = c0 + 1
    have0, have1 = (c0 >= 0) & (c0 < n_loc), (c1 >= 0) & (c1 < n_loc)
    p = np.arange(n_p)

    def two(k):
        S = spatial_sums(mesh, cell, k, slab, wrong)
        return S[p, np.where(have0, c0, 0)], S[p, np.where(have1, c1, 0)]

    rows = []
    with np.errstate(all='ignore'):
        if fields & 3:
            S0, S1 = two(lam)
        if fields & 1:
            rows.append(np.where(have0, w0 * S0, 0.0) + np.where(have1, w1 * S1, 0.0))
        if fields & 2:
            rows.append(np.where(have0, -(S0 / h), 0.0) + np.where(have1, S1 / h, 0.0))
        if fields & 4:
            G = grad_coeffs_model(mesh, cell, 'grad-l0-negated-sum' if wrong == 'grad-l0-negated-sum' else None)
            for j in range(d):
                S0, S1 = two(G[j])
                rows.append(np.where(have0, w0 * S0, 0.0) + np.where(have1, w1 * S1, 0.0))
    out = np.stack(rows)
    out[:, ~valid] = np.nan
    return out


def launch_plan(columns, n_loc):
    """[(k0, n_kc, n_c)]: consecutive requests share a launch while its distinct columns stay at
    or below 96; a request that would bring the count above starts the next one."""
    columns = np.asarray(columns).reshape(-1, 2)
    launches, used, k0 = [], [], 0
    for k, (c0, c1) in enumerate(columns):
        fresh = [c for c in dict.fromkeys((int(c0), int(c1))) if c >= 0 and c not in used]
        if len(used) + len(fresh) > MAX_COLS:
            launches.append((k0, k - k0, len(used)))
            used, k0 = [], k
            fresh = [c for c in dict.fromkeys((int(c0), int(c1))) if c >= 0]
        used += fresh
    launches.append((k0, len(columns) - k0, len(used)))
    return launches


# ---- d. the points -----------------------------------------------------------------------------------
def _faces_of(mesh):
    c = mesh.cells
    f = np.concatenate([np.delete(c, a, axis=1) for a in range(4)])
    return np.unique(np.sort(f, axis=1), axis=0)


SPECIALS = (-0.0, np.inf, -np.inf, np.nan, 5e-324)
POINT_SEED = {name: 100 + i for i, name in enumerate(MESH_NAMES)}


@functools.lru_cache(maxsize=None)
def _points(name):
    mesh, grid = catalogue()[name], grid_of(name)
    pts, d = mesh.points, mesh.d
    rs = np.random.RandomState(POINT_SEED[name])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    widen = grid['widen']
    inbox = lambda n: lo + (hi - lo) * rs.rand(n, d)
    edges = edges_of(mesh)
    sets = [pts.copy(), pts[edges].mean(axis=1), pts[mesh.cells].mean(axis=1)]
    offset = []  # (first, last) of the points placed at lo - widen, hi + widen and one ulp beyond
    s = np.array([0.25, 0.75, 0.125])[np.arange(len(edges)) % 3][:, None]
    sets.append((1.0 - s) * pts[edges[:, 0]] + s * pts[edges[:, 1]])
    if d == 3:
        f = _faces_of(mesh)
        w = np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.125, 0.125, 0.75]])[np.arange(len(f)) % 3]
        sets.append((w[:, 0, None] * pts[f[:, 0]] + w[:, 1, None] * pts[f[:, 1]]) + w[:, 2, None] * pts[f[:, 2]])
    # the faces of the bounding box, lo - widen and hi + widen, one ulp beyond; their corners
    levels = lambda k: [lo[k], hi[k], lo[k] - widen, hi[k] + widen, np.nextafter(lo[k] - widen, -np.inf),
                        np.nextafter(hi[k] + widen, np.inf)]
    count = lambda: sum(len(a) for a in sets)
    for k in range(d):
        for i, v in enumerate(levels(k)):
            x = inbox(12)
            x[:, k] = v
            if i >= 2:
                offset.append((count(), count() + len(x)))
            sets.append(x)
    for i in range(3):
        for corner in range(2 ** d):
            if i >= 1:
                offset.append((count(), count() + 1))
            sets.append(np.array([[levels(k)[2 * i + (corner >> k & 1)] for k in range(d)]]))
    # the bin boundaries, and one ulp to either side
    for k in range(d):
        for i in range(int(grid['bins'][k]) + 1):
            xb = grid['lo'][k] + i / grid['inv_width'][k]
            for v in (np.nextafter(xb, -np.inf), xb, np.nextafter(xb, np.inf)):
                x = inbox(3)
                x[:, k] = v
                if i in (0, int(grid['bins'][k])):  # the ends of the widened box again
                    offset.append((count(), count() + len(x)))
                sets.append(x)
    base = pts[mesh.cells[0]].mean(axis=0)
    for v in SPECIALS:
        for k in range(d):
            x = base.copy()
            x[k] = v
            sets.append(x[None, :])
        sets.append(np.full((1, d), v))
    sets.append(lo - 0.05 * (hi - lo) + 1.1 * (hi - lo) * rs.rand(1000, d))
    out = np.concatenate(sets)
    out.setflags(write=False)
    on_purpose = np.zeros(len(out), dtype=bool)
    for a, b in offset:
        on_purpose[a:b] = True
    on_purpose.setflags(write=False)
    return out, on_purpose


def points_of(name):
    """The point catalogue of a mesh without its designed points, (n, d), read-only."""
    return _points(name)[0]


def placed_at_the_threshold(name):
    """Mask over points_of(name): the points put at lo - widen, at hi + widen and one ulp beyond.
    The widening is 1e-12 extent, so next to a cell as high as the mesh they have min l_a = -1e-12
    by construction."""
    return _points(name)[1]


@functools.lru_cache(maxsize=None)
def all_points_of(name):
    """The seeded catalogue followed by the designed points of the mesh."""
    out = np.concatenate([points_of(name), catalogue()[name].designed])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def located(name):
    """locate_model on all points of a mesh: (cell, lam), computed once, read-only."""
    cell, lam = locate_model(catalogue()[name], grid_of(name), all_points_of(name))
    cell.setflags(write=False), lam.setflags(write=False)
    return cell, lam


@functools.lru_cache(maxsize=None)
def located_all_cells(name):
    out = locate_all_cells(catalogue()[name], all_points_of(name))
    for a in out:
        a.setflags(write=False)
    return out


def slab_of(M, n_loc, seed):
    """Nodal values (M, n_loc): signed, scaled over six decades row by row."""
    rs = np.random.RandomState(seed)
    return rs.randn(M, n_loc) * 10.0 ** rs.randint(-3, 4, size=(M, 1))


def times_of(N, h, seed, n_random=40):
    """0, (N - 1) h, every node, every node +- one ulp, the midpoints, seeded random times, and NaN,
    -0.0, a negative time, T + ulp, +inf."""
    T = float(N - 1) * h
    nodes = np.arange(N) * h
    rs = np.random.RandomState(seed)
    return np.concatenate([[0.0, T], nodes, np.nextafter(nodes, np.inf), np.nextafter(nodes, -np.inf),
                           0.5 * (nodes[1:] + nodes[:-1]), T * rs.rand(n_random),
                           [np.nan, -0.0, -0.25 * h, np.nextafter(T, np.inf), np.inf]])


# ---- b. restatements with one thing wrong -------------------------------------------------------------
WRONG = {'one-product-fused': 'locate', 'l0-grouped': 'locate', 'tie-to-highest': 'locate', 'inside-strict': 'locate',
         'bins-unwidened': 'grid', 'bracket-rounds': 'pairs', 'bracket-unclamped': 'pairs', 'weights-swapped': 'pairs+eval',
         'S-from-the-right': 'pairs+eval', 'grad-l0-negated-sum': 'grad'}
WRONG_MESHES = ('degenerate', 'ledge', 'square 1', 'fan', 'tetfan', 'shuffled2d')
WRONG_SEEDS = (0, 1, 2, 3, 4)


def _outputs(name, seed, where, wrong):
    """What the restatement (wrong = None: the model) of the entry points named in `where` gives
    on the catalogue data of a mesh: a list of arrays."""
    mesh, x = catalogue()[name], all_points_of(name)
    cell, lam = located(name)
    N, h = 9, 0.125
    out = []
    if 'locate' in where:
        out += list(locate_model(mesh, grid_of(name), x, wrong))
    if 'grid' in where:
        out += list(locate_model(mesh, grid_model(mesh, wrong), x))
    if 'grad' in where:
        out.append(grad_coeffs_model(mesh, cell, wrong))
    if 'pairs' in where:
        t = np.resize(times_of(N, h, seed), len(cell))
        out.append(pairs_model(mesh, cell, lam, t, h, N, 0, slab_of(mesh.n_free, N, seed), 7, wrong))
    if 'eval' in where:
        cols, w = requests_of_times(times_of(N, h, seed)[:-5], h, N, 0, N)
        out.append(eval_model(mesh, cell, lam, slab_of(mesh.n_free, N, seed), cols, w, wrong))
    return out


@pytest.mark.parametrize('wrong', sorted(WRONG))
def test_every_wrong_restatement_differs_from_the_model(wrong):
    where = WRONG[wrong]
    for seed in WRONG_SEEDS:
        for name in WRONG_MESHES:
            good, bad = _outputs(name, seed, where, None), _outputs(name, seed, where, wrong)
            if not all(same_bits(g, b) for g, b in zip(good, bad)):
                print('%s: differs on %s, seed %d' % (wrong, name, seed))
                return
    raise AssertionError('%s gives the doubles of the model on all catalogue data' % wrong)


# ---- e. the yardstick ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', MESH_NAMES)
def test_grid_model_is_the_grid_of_the_library(name):
    mesh = catalogue()[name]
    mine, lib = grid_model(mesh), grid_of(name)
    assert sorted(mine) == sorted(lib)
    for key in lib:
        assert same_bits(np.asarray(mine[key]), np.asarray(lib[key])), key
    sizes = np.diff(lib['bin_ptr'])
    print('%-16s %5d cells, %3d bins per axis, lists of %d .. %d cells, %d entries' % (
        name, mesh.nc, lib['bins'][0], sizes.min(), sizes.max(), len(lib['bin_cells'])))


def test_the_catalogue_is_what_it_says():
    cat = catalogue()
    assert tuple(cat) == MESH_NAMES
    for name in ('shuffled2d', 'shuffled3d', 'fan', 'tetfan'):
        neg = (cat[name].signed_measures() < 0).mean()
        assert 0.25 <= neg <= 0.75, (name, neg)
    for name in MESH_NAMES:
        print('%-16s %5.1f %% of the cells have det < 0' % (name, 100.0 * (cat[name].signed_measures() < 0).mean()))
    for a, b in (('lshape_jitter 3', 'shuffled2d'), ('cube 1', 'shuffled3d')):
        assert not np.array_equal(cat[a].points, cat[b].points) and not np.array_equal(cat[a].free, np.sort(cat[b].free))
        assert np.array_equal(np.sort(cat[a].points, axis=0), np.sort(cat[b].points, axis=0))
        assert np.isclose(np.abs(cat[a].signed_measures()).sum(), np.abs(cat[b].signed_measures()).sum(), rtol=1e-12)
    assert np.any(np.diff(cat['shuffled2d'].free) < 0)
    g = np.abs(cat['graded'].signed_measures())
    assert g.max() / g.min() >= 2.0 ** 38
    sizes = np.diff(grid_of('graded')['bin_ptr'])
    assert sizes.max() > cat['graded'].nc // 2 and sizes.min() >= 1  # one bin holds most cells; the largest are everywhere
    V = cat['sliver'].points[cat['sliver'].cells]
    assert np.ptp(V[:, :, 0], axis=1).min() / np.ptp(V[:, :, 1], axis=1).max() >= 0.9e6
    deg = cat['degenerate']
    assert deg.signed_measures()[DEGENERATE_ZERO] == 0.0
    assert np.array_equal(deg.cells[DEGENERATE_TWICE[0]], deg.cells[DEGENERATE_TWICE[1]])


@pytest.mark.parametrize('name', MESH_NAMES)
def test_the_bucket_grid_loses_no_cell(name):
    """Wherever the search over ALL cells finds a point inside, the search over the point's bin
    finds the same cell and the same coordinates, bit for bit.  NO point is left out of that.
    Beside it: the np.longdouble best minimum of no point lies inside (-2e-12, -5e-13), the range
    in which the two searches could be excused for disagreeing -- except the points that were PUT
    there (placed_at_the_threshold, the designed points), which are counted and printed."""
    mesh = catalogue()[name]
    cell, lam = located(name)
    cell_a, lam_a, _ = located_all_cells(name)
    n_seeded = len(points_of(name))
    _, _, best = locate_all_cells(mesh, points_of(name), dtype=np.longdouble)
    with np.errstate(invalid='ignore'):
        near = (best > np.longdouble(-2e-12)) & (best < np.longdouble(-5e-13))
    put = placed_at_the_threshold(name)
    assert (near & ~put).sum() == 0, (name, np.flatnonzero(near & ~put), points_of(name)[near & ~put])
    inside = cell_a >= 0
    print('%-16s %5d points, %5d inside by all cells, %d designed, %d of the %d placed at the threshold are near it' % (
        name, len(cell), inside.sum(), len(cell) - n_seeded, (near & put).sum(), put.sum()))
    assert inside.sum() >= min(mesh.nv, 8)
    assert np.array_equal(cell[inside], cell_a[inside])
    assert same_bits(lam[inside], lam_a[inside])
    assert not (cell[~inside] >= 0).any()  # the bin search sees fewer cells: it finds nothing more


@pytest.mark.parametrize('name', WELL_SHAPED)
def test_located_points_are_reproduced(name):
    """Inside points on the well-shaped meshes: the np.longdouble coordinates of the point in the
    chosen cell, and the model's binary64 ones, give the point back to 1e-13 extent."""
    mesh = catalogue()[name]
    assert mesh.well_shaped
    x = all_points_of(name)
    cell, lam = located(name)
    inside = cell >= 0
    extent = np.ptp(mesh.points, axis=0).max()
    V = mesh.points[mesh.cells[cell[inside]]]
    ld = np.stack([barycentric(V[i:i + 1].astype(np.longdouble), x[inside][i:i + 1])[0, 0] for i in range(inside.sum())])
    for l in (ld, lam[inside]):
        back = np.einsum('pa,pak->pk', l, V.astype(l.dtype))
        assert np.max(np.abs(back - x[inside])) <= 1e-13 * extent
        assert np.max(np.abs(l.sum(axis=1) - 1.0)) <= 1e-14
    assert np.max(np.abs(ld - lam[inside])) <= 1e-13
    assert lam[inside].min() >= INSIDE


@pytest.mark.parametrize('name', EXACT_AT_VERTICES)
def test_eval_model_gives_the_slab_back_at_the_free_vertices(name):
    """Every node a request, every free vertex a point: the block is the slab, exactly.  (A vertex
    of a triangle has the coordinates (1, 0, 0) exactly, in whichever cell wins; of a tetrahedron
    where the cofactors are exact, as on the dyadic cube.)"""
    mesh = catalogue()[name]
    N = 9
    h = 1.0 / (N - 1)
    U = slab_of(mesh.n_free, N, 7)
    cell, lam = locate_model(mesh, grid_of(name), mesh.points[mesh.free])
    assert (cell >= 0).all() and set(np.unique(lam)) <= {0.0, 1.0}
    cols, w = requests_of_times(np.arange(N) * h, h, N, 0, N)
    assert tuple(cols[-1]) == (N - 2, N - 1) and tuple(w[-1]) == (0.0, 1.0) and np.all(w[:-1] == (1.0, 0.0))
    assert np.array_equal(eval_model(mesh, cell, lam, U, cols, w), U.T)
    boundary = np.flatnonzero(mesh.row_of < 0)
    if len(boundary):
        cb, lb = locate_model(mesh, grid_of(name), mesh.points[boundary])
        assert np.all(eval_model(mesh, cb, lb, U, cols, w) == 0.0)


@pytest.mark.parametrize('name', ('shuffled2d', 'tetfan', 'degenerate'))
@pytest.mark.parametrize('N', (2, 9, 129))
def test_pairs_model_is_the_diagonal_of_the_block(name, N):
    """(N - 1) a power of two, h = 1 / (N - 1): -(S / h) = (-1 / h) S, so u, dt (weights -1/h, 1/h)
    and grad_j (the rows of grad_coeffs_model as lam) of the pairs are the diagonals of
    eval_model's blocks."""
    mesh = catalogue()[name]
    h = 1.0 / (N - 1)
    t = times_of(N, h, N)[:-5]
    t = t[(t >= 0.0) & (t <= float(N - 1) * h)]  # the block form takes requests: nothing there refuses a time
    cell, lam = (a[::-7][:len(t)] for a in located(name))  # from the end: the random points, some outside
    t = t[:len(cell)]
    U = slab_of(mesh.n_free, N, N + 1)
    rows = pairs_model(mesh, cell, lam, t, h, N, 0, U, 7)
    cols, w = requests_of_times(t, h, N, 0, N)
    diag = lambda block: block[np.arange(len(t)), np.arange(len(t))]
    assert same_bits(rows[0], diag(eval_model(mesh, cell, lam, U, cols, w)))
    assert same_bits(rows[1], diag(eval_model(mesh, cell, lam, U, cols, np.broadcast_to([-1.0 / h, 1.0 / h], w.shape))))
    G = grad_coeffs_model(mesh, cell)
    for j in range(mesh.d):
        assert same_bits(rows[2 + j], diag(eval_model(mesh, cell, G[j], U, cols, w)))
    assert 0 < np.isnan(rows[0]).sum() < len(t)


def test_the_degenerate_cell_never_wins_and_the_lower_copy_does():
    mesh = catalogue()['degenerate']
    for cell in (located('degenerate')[0], located_all_cells('degenerate')[0]):
        assert not (cell == DEGENERATE_ZERO).any() and not (cell == DEGENERATE_TWICE[1]).any()
        assert (cell == DEGENERATE_TWICE[0]).sum() >= 10
    # the designed points: on the threshold (inside), and just beyond it (outside)
    cell, lam = (a[len(points_of('degenerate')):] for a in located('degenerate'))
    assert cell[0] == 0 and lam[0].min() == INSIDE and cell[1] == -1 and INSIDE > lam[1].min() > 1.001 * INSIDE
    x = mesh.points[mesh.cells[DEGENERATE_TWICE[0]]].mean(axis=0)[None, :]
    assert locate_model(mesh, grid_of('degenerate'), x, 'tie-to-highest')[0][0] == DEGENERATE_TWICE[1]


def test_the_ledge_point_needs_the_widened_lists():
    mesh = catalogue()['ledge']
    cell, lam = locate_model(mesh, grid_of('ledge'), mesh.designed)
    assert cell[0] == 0 and -1e-15 < lam[0].min() < 0.0
    cell, lam = locate_model(mesh, grid_model(mesh, 'bins-unwidened'), mesh.designed)
    assert cell[0] == -1 and np.isnan(lam[0]).all()


def test_launch_plan():
    asc = lambda n: [(c, c + 1) for c in range(n - 1)]
    assert launch_plan([(0, 0)], 1) == [(0, 1, 1)]
    assert launch_plan(asc(96), 300) == [(0, 95, 96)]
    assert launch_plan(asc(97), 300) == [(0, 95, 96), (95, 1, 2)]
    assert [l[2] for l in launch_plan(asc(192), 300)] == [96, 96, 2]
    assert [l[2] for l in launch_plan(asc(300), 300)] == [96, 96, 96, 15]
    assert launch_plan(asc(95) + [(200, 201)], 300) == [(0, 94, 95), (94, 1, 2)]
    assert launch_plan(asc(96) + [(-1, -1), (-1, 7), (200, -1)], 300) == [(0, 97, 96), (97, 1, 1)]
    assert launch_plan([(-1, -1)] * 5, 3) == [(0, 5, 0)]
