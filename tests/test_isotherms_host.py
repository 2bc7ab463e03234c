"""The contract of the isotherms (include/stk.h "isotherms", source/isotherms.py) as a plain
NumPy loop -- the oracle of tests/test_isotherms_gpu.py, which compares the device against it
with array_equal -- checked here against what knows nothing of it: the chord of a line through
the unit square and the section of a plane through the unit cube; against the zone of the
time curves, whose faces the pieces are; and the parts of source/isotherms.py that need no
device: the measures, the tree sums and the argument checks."""
import math

import numpy as np
import pytest
import torch

from source.assembly import free_dofs
from source.isotherms import check_arguments, node_tree_sums, piece_measure, width
from source.postprocess import PostProcessing
from source.problem import problem_helper
from source.time_curves import rows
from test_history_host import same
from test_time_curves_host import (_mesh, cell_geometry, first_cells, numpy_time_curves, planted_values, row_map,
                                   zone_of_cells)

BS = 256
EPS = 2.0**-52

MESHES = {
    'square0': lambda: _mesh('square', 0),  # 8 cells, one free dof
    'square1': lambda: _mesh('square', 1),
    'square2': lambda: _mesh('square', 2),
    'square4': lambda: _mesh('square', 4),  # 2048 cells: eight tiles
    'lshape_jitter3': lambda: _mesh('lshape_jitter', 3),
    'cube1': lambda: _mesh('cube', 1),
    'cube2': lambda: _mesh('cube', 2),
    'first255': lambda: first_cells(_mesh('square', 4), 255),  # tail lanes
    'first256': lambda: first_cells(_mesh('square', 4), 256),  # exactly one tile
    'first257': lambda: first_cells(_mesh('square', 4), 257),  # a second tile of one cell
    'first513': lambda: first_cells(_mesh('square', 4), 513),  # two full tiles and a third of one cell
}
WHOLE = ('square1', 'square2', 'square4', 'lshape_jitter3', 'cube1', 'cube2')  # "from square1 up"
N_PLANTED = 65
THETAS = (0.3, 1.0)


# ---- the contract ---------------------------------------------------------------------------------
def numpy_isotherms(points, cells, row_of, U, theta):
    """The contract: (counts (n_cols, n_tiles) int64, records (n, W)) of the columns of U (M,
    n_cols), the slab rows of the vertices with row_of >= 0 (row_of=None: U holds ALL vertices,
    none carries the Dirichlet zero).  One column at a time, vectorised over the cells; every
    operation is one NumPy operation on doubles, rounded on its own.  The records come column
    by column, cell by cell, in the table's order."""
    points, cells = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    U = np.asarray(U, dtype=np.float64)
    n_cols = U.shape[1]
    nc, d = len(cells), cells.shape[1] - 1
    W = d * d + d + 1
    n_tiles = (nc + BS - 1) // BS
    row_of = np.arange(len(points)) if row_of is None else np.asarray(row_of)
    _, g = cell_geometry(points, cells)
    P, r = points[cells], row_of[cells]
    theta = np.float64(theta)
    counts = np.zeros((n_cols, n_tiles), dtype=np.int64)
    records = [np.zeros((0, W))]
    if np.isinf(theta):  # no piece at all
        return counts, records[0]
    tile_of = np.arange(nc) // BS
    every = np.arange(nc)
    for c in range(n_cols):
        col = U[:, c]
        Uc = np.where(r >= 0, col[np.maximum(r, 0)], 0.0)
        up = Uc > theta
        n = up.sum(axis=1)
        order = np.argsort(~up, axis=1, kind='stable')  # above ones first, each group ascending
        Wv = np.take_along_axis(Uc, order, axis=1)
        Q = P[every[:, None], order]
        rec = np.zeros((nc, 2, W))
        with np.errstate(all='ignore'):
            for j in range(d):
                Gj = Uc[:, 0] * g[:, 0, j]
                for a in range(1, d + 1):
                    Gj = Gj + Uc[:, a] * g[:, a, j]
                rec[:, :, d * d + j] = Gj[:, None]
            rec[:, :, d * d + d] = every[:, None].astype(np.float64)

            def cut(sel, a, b):
                s = (Wv[sel, a] - theta) / (Wv[sel, a] - Wv[sel, b])
                return Q[sel, a] + s[:, None] * (Q[sel, b] - Q[sel, a])

            table = ({1: [[(0, 1), (0, 2)]], 2: [[(1, 2), (0, 2)]]} if d == 2 else
                     {1: [[(0, 1), (0, 2), (0, 3)]], 2: [[(0, 2), (0, 3), (1, 2)], [(0, 3), (1, 2), (1, 3)]],
                      3: [[(0, 3), (1, 3), (2, 3)]]})
            for k, pieces in table.items():
                sel = n == k
                if sel.any():
                    for p, piece in enumerate(pieces):
                        for v, (a, b) in enumerate(piece):
                            rec[sel, p, v * d:(v + 1) * d] = cut(sel, a, b)
        k = np.where((n == 0) | (n == d + 1), 0, np.where((n == 2) & (d == 3), 2, 1))
        keep = np.stack([k >= 1, k == 2], axis=1)
        records.append(rec[keep])  # C order: cell ascending, then the piece
        counts[c] = np.bincount(tile_of, weights=k, minlength=n_tiles).astype(np.int64)
    return counts, np.concatenate(records, axis=0)


def numpy_piece_measure(vertices):
    """The twin of source.isotherms.piece_measure."""
    vertices = np.asarray(vertices, dtype=np.float64)
    a = vertices[:, 1] - vertices[:, 0]
    with np.errstate(all='ignore'):
        if vertices.shape[1] == 2:
            return np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])
        b = vertices[:, 2] - vertices[:, 0]
        c0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        c1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        c2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        return np.sqrt((c0 * c0 + c1 * c1) + c2 * c2) / 2.0


def numpy_node_tree_sums(values, offsets):
    """The twin of source.isotherms.node_tree_sums: node by node, a loop over the steps."""
    values, offsets = np.asarray(values, dtype=np.float64), np.asarray(offsets, dtype=np.int64)
    count = np.diff(offsets)
    P = 1
    while P < (count.max() if len(count) else 0):
        P *= 2
    out = np.zeros(len(count))
    for k in range(len(count)):
        x = np.zeros(P)
        x[:count[k]] = values[offsets[k]:offsets[k + 1]]
        s = P // 2
        with np.errstate(all='ignore'):
            while s >= 1:
                x = x[:s] + x[s:2 * s]
                s //= 2
        out[k] = x[0]
    return out


def numpy_dict(records, counts, d, nodes, h):
    """The dict of the public call from the contract's records and counts of the nodes `nodes`."""
    per_node = counts.sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(per_node)]).astype(np.int64)
    vertices = records[:, :d * d].reshape(-1, d, d)
    grad = records[:, d * d:d * d + d]
    measure = numpy_piece_measure(vertices)
    gg = grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]
    if d == 3:
        gg = gg + grad[:, 2] * grad[:, 2]
    return {'nodes': np.asarray(nodes, dtype=np.int64), 'times': np.array([float(k) * h for k in nodes]),
            'offsets': offsets, 'vertices': vertices, 'grad': grad, 'cell': records[:, d * d + d].astype(np.int64),
            'measure': measure, 'measure_at': numpy_node_tree_sums(measure, offsets),
            'flux_at': numpy_node_tree_sums(measure * np.sqrt(gg), offsets)}


class Planted:
    """A mesh with, per threshold, its planted slab values (M, 65) and the contract's counts
    and records of them: computed once, shared by the tests of both files, never changed."""
    def __init__(self, name):
        self.name, self.mesh = name, MESHES[name]()
        self.points = np.asarray(self.mesh.points, dtype=np.float64)
        self.cells = np.asarray(self.mesh.cells, dtype=np.int64)
        self.row_of = row_map(self.mesh)
        self.d, self.M = self.cells.shape[1] - 1, len(free_dofs(self.mesh))
        self.W = width(self.d)
        self.n_tiles = -(-len(self.cells) // BS)
        self._kept = {}

    def contract(self, U, theta):
        return numpy_isotherms(self.points, self.cells, self.row_of, U, theta)

    def values(self, theta):
        U = planted_values(np.random.RandomState(1000 + len(self.cells)), self.M, N_PLANTED,
                           theta if np.isfinite(theta) else 0.3)
        U.setflags(write=False)
        return U

    def reference(self, theta):
        if theta not in self._kept:
            U = self.values(theta)
            counts, records = self.contract(U, theta)
            counts.setflags(write=False), records.setflags(write=False)
            self._kept[theta] = (U, counts, records)
        return self._kept[theta]

    def cell_values(self, col):
        r = self.row_of[self.cells]
        return np.where(r >= 0, col[np.maximum(r, 0)], 0.0)


_planted = {}


def planted(name):
    if name not in _planted:
        _planted[name] = Planted(name)
    return _planted[name]


# ---- 1. against the chord and the section of a linear function --------------------------------------
def box_section(a, c):
    """The length (d = 2) or area (d = 3) of {a . x = c} within the unit box, from the points
    where it meets the box's edges: nothing of the mesh."""
    d = len(a)
    corners = np.array(np.meshgrid(*[[0.0, 1.0]] * d, indexing='ij')).reshape(d, -1).T
    hits = []
    for i, p in enumerate(corners):
        for q in corners[i + 1:]:
            if np.count_nonzero(p != q) == 1:  # an edge of the box
                fp, fq = a @ p - c, a @ q - c
                assert fp != 0.0 and fq != 0.0
                if (fp < 0.0) != (fq < 0.0):
                    hits.append(p + (fp / (fp - fq)) * (q - p))
    hits = np.array(hits)
    if d == 2:
        assert len(hits) == 2
        return float(np.linalg.norm(hits[1] - hits[0]))
    centre = hits.mean(axis=0)
    e1 = hits[0] - centre
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a / np.linalg.norm(a), e1)
    angle = np.arctan2((hits - centre) @ e2, (hits - centre) @ e1)
    ring = hits[np.argsort(angle)]
    area = 0.0
    for i in range(len(ring)):  # a convex polygon as a fan around its centre
        area += 0.5 * np.linalg.norm(np.cross(ring[i] - centre, ring[(i + 1) % len(ring)] - centre))
    return float(area)


@pytest.mark.parametrize('name', ['square2', 'square4', 'cube1', 'cube2'])
def test_isotherm_of_a_linear_function_is_the_chord_or_the_section(name):
    """u = a . x + b on ALL vertices (row_of=None): the pieces tile the chord of the line, or the
    polygon in which the plane cuts the cube.  Tolerance 16 eps n_pieces measure: a piece's
    measure carries a handful of roundings (the cut, the edge vectors, the products, the
    root), and a sum of n non-negative terms adds at most n eps relative."""
    mesh = MESHES[name]()
    p, cells = np.asarray(mesh.points, dtype=np.float64), np.asarray(mesh.cells, dtype=np.int64)
    d = p.shape[1]
    assert np.array_equal(p.min(axis=0), np.zeros(d)) and np.array_equal(p.max(axis=0), np.ones(d))
    a, b = np.array([1.0, 0.37, -0.61][:d]), 0.1
    u = p @ a + b
    for theta in (0.777, 0.3, 1.0 / 3.0, 1.23):
        assert not np.any(u == theta)  # the line or plane meets no mesh vertex
        counts, records = numpy_isotherms(p, cells, None, u[:, None], theta)
        n = len(records)
        assert n == counts.sum() and n > 0
        got = math.fsum(numpy_piece_measure(records[:, :d * d].reshape(-1, d, d)))
        want = box_section(a, theta - b)
        tol = 16.0 * EPS * n * want
        print(name, theta, 'pieces %d, measure %.15g, analytic %.15g, gap %.2e, tolerance %.2e' % (n, got, want, got - want, tol))
        assert abs(got - want) <= tol
        # the gradient of every piece is a, to rounding, and every vertex lies on the level set
        assert np.abs(records[:, d * d:d * d + d] - a).max() <= 1e-12 * 2.0**(2 + int(name[-1]))
        assert np.abs(records[:, :d * d].reshape(-1, d) @ a + b - theta).max() <= 1e-14
        # the tree sum of the pieces is that measure too
        tree = numpy_node_tree_sums(numpy_piece_measure(records[:, :d * d].reshape(-1, d, d)), [0, n])[0]
        assert abs(tree - want) <= tol


# ---- 2. against the zone of the time curves ----------------------------------------------------------
def _pieces_of(n, d):
    return np.where((n == 0) | (n == d + 1), 0, np.where((n == 2) & (d == 3), 2, 1))


@pytest.mark.parametrize('name', sorted(MESHES))
def test_pieces_are_the_faces_of_the_zone(name):
    """Per cell the piece count follows from the zone's n; every isotherm vertex of a node lies
    inside that node's box of the time curves -- >= and <=, no tolerance: the same doubles."""
    case = planted(name)
    d, at = case.d, rows(case.d)
    vol, _ = cell_geometry(case.points, case.cells)
    P = case.points[case.cells]
    for theta in THETAS:
        U, counts, records = case.reference(theta)
        curves = numpy_time_curves(case.points, case.cells, case.row_of, U, theta)
        lo, hi = curves[at['box_lo']], curves[at['box_hi']]  # (d, n_cols)
        per_column = counts.sum(axis=1)
        start = np.concatenate([[0], np.cumsum(per_column)])
        assert start[-1] == len(records)
        for c in range(U.shape[1]):
            _, _, _, _, n = zone_of_cells(case.cell_values(U[:, c]), P, vol, np.float64(theta))
            k = _pieces_of(n, d)
            rec = records[start[c]:start[c + 1]]
            assert np.array_equal(np.bincount(np.arange(len(k)) // BS, weights=k, minlength=case.n_tiles), counts[c])
            assert np.array_equal(rec[:, d * d + d], np.repeat(np.arange(len(k)), k).astype(np.float64))
            if len(rec):
                X = rec[:, :d * d].reshape(-1, d)
                assert not np.isnan(X).any()
                assert np.all(X >= lo[:, c]) and np.all(X <= hi[:, c]), (name, theta, c)
            else:
                assert np.all(n == 0) or np.all((n == 0) | (n == d + 1))


def _classes(case, theta):
    U, counts, _ = case.reference(theta)
    seen = set()
    for c in range(U.shape[1]):
        seen.update(np.unique((case.cell_values(U[:, c]) > theta).sum(axis=1)).tolist())
    return seen, counts.sum(axis=1)


def test_the_planted_cases_occur():
    """What the other tests rest on, so that a change of the helpers cannot hollow them out."""
    for name in WHOLE:
        case = planted(name)
        for theta in THETAS:
            seen, per_column = _classes(case, theta)
            assert set(range(1, case.d + 1)) <= seen, (name, theta, seen)  # every class n = 1 .. d
            print(name, theta, 'pieces per column %d .. %d' % (per_column.min(), per_column.max()))
    span = lambda name: (lambda per_column: (per_column.min(), per_column.max()))(_classes(planted(name), 0.3)[1])
    assert span('square1') == (6, 26) and span('cube2') == (2116, 3248)
    # an empty node in the middle of the offsets
    empty = np.nonzero(_classes(planted('square1'), 1.0)[1] == 0)[0]
    assert len(empty) == 3 and 0 < empty.min() and empty.max() < N_PLANTED - 1
    # one free dof: a cell has at most one vertex above, and most columns have no piece
    small = planted('square0')
    assert len(small.cells) == 8 and small.M == 1
    assert sorted(int((_classes(small, theta)[1] == 0).sum()) for theta in THETAS) == [41, 49]
    for theta in THETAS:
        assert _classes(small, theta)[0] <= {0, 1}


@pytest.mark.parametrize('name', ['square2', 'cube1'])
def test_a_vertex_at_the_threshold_is_not_above_and_ends_the_piece(name):
    """theta = 1.0: the columns c % 4 == 1 hold integers, many exactly AT theta.  Such a vertex is
    not above; the cut on an edge that ends in it has s == 1.0 and is that vertex (exactly, on
    these meshes of dyadic coordinates), so the cell's pieces have it as a vertex."""
    case = planted(name)
    d, theta = case.d, 1.0
    U, counts, records = case.reference(theta)
    start = np.concatenate([[0], np.cumsum(counts.sum(axis=1))])
    met = 0
    for c in range(1, N_PLANTED, 4):
        Uc = case.cell_values(U[:, c])
        assert np.count_nonzero(U[:, c] == theta) > case.M // 6
        rec = records[start[c]:start[c + 1]]
        cell = rec[:, d * d + d].astype(np.int64)
        n = (Uc > theta).sum(axis=1)
        assert np.array_equal(np.unique(cell), np.nonzero((n > 0) & (n < d + 1))[0])
        # the same pieces as with a threshold a little higher would have, one by one
        higher, _ = case.contract(U[:, c:c + 1], np.nextafter(theta, 2.0))
        assert np.array_equal(higher[0], counts[c])
        for t in np.unique(cell):
            X = rec[cell == t][:, :d * d].reshape(-1, d)
            for b in np.nonzero(Uc[t] == theta)[0]:
                assert (X == case.points[case.cells[t, b]]).all(axis=1).any(), (c, t, b)
                met += 1
    assert met > 20


def test_infinite_thresholds_give_no_piece():
    case = planted('cube1')
    U = case.values(0.3)[:, :3].copy()
    U[0, 1] = np.nan
    for theta in (np.inf, -np.inf):
        counts, records = case.contract(U, theta)
        assert counts.shape == (3, case.n_tiles) and not counts.any() and records.shape == (0, case.W)


# ---- 3. the measures and the tree sums of source/isotherms.py --------------------------------------
@pytest.mark.parametrize('name', ['square1', 'lshape_jitter3', 'cube2'])
def test_measures_and_tree_sums_are_their_numpy_twins(name):
    case = planted(name)
    d = case.d
    U, counts, records = case.reference(1.0)
    per_node = counts.sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(per_node)]).astype(np.int64)
    vertices = records[:, :d * d].reshape(-1, d, d)
    measure = numpy_piece_measure(vertices)
    got = piece_measure(torch.from_numpy(vertices.copy())).numpy()
    assert got.shape == (len(records),) and same(got, measure) and np.all(measure >= 0.0)
    sums = node_tree_sums(torch.from_numpy(measure), torch.from_numpy(offsets)).numpy()
    want = numpy_node_tree_sums(measure, offsets)
    assert same(sums, want)
    if name == 'square1':
        assert np.count_nonzero(per_node == 0) == 3 and np.all(want[per_node == 0] == 0.0)  # empty nodes
    for k in (0, 7, 33):
        assert abs(want[k] - math.fsum(measure[offsets[k]:offsets[k + 1]])) <= EPS * max(per_node[k], 1) * want[k]
    # a node's sum does not depend on the nodes it is asked with
    pick = [0, 3, 4, N_PLANTED - 1]
    part = np.concatenate([measure[offsets[k]:offsets[k + 1]] for k in pick])
    part_offsets = np.concatenate([[0], np.cumsum(per_node[pick])])
    assert same(node_tree_sums(torch.from_numpy(part), torch.from_numpy(part_offsets)).numpy(), want[pick])


def test_tree_sums_of_nothing_and_of_special_values():
    none = node_tree_sums(torch.zeros(0, dtype=torch.float64), torch.zeros(4, dtype=torch.int64))
    assert none.shape == (3,) and none.dtype == torch.float64 and bool((none == 0.0).all())
    assert same(numpy_node_tree_sums(np.zeros(0), np.zeros(4, dtype=np.int64)), np.zeros(3))
    values = np.array([1.0, np.nan, 2.0, np.inf, 3.0, 0.5, 0.25, 0.125, 1e-300])
    offsets = np.array([0, 1, 1, 3, 4, 9])
    got = node_tree_sums(torch.from_numpy(values), torch.from_numpy(offsets)).numpy()
    assert same(got, numpy_node_tree_sums(values, offsets))
    assert got[0] == 1.0 and got[1] == 0.0 and np.isnan(got[2]) and got[3] == np.inf
    assert got[4] == ((3.0 + 1e-300) + 0.25) + (0.5 + 0.125)  # P = 8: x[i] + x[i + 4], then + 2, then + 1
    flat = np.zeros((2, 2, 2))
    assert same(piece_measure(torch.from_numpy(flat)).numpy(), np.zeros(2))


# ---- 4. argument checks that need no device ----------------------------------------------------------
def test_check_arguments():
    assert check_arguments(0.5, None, 5) == (0.5, [0, 1, 2, 3, 4], 2**30)
    assert check_arguments(1, [0, 3, 4], 5, 0) == (1.0, [0, 3, 4], 0)
    assert check_arguments(-np.inf, np.array([2]), 5, 10.5) == (-np.inf, [2], 10.5)
    assert check_arguments(np.inf, (np.int64(0), 4), 5)[1] == [0, 4]
    assert width(2) == 7 and width(3) == 13
    for bad, text in ((dict(threshold=None), r'isotherms\(\) needs a threshold'),
                      (dict(threshold=float('nan')), 'threshold is NaN'),
                      (dict(threshold='hot'), 'must be a number'),
                      (dict(threshold=[0.1, 0.2]), 'must be a number'),  # one threshold per call
                      (dict(nodes=[]), 'names no time node'),
                      (dict(nodes=[0, 5]), r'nodes\[1\] = 5 is not in \[0, 5\)'),
                      (dict(nodes=[-1, 2]), r'nodes\[0\] = -1 is not in'),
                      (dict(nodes=[1, 1]), 'strictly ascending'),
                      (dict(nodes=[3, 2]), 'strictly ascending'),
                      (dict(nodes=[0.5]), 'None or ints'),
                      (dict(nodes=3), 'None or ints'),
                      (dict(max_bytes=-1), 'max_bytes'),
                      (dict(max_bytes=None), 'max_bytes'),
                      (dict(max_bytes=float('nan')), 'max_bytes')):
        a = dict(dict(threshold=0.5, nodes=None, N=5, max_bytes=2**30), **bad)
        with pytest.raises(ValueError, match=text):
            check_arguments(a['threshold'], a['nodes'], a['N'], a['max_bytes'])


class _Recorder(PostProcessing):
    """A driver of nothing but its hooks, which record that they ran."""
    def __init__(self, mesh, mesh_time):
        self._init_postprocessing(mesh, mesh_time, {})
        self.ran = []

    def _trial_vector(self, u, who):
        self.ran.append(('_trial_vector', who))
        return u

    def _adjoint_target(self, out):
        self.ran.append(('_adjoint_target',))
        return None, out


REFUSED = {
    'no threshold': (lambda h, u: h.isotherms(u, None), 'needs a threshold'),
    'NaN threshold': (lambda h, u: h.isotherms(u, float('nan')), 'threshold is NaN'),
    'a node beyond the last': (lambda h, u: h.isotherms(u, 0.5, nodes=[0, 3]), r'nodes\[1\] = 3'),
    'nodes not ascending': (lambda h, u: h.isotherms(u, 0.5, nodes=[1, 0]), 'strictly ascending'),
    'negative max_bytes': (lambda h, u: h.isotherms(u, 0.5, max_bytes=-8), 'max_bytes'),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_a_refused_argument_runs_no_hook_and_builds_no_plan(case):
    """For both drivers at once: the ValueError comes before `u` is looked at (the serial
    driver would upload it there) and before the plan is built."""
    mesh, _, mesh_time = problem_helper('square', J_space=0, J_time=1)[:3]
    assert mesh_time.nv == 3
    call, text = REFUSED[case]
    heat = _Recorder(mesh, mesh_time)
    with pytest.raises(ValueError, match=text):
        call(heat, 'no vector at all')
    assert heat.ran == [] and heat.curves_plan is None


def test_the_library_says_the_width_and_refuses_a_bad_chunk():
    """Host only: neither call touches a GPU."""
    from source import _lib
    lib = _lib.lib()
    assert lib.stk_iso_width(2) == 7 == width(2) and lib.stk_iso_width(3) == 13 == width(3)
    assert lib.stk_iso_width(1) == 0 and lib.stk_iso_width(4) == 0
    for bad in (-1, 33):
        assert lib.stk_iso_tile(bad) != 0 and 'stk_iso_tile: cols = %d' % bad in lib.stk_last_error().decode()
    assert lib.stk_iso_tile(32) == 0 and lib.stk_iso_tile(0) == 0
