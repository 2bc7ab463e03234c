"""The contract of the solidification maps (include/stk.h "solidification maps",
source/solidification.py) as a plain NumPy loop over the columns -- the oracle of
tests/test_solidification_gpu.py, which compares the device against it with array_equal --
checked here against a dense evaluation that knows nothing of the carried state; the host
routines stk_solid_tile_rows against np.unique per tile and stk_solid_cell_order against a
NumPy sort of the same keys; and the argument checks of the public call that need no device.

THE DATA.  `dyadic_values`: nodal values that are integer multiples of 2^-6 in [-1, 2].  On
the uniform meshes grad lambda has entries 0 and +-2^J, so every sum U_0 + U_1 + ... and every
product U_a g_aj, every G_j, G_j G_j and Q is exact in any order, and the loop and the dense
evaluation must agree with array_equal.  The threshold 0.3 has (d + 1) theta = 0.9 or 1.2, no
multiple of 2^-6, so no mean is AT it and no comparison can tie.

THE TOLERANCE on lshape_jitter3, where grad lambda is no dyadic number.  The mean does not
involve the geometry: the crossings, x, t_solid, cooling_rate, n_solid and last_mean stay
exactly equal.  G_j is a sum of d + 1 products, each rounded once, added in d steps: either
evaluation is within (d + 1) u S of the exact sum, u = 2^-53 and S = sum_a |U_a| |g_aj| <= S_max =
2 (d + 1) max|g| (|U| <= 2), so the two differ by at most tol_G = 2 (d + 1) u S_max.
grad_solid = L + x (G - L), x in (0, 1], takes one difference, one product and one sum more,
each rounded to within u of a number of size <= 2 S_max, on operands off by tol_G: at most
3 tol_G + 6 u S_max <= tol_grad = 4 tol_G (as d + 1 >= 3).  Q is d squares of numbers of size <=
S_max that are off by tol_G, plus d roundings of the squares and d - 1 of the sums, each u d
S_max^2 at most: |dQ| <= 2 d S_max tol_G + 2 d^2 u S_max^2 <= tol_Q = 4 d S_max tol_G.
t_max_grad may then name another node where two nodes' Q lie within 2 tol_Q: the test asks
that the loop's node has a dense Q within 2 tol_Q of the dense maximum.  Every test prints its
gaps."""
import types

import numpy as np
import pytest

from source.solidification import FIELDS, NO_ROW, TILE_CELLS, cell_order, check_arguments, n_rows, rows, tile_rows
from test_history_host import same
from test_time_curves_host import HOST_MESHES, _mesh, cell_geometry, first_cells, row_map

THETA = 0.3
N_MAX = 130
U53 = 2.0**-53


# ---- the contract ---------------------------------------------------------------------------------
def cell_tables(mesh):
    """(grad lambda (nc, d + 1, d), rows (nc, d + 1)): the doubles of csrc/p1_mesh.h and the
    slab row of every cell's vertices, -1 on the boundary."""
    cells = np.asarray(mesh.cells, dtype=np.int64)
    _, grad = cell_geometry(mesh.points, cells)
    return grad, row_map(mesh)[cells]


def _cell_column(grad, cell_rows, column):
    """(m (nc,), G [d] of (nc,), Q (nc,)) at one node: every operation one NumPy operation."""
    nl = cell_rows.shape[1]
    d = nl - 1
    U = [np.where(cell_rows[:, a] >= 0, column[np.maximum(cell_rows[:, a], 0)], 0.0) for a in range(nl)]
    s = U[0] + U[1]
    for a in range(2, nl):
        s = s + U[a]
    m = s / float(d + 1)
    G = []
    for j in range(d):
        x = U[0] * grad[:, 0, j] + U[1] * grad[:, 1, j]
        for a in range(2, nl):
            x = x + U[a] * grad[:, a, j]
        G.append(x)
    Q = G[0] * G[0] + G[1] * G[1]
    if d == 3:
        Q = Q + G[2] * G[2]
    return m, G, Q


def numpy_solid_scan(grad, cell_rows, U, k_first, h, theta, state=None):
    """The state (6 + 2 d, nc) after the columns of U (M, n_cols) -- column c the node k_first
    + c --: include/stk.h's loop, one column at a time.  state=None: fresh; else the carried
    state, which is not changed."""
    nc, nl = cell_rows.shape
    d = nl - 1
    at = rows(d)
    U = np.asarray(U, dtype=np.float64)
    assert state is not None or U.shape[1] >= 1
    s = None if state is None else np.array(state, dtype=np.float64)
    with np.errstate(all='ignore'):
        for c in range(U.shape[1]):
            k = k_first + c
            m, G, Q = _cell_column(grad, cell_rows, U[:, c])
            if s is None:
                s = np.empty((n_rows(d), nc))
                s[at['t_solid']] = s[at['cooling_rate']] = np.nan
                s[at['grad_solid']] = np.nan
                s[at['n_solid']] = 0.0
                s[at['max_grad_sq']] = Q
                s[at['t_max_grad']] = float(k) * h
            else:
                higher = Q > s[at['max_grad_sq']]
                s[at['max_grad_sq']] = np.where(higher, Q, s[at['max_grad_sq']])
                s[at['t_max_grad']] = np.where(higher, float(k) * h, s[at['t_max_grad']])
                a, b = s[at['last_mean']].copy(), m
                down = (a > theta) & (b <= theta)
                x = (theta - a) / (b - a)
                s[at['t_solid']] = np.where(down, (float(k - 1) + x) * h, s[at['t_solid']])
                s[at['cooling_rate']] = np.where(down, (a - b) / h, s[at['cooling_rate']])
                for j in range(d):
                    last = s[6 + d + j]
                    s[6 + j] = np.where(down, last + x * (G[j] - last), s[6 + j])
                s[at['n_solid']] = np.where(down, s[at['n_solid']] + 1.0, s[at['n_solid']])
            s[at['last_mean']] = m
            for j in range(d):
                s[6 + d + j] = G[j]
    return s


def dense_solid(grad, cell_rows, U, h, theta):
    """The same state of the nodes 0 .. N - 1 with no carried state: dense (nc, N) means and
    (nc, d, N) gradients, the last crossing by index search, the count by a sum of masks."""
    nc, nl = cell_rows.shape
    d, N = nl - 1, U.shape[1]
    V = np.where((cell_rows >= 0)[:, :, None], U[np.maximum(cell_rows, 0)], 0.0)  # (nc, d + 1, N)
    m = V.sum(axis=1) / float(d + 1)
    G = np.einsum('tan,taj->tjn', V, grad)
    Q = (G * G).sum(axis=1)
    s = np.full((n_rows(d), nc), np.nan)
    at = rows(d)
    s[at['last_mean']], s[at['last_grad']] = m[:, -1], G[:, :, -1].T
    s[at['max_grad_sq']], s[at['t_max_grad']] = Q.max(axis=1), Q.argmax(axis=1).astype(np.float64) * h
    down = (m[:, :-1] > theta) & (m[:, 1:] <= theta)  # element e = the columns e, e + 1
    s[at['n_solid']] = down.sum(axis=1)
    t = np.nonzero(down.any(axis=1))[0]
    if len(t):
        e = N - 2 - down[t, ::-1].argmax(axis=1)
        a, b = m[t, e], m[t, e + 1]
        x = (theta - a) / (b - a)
        s[at['t_solid'], t] = (e.astype(np.float64) + x) * h
        s[at['cooling_rate'], t] = (a - b) / h
        s[6:6 + d, t] = (G[t, :, e] + x[:, None] * (G[t, :, e + 1] - G[t, :, e])).T
    return s, Q


# ---- the data -------------------------------------------------------------------------------------
def dyadic_values(mesh, n=N_MAX, seed=0):
    """(M, n) integer multiples of 2^-6 in [-1, 2].  Rows of vertices in the first fifth of the mesh along x_0
    stay in [-1, 0] (cells of nothing else never get above 0.3); the others hold a value for a few
    nodes (a run of 1 to 6) before they draw the next, so cells cross 0.3 a few times, not at
    every node."""
    from source.assembly import free_dofs
    rng = np.random.RandomState(7000 + seed + len(mesh.cells))
    fd = np.asarray(free_dofs(mesh), dtype=np.int64)
    M = len(fd)
    draws = rng.randint(-64, 129, size=(M, n))
    keep = rng.randint(1, 7, size=(M, 1))
    index = (np.arange(n)[None, :] // keep) * keep  # the node whose draw a node repeats
    U = np.take_along_axis(draws, index, axis=1) / 64.0
    x0 = np.asarray(mesh.points, dtype=np.float64)[:, 0]
    cold = x0[fd] < x0.min() + 0.2 * (x0.max() - x0.min())
    U[cold] = rng.randint(-64, 1, size=(int(cold.sum()), n)) / 64.0
    assert U.min() >= -1.0 and U.max() <= 2.0 and np.array_equal(U * 64.0, np.round(U * 64.0))
    return U


def _time_step(n):
    return 1.0 / float(max(n - 1, 1))


UNIFORM = ('square2', 'square3', 'square4', 'cube1', 'cube2')


# ---- the loop against the dense evaluation ---------------------------------------------------------
@pytest.mark.parametrize('name', UNIFORM)
def test_loop_equals_the_dense_evaluation_on_uniform_meshes(name):
    mesh = HOST_MESHES[name]()
    grad, cell_rows = cell_tables(mesh)
    assert np.array_equal(np.abs(grad), np.abs(grad).max() * (grad != 0.0))  # 0 and +-2^J
    U = dyadic_values(mesh)
    for n in (1, 2, 9, N_MAX):
        h = _time_step(n) if n > 2 else 0.37
        got = numpy_solid_scan(grad, cell_rows, U[:, :n], 0, h, THETA)
        want, _ = dense_solid(grad, cell_rows, U[:, :n], h, THETA)
        assert got.shape == (n_rows(grad.shape[2]), len(cell_rows))
        for q in range(len(want)):
            assert same(got[q], want[q]), (name, n, q)


def test_loop_equals_the_dense_evaluation_within_the_derived_tolerance_on_the_jittered_mesh():
    mesh = HOST_MESHES['lshape_jitter3']()
    grad, cell_rows = cell_tables(mesh)
    d = grad.shape[2]
    at = rows(d)
    U = dyadic_values(mesh)
    h = _time_step(N_MAX)
    got = numpy_solid_scan(grad, cell_rows, U, 0, h, THETA)
    want, Q = dense_solid(grad, cell_rows, U, h, THETA)
    tol_G, tol_grad, tol_Q = jitter_tolerances(grad)
    for key in ('t_solid', 'cooling_rate', 'n_solid', 'last_mean'):  # the geometry takes no part
        assert same(got[at[key]], want[at[key]]), key
    gaps = {'last_grad': (np.abs(got[at['last_grad']] - want[at['last_grad']]).max(), tol_G),
            'grad_solid': (np.nanmax(np.abs(got[at['grad_solid']] - want[at['grad_solid']])), tol_grad),
            'max_grad_sq': (np.abs(got[at['max_grad_sq']] - want[at['max_grad_sq']]).max(), tol_Q)}
    k = np.rint(got[at['t_max_grad']] / h).astype(np.int64)
    assert same(k.astype(np.float64) * h, got[at['t_max_grad']])
    gaps['Q at the loop\'s node'] = ((Q.max(axis=1) - Q[np.arange(len(k)), k]).max(), 2.0 * tol_Q)
    for key, (gap, tol) in gaps.items():
        print('lshape_jitter3 %s: loop against dense %.3e (tolerance %.3e)' % (key, gap, tol))
        assert gap <= tol, key
    assert same(np.isnan(got[at['grad_solid']]), np.isnan(want[at['grad_solid']]))


def jitter_tolerances(grad):
    """(tol_G, tol_grad, tol_Q) of the module docstring for |U| <= 2."""
    nl, d = grad.shape[1], grad.shape[2]
    S_max = 2.0 * nl * np.abs(grad).max()
    tol_G = 2.0 * nl * U53 * S_max
    return tol_G, 4.0 * tol_G, 4.0 * d * S_max * tol_G


@pytest.mark.parametrize('name', ['square3', 'square4', 'cube2', 'lshape_jitter3'])
def test_the_data_does_its_job(name):
    """The seeds are checked here, on the CPU, before the GPU tests rely on them."""
    mesh = HOST_MESHES[name]()
    grad, cell_rows = cell_tables(mesh)
    at = rows(grad.shape[2])
    U = dyadic_values(mesh)
    s = numpy_solid_scan(grad, cell_rows, U, 0, _time_step(N_MAX), THETA)
    n = s[at['n_solid']]
    first, _, _ = _cell_column(grad, cell_rows, U[:, 0])
    print('%s: %d cells, %d with a crossing, %d with two or more, %d above at node 0, %d never' %
          (name, len(n), (n >= 1).sum(), (n >= 2).sum(), (first > THETA).sum(), (n == 0).sum()))
    assert (n >= 1).sum() * 4 >= len(n) and (n >= 2).any() and (first > THETA).any() and (n == 0).any()
    assert same(np.isnan(s[at['t_solid']]), n == 0) and same(np.isnan(s[at['grad_solid']]).any(axis=0), n == 0)
    # no mean is AT the threshold, none within 2^-11 of it: no comparison can tie
    for c in range(N_MAX):
        m, _, _ = _cell_column(grad, cell_rows, U[:, c])
        assert np.abs(m - THETA).min() > 2.0**-11


@pytest.mark.parametrize('name', ['square2', 'cube1', 'lshape_jitter3'])
def test_cutting_the_columns_anywhere_reproduces_the_one_shot_doubles(name):
    mesh = HOST_MESHES[name]()
    grad, cell_rows = cell_tables(mesh)
    n, h = 12, 0.1
    U = dyadic_values(mesh, n)
    whole = numpy_solid_scan(grad, cell_rows, U, 0, h, THETA)
    for cut in range(1, n):
        head = numpy_solid_scan(grad, cell_rows, U[:, :cut], 0, h, THETA)
        kept = head.copy()
        both = numpy_solid_scan(grad, cell_rows, U[:, cut:], cut, h, THETA, state=head)
        assert same(both, whole), cut
        assert same(head, kept)  # the carried state is not changed
    # no column and a carried state: the state
    assert same(numpy_solid_scan(grad, cell_rows, U[:, :0], n, h, THETA, state=whole), whole)
    # three pieces
    s = numpy_solid_scan(grad, cell_rows, U[:, :3], 0, h, THETA)
    s = numpy_solid_scan(grad, cell_rows, U[:, 3:4], 3, h, THETA, state=s)
    assert same(numpy_solid_scan(grad, cell_rows, U[:, 4:], 4, h, THETA, state=s), whole)


# ---- ties ------------------------------------------------------------------------------------------
def _one_cell():
    """One triangle (0, 0), (1, 0), (0, 1) whose three vertices are the slab rows 0, 1, 2."""
    cells = np.array([[0, 1, 2]], dtype=np.int64)
    _, grad = cell_geometry(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), cells)
    return grad, cells.copy()


def test_a_mean_at_the_threshold():
    grad, cell_rows = _one_cell()
    at = rows(2)
    # three equal vertex values v: the mean is ((v + v) + v) / 3 = v exactly for these
    means = np.array([1.0, 0.5, 0.25, 1.0, 0.75])
    U = np.repeat(means[None, :], 3, axis=0)
    s = numpy_solid_scan(grad, cell_rows, U[:, :2], 0, 0.25, 0.5)
    # going down TO the threshold counts, with x == 1.0: the crossing sits at the node
    assert s[at['n_solid'], 0] == 1.0 and s[at['t_solid'], 0] == 0.25 and s[at['cooling_rate'], 0] == 2.0
    # AT the threshold as `a` starts no crossing: 0.5 -> 0.25 changes nothing
    s3 = numpy_solid_scan(grad, cell_rows, U[:, :3], 0, 0.25, 0.5)
    assert same(s3[:5], s[:5]) and s3[at['last_mean'], 0] == 0.25
    # and a later crossing replaces the earlier one: 1.0 -> 0.75 is none, though
    s5 = numpy_solid_scan(grad, cell_rows, U, 0, 0.25, 0.5)
    assert s5[at['n_solid'], 0] == 1.0 and s5[at['t_solid'], 0] == 0.25
    # a constant field has no gradient: Q == 0 at every node, the earliest node keeps the maximum
    assert s5[at['max_grad_sq'], 0] == 0.0 and s5[at['t_max_grad'], 0] == 0.0
    assert same(s5[at['grad_solid'], 0], np.zeros(2))


def test_the_earliest_node_wins_the_largest_gradient():
    grad, cell_rows = _one_cell()
    at = rows(2)
    U = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 2.0, -2.0], [0.0, 0.0, 0.0, 0.0]])  # G = (U_1, 0)
    s = numpy_solid_scan(grad, cell_rows, U, 3, 0.5, 10.0)
    assert s[at['max_grad_sq'], 0] == 4.0 and s[at['t_max_grad'], 0] == 4 * 0.5  # node 4, not 5 or 6
    assert s[at['n_solid'], 0] == 0.0 and np.isnan(s[at['t_solid'], 0])


def test_a_nan_makes_no_crossing_and_leaves_the_largest_gradient():
    grad, cell_rows = _one_cell()
    at = rows(2)
    U = np.array([[2.0, np.nan, -1.0, 2.0, -1.0], [2.0, 2.0, -1.0, 2.0, -1.0], [2.0, 2.0, -1.0, 2.0, -1.0]])
    s = numpy_solid_scan(grad, cell_rows, U[:, :3], 0, 1.0, 0.5)
    # 2 -> NaN and NaN -> -1 are no crossings; Q of the NaN column is NaN and replaces nothing
    assert s[at['n_solid'], 0] == 0.0 and np.isnan(s[at['t_solid'], 0])
    assert s[at['max_grad_sq'], 0] == 0.0 and s[at['t_max_grad'], 0] == 0.0
    s = numpy_solid_scan(grad, cell_rows, U, 0, 1.0, 0.5)
    assert s[at['n_solid'], 0] == 1.0 and s[at['t_solid'], 0] == 3.5 and s[at['cooling_rate'], 0] == 3.0
    # a NaN in the FIRST column stays in max_grad_sq: nothing is greater than NaN
    s = numpy_solid_scan(grad, cell_rows, U[:, 1:], 0, 1.0, 0.5)
    assert np.isnan(s[at['max_grad_sq'], 0]) and s[at['t_max_grad'], 0] == 0.0 and s[at['n_solid'], 0] == 1.0


def test_infinite_thresholds():
    mesh = HOST_MESHES['square2']()
    grad, cell_rows = cell_tables(mesh)
    at = rows(2)
    U = dyadic_values(mesh, 9)
    up = numpy_solid_scan(grad, cell_rows, U, 0, 0.125, np.inf)
    down = numpy_solid_scan(grad, cell_rows, U, 0, 0.125, -np.inf)
    for s in (up, down):  # nothing is above +inf, nothing finite is at or below -inf
        assert np.all(s[at['n_solid']] == 0.0) and np.isnan(s[at['t_solid']]).all()
    assert same(up, down)


# ---- the host routine of the library -----------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(HOST_MESHES) + ['first1', 'first255', 'first256', 'first257', 'first513'])
def test_tile_rows_routine_against_np_unique(name):
    mesh = first_cells(_mesh('square', 4), int(name[5:])) if name.startswith('first') else HOST_MESHES[name]()
    cells = np.asarray(mesh.cells, dtype=np.int64)
    row_of = row_map(mesh)
    ptr, listed, pos = tile_rows(cells, row_of)
    n_tiles = -(-len(cells) // TILE_CELLS)
    assert ptr.dtype == np.int32 and listed.dtype == np.int32 and pos.dtype == np.uint16
    assert ptr.shape == (n_tiles + 1,) and ptr[0] == 0 and pos.shape == cells.shape
    cell_rows = row_of[cells]
    for i in range(n_tiles):
        mine = cell_rows[TILE_CELLS * i:TILE_CELLS * (i + 1)]
        want = np.unique(mine[mine >= 0])
        got = listed[ptr[i]:ptr[i + 1]]
        assert np.array_equal(got, want), (name, i)
        p = pos[TILE_CELLS * i:TILE_CELLS * (i + 1)]
        assert np.array_equal(p == NO_ROW, mine < 0)
        assert np.array_equal(got[p[mine >= 0]], mine[mine >= 0])
    assert ptr[-1] == len(listed)


def test_tile_rows_routine_refuses():
    from source import _lib
    lib = _lib.lib()
    cells = np.array([[0, 1, 2]], dtype=np.int64)
    row_of = np.array([0, -1, 1], dtype=np.int32)
    ptr, listed, pos = np.full(2, 77, dtype=np.int32), np.full(3, 77, dtype=np.int32), np.full((1, 3), 77, dtype=np.uint16)
    good = [2, 3, 1, cells.ctypes.data, row_of.ctypes.data, ptr.ctypes.data, listed.ctypes.data, pos.ctypes.data]
    bad_cells = np.array([[0, 3, 2]], dtype=np.int64)
    bad_rows = np.array([0, -2, 1], dtype=np.int32)
    for place, value, text in ((0, 4, 'd = 4'), (1, 0, 'nv = 0'), (2, 0, 'nc = 0'), (3, None, 'cells is null'),
                               (4, None, 'row_of is null'), (5, None, 'tile_ptr is null'), (6, None, 'tile_rows is null'),
                               (7, None, 'cell_pos is null'), (3, bad_cells.ctypes.data, 'vertex 3'),
                               (4, bad_rows.ctypes.data, 'row_of[1] = -2')):
        args = list(good)
        args[place] = value
        assert lib.stk_solid_tile_rows(*args) != 0 and text in lib.stk_last_error().decode(), text
    assert np.all(ptr == 77) and np.all(listed == 77) and np.all(pos == 77)
    assert lib.stk_solid_tile_rows(*good) == 0
    assert ptr.tolist() == [0, 2] and listed[:2].tolist() == [0, 1] and pos.tolist() == [[0, NO_ROW, 1]]
    assert lib.stk_solid_rows(2) == 10 == n_rows(2) and lib.stk_solid_rows(3) == 12 == n_rows(3)
    assert lib.stk_solid_rows(4) == 0


def numpy_cell_order(points, cells):
    """The order of include/stk.h: the centroid's 16 bits per axis over the box of all points,
    interleaved with axis 0 lowest, sorted by (key, cell)."""
    p, cells = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    d = p.shape[1]
    key = np.zeros(len(cells), dtype=np.uint64)
    for j in range(d):
        x = p[cells[:, 0], j] + p[cells[:, 1], j]
        for a in range(2, d + 1):
            x = x + p[cells[:, a], j]
        x = x / float(d + 1)
        lo, hi = p[:, j].min(), p[:, j].max()
        q = np.clip((x - lo) / (hi - lo) * 65535.0, 0.0, 65535.0).astype(np.uint64) if hi > lo else np.zeros(len(cells), np.uint64)
        for b in range(16):
            key |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(d * b + j)
    return np.lexsort((np.arange(len(cells)), key)).astype(np.int32)


@pytest.mark.parametrize('name', sorted(HOST_MESHES) + ['first257'])
def test_cell_order_routine_against_a_numpy_sort(name):
    mesh = first_cells(_mesh('square', 4), 257) if name == 'first257' else HOST_MESHES[name]()
    cells = np.asarray(mesh.cells, dtype=np.int64)
    order = cell_order(mesh)
    assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(len(cells)))
    assert np.array_equal(order, numpy_cell_order(mesh.points, cells))
    assert np.array_equal(cell_order(mesh), order)  # the same on every run
    # what it is for: the tiles of the ordered cells touch fewer distinct rows
    row_of = row_map(mesh)
    listed = [len(tile_rows(c, row_of)[1]) for c in (cells, cells[order])]
    print('%s: %d rows listed over the tiles in the caller\'s order, %d along the Z-curve' % (name, listed[0], listed[1]))
    if len(cells) >= 4 * TILE_CELLS:
        assert 2 * listed[1] < listed[0]


def test_cell_order_routine_refuses():
    from source import _lib
    lib = _lib.lib()
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    cells = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int64)
    order = np.full(2, 77, dtype=np.int32)
    good = [2, 4, 2, pts.ctypes.data, cells.ctypes.data, order.ctypes.data]
    bad = np.array([[0, 1, 2], [1, 4, 2]], dtype=np.int64)
    for place, value, text in ((0, 4, 'bad arguments'), (2, 0, 'bad arguments'), (3, None, 'bad arguments'),
                               (4, bad.ctypes.data, 'vertex 4'), (5, None, 'order is null')):
        args = list(good)
        args[place] = value
        assert lib.stk_solid_cell_order(*args) != 0 and text in lib.stk_last_error().decode(), text
    assert np.all(order == 77)
    assert lib.stk_solid_cell_order(*good) == 0 and order.tolist() == [0, 1]
    for value in (-1, 2):
        assert lib.stk_solid_order(value) != 0 and 'caller_order = %d' % value in lib.stk_last_error().decode()
    assert lib.stk_solid_order(1) == 0 and lib.stk_solid_order(0) == 0


def test_tile_setting_refuses_values_out_of_range():
    from source import _lib
    lib = _lib.lib()
    for cols, kib, text in ((-1, 0, 'cols = -1'), (129, 0, 'cols = 129'), (0, -1, 'lds_kib = -1'), (0, 65, 'lds_kib = 65')):
        assert lib.stk_solid_tile(cols, kib) != 0 and text in lib.stk_last_error().decode(), text
    assert lib.stk_solid_tile(128, 64) == 0 and lib.stk_solid_tile(0, 0) == 0


# ---- argument checks that need no device ------------------------------------------------------------------
def test_check_arguments():
    assert check_arguments(0.5) == (0.5, FIELDS) and check_arguments(1) == (1.0, FIELDS)
    assert check_arguments(-np.inf) == (-np.inf, FIELDS) and check_arguments(np.inf) == (np.inf, FIELDS)
    assert len(FIELDS) == 8
    with pytest.raises(ValueError, match='needs a threshold'):
        check_arguments(None)
    with pytest.raises(ValueError, match='threshold is NaN'):
        check_arguments(float('nan'))
    with pytest.raises(ValueError, match='must be a number'):
        check_arguments([0.1, 0.2])  # one threshold per call
    with pytest.raises(ValueError, match=r'points of shape \(5, 3\)'):
        check_arguments(0.5, np.zeros((5, 3)), 2)
    with pytest.raises(ValueError, match=r'points of shape \(5,\)'):
        check_arguments(0.5, np.zeros(5), 2)
    assert check_arguments(0.5, np.zeros((5, 2)), 2) == (0.5, FIELDS)
    assert check_arguments(0.5, types.SimpleNamespace(n_p=4), 2) == (0.5, FIELDS)  # located points carry no shape
    with pytest.raises(ValueError, match='fields must name'):
        check_arguments(0.5, fields=('t_solid', 'peak'))
    assert check_arguments(0.5, fields='G') == (0.5, ('G',))
    assert check_arguments(0.5, fields=['front_speed', 'n_solid']) == (0.5, ('front_speed', 'n_solid'))


def test_the_public_call_checks_before_it_touches_anything():
    """source.solidification.solidification_maps is the body of both drivers' call; with a heat
    of a mesh and nothing else it can only get as far as the checks."""
    from source.solidification import solidification_maps
    heat = types.SimpleNamespace(_sample_meshes=(HOST_MESHES['square2'](), None))
    with pytest.raises(ValueError, match='needs a threshold'):
        solidification_maps(heat, None, None)
    with pytest.raises(ValueError, match='threshold is NaN'):
        solidification_maps(heat, None, float('nan'))
    with pytest.raises(ValueError, match='points of shape'):
        solidification_maps(heat, None, 0.5, points=np.zeros((3, 3)))
    with pytest.raises(ValueError, match='fields must name'):
        solidification_maps(heat, None, 0.5, fields=('dose',))
