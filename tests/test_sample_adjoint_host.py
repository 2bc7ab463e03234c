"""The adjoint of paired sampling, the parts that need no GPU: ``numpy_sample_adjoint``, the
contract of stk_sample_pairs_adjoint (include/stk.h "the adjoint of paired sampling") as a
plain loop with the chunk rule, which tests/test_sample_adjoint_gpu.py compares the device
with bit for bit; the identity sum_p w_p (E U)_p = <E^T w, U> against the forward oracle
``numpy_sample_along``; the chunk rule itself; `used`; and the ValueErrors of
``SamplePlan.adjoint_pairs``, which are raised before anything touches a GPU.

Tolerance of the identity, with h the time step and max|G| the largest gradient coefficient
of the forward oracle: 1e-12 sum|w_p| max|U| {1, 1 / h, max|G|} for u, dt, grad -- the scales
of VALUE_TOL and DERIV_TOL (tests/test_sample_along_host.py) times the weights.  Both sides
are sums of the same n_terms products in different orders, so they differ by at most
n_terms 2^-53 of that scale; measured here on the six meshes: <= 4.5e-18 of the scale (grad
on square J = 1, N = 5).  An index or sign error is O(1)."""
import os

import numpy as np
import pytest

from conftest import REPO
from test_sample_along_host import DERIV_TOL, _inverses_of, inv_grad_coeffs, numpy_sample_along
from test_sampling_host import INSIDE, MESHES, VALUE_TOL, _FakeComm, mesh_of, oracle_located, point_sets

CHUNK = 512  # STK_SAMPLE_ADJ_CHUNK
FIELDS = ('u', 'dt', 'grad')
SETS = ('random', 'vertices', 'centroids', 'midpoints')


# ---- the oracle ------------------------------------------------------------------------
def chunk_sum(terms, chunk=CHUNK):
    """The sum of a destination's terms by the chunk rule: chunks of `chunk` consecutive
    terms, each summed from the left starting with its first term, the chunk sums added
    from the left in chunk order.  Python floats: every sum rounded on its own."""
    total = None
    for a in range(0, len(terms), chunk):
        part = terms[a]
        for x in terms[a + 1:a + chunk]:
            part = part + x
        total = part if total is None else total + part
    return total


def numpy_sample_adjoint(mesh, N, w, times, cell, lam, field, G=None, mesh_time=None):
    """E^T w on the whole time mesh: (out (N, M), used (n_p,)) -- time-major, free dofs in
    ascending vertex order.  w (n_p,), for 'grad' (d, n_p); cell (n_p,), lam (n_p, d + 1) as
    a locate returned them; G (d, n_p, d + 1) = [j, p, b] the gradient coefficients d_j l_b
    per point (only for 'grad').  Point p is used when cell >= 0, its time is no NaN and lies
    in [0, (N - 1) h]; its terms go to the nodes e, e + 1 of the time rule and to the free
    vertices of its cell, in the order p, a, b; every entry is the chunk_sum of its terms,
    0.0 without any.  A slab of the nodes [t_begin, t_end) is out[t_begin:t_end]."""
    from source.assembly import free_dofs
    from source.mesh import construct_interval
    assert field in FIELDS
    mesh_time = construct_interval(N=N - 1) if mesh_time is None else mesh_time
    h = float(mesh_time.h)
    fd = np.asarray(free_dofs(mesh))
    row_of = np.full(mesh.nv, -1, dtype=np.int64)
    row_of[fd] = np.arange(len(fd))
    w, times, lam = np.asarray(w, dtype=np.float64), np.asarray(times, dtype=np.float64), np.asarray(lam)
    n_p, d = len(times), mesh.cells.shape[1] - 1
    assert w.shape == ((d, n_p) if field == 'grad' else (n_p,)) and lam.shape == (n_p, d + 1)
    t_last = float(N - 1) * h
    used = np.zeros(n_p, dtype=bool)
    lists = {}
    for p in range(n_p):
        t = float(times[p])
        if not (cell[p] >= 0 and t >= 0.0 and t <= t_last):  # NaN fails both comparisons
            continue
        used[p] = True
        x = t / h
        ef = min(float(np.floor(x)), float(N - 2))
        e, s = int(ef), x - ef
        wa = (1.0 - s, s)
        verts = mesh.cells[cell[p]]
        if field == 'grad':
            q = []
            for b in range(d + 1):
                acc = float(w[0, p]) * float(G[0, p, b])
                for j in range(1, d):
                    acc = acc + float(w[j, p]) * float(G[j, p, b])
                q.append(acc)
            terms = [[wa[a] * q[b] for b in range(d + 1)] for a in range(2)]
        else:
            wp = float(w[p])
            if field == 'u':
                k = (wp * wa[0], wp * wa[1])
            else:
                k = (-(wp / h), wp / h)
            terms = [[k[a] * float(lam[p, b]) for b in range(d + 1)] for a in range(2)]
        for a in range(2):
            for b in range(d + 1):
                r = row_of[verts[b]]
                if r >= 0:
                    lists.setdefault((e + a, int(r)), []).append(terms[a][b])
    out = np.zeros((N, len(fd)))
    for (col, r), terms in lists.items():
        out[col, r] = chunk_sum(terms)
    numpy_sample_adjoint.longest = max([len(v) for v in lists.values()], default=0)
    return out, used


def numpy_sample_adjoint_short(mesh, N, w, times, cell, lam, field, G=None):
    """The same doubles without the Python loop, for many pairs whose lists all stay within
    one chunk (asserted): the terms by elementwise NumPy, every operation rounded on its own,
    and np.add.at, which adds them one after the other in the order p, a, b."""
    from source.assembly import free_dofs
    from source.mesh import construct_interval
    h = float(construct_interval(N=N - 1).h)
    fd = np.asarray(free_dofs(mesh))
    row_of = np.full(mesh.nv, -1, dtype=np.int64)
    row_of[fd] = np.arange(len(fd))
    w, times, lam = np.asarray(w, dtype=np.float64), np.asarray(times, dtype=np.float64), np.asarray(lam)
    with np.errstate(invalid='ignore'):
        used = (np.asarray(cell) >= 0) & (times >= 0.0) & (times <= float(N - 1) * h)
    t = np.where(used, times, 0.0)
    x = t / h
    ef = np.minimum(np.floor(x), float(N - 2))
    s = x - ef
    wa = np.stack([1.0 - s, s], axis=1)  # (n_p, 2)
    if field == 'grad':
        q = w[0][:, None] * G[0]
        for j in range(1, len(w)):
            q = q + w[j][:, None] * G[j]
        terms = wa[:, :, None] * q[:, None, :]
    else:
        k = w[:, None] * wa if field == 'u' else np.stack([-(w / h), w / h], axis=1)
        terms = k[:, :, None] * lam[:, None, :]
    rows = row_of[mesh.cells[np.where(used, cell, 0)]]  # (n_p, d + 1)
    cols = ef.astype(np.int64)[:, None] + np.arange(2)[None, :]
    keep = used[:, None, None] & (rows >= 0)[:, None, :] & np.ones((1, 2, 1), dtype=bool)
    index = (cols[:, :, None] * len(fd) + rows[:, None, :])[keep]
    longest = int(np.bincount(index).max()) if index.size else 0
    assert longest <= CHUNK, longest
    out = np.zeros(N * len(fd))
    np.add.at(out, index, terms[keep])
    numpy_sample_adjoint_short.longest = longest
    return out.reshape(N, len(fd)), used


def adjoint_times(N, n_p, seed=0):
    """0, T, every node, the element midpoints, seeded random times; again and again."""
    nodes = np.arange(N) / (N - 1.0)
    h = 1.0 / (N - 1)
    pool = np.concatenate([[0.0, 1.0, 0.5 * h], nodes, nodes[:-1] + 0.5 * h, np.random.RandomState(N + seed).rand(131)])
    return np.resize(pool, n_p)


def oracle_points(problem, J):
    """(points, cell with -1 outside, lam) of the four point sets together, by numpy_locate."""
    sets = point_sets(problem, J)
    located = [oracle_located(problem, J, k) for k in SETS]
    points = np.concatenate([sets[k] for k in SETS])
    cell, lam, low = (np.concatenate([l[i] for l in located]) for i in range(3))
    return points, np.where(low >= INSIDE, cell, -1), lam


def scales_of(U, h, max_G):
    m = np.max(np.abs(U))
    return {'u': VALUE_TOL * m, 'dt': DERIV_TOL * m / h, 'grad': DERIV_TOL * m * max_G}


# ---- the identity <E^T w, U> = w . (E U) ---------------------------------------------------
@pytest.mark.parametrize('N', [2, 5, 9, 65])
@pytest.mark.parametrize('problem,J', MESHES)
def test_adjoint_identity_against_the_forward_oracle(problem, J, N):
    from source.assembly import free_dofs
    mesh = mesh_of(problem, J)
    d = mesh.points.shape[1]
    points, cell, lam = oracle_points(problem, J)
    n_p, h = len(points), 1.0 / (N - 1)
    times = adjoint_times(N, n_p)
    assert {0.0, 1.0, 0.5 * h} <= set(times.tolist()) and set(np.arange(N) / (N - 1.0)) <= set(times.tolist())
    rs = np.random.RandomState(100 * N + J)
    U = rs.randn(N, len(free_dofs(mesh)))
    Ainv = _inverses_of(problem, J)
    forward = numpy_sample_along(mesh, U, times, points, cell=cell, Ainv=Ainv)
    inside = forward['inside']
    assert 0 < inside.sum() < n_p
    G = inv_grad_coeffs(mesh, Ainv)[np.where(inside, cell, 0)].transpose(2, 0, 1)  # (d, n_p, d + 1)
    scales = scales_of(U, h, forward['max_G'])
    worst = {}
    for field in FIELDS:
        w = rs.randn(d, n_p) if field == 'grad' else rs.randn(n_p)
        out, used = numpy_sample_adjoint(mesh, N, w, times, cell, lam, field, G=G)
        assert np.array_equal(used, inside)
        lhs = float(np.sum(out * U))
        rhs = float(np.sum((w * forward[field])[..., inside]))
        bound = scales[field] * float(np.sum(np.abs(w[..., inside])))
        worst[field] = abs(lhs - rhs) / bound * 1e-12
        assert abs(lhs - rhs) <= bound, (field, lhs, rhs)
        assert abs(rhs) > 1e3 * bound  # the two sides are no zeros
    print('%s J=%d N=%d: |<E^T w, U> - w . E U| over sum|w| max|U| {1, 1/h, max|G|}: %s' % (
        problem, J, N, ', '.join('%s %.1e' % kv for kv in worst.items())))


# ---- the chunk rule ------------------------------------------------------------------------
def test_chunk_rule():
    rs = np.random.RandomState(3)
    for n in (1, 2, 511, 512):
        terms = [float(x) for x in rs.randn(n) * 10.0 ** rs.randint(-8, 8, n)]
        plain = terms[0]
        for x in terms[1:]:
            plain = plain + x
        assert chunk_sum(terms) == plain, n
    # 1 300 terms: three chunks of 512, 512 and 276, written out by hand
    terms = [float(x) for x in rs.randn(1300) * 10.0 ** rs.randint(-8, 8, 1300)]
    parts = []
    for a, b in ((0, 512), (512, 1024), (1024, 1300)):
        part = terms[a]
        for x in terms[a + 1:b]:
            part = part + x
        parts.append(part)
    by_hand = (parts[0] + parts[1]) + parts[2]
    plain = terms[0]
    for x in terms[1:]:
        plain = plain + x
    assert chunk_sum(terms) == by_hand
    assert by_hand != plain  # another shape of sum: these terms tell them apart
    assert abs(by_hand - plain) <= 1300 * 2.0 ** -53 * sum(abs(x) for x in terms)
    # 513 terms: the last chunk is one term
    terms = terms[:513]
    head = terms[0]
    for x in terms[1:512]:
        head = head + x
    assert chunk_sum(terms) == head + terms[512]


def test_oracle_sums_a_long_list_by_chunks():
    """1 300 copies of one pair: every entry the pair touches is the chunk sum of 1 300 equal
    terms, which is not the plain sum from the left."""
    problem, J, N = 'square', 3, 5
    mesh = mesh_of(problem, J)
    cell_o, lam_o, _ = oracle_located(problem, J, 'centroids')
    c = int(np.flatnonzero(np.all(~mesh.boundary[mesh.cells], axis=1))[0])
    n = 1300
    cell, lam = np.full(n, cell_o[c]), np.tile(lam_o[c], (n, 1))
    out, used = numpy_sample_adjoint(mesh, N, np.full(n, 0.1), np.full(n, 0.3), cell, lam, 'u')
    assert used.all() and numpy_sample_adjoint.longest == n and np.count_nonzero(out) == 2 * 3
    single, _ = numpy_sample_adjoint(mesh, N, np.full(1, 0.1), np.full(1, 0.3), cell[:1], lam[:1], 'u')
    for col, r in zip(*np.nonzero(out)):
        assert out[col, r] == chunk_sum([single[col, r]] * n)


def test_the_loop_free_oracle_is_the_oracle():
    for (problem, J), N in zip(MESHES, (2, 5, 9, 65, 9, 5)):
        mesh = mesh_of(problem, J)
        d = mesh.points.shape[1]
        points, cell, lam = oracle_points(problem, J)
        n_p = len(points)
        times = adjoint_times(N, n_p)
        times[5], times[6] = float('nan'), -0.25
        G = inv_grad_coeffs(mesh, _inverses_of(problem, J))[np.where(cell >= 0, cell, 0)].transpose(2, 0, 1)
        rs = np.random.RandomState(N)
        for field in FIELDS:
            w = rs.randn(d, n_p) if field == 'grad' else rs.randn(n_p)
            a, used_a = numpy_sample_adjoint(mesh, N, w, times, cell, lam, field, G=G)
            b, used_b = numpy_sample_adjoint_short(mesh, N, w, times, cell, lam, field, G=G)
            assert np.array_equal(a, b) and np.array_equal(used_a, used_b), (problem, field)
            assert numpy_sample_adjoint_short.longest == numpy_sample_adjoint.longest > 1


# ---- used ---------------------------------------------------------------------------------
def test_used_is_inside_and_the_time_check():
    problem, J, N = 'lshape_jitter', 3, 9
    mesh = mesh_of(problem, J)
    points, cell, lam = oracle_points(problem, J)
    points, cell, lam = points[:600], cell[:600], lam[:600]
    times = adjoint_times(N, 600)
    bad = {3: float('nan'), 10: -1e-9, 17: 1.0 + 1e-9, 40: float('inf'), 41: -0.0, 42: 1.0, 43: 0.0}
    for p, t in bad.items():
        times[p] = t
    time_ok = (times >= 0.0) & (times <= 1.0)  # False for NaN
    U = np.random.RandomState(1).randn(N, int((~mesh.boundary).sum()))
    forward = numpy_sample_along(mesh, U, np.where(time_ok, times, 0.5), points, cell=cell, Ainv=_inverses_of(problem, J))
    assert not time_ok[[3, 10, 17, 40]].any() and time_ok[[41, 42, 43]].all()
    w = np.random.RandomState(2).randn(600)
    w[3] = float('nan')  # the weight of an unused pair is not looked at
    out, used = numpy_sample_adjoint(mesh, N, w, times, cell, lam, 'u')
    assert np.array_equal(used, forward['inside'] & time_ok) and 0 < used.sum() < 600
    assert np.isfinite(out).all()
    # nothing added by the unused ones: the same as leaving them out
    keep = used
    again, used2 = numpy_sample_adjoint(mesh, N, w[keep], times[keep], cell[keep], lam[keep], 'u')
    assert used2.all() and np.array_equal(out, again)


# ---- what adjoint_pairs refuses, before any GPU work ---------------------------------------
def test_adjoint_pairs_refuses_wrong_shapes_and_fields():
    import torch
    from source.mpi_vector import DofDistributionMPI
    from source.sampling import Located, SamplePlan, _check_adjoint_arguments
    plan = SamplePlan.__new__(SamplePlan)  # no device plan behind it: reaching the library would fail otherwise
    plan.d, plan.n_free, plan.mesh_time = 2, 49, None
    n_p = 7
    located = Located(torch.zeros(n_p, dtype=torch.int32), torch.zeros((n_p, 3), dtype=torch.float64))
    distr = DofDistributionMPI(_FakeComm(0, 1), 5, 49)
    w, t = np.zeros(n_p), np.zeros(n_p)
    refused = [
        dict(weights=w, times=t, field='laplace'),
        dict(weights=w, times=t, field=('u', 'dt')),
        dict(weights=w, times=t, field=1),
        dict(weights=np.zeros(n_p + 1), times=t),
        dict(weights=np.zeros((2, n_p)), times=t),
        dict(weights=np.zeros((2, n_p)), times=t, field='dt'),
        dict(weights=w, times=t, field='grad'),
        dict(weights=np.zeros((3, n_p)), times=t, field='grad'),
        dict(weights=np.zeros((n_p, 2)), times=t, field='grad'),
        dict(weights=torch.zeros(n_p - 1), times=t),
        dict(weights=w, times=np.zeros(n_p - 1)),
        dict(weights=w, times=np.zeros((n_p, 1))),
        dict(weights=w, times=torch.zeros(())),
        dict(weights=w, times=t, accumulate=True),  # nothing to add to
    ]
    for kw in refused:
        with pytest.raises(ValueError):
            plan.adjoint_pairs(distr, located=located, **kw)
    with pytest.raises(ValueError):  # a distribution of another space
        plan.adjoint_pairs(DofDistributionMPI(_FakeComm(0, 1), 5, 50), w, t, located)
    with pytest.raises(ValueError):  # a time mesh of one node has no element
        plan.adjoint_pairs(DofDistributionMPI(_FakeComm(0, 1), 1, 49), w, t, located)
    # what it takes: arrays, lists and tensors of the right shape come back unchanged in shape
    for field, shape in (('u', (n_p,)), ('dt', (n_p,)), ('grad', (2, n_p))):
        ww, tt = _check_adjoint_arguments(2, n_p, np.zeros(shape).tolist(), torch.zeros(n_p), field)
        assert tuple(ww.shape) == shape and tuple(tt.shape) == (n_p,)


def test_library_declares_the_adjoint_calls():
    from source import _lib
    names = ('stk_sample_pairs_adjoint', 'stk_sample_pairs_adjoint_work_size')
    assert set(names) <= set(_lib.EXPORTED_SYMBOLS) and all(hasattr(_lib.lib(), name) for name in names)
    header = open(os.path.join(REPO, 'include', 'stk.h')).read()
    assert '#define STK_SAMPLE_ADJ_CHUNK %d\n' % CHUNK in header
