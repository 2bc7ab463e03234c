#!/usr/bin/env python3
"""Every entry point of the three device engines on a P1 mesh -- load vectors
(csrc/load_dev.hip), error norms (csrc/err_norms.hip), sampling and its adjoint
(csrc/sample.hip) -- on small fixed-seed inputs, written as ONE .npz: the check that a change
to their shared code (csrc/p1_mesh.h) changes no bit.

    python3 tools/p1_engines_dump.py --out new.npz [--lib OTHER/libstk.so]
    python3 tools/p1_engines_dump.py --compare old.npz new.npz

Shapes: square and L-shape at J_space = 2, cube at J_space = 1; the mesh's own quadrature rule,
n_k = 2; 130 points (two full tiles of the eval kernel and a short one) with points outside the
mesh, on vertices and on edges, and one NaN time; a rank's view of a slab of N = 5 time nodes
that starts at node 1 and holds 3, so both kinds of "column on another rank" occur; even and
odd leading dimension.  --compare lists every array and exits 1 if one differs in any byte.
Needs a GPU (not for --compare)."""
import argparse
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'spacetime-fullgrid-parallel_amd'))

MESHES = (('square', 2), ('lshape', 2), ('cube', 1))
N, T_BEGIN, N_LOC, N_K, N_P = 5, 1, 3, 2, 130


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    print('%s against %s' % (path_a, path_b))
    bad = sorted(set(a.files) ^ set(b.files))
    for name in sorted(set(a.files) & set(b.files)):
        x, y = a[name], b[name]
        same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        print('%-44s %-8s %-14s %8d bytes  %s' % (name, x.dtype, x.shape, x.nbytes, 'identical' if same else 'DIFFERENT'))
        if not same:
            bad.append(name)
    print('%d arrays, %d different or missing: %s' % (len(a.files), len(bad), bad if bad else 'byte for byte the same'))
    return 1 if bad else 0


def points_of(mesh, rs):
    """N_P points: vertices, edge midpoints, centroids, seeded ones in the stretched box."""
    pts, cells = mesh.points, mesh.cells
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    sets = [pts[:30], 0.5 * (pts[cells[:30, 0]] + pts[cells[:30, 1]]), pts[cells[:20]].mean(axis=1)]
    n = N_P - sum(len(s) for s in sets)
    sets.append(lo - 0.2 * (hi - lo) + 1.4 * (hi - lo) * rs.rand(n, pts.shape[1]))
    return np.ascontiguousarray(np.concatenate(sets))


def dump_mesh(out, problem, J):
    import torch
    from source import _lib
    from source.assembly import DeviceLoadPlan
    from source.error_norms import ErrorPlan
    from source.mesh import construct_interval
    from source.problem import problem_helper
    from source.sampling import SamplePlan, time_weights
    lib, dev = _lib.lib(), _lib.compute_device()
    mesh = problem_helper(problem, J_space=J, J_time=1)[0]
    mesh_time = construct_interval(N=N - 1)
    rs = np.random.RandomState(1000 + 10 * J + len(problem))
    key = lambda name: '%s_J%d.%s' % (problem, J, name)
    host = lambda t: t.cpu().numpy()
    rand = lambda *shape: torch.from_numpy(rs.randn(*shape)).to(dev)

    # ---- load vectors: stk_load_points, stk_load_columns ------------------------------------
    load = DeviceLoadPlan(mesh, max_k=4)
    M, nc, d, nq = load.n_free, load.nc, load.d, len(load.qw)
    out[key('load_points')] = host(load.points())
    f, coef = rand(N_K, nc, nq), rs.randn(N_K, 2)
    for name, plan in (('load', load), ('load_ordered', DeviceLoadPlan(mesh, max_k=N_K, row_order=rs.permutation(M)))):
        buf = rand(M, 4)
        plan.columns(f, coef, buf, 1)
        out[key(name + '_columns')] = host(buf)
        plan.columns(f, coef, buf, 1, accumulate=True)
        out[key(name + '_columns_accumulated')] = host(buf)

    # ---- error norms: stk_err_points, stk_err_element with and without gf ------------------
    err = ErrorPlan(mesh, mesh_time)
    out[key('err_points')] = host(err.points())
    gf, u = rand(N_K, d, nc, nq), rand(M, 4)
    s = np.array([0.25, 0.875])
    for name, g in (('err_element', gf), ('err_element_no_gf', None)):
        out4 = torch.zeros(4, dtype=torch.float64, device=dev)
        err.element(f, g, 1.0 - s, s, [0.5, 0.75], _lib.ptr(u) + 8, 4, _lib.ptr(u) + 16, 4, out4)
        out[key(name)] = host(out4)

    # ---- sampling: locate, eval, grad_coeffs, pairs, adjoint --------------------------------
    plan = SamplePlan(mesh, mesh_time)
    loc = plan.locate(points_of(mesh, rs))
    out[key('locate_cell')], out[key('locate_lam')] = host(loc.cell), host(loc.lam)
    assert (out[key('locate_cell')] < 0).any() and (out[key('locate_cell')] >= 0).any()
    out[key('grad_coeffs')] = host(plan.grad_coeffs(loc))
    times = mesh_time.T * rs.rand(N_P)
    times[:4] = [0.0, mesh_time.T, float('nan'), 0.5 * mesh_time.h]
    t_dev = torch.from_numpy(times).to(dev)
    h = float(mesh_time.h)
    for ld in (4, 3):  # 4: the 16-byte loads where they apply; 3: 8-byte loads everywhere
        slab = rand(M, ld)
        columns, weights = time_weights(mesh_time, np.linspace(0.0, mesh_time.T, 7), T_BEGIN, T_BEGIN + N_LOC)
        block = torch.empty((7, N_P), dtype=torch.float64, device=dev)
        _lib.check(lib.stk_sample_eval(_lib.stream(), plan._plan, N_P, _lib.ptr(loc.cell), _lib.ptr(loc.lam), M, N_LOC, ld,
                                       _lib.ptr(slab), 7, columns.ctypes.data, weights.ctypes.data, N_P, _lib.ptr(block)))
        out[key('eval_ld%d' % ld)] = host(block)
        for mask in (1, 2, 4, 7):
            rows = torch.empty(((mask & 1) + (mask >> 1 & 1) + (mask >> 2) * d, N_P), dtype=torch.float64, device=dev)
            _lib.check(lib.stk_sample_pairs(_lib.stream(), plan._plan, N_P, _lib.ptr(loc.cell), _lib.ptr(loc.lam),
                                            _lib.ptr(t_dev), h, N, T_BEGIN, M, N_LOC, ld, _lib.ptr(slab), mask, N_P,
                                            _lib.ptr(rows)))
            out[key('pairs_ld%d_fields%d' % (ld, mask))] = host(rows)
        size = ctypes.c_int64()
        _lib.check(lib.stk_sample_pairs_adjoint_work_size(N_P, d, ctypes.addressof(size)))
        work = torch.empty(max(size.value, 256), dtype=torch.uint8, device=dev)
        for field in (1, 2, 4):
            w = rand(d if field == 4 else 1, N_P)
            target = torch.full((M, ld), 7.0, dtype=torch.float64, device=dev)
            used = torch.empty(N_P, dtype=torch.uint8, device=dev)
            for accumulate in (0, 1):
                _lib.check(lib.stk_sample_pairs_adjoint(
                    _lib.stream(), plan._plan, N_P, _lib.ptr(loc.cell), _lib.ptr(loc.lam), _lib.ptr(t_dev), h, N, T_BEGIN, M,
                    N_LOC, ld, _lib.ptr(target), _lib.ptr(w), N_P, field, accumulate, _lib.ptr(used), _lib.ptr(work),
                    work.numel()))
                out[key('adjoint_ld%d_field%d_accumulate%d' % (ld, field, accumulate))] = host(target)
            out[key('adjoint_ld%d_field%d_used' % (ld, field))] = host(used)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='p1_engines.npz')
    ap.add_argument('--lib', default=None, help='the libstk.so to load instead of the built one')
    ap.add_argument('--compare', nargs=2, metavar='NPZ', help='compare two dumps byte for byte')
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    import torch
    from source import _lib
    assert torch.cuda.is_available(), 'p1_engines_dump.py runs the kernels: it needs a GPU'
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    out = {}
    for problem, J in MESHES:
        dump_mesh(out, problem, J)
    torch.cuda.synchronize()
    np.savez(args.out, **out)
    print('%s: %d arrays from %s' % (args.out, len(out), _lib.LIB_PATH))
    return 0


if __name__ == '__main__':
    sys.exit(main())
