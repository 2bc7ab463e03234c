#!/usr/bin/env python3
"""What sampling along trajectories costs on one GPU (default: square_moving_source at
J_time = 6, J_space = 9 -- a slab of 1 046 529 rows by 65 time nodes, 544 MB -- and
2^20 pairs (t_p, x_p)), in two orders of the pairs:

* ``trajectory``: times ascending from 0 to T, points on the path of the moving source with
  Gaussian scatter 0.1 -- a caller's probe, tracers released along a path;
* ``random``: times uniform in [0, T], points uniform in the bounding box.

For ``fields=('u',)`` and for all fields (u, dt, grad):

* SamplePlan.evaluate_pairs (stk_sample_pairs), device events around `reps` calls, best and
  median of `rounds`;
* the SAME quantities composed from torch on the device on the same located points: index
  gathers of the 2 (d + 1) slab entries of every point (the slab rows of its vertices and
  the gradient coefficients handed over ready-made), the weighted sums in the kernel's
  order -- what a user would write without the kernel.  The two forms take turns in one
  process after a warm-up, and are compared entry by entry.

Per case: ns per point; algorithmic bytes per second, the bytes being per point t (8),
cell (4), lam (8 (d + 1)), the cell's vertices and their slab rows (8 (d + 1)), the slab
entries (16 (d + 1)), with the gradient the vertex coordinates (8 d (d + 1)), and 8 per
value written; slab line requests per second, (d + 1) per point inside the mesh (the two
entries of a row are neighbours); the ratio to the composition.

Kernel times proper come from a run of their own under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python3 tools/sample_along_time.py --kernel-only
    python3 tools/sample_along_time.py --trace DIR/*/*kernel_trace.csv
(--kernel-only launches, per case in the order above, one warm-up and `rounds` kernels and
nothing else; --trace reads their durations back by that order).

Writes one JSON line per figure to stdout; needs a GPU (not for --trace)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'spacetime-fullgrid-parallel_amd'))

ORDERS = ('trajectory', 'random')
FIELD_SETS = (('u',), ('u', 'dt', 'grad'))
KERNEL = 'sample_pairs_kernel'


def cases():
    return [(order, fields) for order in ORDERS for fields in FIELD_SETS]


def bytes_per_point(d, fields):
    n_rows = ('u' in fields) + ('dt' in fields) + d * ('grad' in fields)
    read = 8 + 4 + 8 * (d + 1) + 8 * (d + 1) + 16 * (d + 1) + (8 * d * (d + 1) if 'grad' in fields else 0)
    return read + 8 * n_rows


def pairs_of(order, n_p, mesh_space, mesh_time, path, seed=5):
    rs = np.random.RandomState(seed)
    lo, hi = mesh_space.points.min(axis=0), mesh_space.points.max(axis=0)
    if order == 'trajectory':
        times = np.linspace(0.0, mesh_time.T, n_p)
        points = np.asarray(path(times)) + 0.1 * rs.randn(n_p, len(lo))
    else:
        times = mesh_time.T * rs.rand(n_p)
        points = lo + (hi - lo) * rs.rand(n_p, len(lo))
    return times, points


def torch_pairs(torch, slab, ld, rows, lam, coeffs, times, h, N, fields):
    """The fields from torch alone: rows (n_p, d + 1) int64 slab rows of the points'
    vertices (-1: boundary), lam (n_p, d + 1), coeffs (d, n_p, d + 1), times (n_p,)."""
    x = times / h
    e = torch.clamp(torch.floor(x), max=N - 2)
    w1 = x - e
    w0 = 1.0 - w1
    at = rows.clamp(min=0) * ld + e.long()[:, None]
    flat = slab.reshape(-1)
    zero = torch.zeros((), dtype=slab.dtype, device=slab.device)
    free = rows >= 0
    u0 = torch.where(free, flat[at], zero)
    u1 = torch.where(free, flat[at + 1], zero)

    def spatial(k, v):
        s = k[:, 0] * v[:, 0]
        for a in range(1, k.shape[1]):
            s = s + k[:, a] * v[:, a]
        return s

    out = {}
    if 'u' in fields or 'dt' in fields:
        s0, s1 = spatial(lam, u0), spatial(lam, u1)
        if 'u' in fields:
            out['u'] = w0 * s0 + w1 * s1
        if 'dt' in fields:
            out['dt'] = (-(s0 / h)) + s1 / h
    if 'grad' in fields:
        out['grad'] = torch.stack([w0 * spatial(g, u0) + w1 * spatial(g, u1) for g in coeffs])
    return out


def summarise_trace(path, rounds):
    rows = []
    for r in csv.DictReader(open(path)):
        if KERNEL in r['Kernel_Name']:
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp'])))
    rows.sort()
    per_case = rounds + 1
    assert len(rows) == per_case * len(cases()), (len(rows), per_case, len(cases()))
    for i, (order, fields) in enumerate(cases()):
        ns = [e - s for s, e in rows[i * per_case + 1:(i + 1) * per_case]]  # without the warm-up
        print(json.dumps({'profiled_case': order, 'fields': list(fields), 'kernel_ns': ns, 'best_kernel_ns': min(ns),
                          'median_kernel_ns': float(np.median(ns))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square_moving_source')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--pairs', type=int, default=1 << 20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20, help='calls per timed round')
    ap.add_argument('--kernel-only', action='store_true', help='only the kernel launches: the run under the profiler')
    ap.add_argument('--trace', default=None, help='summarise the kernel trace CSV of a --kernel-only run')
    args = ap.parse_args()
    if args.trace:
        return summarise_trace(args.trace, args.rounds)

    import torch
    from source import _lib
    from source.assembly import free_dofs
    from source.linop import self_distribution
    from source.mpi_vector import KronVectorMPI
    from source.problem import problem_helper
    from source.sampling import SamplePlan
    assert torch.cuda.is_available(), 'sample_along_time.py measures on a GPU'
    t0 = time.perf_counter()
    mesh_space, _, mesh_time, data, _ = problem_helper(args.problem, J_space=args.J_space, J_time=args.J_time)
    assert 'path' in data, 'the trajectory order follows the path of the problem: %s has none' % args.problem
    N, M, d = mesh_time.nv, len(free_dofs(mesh_space)), mesh_space.points.shape[1]
    plan = SamplePlan(mesh_space, mesh_time)
    torch.cuda.synchronize()
    n_p, h = args.pairs, float(mesh_time.h)
    dev = _lib.compute_device()
    torch.manual_seed(3)
    vec = KronVectorMPI.around(self_distribution(N, M), torch.randn((M, N + (N & 1)), dtype=torch.float64, device=dev))
    print(json.dumps({'problem': args.problem, 'N': N, 'M': M, 'cells': len(mesh_space.cells), 'pairs': n_p,
                      'slab_bytes': 8 * M * vec.ld, 'kernel_only': args.kernel_only, 'rounds': args.rounds,
                      'reps': args.reps,
                      'setup_s': time.perf_counter() - t0}), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        """seconds per call over `reps` calls between two device events"""
        e0.record()
        for _ in range(args.reps):
            out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / args.reps, out

    cells = _lib.to_dev(np.ascontiguousarray(mesh_space.cells, dtype=np.int64))
    row_of = np.full(mesh_space.nv, -1, dtype=np.int64)
    row_of[free_dofs(mesh_space)] = np.arange(M)
    row_of = _lib.to_dev(row_of)
    for order in ORDERS:
        times, points = pairs_of(order, n_p, mesh_space, mesh_time, data['path'])
        t_dev = torch.from_numpy(times).to(dev)
        loc = plan.locate(torch.from_numpy(points).to(dev))
        inside = int(loc.inside.sum())
        if not args.kernel_only:
            rows = row_of[cells[loc.cell.long().clamp(min=0)]]
            coeffs = plan.grad_coeffs(loc)
        for fields in FIELD_SETS:
            kernel = lambda: plan.evaluate_pairs(vec, t_dev, loc, fields=fields)
            kernel()  # warm-up: the code object, the allocator's blocks
            if args.kernel_only:
                for _ in range(args.rounds):
                    kernel()
                torch.cuda.synchronize()
                continue
            composed = lambda: torch_pairs(torch, vec.buf, vec.ld, rows, loc.lam, coeffs, t_dev, h, N, fields)
            composed()
            k_s, t_s = [], []
            for _ in range(args.rounds):  # the two forms take turns
                k_s.append(timed(kernel)[0])
                t_s.append(timed(composed)[0])
            got, ref = kernel(), composed()
            ok = loc.inside
            diff = {f: float((got[f][..., ok] - ref[f][..., ok]).abs().max()) for f in fields}
            nan_outside = all(bool(torch.isnan(got[f][..., ~ok]).all()) for f in fields)
            best_k, best_t = min(k_s), min(t_s)
            algorithmic = bytes_per_point(d, fields) * n_p
            print(json.dumps({'case': order, 'fields': list(fields), 'points_inside': inside, 'kernel_s': k_s, 'torch_s': t_s,
                              'best_kernel_s': best_k, 'median_kernel_s': float(np.median(k_s)),
                              'best_torch_s': best_t, 'median_torch_s': float(np.median(t_s)),
                              'kernel_ns_per_point': best_k / n_p * 1e9, 'torch_ns_per_point': best_t / n_p * 1e9,
                              'torch_over_kernel': best_t / best_k, 'algorithmic_bytes': algorithmic,
                              'kernel_GBps': algorithmic / best_k * 1e-9, 'torch_GBps': algorithmic / best_t * 1e-9,
                              'kernel_slab_line_requests_per_s': (d + 1) * inside / best_k,
                              'largest_difference_kernel_torch': diff, 'nan_outside': nan_outside}), flush=True)


if __name__ == '__main__':
    main()
