#!/usr/bin/env python3
"""What the history maps cost on one GPU (default: the square at J_time = 6, J_space = 9 --
a slab of 1 046 529 rows by 65 time nodes, 544 MB -- and a 1024^2 raster):

* the nodal form: stk_history_scan on the slab (device events, one warm-up, best of `rounds`
  with the median beside it), for several tile shapes of the slab kernel (stk_history_tile:
  rows per workgroup, LDS per workgroup -- which sets the columns per chunk);
* the SAME quantities composed from torch on buf[:, :n_loc] -- what a user would write
  without the kernel: max with indices, trapezoid, diff / h with max and min, and the
  `where` form of the three threshold branches with sum -- timed in the same process, the
  forms taking turns (rounds interleaved), and compared entry by entry;
* the per-point form on the raster: sample at the nodes in column chunks + the time-major
  scan, and the sampling alone.

Algorithmic bytes of the nodal form = the slab read once (8 M ld) + the state written once
(72 M), over the best time, in TB/s -- to be read beside the 4.9-5.2 TB/s of this
repository's pure streams.

Writes one JSON line per figure to stdout; needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'spacetime-fullgrid-parallel_amd'))

# (rows per workgroup, LDS per workgroup in KiB) of the slab kernel: stk_history_tile
TILES = ((64, 40), (128, 40), (256, 40), (256, 20), (256, 10), (512, 40), (512, 20))


def torch_composition(v, h, theta):
    """peak, t_peak, dose, max_rate, min_rate and time_above of the rows of `v` (M, n) --
    a view buf[:, :n_loc] of a slab -- from torch alone."""
    peak, at = v.max(dim=1)
    dose = torch.trapezoid(v, dx=h, dim=1)
    rate = torch.diff(v, dim=1) / h
    a, b = v[:, :-1], v[:, 1:]
    a_up, b_up = a > theta, b > theta
    x = (theta - a) / (b - a)
    zero = torch.zeros((), dtype=v.dtype, device=v.device)
    seg = torch.where(a_up & b_up, h + zero,
                      torch.where(b_up & ~a_up, h * (1.0 - x), torch.where(a_up & ~b_up, h * x, zero)))
    return {'peak': peak, 't_peak': at.to(v.dtype) * h, 'dose': dose, 'max_rate': rate.max(dim=1).values,
            'min_rate': rate.min(dim=1).values, 'time_above': seg.sum(dim=1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--raster', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--threshold', type=float, default=0.3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'history_time.py measures on a GPU'
    from source import _lib
    from source.assembly import free_dofs
    from source.history import STATE_ROWS, history_points_collective, history_scan
    from source.linop import self_distribution
    from source.mpi_vector import KronVectorMPI
    from source.problem import problem_helper
    from source.sampling import SamplePlan, raster, sample_collective

    mesh_space, _, mesh_time, _, _ = problem_helper(args.problem, J_space=args.J_space, J_time=args.J_time)
    N, M, h, theta = mesh_time.nv, len(free_dofs(mesh_space)), float(mesh_time.h), args.threshold
    dev = _lib.compute_device()
    ld = N + (N & 1)
    vec = KronVectorMPI.around(self_distribution(N, M), torch.randn((M, ld), dtype=torch.float64, device=dev))
    state = torch.empty((len(STATE_ROWS), M), dtype=torch.float64, device=dev)
    algorithmic = 8 * M * ld + 8 * len(STATE_ROWS) * M
    print(json.dumps({'problem': args.problem, 'N': N, 'M': M, 'ld': ld, 'slab_MB': 8e-6 * M * ld,
                      'algorithmic_bytes': algorithmic, 'threshold': theta}), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    def kernel(tile):
        _lib.check(_lib.lib().stk_history_tile(*tile))
        return history_scan(vec.buf, M, N, (ld, 1), 0, h, theta, state, fresh=True)

    composed = lambda: torch_composition(vec.buf[:, :N], h, theta)
    for tile in TILES:
        kernel(tile)
    composed()  # warm-up: code objects, the allocator's blocks
    k_s, t_s = {tile: [] for tile in TILES}, []
    for _ in range(args.rounds):  # the forms take turns
        for tile in TILES:
            k_s[tile].append(timed(lambda: kernel(tile))[0])
        t_s.append(timed(composed)[0])
    ref = composed()
    kernel((0, 0))
    diffs = {f: float((state[STATE_ROWS.index(f)] - ref[f]).abs().max()) for f in ref}
    del ref
    best_t = min(t_s)
    for tile in TILES:
        best_k = min(k_s[tile])
        print(json.dumps({'case': 'nodal', 'tile_rows': tile[0], 'tile_lds_KiB': tile[1], 'kernel_s': k_s[tile],
                          'best_kernel_s': best_k,
                          'median_kernel_s': float(np.median(k_s[tile])), 'torch_s': t_s, 'best_torch_s': best_t,
                          'median_torch_s': float(np.median(t_s)), 'torch_over_kernel': best_t / best_k,
                          'kernel_TBps': algorithmic / best_k * 1e-12, 'torch_TBps': algorithmic / best_t * 1e-12,
                          'pure_stream_TBps': [4.9, 5.2]}), flush=True)
    print(json.dumps({'case': 'nodal', 'largest_difference_kernel_torch': diffs}), flush=True)

    plan = SamplePlan(mesh_space, mesh_time)
    located = plan.locate(raster(mesh_space, args.raster))
    from source.history import plan_chunks
    chunks = plan_chunks(N, located.n_p)

    def sampling_alone():
        for k0, k1 in chunks:
            sample_collective(plan, vec, np.arange(k0, k1) * h, located)

    points_form = lambda: history_points_collective(plan, vec, located, theta)
    points_form(), sampling_alone()
    p_s, s_s = [], []
    for _ in range(args.rounds):
        p_s.append(timed(points_form)[0])
        s_s.append(timed(sampling_alone)[0])
    print(json.dumps({'case': 'points', 'points': located.n_p, 'inside': int(located.inside.sum()),
                      'column_chunks': chunks, 'points_form_s': p_s, 'best_points_form_s': min(p_s),
                      'median_points_form_s': float(np.median(p_s)), 'sampling_alone_s': s_s,
                      'best_sampling_alone_s': min(s_s), 'median_sampling_alone_s': float(np.median(s_s))}), flush=True)


if __name__ == '__main__':
    main()
