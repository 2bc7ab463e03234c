#!/usr/bin/env python3
"""What sampling the solution costs on one GPU (default: the square at J_time = 6,
J_space = 9 -- a slab of 1 046 529 rows by 65 time nodes -- and a 1024^2 raster):

* the construction of the plan (mesh upload, bucket grid on the host threads), wall clock;
* stk_sample_locate for the raster (device events, best of `rounds` after a warm-up);
* SamplePlan.evaluate for the raster at all 65 nodes, and at 5 equally spaced times;
* the SAME blocks composed from torch on the device, on the same located points: the
  d + 1 rows of every point by index_select, the weighted sums in the kernel's order, the
  two time columns of every request, transposed into the (n_k, n_p) block -- what a user
  would write without the kernel; timed in the same process, the two forms taking turns
  (rounds interleaved), and compared entry by entry.

For each evaluate case: algorithmic bytes = the block written once + every distinct slab
row the points need read once (8 n_loc bytes each) + the located points (cell, lam), over
the best time, in TB/s and as a share of the 8 TB/s HBM peak.  The slab (544 MB) and the
65-node block (545 MB) are each larger than the 256 MB Infinity Cache.

Writes one JSON line per figure to stdout; needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'spacetime-fullgrid-parallel_amd'))
from source import _lib  # noqa: E402
from source.assembly import free_dofs  # noqa: E402
from source.linop import self_distribution  # noqa: E402
from source.mpi_vector import KronVectorMPI  # noqa: E402
from source.problem import problem_helper  # noqa: E402
from source.sampling import SamplePlan, raster, time_weights  # noqa: E402

HBM_PEAK = 8e12  # bytes / s


def torch_block(vec, rows, lam, columns, weights, chunk):
    """The block from torch alone: rows (n_p, d + 1) int64 slab rows of the points'
    vertices (-1: boundary), lam (n_p, d + 1), requests as device tensors."""
    n_p, n_k = rows.shape[0], columns.shape[0]
    out = torch.empty((n_k, n_p), dtype=torch.float64, device=rows.device)
    slab = vec.buf
    for a in range(0, n_p, chunk):
        r, l = rows[a:a + chunk], lam[a:a + chunk]
        s = None
        for k in range(r.shape[1]):
            g = slab.index_select(0, r[:, k].clamp(min=0))  # (chunk, ld): whole rows
            g = torch.where((r[:, k] >= 0)[:, None], g, torch.zeros((), dtype=g.dtype, device=g.device))
            term = l[:, k, None] * g
            s = term if s is None else s + term
        p0 = weights[:, 0] * s.index_select(1, columns[:, 0])
        p1 = weights[:, 1] * s.index_select(1, columns[:, 1])
        out[:, a:a + chunk] = (p0 + p1).t()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--raster', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=1 << 18, help='points per step of the torch composition')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'sample_time.py measures on a GPU'
    t0 = time.perf_counter()
    mesh_space, _, mesh_time, _, _ = problem_helper(args.problem, J_space=args.J_space, J_time=args.J_time)
    N, M, d = mesh_time.nv, len(free_dofs(mesh_space)), mesh_space.points.shape[1]
    t1 = time.perf_counter()
    plan = SamplePlan(mesh_space, mesh_time)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    points = raster(mesh_space, args.raster)
    n_p = len(points)
    print(json.dumps({'problem': args.problem, 'N': N, 'M': M, 'cells': len(mesh_space.cells), 'points': n_p,
                      'meshes_s': t1 - t0, 'plan_s': t2 - t1}), flush=True)

    dev = _lib.compute_device()
    vec = KronVectorMPI.around(self_distribution(N, M), torch.randn((M, N + (N & 1)), dtype=torch.float64, device=dev))
    x = torch.from_numpy(points).to(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    locate_s = [timed(lambda: plan.locate(x))[0] for _ in range(args.rounds + 1)][1:]
    loc = plan.locate(x)
    inside = int(loc.inside.sum())
    print(json.dumps({'locate_s': locate_s, 'best_locate_s': min(locate_s), 'points_inside': inside,
                      'locate_Mpoints_per_s': n_p / min(locate_s) * 1e-6}), flush=True)

    # what the torch form needs beside the located points: the slab rows of their vertices
    cells = _lib.to_dev(np.ascontiguousarray(mesh_space.cells, dtype=np.int64))
    row_of = np.full(mesh_space.nv, -1, dtype=np.int64)
    row_of[free_dofs(mesh_space)] = np.arange(M)
    rows = _lib.to_dev(row_of)[cells[loc.cell.long().clamp(min=0)]]
    distinct_rows = int(torch.unique(rows[rows >= 0]).numel())

    for label, times in (('all_nodes', mesh_time.nodes), ('five_times', np.linspace(0.0, mesh_time.T, 5))):
        columns, weights = time_weights(mesh_time, times, 0, N)
        n_k = len(times)
        cols_d, w_d = _lib.to_dev(columns.astype(np.int64)), _lib.to_dev(weights)
        out = torch.empty((n_k, n_p), dtype=torch.float64, device=dev)
        kernel = lambda: plan.evaluate(vec, times, loc, out=out)
        composed = lambda: torch_block(vec, rows, loc.lam, cols_d, w_d, args.chunk)
        kernel(), composed()  # warm-up: code objects, the allocator's blocks
        k_s, t_s = [], []
        for _ in range(args.rounds):  # the two forms take turns
            k_s.append(timed(kernel)[0])
            t_s.append(timed(composed)[0])
        ref = composed()
        both = ~torch.isnan(out)
        diff = float((out[both] - ref[both]).abs().max()) if inside == n_p else None
        algorithmic = 8 * n_k * n_p + 8 * N * distinct_rows + n_p * (4 + 8 * (d + 1))
        best_k, best_t = min(k_s), min(t_s)
        print(json.dumps({'case': label, 'requests': n_k, 'kernel_s': k_s, 'torch_s': t_s,
                          'best_kernel_s': best_k, 'median_kernel_s': float(np.median(k_s)),
                          'best_torch_s': best_t, 'median_torch_s': float(np.median(t_s)),
                          'torch_over_kernel': best_t / best_k, 'distinct_slab_rows': distinct_rows,
                          'algorithmic_bytes': algorithmic, 'kernel_TBps': algorithmic / best_k * 1e-12,
                          'kernel_share_of_hbm_peak': algorithmic / best_k / HBM_PEAK,
                          'torch_TBps': algorithmic / best_t * 1e-12,
                          'largest_difference_kernel_torch': diff}), flush=True)
        del out, ref


if __name__ == '__main__':
    main()
