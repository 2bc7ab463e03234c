#!/usr/bin/env python3
"""What the adjoint of trajectory sampling costs on one GPU (default: square_moving_source
at J_time = 6, J_space = 9 -- a slab of 1 046 529 rows by 65 time nodes, 552 MB -- and 2^20
pairs (t_p, x_p)), in the two orders of tools/sample_along_time.py:

* ``trajectory``: times ascending from 0 to T, points on the path of the moving source with
  Gaussian scatter 0.1;
* ``random``: times uniform in [0, T], points uniform in the bounding box.

For field 'u' and field 'grad', three forms of E^T w on the SAME located points, taking
turns in one process after a warm-up:

* ``kernel``: SamplePlan.adjoint_pairs (stk_sample_pairs_adjoint): zero fill, one record
  per term, a stable sort by destination, one summing pass; device events around `reps`
  calls, best and median of `rounds`;
* ``atomic``: the terms from torch on the device and one
  ``index_put_(accumulate=True)`` -- what a user would write;
* ``deterministic``: the same under ``torch.use_deterministic_algorithms(True)``.

There is no speed gate: the times are reported as they fall.  What the kernel buys is
the contract -- every entry a sum of one fixed order -- so per case the log also has: the
longest destination list and the number of entries with terms; the largest difference of
each torch form to the kernel, over max |kernel|; and, over `repeats` fresh runs of each
form on the same input, how many reproduced the first run bit for bit.

Writes one JSON line per figure to stdout; needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'spacetime-fullgrid-parallel_amd'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sample_along_time import ORDERS, pairs_of  # noqa: E402

FIELDS = ('u', 'grad')


def torch_terms(torch, rows, lam, coeffs, w, times, h, N, ld, field, dump):
    """(destinations, terms) of every pair, flat in the order p, a, b: destinations index
    the flat slab (row ld + column); a term that is dropped -- an unused pair, a boundary
    vertex -- goes with the value 0 to the padding column of its row (odd N) or to the entry
    `dump` behind the slab.  rows (n_p, d + 1) int64 slab rows
    of the vertices (-1: boundary; -2: the pair is outside the mesh)."""
    used = ~(rows == -2).any(dim=1) & (times >= 0.0) & (times <= (N - 1) * h)  # a NaN time fails both
    x = torch.where(used, times, torch.zeros_like(times)) / h
    e = torch.clamp(torch.floor(x), max=N - 2)
    w1 = x - e
    wa = torch.stack([1.0 - w1, w1], dim=1)  # (n_p, 2)
    if field == 'grad':
        q = w[0][:, None] * coeffs[0]
        for j in range(1, w.shape[0]):
            q = q + w[j][:, None] * coeffs[j]
        terms = wa[:, :, None] * q[:, None, :]
    else:
        terms = (w[:, None] * wa)[:, :, None] * lam[:, None, :]
    keep = (used[:, None] & (rows >= 0))[:, None, :].expand(-1, 2, -1)
    at = rows.clamp(min=0)[:, None, :] * ld + (e.long()[:, None] + torch.arange(2, device=rows.device)[None, :])[:, :, None]
    if ld > N:  # spread over the padding column, so that the atomic form meets no hot spot of zeros
        spare = (rows.clamp(min=0) * ld + (ld - 1))[:, None, :].expand(-1, 2, -1)
    else:
        spare = torch.full_like(at, dump)
    at = torch.where(keep, at, spare)
    terms = torch.where(keep, terms, torch.zeros_like(terms))
    return at.reshape(-1), terms.reshape(-1), keep.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square_moving_source')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--pairs', type=int, default=1 << 20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3, help='calls per timed round')
    ap.add_argument('--repeats', type=int, default=5, help='fresh runs per form for the reproducibility count')
    args = ap.parse_args()

    import torch
    from source import _lib
    from source.assembly import free_dofs
    from source.linop import self_distribution
    from source.mpi_vector import KronVectorMPI
    from source.problem import problem_helper
    from source.sampling import SamplePlan
    assert torch.cuda.is_available(), 'sample_adjoint_time.py measures on a GPU'
    t0 = time.perf_counter()
    mesh_space, _, mesh_time, data, _ = problem_helper(args.problem, J_space=args.J_space, J_time=args.J_time)
    assert 'path' in data, 'the trajectory order follows the path of the problem: %s has none' % args.problem
    N, M, d = mesh_time.nv, len(free_dofs(mesh_space)), mesh_space.points.shape[1]
    plan = SamplePlan(mesh_space, mesh_time)
    torch.cuda.synchronize()
    n_p, h = args.pairs, float(mesh_time.h)
    dev = _lib.compute_device()
    distr = self_distribution(N, M)
    out = KronVectorMPI(distr)
    ld = out.ld
    print(json.dumps({'problem': args.problem, 'N': N, 'M': M, 'cells': len(mesh_space.cells), 'pairs': n_p,
                      'records': 2 * (d + 1) * n_p, 'slab_bytes': 8 * M * ld, 'rounds': args.rounds, 'reps': args.reps,
                      'repeats': args.repeats, 'setup_s': time.perf_counter() - t0}), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / args.reps

    cells = _lib.to_dev(np.ascontiguousarray(mesh_space.cells, dtype=np.int64))
    row_of = np.full(mesh_space.nv, -1, dtype=np.int64)
    row_of[free_dofs(mesh_space)] = np.arange(M)
    row_of = _lib.to_dev(row_of)
    flat = torch.zeros(M * ld + 1, dtype=torch.float64, device=dev)  # the torch forms' slab and the dump entry
    for order in ORDERS:
        times, points = pairs_of(order, n_p, mesh_space, mesh_time, data['path'])
        t_dev = torch.from_numpy(times).to(dev)
        loc = plan.locate(torch.from_numpy(points).to(dev))
        inside = int(loc.inside.sum())
        rows = torch.where(loc.inside[:, None], row_of[cells[loc.cell.long().clamp(min=0)]],
                           torch.full((1, 1), -2, dtype=torch.int64, device=dev))
        coeffs = plan.grad_coeffs(loc)
        rs = np.random.RandomState(9)
        for field in FIELDS:
            w = torch.from_numpy(rs.randn(d, n_p) if field == 'grad' else rs.randn(n_p)).to(dev)

            def kernel():
                return plan.adjoint_pairs(distr, w, t_dev, loc, field=field, out=out)[0]

            def scatter(deterministic):
                torch.use_deterministic_algorithms(deterministic)
                try:
                    at, terms, _ = torch_terms(torch, rows, loc.lam, coeffs, w, t_dev, h, N, ld, field, M * ld)
                    flat.zero_()
                    flat.index_put_((at,), terms, accumulate=True)
                finally:
                    torch.use_deterministic_algorithms(False)
                return flat

            at, _, keep = torch_terms(torch, rows, loc.lam, coeffs, w, t_dev, h, N, ld, field, M * ld)
            counts = torch.bincount(at[keep], minlength=1)
            longest, entries = int(counts.max()), int((counts > 0).sum())
            del at, keep, counts
            kernel(), scatter(False), scatter(True)  # warm-up
            k_s, a_s, d_s = [], [], []
            for _ in range(args.rounds):  # the forms take turns
                k_s.append(timed(kernel))
                a_s.append(timed(lambda: scatter(False)))
                d_s.append(timed(lambda: scatter(True)))
            ref = kernel().buf.reshape(-1).clone()
            scale = float(ref.abs().max())
            same, diff = {}, {}
            for name, fn in (('kernel', lambda: kernel().buf.reshape(-1)), ('atomic', lambda: scatter(False)[:M * ld]),
                             ('deterministic', lambda: scatter(True)[:M * ld])):
                first = fn().clone()
                same[name] = sum(int(torch.equal(fn(), first)) for _ in range(args.repeats))
                diff[name] = float((first - ref).abs().max()) / scale
            best = {'kernel': min(k_s), 'atomic': min(a_s), 'deterministic': min(d_s)}
            print(json.dumps({'case': order, 'field': field, 'points_inside': inside, 'entries_with_terms': entries,
                              'longest_destination_list': longest, 'kernel_s': k_s, 'atomic_s': a_s, 'deterministic_s': d_s,
                              'best_s': best, 'median_s': {'kernel': float(np.median(k_s)), 'atomic': float(np.median(a_s)),
                                                           'deterministic': float(np.median(d_s))},
                              'ns_per_pair': {k: v / n_p * 1e9 for k, v in best.items()},
                              'atomic_over_kernel': best['atomic'] / best['kernel'],
                              'deterministic_over_kernel': best['deterministic'] / best['kernel'],
                              'repeats_equal_to_the_first_run': same, 'repeats': args.repeats,
                              'largest_difference_to_kernel_over_max': diff}), flush=True)


if __name__ == '__main__':
    main()
