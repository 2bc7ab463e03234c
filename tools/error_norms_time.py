#!/usr/bin/env python3
"""What the error norms against an exact solution cost on one GPU (default:
square_nonseparable at J_time = 6, J_space = 9 -- 2 097 152 triangles, a slab of 1 046 529
rows by 65 time nodes, 64 time elements of 4 Gauss points):

* the construction of the plan (mesh upload, |T| and the gradients on the device), wall clock;
* the whole error_norms call (device events, one warm-up, best and median of `rounds`);
* torch's evaluation of exact and exact_grad at the quadrature points for all elements
  alone -- its share of the call;
* stk_err_element for one element on values already there (the two launches), with and
  without the gradient;
* the SAME four sums composed from torch on the device, on the same values: the d + 1 rows of
  every cell by index_select, the weighted sums in the kernel's order, sum() over the cells
  -- what a user would write without the kernel; timed in the same process, the two forms
  taking turns (rounds interleaved), and compared.

Algorithmic bytes of one element = f and gf read once (8 n_k (1 + d) nc nq) + the d + 1 row
entries of every cell at both time nodes (16 (d + 1) nc) + |T| (8 nc) + the gradients
(8 (d + 1) d nc) + the cells (4 (d + 1) nc), over the best time, in TB/s and as a share of
the 8 TB/s HBM peak.  f alone (403 MB) is larger than the 256 MB Infinity Cache.

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
from source.error_norms import ErrorPlan, error_norms_collective, evaluate_exact, time_rule  # noqa: E402
from source.linop import self_distribution  # noqa: E402
from source.mpi_vector import KronVectorMPI  # noqa: E402
from source.problem import problem_helper  # noqa: E402

HBM_PEAK = 8e12  # bytes / s


def torch_element(rows, vol, grad, qw, ql, w_lo, w_hi, c, f, gf, lo, hi):
    """The four sums from torch alone: rows (nc, d + 1) int64 slab rows of the cells'
    vertices (-1: boundary), lo / hi contiguous (M,) rows of the two time nodes."""
    free = rows >= 0
    zero = torch.zeros((), dtype=lo.dtype, device=lo.device)
    lo_c = torch.where(free, lo.index_select(0, rows.clamp(min=0).reshape(-1)).reshape(rows.shape), zero)
    hi_c = torch.where(free, hi.index_select(0, rows.clamp(min=0).reshape(-1)).reshape(rows.shape), zero)
    acc = torch.zeros(4, dtype=lo.dtype, device=lo.device)
    for k in range(len(c)):
        U = w_lo[k] * lo_c + w_hi[k] * hi_c  # (nc, d + 1)
        e = f[k] - U @ ql.t()  # (nc, nq)
        parts = [((e * e * qw).sum(dim=1) * vol).sum(), zero, ((f[k] * f[k] * qw).sum(dim=1) * vol).sum(), zero]
        if gf is not None:
            G = torch.einsum('ca,caj->jc', U, grad)  # (d, nc)
            eg = gf[k] - G[:, :, None]
            parts[1] = ((eg * eg * qw).sum(dim=(0, 2)) * vol).sum()
            parts[3] = ((gf[k] * gf[k] * qw).sum(dim=(0, 2)) * vol).sum()
        acc = acc + c[k] * torch.stack(parts)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square_nonseparable')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'error_norms_time.py measures on a GPU'
    t0 = time.perf_counter()
    mesh_space, _, mesh_time, data, _ = problem_helper(args.problem, J_space=args.J_space, J_time=args.J_time)
    exact, exact_grad = data['exact'], data['exact_grad']
    N, M, d = mesh_time.nv, len(free_dofs(mesh_space)), mesh_space.points.shape[1]
    nc = len(mesh_space.cells)
    t1 = time.perf_counter()
    plan = ErrorPlan(mesh_space, mesh_time)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    nq = len(plan.qw)
    print(json.dumps({'problem': args.problem, 'N': N, 'M': M, 'cells': nc, 'nq': nq, 'meshes_s': t1 - t0,
                      'plan_s': t2 - t1}), flush=True)

    dev = _lib.compute_device()
    # the interpolant of the exact solution plus a perturbation: an error of realistic size
    pts = mesh_space.points[free_dofs(mesh_space)]
    nodes = mesh_time.h * np.arange(N)
    U = exact(nodes[:, None], *(pts[None, :, k] for k in range(d))) * (1.0 + 1e-3 * np.random.RandomState(1).rand(N, M))
    vec = KronVectorMPI(self_distribution(N, M), U)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    def stats(label, seconds, **more):
        rec = {label + '_s': seconds, 'best_' + label + '_s': min(seconds), 'median_' + label + '_s': float(np.median(seconds))}
        rec.update(more)
        print(json.dumps(rec), flush=True)
        return min(seconds)

    s, c = time_rule(mesh_time)

    def evaluate_all():
        for e in range(N - 1):
            evaluate_exact(plan, exact, exact_grad, mesh_time.h * (e + s))

    whole = lambda: error_norms_collective(plan, vec, exact, exact_grad)
    whole(), evaluate_all()  # warm-up: code objects, the allocator's blocks, the points
    whole_s, eval_s = [], []
    for _ in range(args.rounds):
        whole_s.append(timed(whole)[0])
        eval_s.append(timed(evaluate_all)[0])
    norms = whole()
    best_whole = stats('error_norms', whole_s, elements=N - 1,
                       norms={k: v for k, v in norms.items() if k not in ('per_element', 'l2_at')},
                       l2_at=norms['l2_at'].tolist())
    best_eval = stats('torch_evaluation_of_exact', eval_s)
    print(json.dumps({'share_of_torch_evaluation': best_eval / best_whole,
                      'rest_per_element_s': (best_whole - best_eval) / (N - 1)}), flush=True)

    # one element on values already there: the kernel and the torch composition take turns
    e = (N - 1) // 2
    f, gf = evaluate_exact(plan, exact, exact_grad, mesh_time.h * (e + s))
    lo, hi = vec.buf[:, e].contiguous(), vec.buf[:, e + 1].contiguous()
    cells = _lib.to_dev(np.ascontiguousarray(mesh_space.cells, dtype=np.int64))
    row_of = np.full(mesh_space.nv, -1, dtype=np.int64)
    row_of[free_dofs(mesh_space)] = np.arange(M)
    rows = _lib.to_dev(row_of)[cells]
    from source.assembly import _simplex_geometry
    vol_h, grad_h = _simplex_geometry(mesh_space)
    vol, grad = _lib.to_dev(vol_h), _lib.to_dev(grad_h)
    qw_d, ql_d = _lib.to_dev(plan.qw), _lib.to_dev(plan.ql)
    w_lo_d, w_hi_d, c_d = _lib.to_dev(1.0 - s), _lib.to_dev(s), _lib.to_dev(c)
    out4 = torch.zeros(4, dtype=torch.float64, device=dev)
    base = vec.buf.data_ptr()
    for label, g in (('with_gradient', gf), ('without_gradient', None)):
        kernel = lambda: plan.element(f, g, 1.0 - s, s, c, base + 8 * e, vec.ld, base + 8 * (e + 1), vec.ld, out4)
        composed = lambda: torch_element(rows, vol, grad, qw_d, ql_d, w_lo_d, w_hi_d, c_d, f, g, lo, hi)
        kernel(), composed()
        k_s, t_s = [], []
        for _ in range(args.rounds):
            k_s.append(timed(kernel)[0])
            t_s.append(timed(composed)[0])
        ref = composed()
        rel = float(((out4 - ref).abs() / ref.abs().clamp(min=1e-300)).max())
        algorithmic = (8 * len(c) * (1 + (d if g is not None else 0)) * nc * nq + 16 * (d + 1) * nc + 8 * nc
                       + (8 * (d + 1) * d * nc if g is not None else 0) + 4 * (d + 1) * nc)
        best_k, best_t = min(k_s), min(t_s)
        print(json.dumps({'case': label, 'kernel_s': k_s, 'torch_s': t_s, 'best_kernel_s': best_k,
                          'median_kernel_s': float(np.median(k_s)), 'best_torch_s': best_t,
                          'median_torch_s': float(np.median(t_s)), 'torch_over_kernel': best_t / best_k,
                          'algorithmic_bytes': algorithmic, 'kernel_TBps': algorithmic / best_k * 1e-12,
                          'kernel_share_of_hbm_peak': algorithmic / best_k / HBM_PEAK,
                          'torch_TBps': algorithmic / best_t * 1e-12,
                          'largest_relative_difference_kernel_torch': rel, 'out4': out4.tolist()}), flush=True)


if __name__ == '__main__':
    main()
