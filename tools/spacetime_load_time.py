#!/usr/bin/env python3
"""What the load of a non-separable right-hand side costs on one GPU (default
square_nonseparable at J_time = 6, J_space = 9: 64 time elements x 4 Gauss points = 256
spatial load vectors on 2.1 M triangles x 6 Dunavant points):

* the whole device build of g (assembly.fill_test_space_slab: the callable evaluated with
  torch on the device, then stk_load_columns per time element), wall clock around a
  device synchronise, best of `rounds`;
* its two parts alone, each best of `rounds`: the evaluation of the callable for all
  elements, and the kernels for all elements on values that are already there (device
  events; the values of three elements in turn, more than the Infinity Cache holds);
* the kernels' algorithmic bytes per element -- f read once, the shares written and
  read once, |T| per time point, the incidence lists and the column pair -- over their
  time, as a share of the 8 TB/s HBM peak;
* the same g through space_load on the host threads of libstk with the NumPy form of the
  callable, one call per time point (`--host-points` of them, default all): the only
  route there was before the device engine; and the largest difference of the two slabs.

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
from source.assembly import (DeviceLoadPlan, fill_test_space_slab, free_dofs,  # noqa: E402
                             space_load, tile_row_order, time_rule_test_space)
from source.problem import problem_helper  # noqa: E402

HBM_PEAK = 8e12  # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square_nonseparable')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-points', type=int, default=None, help='time points of the host route (default: all)')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'spacetime_load_time.py measures on a GPU'
    t0 = time.perf_counter()
    mesh_space, _, mesh_time, data, _ = problem_helper(args.problem, J_space=args.J_space, J_time=args.J_time)
    g = data['g'][0]
    n_el, M, nc = mesh_time.nv - 1, len(free_dofs(mesh_space)), len(mesh_space.cells)
    t1 = time.perf_counter()
    order = tile_row_order(mesh_space)
    t2 = time.perf_counter()
    plan = DeviceLoadPlan(mesh_space, row_order=order)
    pts = plan.points()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    d, nq, n_k = plan.d, pts.shape[2], 4
    print(json.dumps({'problem': args.problem, 'time_elements': n_el, 'M': M, 'cells': nc, 'points_per_cell': nq,
                      'time_points_per_element': n_k, 'evaluations_of_g': n_el * n_k * nc * nq,
                      'meshes_s': t1 - t0, 'tile_order_s': t2 - t1, 'plan_and_points_s': t3 - t2}))
    slab = torch.zeros((M, 2 * n_el), dtype=torch.float64, device=_lib.compute_device())

    def whole():
        fill_test_space_slab(plan, mesh_time, g, 0, n_el, slab)

    s, coef = time_rule_test_space(mesh_time)

    def evaluate(e):
        t = torch.from_numpy(mesh_time.h * (e + s)).to(pts.device).reshape(n_k, 1, 1)
        return g(t, *pts)

    def evaluation():
        for e in range(n_el):
            evaluate(e)

    def wall(fn):
        torch.cuda.synchronize()
        begin = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - begin

    whole()  # warm-up: code objects, the allocator's blocks
    build = [wall(whole) for _ in range(args.rounds)]
    evaluation_s = [wall(evaluation) for _ in range(args.rounds)]
    # values of three different elements in turn, 1.2 GB at config 3: no call finds its f in
    # the 256 MB Infinity Cache, as in the real path, where every element's f is new
    fs = [evaluate(e).contiguous() for e in (0, n_el // 2, n_el - 1)]
    scratch = torch.zeros_like(slab)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernels = []
    for _ in range(args.rounds + 1):
        e0.record()
        for e in range(n_el):
            plan.columns(fs[e % 3], coef, scratch, e)
        e1.record()
        e1.synchronize()
        kernels.append(e0.elapsed_time(e1) * 1e-3)
    kernels = kernels[1:]
    ns = (d + 1) * nc
    per_element = 8 * n_k * nc * nq + 2 * 8 * n_k * ns + 8 * n_k * nc + 4 * ns + 8 * M + 16 * M
    best_k = min(kernels)
    print(json.dumps({'device_build_s': build, 'best_device_build_s': min(build),
                      'evaluation_s': evaluation_s, 'best_evaluation_s': min(evaluation_s),
                      'kernels_s': kernels, 'best_kernels_s': best_k,
                      'kernels_ms_per_element': best_k / n_el * 1e3,
                      'kernel_bytes_per_element': per_element,
                      'kernels_TBps': per_element * n_el / best_k * 1e-12,
                      'kernels_share_of_hbm_peak': per_element * n_el / best_k / HBM_PEAK}))

    # the host route: one space_load per time point, NumPy form of the callable
    n_host = n_el * n_k if args.host_points is None else min(args.host_points, n_el * n_k)
    times = (mesh_time.h * (np.arange(n_el)[:, None] + s[None, :])).reshape(-1)
    host = np.zeros((2 * n_el, M))
    begin = time.perf_counter()
    for j in range(n_host):
        L = space_load(mesh_space, lambda *x: g(times[j], *x))
        e, k = divmod(j, n_k)
        host[2 * e:2 * e + 2] += coef[k][:, None] * L[None, :]
        if (j + 1) % 32 == 0:
            print('host route: %d of %d time points, %.1f s' % (j + 1, n_host, time.perf_counter() - begin),
                  file=sys.stderr, flush=True)
    host_s = time.perf_counter() - begin
    rows = 2 * (n_host // n_k)
    record = {'host_time_points': n_host, 'host_s': host_s, 'host_s_per_time_point': host_s / n_host,
              'host_s_for_all_time_points': host_s / n_host * n_el * n_k,
              'host_over_device_build': host_s / n_host * n_el * n_k / min(build)}
    if rows:
        whole()
        dev = slab.t()[:rows].cpu().numpy()
        record['largest_difference_over_largest_entry'] = float(np.max(np.abs(dev - host[:rows])) / np.max(np.abs(host[:rows])))
    print(json.dumps(record))


if __name__ == '__main__':
    main()
