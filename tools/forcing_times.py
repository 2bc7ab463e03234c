#!/usr/bin/env python3
"""What the forcing path costs on one GPU (default J_time = 6, J_space = 9):

* one apply of B and one of B^T (mpi_kron.ElementKronMatMPI), fused form
  (stk_kron_pack_elem_apply / _t) against the composed one (the row engine's
  stk_ell_spmm per matrix, then the time stage stk_elem_time_apply / _t), alternating
  in one process, device events around `reps` applies (a quarter of a second and more
  per window) after a warm-up, outputs compared;
* the algorithmic bytes of one apply, 24 N M + 4 n_slots + 8 M per direction (the node
  slab once, the test-space slab once -- two columns per element --, the slot stream,
  the ghost pair), as a fraction of the 8 TB/s HBM peak;
* what forcing adds to a solve: forming B^T K g (one multigrid apply on the 2 (N - 1)
  test-space columns and one element pass) and errors(), beside the PCG loop alone of
  the forced problem and of the homogeneous one (`square`) built in the same process
  -- both timed around linalg.PCG on a right-hand side that is already there, so the
  per-iteration figures hold the same work.

Writes one JSON line per figure to stdout; needs a GPU."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'spacetime-fullgrid-parallel_amd'))
import heateq_mpi as hm  # noqa: E402
from source.mpi_kron import ElementKronMatMPI  # noqa: E402
from source.mpi_vector import KronVectorMPI  # noqa: E402

HBM_PEAK = 8e12  # bytes / s


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--reps', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'forcing_times.py measures on a GPU'
    h = hm.HeatEquationMPI(J_space=args.J_space, J_time=args.J_time, problem='square_forced')
    dd, dt = h.dofs_distr, h.dofs_test
    N, M = h.N, h.M
    x = KronVectorMPI(dd)
    x.buf[:, :x.n_loc] = torch.rand((M, x.n_loc), dtype=torch.float64, device=x.buf.device)
    y = KronVectorMPI(dt)
    y.buf.copy_(torch.rand_like(y.buf))
    ops = {'B': (h.B, x, torch.empty_like(y.buf)), 'BT': (h.BT, y, torch.empty_like(x.buf))}
    packed = h.B.fused_plan()
    assert packed is not None, 'no packed plan with a dictionary: nothing to compare'
    n_slots = packed.n_units * packed.K
    alg_bytes = 24 * N * M + 4 * n_slots + 8 * M
    print(json.dumps({'N': N, 'M': M, 'rows_per_unit': packed.rows_per_unit, 'K': packed.K, 'n_slots': n_slots,
                      'algorithmic_bytes': alg_bytes}))
    for name, (op, vec, out) in ops.items():
        results, ms = {}, {'fused': [], 'composed': []}
        for rnd in range(args.rounds + 1):  # round 0: warm-up of both forms
            for form in ('fused', 'composed'):
                ElementKronMatMPI.use_fused = form == 'fused'
                t = timed(lambda: op.apply_buf(vec.buf, None, out), args.reps if rnd else 3)
                if rnd:
                    ms[form].append(t)
                else:
                    results[form] = out.clone()
        ElementKronMatMPI.use_fused = True
        best = {form: min(v) for form, v in ms.items()}
        print(json.dumps({'operator': name, 'ms_fused': ms['fused'], 'ms_composed': ms['composed'],
                          'best_fused_ms': best['fused'], 'best_composed_ms': best['composed'],
                          'fused_over_composed': best['fused'] / best['composed'],
                          'fused_TBps': alg_bytes / best['fused'] * 1e-9,
                          'fused_share_of_hbm_peak': alg_bytes / (best['fused'] * 1e-3) / HBM_PEAK,
                          'composed_share_of_hbm_peak': alg_bytes / (best['composed'] * 1e-3) / HBM_PEAK,
                          'outputs_equal': bool(torch.equal(results['fused'], results['composed']))}))

    # the right-hand side and the solve
    def form_f():
        kg = KronVectorMPI.around(dt, h.Kinv_x.apply(h.g.buf, n_loc=h.g.n_loc))
        return h.BT @ kg

    form_f()
    f_ms = min(timed(form_f, 5) for _ in range(3))
    import time
    from source.linalg import PCG

    def pcg_loop(heat, rhs):
        """(seconds, iterations) of the PCG loop alone, second of two runs."""
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w, iters = PCG(heat.WT_S_W, heat.P, rhs)
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
        return seconds, iters, w

    forced_s, forced_iters, w = pcg_loop(h, h.WT @ h.f)
    u = h.W @ w
    h.errors(u)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    errors = h.errors(u)
    torch.cuda.synchronize()
    errors_s = time.perf_counter() - t0
    del h, ops, x, y, u, w
    torch.cuda.empty_cache()
    plain = hm.HeatEquationMPI(J_space=args.J_space, J_time=args.J_time, problem='square')
    plain_s, plain_iters, _ = pcg_loop(plain, plain.rhs)
    print(json.dumps({'form_BT_K_g_ms': f_ms, 'errors_ms': errors_s * 1e3,
                      'forced_pcg_s': forced_s, 'forced_iterations': forced_iters,
                      'forced_ms_per_iteration': forced_s / forced_iters * 1e3,
                      'homogeneous_pcg_s': plain_s, 'homogeneous_iterations': plain_iters,
                      'homogeneous_ms_per_iteration': plain_s / plain_iters * 1e3,
                      'BT_K_g_over_one_homogeneous_iteration': f_ms / (plain_s / plain_iters * 1e3),
                      'error_alg': errors[0], 'error_Yprime': errors[1]}))


if __name__ == '__main__':
    main()
