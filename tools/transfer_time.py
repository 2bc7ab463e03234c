#!/usr/bin/env python3
"""What the level transfer costs and what nesting saves, on one GPU (default: J_time = 6,
J_space = 9 -- a fine slab of 1 046 529 rows by 65 time nodes, 553 MB with its pad column):

* stk_transfer_prolong for (time levels a, space levels) = (1, 1), (0, 1), (1, 0) into the fine
  slab (device events, one warm-up, best of `rounds` with the median beside it), for the tile
  shapes of the kernel (stk_transfer_tile: fine rows per workgroup);
* the SAME doubles composed from torch -- two index_select of the parents' rows, the masks of
  the boundary, add, halve, and the strided interleaving writes in time -- timed in the same
  process, the forms taking turns (rounds interleaved), and checked equal entry for entry;
* copy_ and zero_ of a tensor of the fine slab's size in the same run: the stream yardsticks;
* (--solves 1) the moving source and square_forced solved with --nested 0, 1, 2: iterations per
  level, solve time (prolongations included), set-up time of the extra levels, and the error
  norms where the problem has an exact solution.

Algorithmic bytes of a transfer = the coarse slab read once + the fine columns written once.

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

TILES = ((64, 64), (128, 64), (256, 64), (64, 8))  # (rows per workgroup, LDS per workgroup in KiB)
CASES = ((1, 1), (0, 1), (1, 0))  # (time levels a, space levels)


def torch_composition(parents, a, uc, out):
    """The contract of the level transfer from torch alone: `parents` (M_f, 2) int64 device
    tensor, `uc` (M_c, N_c) the coarse columns 0 .. N_c - 1, into the columns
    0 .. 2^a (N_c - 1) of `out` (M_f, ld).  Every product and sum is a kernel of its own, so
    the roundings are the contract's."""
    p0, p1 = parents[:, 0], parents[:, 1]
    zero = torch.zeros((), dtype=uc.dtype, device=uc.device)
    if uc.shape[0] == 0:
        s = torch.zeros((len(parents), uc.shape[1]), dtype=uc.dtype, device=uc.device)
    else:
        A = torch.where((p0 >= 0)[:, None], uc.index_select(0, p0.clamp(min=0)), zero)
        B = torch.where((p1 >= 0)[:, None], uc.index_select(0, p1.clamp(min=0)), zero)
        s = torch.where(((p0 == p1) & (p0 >= 0))[:, None], A, (A + B) * 0.5)
    n_fine = ((uc.shape[1] - 1) << a) + 1
    out[:, 0:n_fine:1 << a] = s
    for rem in range(1, 1 << a):
        w1 = rem / 2.0**a
        w0 = 1.0 - w1
        out[:, rem:n_fine:1 << a] = w0 * s[:, :-1] + w1 * s[:, 1:]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--solves', type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'transfer_time.py measures on a GPU'
    from source import _lib
    from source.problem import problem_helper
    from source.transfer import TransferPlan, identity_rows, parent_rows, prolong_window

    dev = _lib.compute_device()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    fine = problem_helper(args.problem, J_space=args.J_space, J_time=args.J_time)[0:3:2]
    N_f = fine[1].nv
    ld = N_f + (N_f & 1)
    out = other = None
    for a, s in CASES:
        coarse = problem_helper(args.problem, J_space=args.J_space - s, J_time=args.J_time - a)[0:3:2]
        plan = TransferPlan(coarse, fine)
        M_f, M_c, N_c = plan.M_fine, plan.M_coarse, plan.N_coarse
        if out is None:
            out = torch.empty((M_f, ld), dtype=torch.float64, device=dev)
            other = torch.empty((M_f, ld), dtype=torch.float64, device=dev)
        uc = torch.randn((M_c, N_c), dtype=torch.float64, device=dev)
        table = torch.from_numpy((parent_rows(fine[0]) if s else identity_rows(M_f)).astype(np.int64)).to(dev)
        algorithmic = 8 * M_c * N_c + 8 * M_f * N_f
        print(json.dumps({'case': 'shape', 'a': a, 'space_levels': s, 'M_fine': M_f, 'M_coarse': M_c, 'N_fine': N_f,
                          'N_coarse': N_c, 'fine_slab_MB': 8e-6 * M_f * ld, 'algorithmic_bytes': algorithmic}),
              flush=True)

        def kernel(tile):
            _lib.check(_lib.lib().stk_transfer_tile(*tile))
            return prolong_window(plan, uc, N_c, N_c, out, ld, 0, N_f)

        composed = lambda: torch_composition(table, a, uc, other)  # noqa: E731
        for tile in TILES:
            kernel(tile)
        composed()
        k_s, t_s, c_s, z_s = {tile: [] for tile in TILES}, [], [], []
        for _ in range(args.rounds):  # the forms take turns
            for tile in TILES:
                k_s[tile].append(timed(lambda: kernel(tile))[0])
            t_s.append(timed(composed)[0])
        kernel((0, 0))
        equal = bool(torch.equal(out[:, :N_f], other[:, :N_f]))
        for _ in range(args.rounds):  # the stream yardsticks of the same run
            c_s.append(timed(lambda: other.copy_(out))[0])
            z_s.append(timed(lambda: other.zero_())[0])
        best_t, best_c, best_z = min(t_s), min(c_s), min(z_s)
        for tile in TILES:
            best_k = min(k_s[tile])
            print(json.dumps({'case': 'transfer', 'a': a, 'space_levels': s, 'tile_rows': tile[0],
                              'tile_lds_KiB': tile[1], 'best_kernel_s': best_k,
                              'median_kernel_s': float(np.median(k_s[tile])), 'kernel_TBps': algorithmic / best_k * 1e-12,
                              'best_torch_s': best_t, 'median_torch_s': float(np.median(t_s)),
                              'torch_over_kernel': best_t / best_k, 'best_copy_s': best_c, 'best_zero_s': best_z,
                              'copy_TBps': 16 * M_f * ld / best_c * 1e-12, 'zero_TBps': 8 * M_f * ld / best_z * 1e-12,
                              'kernel_over_zero': best_k / best_z, 'kernel_over_copy': best_k / best_c}), flush=True)
        print(json.dumps({'case': 'transfer', 'a': a, 'space_levels': s,
                          'kernel_equals_composition_entry_for_entry': equal}), flush=True)
        assert equal
        del plan, uc, table
    del out, other
    torch.cuda.empty_cache()
    if args.solves:
        solves(args)


def solves(args):
    """--nested 0, 1, 2 on the moving source and on square_forced: one JSON line each."""
    import heateq_mpi as hm
    from source import driver
    from source.comm import Comm
    comm = Comm(distributed=False)
    for problem in ('square_moving_source', 'square_forced'):
        build = lambda J_time, J_space: hm.HeatEquationMPI(J_space=J_space, J_time=J_time, problem=problem,  # noqa: E731
                                                           comm=comm)
        heat = build(args.J_time, args.J_space)
        heat.solve(kmax=3)  # warm-up: code objects, workspaces
        for nested in (0, 1, 2):
            set_up = solve = 0.0
            before, u, counts = None, None, []
            for level in driver.nested_levels(args.J_time, args.J_space, nested) + [None]:
                torch.cuda.synchronize()
                began = time.perf_counter()
                this = heat if level is None else build(*level)
                torch.cuda.synchronize()
                set_up += time.perf_counter() - began
                began = time.perf_counter()
                x0 = None if before is None else this.prolong_from(before, u)
                u, iters = this.solve(x0=x0)
                torch.cuda.synchronize()
                solve += time.perf_counter() - began
                counts.append(iters)
                before = this
            line = {'case': 'nested', 'problem': problem, 'nested': nested, 'iterations_coarsest_first': counts,
                    'solve_s': solve, 'set_up_of_extra_levels_s': set_up}
            if heat._exact[0] is not None:
                norms = heat.error_norms(u)
                line.update(l2_l2=norms['l2_l2'], l2_h1=norms['l2_h1'])
            print(json.dumps(line), flush=True)
            del before, u
        del heat
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
