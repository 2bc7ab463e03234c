#!/usr/bin/env python3
"""What the restriction P^T costs on one GPU (default: J_time = 6, J_space = 9 -- a fine slab of
1 046 529 rows by 65 time nodes, 553 MB with its pad column):

* stk_transfer_restrict for (time levels a, space levels) = (1, 1), (0, 1), (1, 0) from the fine
  slab (device events, one warm-up, best of `rounds` with the median beside it), for the tile
  shapes of the kernel (stk_restrict_tile: coarse rows per workgroup, LDS per workgroup);
* the composition from torch -- a sparse CSR product with P_x^T, then a dense product with
  P_t^T -- timed in the same process, the forms taking turns (rounds interleaved), and compared
  entrywise within K 2^-53 (|P|^T |f|), K = the terms of the longest sum plus two (its
  summation order is not the kernel's);
* copy_ of a tensor of the fine slab's size and stk_transfer_prolong for the same pair in the
  same run: the yardsticks.

Bytes the kernel must move = the fine slab read once + the coarse slab written once.

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

TILES = ((16, 64), (32, 64), (64, 64), (128, 64), (32, 16))  # (coarse rows per workgroup, LDS per workgroup in KiB)
CASES = ((1, 1), (0, 1), (1, 0))  # (time levels a, space levels)


def space_matrix_T(parents, M_c, device):
    """P_x^T (M_c, M_f) of a parents table (NumPy, (M_f, 2)) as a torch sparse CSR tensor."""
    import scipy.sparse as sp
    parents = np.asarray(parents, dtype=np.int64)
    rows, cols, vals = [], [], []
    copy = (parents[:, 0] == parents[:, 1]) & (parents[:, 0] >= 0)
    idx = np.flatnonzero(copy)
    rows.append(parents[idx, 0]), cols.append(idx), vals.append(np.ones(len(idx)))
    for side in (0, 1):
        idx = np.flatnonzero(~copy & (parents[:, side] >= 0) & (parents[:, 0] != parents[:, 1]))
        rows.append(parents[idx, side]), cols.append(idx), vals.append(np.full(len(idx), 0.5))
    mat = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                        shape=(M_c, len(parents)))
    mat.sort_indices()
    return torch.sparse_csr_tensor(torch.from_numpy(mat.indptr.astype(np.int64)),
                                   torch.from_numpy(mat.indices.astype(np.int64)), torch.from_numpy(mat.data),
                                   size=mat.shape, dtype=torch.float64, device=device)


def time_matrix_T(a, N_c, device):
    """P_t^T as the dense (N_f, N_c) right factor: entry (k, q) is the weight of the fine node k
    in the stencil of the coarse node q."""
    N_f = ((N_c - 1) << a) + 1
    mat = np.zeros((N_f, N_c))
    for q in range(N_c):
        for k in range(max(0, ((q - 1) << a) + 1), min(N_f - 1, ((q + 1) << a) - 1) + 1):
            mat[k, q] = 1.0 - abs(k - (q << a)) / 2.0**a
    return torch.from_numpy(mat).to(device)


def torch_composition(PxT, PtT, f):
    """P^T f from torch alone: `f` (M_f, N_f) -> (M_c, N_c); PxT None: time only."""
    g = f if PxT is None else torch.sparse.mm(PxT, f)
    return g @ PtT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'restrict_time.py measures on a GPU'
    from source import _lib
    from source.problem import problem_helper
    from source.transfer import TransferPlan, parent_rows, prolong_window, restrict_window

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
    f = other = None
    for a, s in CASES:
        coarse = problem_helper(args.problem, J_space=args.J_space - s, J_time=args.J_time - a)[0:3:2]
        plan = TransferPlan(coarse, fine)
        M_f, M_c, N_c = plan.M_fine, plan.M_coarse, plan.N_coarse
        if f is None:
            f = torch.randn((M_f, ld), dtype=torch.float64, device=dev)
            other = torch.empty((M_f, ld), dtype=torch.float64, device=dev)
        ldc = N_c + (N_c & 1)
        out = torch.zeros((M_c, ldc), dtype=torch.float64, device=dev)
        uc = torch.randn((M_c, N_c), dtype=torch.float64, device=dev)
        table = parent_rows(fine[0]) if s else None
        PxT = space_matrix_T(table, M_c, dev) if s else None
        PtT = time_matrix_T(a, N_c, dev)
        longest = (int(np.diff(PxT.crow_indices().cpu().numpy()).max()) if s else 1) * ((2 << a) - 1)
        must_move = 8 * M_f * N_f + 8 * M_c * N_c
        print(json.dumps({'case': 'shape', 'a': a, 'space_levels': s, 'M_fine': M_f, 'M_coarse': M_c, 'N_fine': N_f,
                          'N_coarse': N_c, 'fine_slab_MB': 8e-6 * M_f * ld, 'bytes_the_kernel_must_move': must_move,
                          'entries_of_the_transposed_table': int(PxT._nnz()) if s else M_f,
                          'terms_of_the_longest_sum': longest}), flush=True)
        f_cols = f[:, :N_f]

        def kernel(tile):
            _lib.check(_lib.lib().stk_restrict_tile(*tile))
            return restrict_window(plan, f, ld, 0, N_f, out, ldc, 0, N_c)

        composed = lambda: torch_composition(PxT, PtT, f_cols)  # noqa: E731
        prolonged = lambda: prolong_window(plan, uc, N_c, N_c, other, ld, 0, N_f)  # noqa: E731
        for tile in TILES:
            kernel(tile)
        ref = composed()
        prolonged()
        k_s, t_s, c_s, p_s = {tile: [] for tile in TILES}, [], [], []
        for _ in range(args.rounds):  # the forms take turns
            for tile in TILES:
                k_s[tile].append(timed(lambda: kernel(tile))[0])
            t_s.append(timed(composed)[0])
            p_s.append(timed(prolonged)[0])
            c_s.append(timed(lambda: other.copy_(f))[0])
        kernel((0, 0))
        size = torch_composition(PxT, PtT, f_cols.abs())  # every weight is positive: |P|^T |f|
        gap = float(((out[:, :N_c] - ref).abs() / size).max())
        bound = (longest + 2) * 2.0**-53
        best_t, best_c, best_p = min(t_s), min(c_s), min(p_s)
        for tile in TILES:
            best_k = min(k_s[tile])
            print(json.dumps({'case': 'restrict', 'a': a, 'space_levels': s, 'tile_rows': tile[0],
                              'tile_lds_KiB': tile[1], 'best_kernel_s': best_k,
                              'median_kernel_s': float(np.median(k_s[tile])), 'kernel_TBps': must_move / best_k * 1e-12,
                              'best_torch_s': best_t, 'median_torch_s': float(np.median(t_s)),
                              'torch_over_kernel': best_t / best_k, 'best_copy_s': best_c,
                              'copy_TBps': 16 * M_f * ld / best_c * 1e-12, 'best_prolong_s': best_p,
                              'kernel_over_copy': best_k / best_c, 'kernel_over_prolong': best_k / best_p}), flush=True)
        print(json.dumps({'case': 'restrict', 'a': a, 'space_levels': s, 'largest_gap_over_size': gap,
                          'bound_K_2^-53': bound}), flush=True)
        assert gap <= bound, (gap, bound)
        del plan, out, uc, PxT, PtT, ref, size
    del f, other
    torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
