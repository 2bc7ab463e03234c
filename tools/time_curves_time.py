#!/usr/bin/env python3
"""What the time curves cost on one GPU (default: the square at J_time = 6, J_space = 9 -- a
slab of 1 046 529 rows by 65 time nodes, 2 097 152 cells):

* the call: stk_curves_eval on the whole slab with a threshold (device events, one warm-up,
  best of `rounds` with the median beside it), for several column chunks (stk_curves_tile);
* its two kernels, cells and finish, from one profiled call (torch.profiler; left out with a
  note where the profiler does not see the library's launches);
* the SAME sums composed from torch -- what a user would write without the kernel:
  index_select of the cells' rows into an (nc, d + 1, N) temporary, then the weighted sums
  for heat, l2_sq, h1_sq and outflow -- and the extrema (peak, peak_row) separately, timed in
  the same process, the forms taking turns, and compared entry by entry.  The composition
  has no zone fields: the kernel computes more;
* the call once more on a field like a solution's (a moving bump: few cut cells), where the
  `randn` data above makes every cell a cut cell.

Algorithmic bytes of the call = the slab read once (8 M ld) + the cell tables once per column
chunk + the tile partials written and read once, over the best time, in TB/s and as a share
of the 8 TB/s HBM peak of the MI355X.

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

CHUNKS = (8, 1, 2, 4, 16, 32)  # columns a workgroup takes in turn: stk_curves_tile
HBM_PEAK_TBPS = 8.0


class Composition:
    """The mesh tables of the torch composition, on the device of `like`."""
    def __init__(self, mesh, like):
        from source.assembly import _simplex_geometry, free_dofs
        from source.time_curves import boundary_faces
        cells = np.ascontiguousarray(mesh.cells, dtype=np.int64)
        self.nc, self.d = len(cells), cells.shape[1] - 1
        fd = np.asarray(free_dofs(mesh), dtype=np.int64)
        row_of = np.full(mesh.nv, -1, dtype=np.int64)
        row_of[fd] = np.arange(len(fd))
        rows = row_of[cells]
        vol, grad = _simplex_geometry(mesh)
        faces = boundary_faces(cells)
        bits = ((faces[:, None] >> np.arange(self.d + 1)) & 1).astype(np.float64)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(like.device)
        self.rows = dev(np.maximum(rows, 0).reshape(-1))
        self.free = dev((rows >= 0).astype(np.float64))
        self.vol, self.grad, self.bits = dev(np.asarray(vol, dtype=np.float64)), dev(np.asarray(grad, dtype=np.float64)), dev(bits)

    def sums(self, v):
        """heat, l2_sq, h1_sq, outflow of the columns of `v` (M, n), a view buf[:, :n_loc]."""
        d, n = self.d, v.shape[1]
        U = v.index_select(0, self.rows).reshape(self.nc, d + 1, n) * self.free[:, :, None]
        S = U.sum(dim=1)
        w = self.vol[:, None]
        heat = (w * S).sum(dim=0) / (d + 1)
        l2 = (w * (S * S + (U * U).sum(dim=1))).sum(dim=0) / ((d + 1) * (d + 2))
        G = torch.einsum('tan,taj->tjn', U, self.grad)
        h1 = (w * (G * G).sum(dim=1)).sum(dim=0)
        dots = torch.einsum('tjn,taj->tan', G, self.grad)
        outflow = (d * w * (self.bits[:, :, None] * dots).sum(dim=1)).sum(dim=0)
        return {'heat': heat, 'l2_sq': l2, 'h1_sq': h1, 'outflow': outflow}

    @staticmethod
    def extrema(v):
        """peak and the LOWEST row that has it (torch.max names one of them, not the lowest)."""
        peak = v.max(dim=0).values
        index = torch.arange(v.shape[0], device=v.device)[:, None].expand_as(v)
        row = torch.where(v == peak[None], index, v.shape[0]).min(dim=0).values
        return {'peak': peak, 'peak_row': row}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--threshold', type=float, default=0.3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_curves_time.py measures on a GPU'
    from source import _lib
    from source.problem import problem_helper
    from source.time_curves import CurvesPlan, curves_eval, n_rows, rows

    mesh_space, _, mesh_time, _, _ = problem_helper(args.problem, J_space=args.J_space, J_time=args.J_time)
    plan = CurvesPlan(mesh_space, mesh_time)
    N, M, d, nc, theta = mesh_time.nv, plan.n_free, plan.d, plan.nc, args.threshold
    dev = _lib.compute_device()
    ld = N + (N & 1)
    buf = torch.randn((M, ld), dtype=torch.float64, device=dev)
    table = torch.empty((n_rows(d), N), dtype=torch.float64, device=dev)
    R, n_work = n_rows(d), max(-(-nc // 256), -(-M // 256))
    tables = nc * (8 + 8 * (d + 1) * d + 1 + 4 * (d + 1)) + mesh_space.nv * (8 * d + 4)

    def table_reads(chunk):
        """How often a workgroup reads its cells' tables over a call: once per column chunk of
        every batch, the batches those of stk_curves_eval under its 8 MiB cap on the partials
        (at config 3 a batch holds 9 columns, so chunks of 16 and 32 become chunks of 9)."""
        batch = min(max((8 << 20) // (8 * R * n_work), 1), 32768)
        if batch > chunk:
            batch -= batch % chunk
        return sum(-(-min(batch, N - c0) // chunk) for c0 in range(0, N, batch))

    def algorithmic(chunk):
        return 8 * M * ld + tables * table_reads(chunk) + 2 * 8 * R * n_work * N

    print(json.dumps({'problem': args.problem, 'N': N, 'M': M, 'nc': nc, 'ld': ld, 'slab_MB': 8e-6 * M * ld,
                      'cell_tables_MB': 1e-6 * tables, 'partials_MB': 8e-6 * R * n_work * N, 'threshold': theta}), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    def kernel(chunk):
        _lib.check(_lib.lib().stk_curves_tile(chunk))
        return curves_eval(plan, buf, M, N, ld, theta, table, N)

    comp = Composition(mesh_space, buf)
    view = buf[:, :N]
    for chunk in CHUNKS:
        kernel(chunk)
    comp.sums(view), comp.extrema(view)  # warm-up: code objects, the allocator's blocks
    k_s, s_s, x_s = {chunk: [] for chunk in CHUNKS}, [], []
    for _ in range(args.rounds):  # the forms take turns
        for chunk in CHUNKS:
            k_s[chunk].append(timed(lambda: kernel(chunk))[0])
        s_s.append(timed(lambda: comp.sums(view))[0])
        x_s.append(timed(lambda: comp.extrema(view))[0])
    kernel(0)
    at = rows(d)
    ref = dict(comp.sums(view), **comp.extrema(view))
    diffs = {k: float((table[at[k]] - ref[k].to(torch.float64)).abs().max()) for k in ref}
    sizes = {k: float(table[at[k]].abs().max()) for k in ref}
    del ref
    best_s, best_x = min(s_s), min(x_s)
    for chunk in CHUNKS:
        best_k, bytes_ = min(k_s[chunk]), algorithmic(chunk)
        print(json.dumps({'case': 'call', 'chunk_cols': chunk, 'table_reads': table_reads(chunk), 'kernel_s': k_s[chunk],
                          'best_kernel_s': best_k,
                          'median_kernel_s': float(np.median(k_s[chunk])), 'algorithmic_bytes': bytes_,
                          'kernel_TBps': bytes_ / best_k * 1e-12, 'share_of_HBM_peak': bytes_ / best_k * 1e-12 / HBM_PEAK_TBPS,
                          'torch_sums_over_kernel': best_s / best_k,
                          'torch_sums_and_extrema_over_kernel': (best_s + best_x) / best_k}), flush=True)
    print(json.dumps({'case': 'torch', 'sums_s': s_s, 'best_sums_s': best_s, 'median_sums_s': float(np.median(s_s)),
                      'extrema_s': x_s, 'best_extrema_s': best_x, 'median_extrema_s': float(np.median(x_s)),
                      'temporary_GB': 8e-9 * nc * (d + 1) * N}), flush=True)
    print(json.dumps({'case': 'call', 'largest_difference_kernel_torch': diffs, 'largest_value': sizes}), flush=True)

    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            kernel(0)
            torch.cuda.synchronize()
        split = {}
        for ev in prof.key_averages():
            for name in ('curves_cells_kernel', 'curves_finish_kernel'):
                if name in ev.key:
                    total = getattr(ev, 'device_time_total', None) or getattr(ev, 'cuda_time_total', 0.0)
                    split[name] = {'launches': ev.count, 'total_s': total * 1e-6}
        print(json.dumps({'case': 'kernels', 'one_call': split or 'the profiler saw no launch of the library'}), flush=True)
    except Exception as err:  # the figures above stand without the split
        print(json.dumps({'case': 'kernels', 'one_call': 'not measured: %s' % err}), flush=True)

    # the same call on a field like a solution's: a bump of width 0.1 whose centre moves along
    # the first axis -- few cells are cut by the level set, and whole wavefronts walk one branch
    x = torch.from_numpy(plan.row_points).to(dev)
    centre = torch.full((N, d), 0.5, dtype=torch.float64, device=dev)
    centre[:, 0] = torch.linspace(0.25, 0.75, N, dtype=torch.float64, device=dev)
    view.copy_(torch.exp(-((x[:, None, :] - centre[None, :, :])**2).sum(dim=2) / 0.01))
    del x
    kernel(0)
    b_s = [timed(lambda: kernel(0))[0] for _ in range(args.rounds)]
    at_measure = float(table[at['measure_above']].mean())
    print(json.dumps({'case': 'call on a moving bump', 'chunk_cols': CHUNKS[0], 'kernel_s': b_s, 'best_kernel_s': min(b_s),
                      'median_kernel_s': float(np.median(b_s)), 'mean_measure_above': at_measure,
                      'kernel_TBps': algorithmic(CHUNKS[0]) / min(b_s) * 1e-12,
                      'share_of_HBM_peak': algorithmic(CHUNKS[0]) / min(b_s) * 1e-12 / HBM_PEAK_TBPS}), flush=True)


if __name__ == '__main__':
    main()
