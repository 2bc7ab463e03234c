#!/usr/bin/env python3
"""What the isotherms cost on one GPU (default: square_moving_source at J_time = 6, J_space = 9
-- a slab of 1 046 529 rows by 65 time nodes, 2 097 152 cells):

* on the SOLVED moving source, all nodes, at the threshold given (default 0.3) and at half the
  solution's maximum (the default threshold lies above the maximum of this problem at this
  size: no piece at all, the case in which `fill` has nothing to do): stk_iso_count,
  stk_iso_fill and the whole public call ``heat.isotherms`` (device events, one warm-up, best of
  `rounds` with the median beside it), and the pieces per node;
* on `randn` data, where almost every cell is cut, restricted to so few nodes (--randn_nodes)
  that the table stays under max_bytes: the same, for several column chunks (stk_iso_tile);
* in the same process, the forms taking turns: ``time_curves(u, threshold)`` of the same
  columns, for scale -- it makes the same cut and reduces it -- and the SAME records composed
  from torch, what a user would write without the kernel: index_select of the cells' rows
  into an (nc, d + 1, n) temporary, the class masks, nonzero, a stable sort of the cut cells'
  vertices, the cuts; compared with the kernel's records entry by entry.

Algorithmic bytes of count = the slab's columns read once + the cells and row map once per
column chunk + the counts; of fill = the counts and the prefix + per non-empty tile what count
reads plus the points and gradients + the records written; over the best time, in TB/s.

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

CHUNKS = (8, 1, 2, 4, 16, 32)  # columns a workgroup takes in turn: stk_iso_tile
TILE = 256


class Composition:
    """The mesh tables of the torch composition, on the device of `like`."""
    def __init__(self, mesh, like):
        from source.assembly import _simplex_geometry, free_dofs
        cells = np.ascontiguousarray(mesh.cells, dtype=np.int64)
        self.nc, self.d = len(cells), cells.shape[1] - 1
        fd = np.asarray(free_dofs(mesh), dtype=np.int64)
        row_of = np.full(mesh.nv, -1, dtype=np.int64)
        row_of[fd] = np.arange(len(fd))
        rows = row_of[cells]
        _, grad = _simplex_geometry(mesh)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(like.device)
        self.rows = dev(np.maximum(rows, 0).reshape(-1))
        self.free = dev(rows >= 0)
        self.grad = dev(np.asarray(grad, dtype=np.float64))
        self.points = dev(np.asarray(mesh.points, dtype=np.float64)[cells])  # (nc, d + 1, d)

    def records(self, v, theta):
        """(counts (n, n_tiles) int64, records (n_pieces, W)) of the columns of `v` (M, n), a
        view buf[:, :n]: the contract's records in the contract's order."""
        d, nc, n = self.d, self.nc, v.shape[1]
        W = d * d + d + 1
        dev = v.device
        n_tiles = -(-nc // TILE)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        U = torch.where(self.free[:, :, None], v.index_select(0, self.rows).reshape(nc, d + 1, n), zero)
        up = U > theta
        above = up.sum(dim=1)  # (nc, n)
        k = ((above > 0) & (above < d + 1)).to(torch.int64)
        if d == 3:
            k = k + (above == 2)
        if not np.isfinite(theta):
            k = torch.zeros_like(k)
        padded = torch.zeros((n_tiles * TILE, n), dtype=torch.int64, device=dev)
        padded[:nc] = k
        counts = padded.reshape(n_tiles, TILE, n).sum(dim=1).t().contiguous()
        col, cell = torch.nonzero(k.t() > 0, as_tuple=True)  # column by column, cell by cell
        Uc, upc = U[cell, :, col], up[cell, :, col]            # (m, d + 1)
        order = torch.sort((~upc).to(torch.int8), dim=1, stable=True).indices  # above ones first
        Wv = torch.gather(Uc, 1, order)
        Q = torch.gather(self.points[cell], 1, order[:, :, None].expand(-1, -1, d))
        na = above[cell, col]

        def cut(a, b):
            s = (Wv[:, a] - theta) / (Wv[:, a] - Wv[:, b])
            return Q[:, a] + s[:, None] * (Q[:, b] - Q[:, a])

        rec = torch.zeros((len(cell), 2, W), dtype=torch.float64, device=dev)
        if d == 2:
            one = (na == 1)[:, None]
            rec[:, 0, 0:2] = torch.where(one, cut(0, 1), cut(1, 2))
            rec[:, 0, 2:4] = cut(0, 2)
        else:
            c01, c02, c03, c12, c13, c23 = cut(0, 1), cut(0, 2), cut(0, 3), cut(1, 2), cut(1, 3), cut(2, 3)
            one, two = (na == 1)[:, None], (na == 2)[:, None]
            rec[:, 0, 0:3] = torch.where(one, c01, torch.where(two, c02, c03))
            rec[:, 0, 3:6] = torch.where(one, c02, torch.where(two, c03, c13))
            rec[:, 0, 6:9] = torch.where(one, c03, torch.where(two, c12, c23))
            rec[:, 1, 0:3], rec[:, 1, 3:6], rec[:, 1, 6:9] = c03, c12, c13
        g = self.grad[cell]
        for j in range(d):
            Gj = Uc[:, 0] * g[:, 0, j]
            for a in range(1, d + 1):
                Gj = Gj + Uc[:, a] * g[:, a, j]
            rec[:, :, d * d + j] = Gj[:, None]
        rec[:, :, d * d + d] = cell.to(torch.float64)[:, None]
        keep = torch.stack([torch.ones_like(na, dtype=torch.bool), k[cell, col] == 2], dim=1)
        return counts, rec[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square_moving_source')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--threshold', type=float, default=0.3)
    ap.add_argument('--randn_nodes', type=int, default=2, help='nodes of the randn case: the table must stay under max_bytes')
    ap.add_argument('--no-solve', action='store_true', help='leave out the solved problem')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'isotherms_time.py measures on a GPU'
    import heateq_mpi as hm
    from source import _lib
    from source.comm import Comm
    from source.isotherms import MAX_BYTES, iso_count, iso_fill, width
    from source.mpi_vector import KronVectorMPI
    from source.time_curves import curves_eval, n_rows

    heat = hm.HeatEquationMPI(J_space=args.J_space, J_time=args.J_time, problem=args.problem, comm=Comm(distributed=False))
    mesh_space = heat._sample_meshes[0]
    u = KronVectorMPI(heat.dofs_distr)
    heat.time_curves(u)  # builds the plan both calls share
    plan = heat.curves_plan
    N, M, d, nc, ld = u.N, u.M, plan.d, plan.nc, u.ld
    W, n_tiles = width(d), -(-nc // TILE)
    dev = u.buf.device
    cells_bytes, geometry_bytes = nc * 4 * (d + 1) + mesh_space.nv * 4, nc * 8 * (d + 1) * d + mesh_space.nv * 8 * d
    print(json.dumps({'problem': args.problem, 'N': N, 'M': M, 'nc': nc, 'ld': ld, 'n_tiles': n_tiles, 'record_doubles': W,
                      'slab_MB': 8e-6 * M * ld, 'counts_MB': 8e-6 * N * n_tiles, 'max_bytes': MAX_BYTES}), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    comp = Composition(mesh_space, u.buf)
    curves = torch.empty((n_rows(d), N), dtype=torch.float64, device=dev)

    def measure(case, theta, n, chunks, with_call):
        """The columns [0, n) of the slab: count, fill, the whole call, time_curves, torch."""
        nodes = list(range(n))
        counts = torch.zeros((n, n_tiles), dtype=torch.int64, device=dev)

        def count(chunk):
            _lib.check(_lib.lib().stk_iso_tile(chunk))
            return iso_count(plan, u.buf, M, n, ld, theta, counts)

        count(0)
        flat = counts.reshape(-1)
        first = torch.cumsum(flat, 0) - flat
        total = int(flat.sum())
        full_tiles = int((flat > 0).sum())
        table = torch.zeros((max(total, 1), W), dtype=torch.float64, device=dev)

        def fill(chunk):
            _lib.check(_lib.lib().stk_iso_tile(chunk))
            return iso_fill(plan, u.buf, M, n, ld, theta, counts, first, total, table)

        view = u.buf[:, :n]
        for chunk in chunks:
            count(chunk), fill(chunk)
        _lib.check(_lib.lib().stk_iso_tile(0))
        call = lambda: heat.isotherms(u, theta, nodes=nodes)
        scale = lambda: curves_eval(plan, u.buf, M, n, ld, theta, curves, N)
        torch_form = lambda: comp.records(view, theta)
        if with_call:
            call()
        scale(), torch_form()  # warm-up: code objects, the allocator's blocks
        c_s, f_s, w_s, t_s, p_s = {c: [] for c in chunks}, {c: [] for c in chunks}, [], [], []
        for _ in range(args.rounds):  # the forms take turns
            for chunk in chunks:
                c_s[chunk].append(timed(lambda: count(chunk))[0])
                f_s[chunk].append(timed(lambda: fill(chunk))[0])
            _lib.check(_lib.lib().stk_iso_tile(0))
            if with_call:
                w_s.append(timed(call)[0])
            t_s.append(timed(scale)[0])
            p_s.append(timed(torch_form)[0])
        per_node = counts.sum(dim=1).cpu().numpy()
        print(json.dumps({'case': case, 'threshold': theta, 'nodes': n, 'pieces': total, 'records_MB': 8e-6 * total * W,
                          'pieces_per_node_min': int(per_node.min()), 'pieces_per_node_max': int(per_node.max()),
                          'pieces_per_node_mean': float(per_node.mean()), 'tiles_with_a_piece': full_tiles,
                          'tiles': n * n_tiles}), flush=True)
        best_t, best_p = min(t_s), min(p_s)
        for chunk in chunks:
            groups = -(-n // chunk)
            count_bytes = 8 * M * n + cells_bytes * groups + 8 * n * n_tiles
            fill_bytes = (2 * 8 * n * n_tiles + 8 * W * total
                          + full_tiles * TILE * (8 * (d + 1) + (4 * (d + 1) + 8 * (d + 1) * d * 2) / min(chunk, n)))
            best_c, best_f = min(c_s[chunk]), min(f_s[chunk])
            print(json.dumps({'case': case, 'chunk_cols': chunk, 'count_s': c_s[chunk], 'best_count_s': best_c,
                              'median_count_s': float(np.median(c_s[chunk])), 'fill_s': f_s[chunk], 'best_fill_s': best_f,
                              'median_fill_s': float(np.median(f_s[chunk])), 'count_algorithmic_bytes': count_bytes,
                              'count_TBps': count_bytes / best_c * 1e-12, 'fill_algorithmic_bytes': fill_bytes,
                              'fill_TBps': fill_bytes / best_f * 1e-12,
                              'time_curves_over_count_and_fill': best_t / (best_c + best_f),
                              'torch_over_count_and_fill': best_p / (best_c + best_f)}), flush=True)
        print(json.dumps({'case': case, 'whole_call_s': w_s, 'best_whole_call_s': min(w_s) if w_s else None,
                          'median_whole_call_s': float(np.median(w_s)) if w_s else None,
                          'time_curves_s': t_s, 'best_time_curves_s': best_t, 'median_time_curves_s': float(np.median(t_s)),
                          'torch_s': p_s, 'best_torch_s': best_p, 'median_torch_s': float(np.median(p_s)),
                          'torch_temporary_GB': 8e-9 * nc * (d + 1) * n}), flush=True)
        fill(0)
        t_counts, t_records = torch_form()
        same = lambda a, b: bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()) if a.shape == b.shape else False
        print(json.dumps({'case': case, 'kernel_against_torch': {
            'counts_equal': bool(torch.equal(t_counts, counts)), 'records_equal': same(t_records, table[:total]),
            'entries_that_differ': int((t_records != table[:total]).sum()) if t_records.shape == table[:total].shape else None}}),
            flush=True)

    if not args.no_solve:
        import time
        t0 = time.perf_counter()
        solution, iters = heat.solve()
        torch.cuda.synchronize()
        u.buf.copy_(solution.buf)
        peak = float(u.buf[:, :N].max())
        print(json.dumps({'case': 'solved', 'iterations': iters, 'solve_s': time.perf_counter() - t0, 'largest_value': peak}),
              flush=True)
        del solution
        measure('solved', args.threshold, N, (8,), True)
        measure('solved, half the maximum', 0.5 * peak, N, CHUNKS, True)
    n = max(min(args.randn_nodes, N), 1)
    u.buf[:, :N].copy_(torch.randn((M, N), dtype=torch.float64, device=dev))
    assert 2 * nc * n * 8 * W <= MAX_BYTES, 'too many nodes for randn data: the table would pass max_bytes'
    measure('randn', args.threshold, n, tuple(c for c in CHUNKS if c <= max(n, 8)), True)


if __name__ == '__main__':
    main()
