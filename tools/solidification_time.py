#!/usr/bin/env python3
"""What the solidification maps cost on one GPU (default: square_moving_source at J_time = 6,
J_space = 9 -- a slab of 1 046 529 rows by 65 time nodes, 2 097 152 cells):

* the call: stk_solid_scan on the whole slab (device events, one warm-up, best of `rounds`
  with the median beside it), on `randn` data with the threshold 0.3, for several launch
  forms (stk_solid_tile: the LDS budget of a workgroup, or the columns of a chunk), and for a
  plan that cuts its tiles from the cells in the caller's order (stk_solid_order(1)) beside
  the default, the cells along a Z-curve;
* the SAME fields composed from torch -- what a user would write without the kernel:
  index_select of the cells' rows in column chunks (the whole (nc, d + 1, N) temporary would
  be 3.3 GB), means and gradients, masks of the downward crossings, the last crossing by a
  reversed argmax, the running maximum of |grad|^2 -- timed in the same process, the forms
  taking turns, and compared entry by entry;
* the history scan of the same slab (stk_history_scan), the natural yardstick: it reads
  every row once, the solidification scan once per tile that touches it;
* the call and the composition once more on the SOLVED moving source (--no-solve leaves it
  out), the threshold at half the solution's maximum.

Bytes of the call: `algorithmic` = the slab read once + the state written once + the plan's
tables once; `requested` = what the kernel asks for: every tile's row list times the columns,
the state, the tables.  Both over the best time, in TB/s.

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

# (cols, lds_kib) of stk_solid_tile: the default first, then budgets, then chunks under 64 KiB
FORMS = ((0, 0), (0, 8), (0, 24), (0, 32), (0, 48), (0, 64), (1, 0), (5, 0), (9, 0), (13, 0), (17, 0), (33, 0), (65, 0))
CALLER_FORMS = ((0, 0), (5, 0))  # ... and for the plan in the caller's order
COMPOSITION_CHUNK = 8  # columns per index_select of the composition: a 0.45 GB temporary at the default size


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
        self.free = dev((rows >= 0).astype(np.float64))
        self.grad = dev(np.asarray(grad, dtype=np.float64))

    def fields(self, v, h, theta, chunk=COMPOSITION_CHUNK):
        """t_solid, cooling_rate, n_solid (float64), grad_solid (d, nc), max_grad_sq, t_max_grad
        of the columns of `v` (M, N), a view buf[:, :N]: node k is column k."""
        d, nc, N = self.d, self.nc, v.shape[1]
        dev = v.device
        nan = torch.full((nc,), float('nan'), dtype=torch.float64, device=dev)
        t_solid, cooling, grad_solid = nan.clone(), nan.clone(), nan.repeat(d, 1)
        n_solid = torch.zeros(nc, dtype=torch.float64, device=dev)
        max_q = t_max = None
        lanes = torch.arange(nc, device=dev)
        # divisors as device tensors: torch divides by a Python number by multiplying with its
        # reciprocal, which is not the quotient the contract takes
        by_vertices = torch.tensor([float(d + 1)], dtype=torch.float64, device=dev)
        by_h = torch.tensor([float(h)], dtype=torch.float64, device=dev)
        for c0 in range(0, N, chunk):
            first = max(c0 - 1, 0)  # one column of overlap: the element that ends at c0
            c1 = min(c0 + chunk, N)
            U = v[:, first:c1].index_select(0, self.rows).reshape(nc, d + 1, c1 - first) * self.free[:, :, None]
            m = U.sum(dim=1) / by_vertices
            G = torch.einsum('tan,taj->tjn', U, self.grad)
            Q = (G * G).sum(dim=1)
            own = Q[:, c0 - first:]  # the chunk's own columns
            top = own.max(dim=1).values
            index = torch.arange(c0, c1, device=dev)[None, :].expand_as(own)
            node = torch.where(own == top[:, None], index, N).min(dim=1).values  # the EARLIEST node that has it
            if max_q is None:
                max_q, t_max = top, node.to(torch.float64) * h
            else:
                higher = top > max_q
                max_q, t_max = torch.where(higher, top, max_q), torch.where(higher, node.to(torch.float64) * h, t_max)
            if m.shape[1] < 2:
                continue
            down = (m[:, :-1] > theta) & (m[:, 1:] <= theta)
            n_solid = n_solid + down.sum(dim=1)
            has = down.any(dim=1)
            e = down.shape[1] - 1 - down.flip(1).to(torch.int8).argmax(dim=1)  # the LAST crossing of the chunk
            a, b = m[lanes, e], m[lanes, e + 1]
            x = (theta - a) / (b - a)
            t_solid = torch.where(has, ((first + e).to(torch.float64) + x) * h, t_solid)
            cooling = torch.where(has, (a - b) / by_h, cooling)
            L, R = G[lanes, :, e].t(), G[lanes, :, e + 1].t()  # (d, nc)
            grad_solid = torch.where(has[None, :], L + x[None, :] * (R - L), grad_solid)
        return {'t_solid': t_solid, 'cooling_rate': cooling, 'n_solid': n_solid, 'grad_solid': grad_solid,
                'max_grad_sq': max_q, 't_max_grad': t_max}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--problem', default='square_moving_source')
    ap.add_argument('--J_time', type=int, default=6)
    ap.add_argument('--J_space', type=int, default=9)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--threshold', type=float, default=0.3)
    ap.add_argument('--no-solve', action='store_true', help='leave out the solved moving source')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'solidification_time.py measures on a GPU'
    from source import _lib
    from source.history import STATE_ROWS, history_scan
    from source.problem import problem_helper
    from source.solidification import SolidPlan, cell_order, n_rows, rows, solid_scan, tile_rows

    mesh_space, _, mesh_time, _, _ = problem_helper(args.problem, J_space=args.J_space, J_time=args.J_time)
    plans = {'z-curve': SolidPlan(mesh_space, mesh_time)}
    _lib.check(_lib.lib().stk_solid_order(1))
    plans['caller'] = SolidPlan(mesh_space, mesh_time)
    _lib.check(_lib.lib().stk_solid_order(0))
    plan = plans['z-curve']
    N, M, d, nc, h = mesh_time.nv, plan.n_free, plan.d, plan.nc, float(mesh_time.h)
    dev = _lib.compute_device()
    ld = N + (N & 1)
    buf = torch.randn((M, ld), dtype=torch.float64, device=dev)
    R = n_rows(d)
    state = torch.empty((R, nc), dtype=torch.float64, device=dev)
    hist = torch.empty((len(STATE_ROWS), M), dtype=torch.float64, device=dev)
    at = rows(d)

    cells = np.ascontiguousarray(mesh_space.cells, dtype=np.int64)
    from source.assembly import free_dofs
    fd = np.asarray(free_dofs(mesh_space), dtype=np.int64)
    row_of = np.full(mesh_space.nv, -1, dtype=np.int32)
    row_of[fd] = np.arange(len(fd), dtype=np.int32)
    lengths, requested = {}, {}
    algorithmic = 8 * M * N + 8 * R * nc + nc * (8 * (d + 1) * d + 2 * (d + 1) + 4)
    print(json.dumps({'problem': args.problem, 'N': N, 'M': M, 'nc': nc, 'ld': ld, 'slab_MB': 8e-6 * M * ld,
                      'state_MB': 8e-6 * R * nc, 'algorithmic_bytes': algorithmic}), flush=True)
    for order, placed in (('z-curve', cells[cell_order(mesh_space)]), ('caller', cells)):
        ptr, listed, _ = tile_rows(placed, row_of)
        lengths[order] = np.diff(ptr)
        tables = nc * (8 * (d + 1) * d + 2 * (d + 1) + 4) + 4 * (len(listed) + len(ptr))
        requested[order] = 8 * len(listed) * N + 8 * R * nc + tables
        print(json.dumps({'order': order, 'plan_tables_MB': 1e-6 * tables, 'tiles': len(ptr) - 1,
                          'longest_tile_list': int(lengths[order].max()), 'mean_tile_list': float(lengths[order].mean()),
                          'row_fetches_per_row': len(listed) / M, 'requested_bytes': requested[order]}), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    def kernel(form, theta, order='z-curve'):
        _lib.check(_lib.lib().stk_solid_tile(*form))
        return solid_scan(plans[order], buf, M, N, ld, 0, h, theta, state, fresh=True)

    def history(theta):
        return history_scan(buf, M, N, (ld, 1), 0, h, theta, hist, fresh=True)

    def chunk_of(form, order):
        """The columns per chunk stk_solid_scan takes for a form: its rule, restated."""
        longest = max(int(lengths[order].max()), 1)
        widest = (65536 if form[0] else (form[1] or 16) * 1024) // (8 * longest) - 1
        if form[0]:
            widest = min(widest, form[0])
        widest = max(min(widest, 128), 1)
        n_chunks = -(-N // widest)
        return -(-N // n_chunks)

    comp = Composition(mesh_space, buf)
    view = buf[:, :N]

    def compare(theta):
        ref = comp.fields(view, h, theta)
        kernel((0, 0), theta)
        out = {}
        for key, value in ref.items():
            mine = state[at[key]]
            both_nan = torch.isnan(mine) & torch.isnan(value)
            gap = torch.where(both_nan, torch.zeros_like(mine), (mine - value).abs())
            out[key] = {'largest_difference': float(gap.max()), 'entries_that_differ': int((gap != 0).sum()),
                        'largest_value': float(torch.nan_to_num(mine.abs()).max())}
        n = state[at['n_solid']]
        out['cells_with_a_crossing'] = int((n >= 1).sum())
        out['mean_crossings'] = float(n.mean())
        return out

    def measure(case, theta, forms):
        """forms: (order, (cols, lds_kib))."""
        for order, form in forms:
            kernel(form, theta, order)
        comp.fields(view, h, theta), history(theta)  # warm-up: code objects, the allocator's blocks
        k_s, c_s, h_s = {form: [] for form in forms}, [], []
        for _ in range(args.rounds):  # the forms take turns
            for order, form in forms:
                k_s[order, form].append(timed(lambda: kernel(form, theta, order))[0])
            c_s.append(timed(lambda: comp.fields(view, h, theta))[0])
            h_s.append(timed(lambda: history(theta))[0])
        best_c, best_h = min(c_s), min(h_s)
        for order, form in forms:
            times = k_s[order, form]
            best_k = min(times)
            print(json.dumps({'case': case, 'threshold': theta, 'order': order, 'tile_cols': form[0], 'tile_lds_kib': form[1],
                              'chunk_cols': chunk_of(form, order), 'kernel_s': times, 'best_kernel_s': best_k,
                              'median_kernel_s': float(np.median(times)),
                              'algorithmic_TBps': algorithmic / best_k * 1e-12,
                              'requested_TBps': requested[order] / best_k * 1e-12, 'torch_over_kernel': best_c / best_k,
                              'kernel_over_history_scan': best_k / best_h}), flush=True)
        print(json.dumps({'case': case, 'torch_s': c_s, 'best_torch_s': best_c, 'median_torch_s': float(np.median(c_s)),
                          'torch_chunk_cols': COMPOSITION_CHUNK,
                          'torch_temporary_GB': 8e-9 * nc * (d + 1) * (COMPOSITION_CHUNK + 1),
                          'whole_temporary_GB': 8e-9 * nc * (d + 1) * N}), flush=True)
        print(json.dumps({'case': case, 'history_scan_s': h_s, 'best_history_scan_s': best_h,
                          'median_history_scan_s': float(np.median(h_s)),
                          'history_TBps': (8 * M * N + 72 * M) / best_h * 1e-12}), flush=True)
        kernel((0, 0), theta)
        print(json.dumps({'case': case, 'kernel_against_torch': compare(theta)}), flush=True)

    measure('randn', args.threshold, [('z-curve', f) for f in FORMS] + [('caller', f) for f in CALLER_FORMS])
    _lib.check(_lib.lib().stk_solid_tile(0, 0))

    if not args.no_solve:
        import time

        import heateq_mpi as hm
        from source.comm import Comm
        t0 = time.perf_counter()
        heat = hm.HeatEquationMPI(J_space=args.J_space, J_time=args.J_time, problem=args.problem,
                                  comm=Comm(distributed=False))
        u, iters = heat.solve()
        torch.cuda.synchronize()
        assert (u.M, u.N) == (M, N), (u.M, u.N, M, N)
        view.copy_(u.buf[:, :N])
        peak = float(view.max())
        print(json.dumps({'case': 'solved', 'iterations': iters, 'set_up_and_solve_s': time.perf_counter() - t0,
                          'largest_value': peak}), flush=True)
        del heat, u
        measure('solved', 0.5 * peak, [('z-curve', (0, 0)), ('caller', (0, 0))])
        _lib.check(_lib.lib().stk_solid_tile(0, 0))


if __name__ == '__main__':
    main()
