"""What the two command-line drivers (heateq_mpi.py, heateq_mpi_timing.py) share:
the command line of the reference's drivers, the lines they print, the
per-operator counters and the gathered record (reference heateq_mpi.py:259-312,
heateq_mpi_timing.py:62-128)."""
import argparse
import base64
import pickle
import sys
import zlib

import numpy as np
import torch

from .comm import MPI

# (flag, type, default, help): the options both reference drivers take
_PROBLEM_OPTIONS = (
    ('problem', str, 'square', 'problem type (square, lshape, cube, square_forced, cube_forced,'
     ' square_nonseparable, cube_nonseparable, square_moving_source)'),
    ('J_time', int, 7, 'number of time refines'),
    ('J_space', int, 7, 'number of space refines'),
    ('smoothsteps', int, 3, 'number of smoothing steps'),
    ('vcycles', int, 2, 'number of vcycles'),
    ('wavelettransform', str, 'composite', 'type of wavelettransform'),
    ('alpha', float, 0.3, 'alpha'),
)
OPERATORS = ('W', 'S', 'WT', 'P')
# the solve drivers' options for sampling the solution (never constructor arguments)
SAMPLE_OPTIONS = (
    ('sample_out', str, None, 'write the solution sampled on a raster at equally spaced times to this .npz'),
    ('sample_times', int, 5, 'number of equally spaced sample times from 0 to T'),
    ('sample_raster', int, 129, 'raster points per axis over the bounding box of the mesh'),
    ('error_norms', int, 0, '1: after the solve, the L2(L2), L2(H1) and final-time L2 norms of the error against'
     ' the exact solution of the problem, by quadrature on the device'),
)
# ... and for following the problem's path (data['path']) through the solution
TRACK_OPTIONS = (
    ('track_out', str, None, 'write the solution, its time derivative and its gradient along the path of the'
     ' problem (e.g. under the moving source) to this .npz'),
    ('track_points', int, 1025, 'number of equally spaced times from 0 to T along the path'),
)
# ... and for the history maps of the solution (peak, dose, rates, threshold times)
HISTORY_OPTIONS = (
    ('history_out', str, None, 'write the history maps of the solution (peak, t_peak, dose, max_rate, min_rate; with a'
     ' threshold also time_above, t_first, t_last) on a raster to this .npz'),
    ('history_threshold', float, None, 'threshold of the history maps (default: none)'),
    ('history_raster', int, 129, 'raster points per axis over the bounding box of the mesh'),
)
# ... and for the time curves of the solution (heat content, norms, outflow, peak, hot zone)
CURVES_OPTIONS = (
    ('curves_out', str, None, 'write the time curves of the solution (heat, l2_sq, h1_sq, outflow, peak, peak_row,'
     ' peak_point per time node; with a threshold also measure_above, moment_above, centroid_above, box_lo, box_hi)'
     ' to this .npz'),
    ('curves_threshold', float, None, 'threshold of the hot zone of the time curves (default: none)'),
)
# ... and for the solidification maps of the solution (front time, cooling rate, gradient, front speed per cell)
SOLID_OPTIONS = (
    ('solid_out', str, None, 'write the solidification maps of the solution (t_solid, cooling_rate, grad_solid, G,'
     ' front_speed, n_solid, max_grad, t_max_grad per cell, with the centroids) to this .npz; needs --solid_threshold'),
    ('solid_threshold', float, None, 'threshold whose last downward crossing by a cell\'s mean is its solidification'),
)
# ... and for the isotherms of the solution (the level-set segments or triangles per time node)
ISO_OPTIONS = (
    ('iso_out', str, None, 'write the isotherm {u_h = threshold} of the solution at time nodes (nodes, times, offsets,'
     ' vertices, grad, cell, measure, measure_at, flux_at) to this .npz; needs --iso_threshold'),
    ('iso_threshold', float, None, 'threshold of the isotherms'),
    ('iso_every', int, 1, 'every K-th time node from 0 (default 1: every node)'),
)
# ... and for nested iteration: the solve started from the prolonged solution of coarser levels
NESTED_OPTIONS = (
    ('nested', int, 0, 'solve the L coarser problems (J_time - l, J_space - l), l = L .. 1, first, from the coarsest up,'
     ' each started from the prolonged solution of the one before (prolong_from, solve(x0=)); default 0: none'),
    ('nested_rhs', str, 'own', 'right-hand side of the coarser problems of --nested: own (each level assembles its f'
     ' from the forcing; the default) or restricted (P^T f of the finest level\'s f, restrict_to)'),
)


def device_mb():
    """Device memory in use by this process, MB (the reference reports host RSS;
    the vectors and matrices live in HBM here)."""
    return torch.cuda.memory_allocated() / 1048576 if torch.cuda.is_available() else 0.0


def parse(description, argv, extra=(), defaults=None):
    """`defaults`: a driver's own defaults where the reference's drivers differ (its
    timing script takes wavelettransform='original', heateq_mpi_timing.py:35-37, its solve
    driver 'composite', heateq_mpi.py:225-228)."""
    parser = argparse.ArgumentParser(description=description)
    for flag, kind, default, text in _PROBLEM_OPTIONS + tuple(extra):
        parser.add_argument('--' + flag, type=kind, default=(defaults or {}).get(flag, default), help=text)
    return parser.parse_args(argv)


def solver_arguments(args):
    """Keyword arguments of HeatEquationMPI from a parsed command line."""
    keys = [flag for flag, _, _, _ in _PROBLEM_OPTIONS] + ['schur', 'arithmetic']
    return {k: getattr(args, k) for k in keys if hasattr(args, k)}


def start(args):
    """Communicator, rank and size; refuses more ranks than time steps and
    prints the opening lines on rank 0."""
    comm = MPI.COMM_WORLD
    rank, size = comm.Get_rank(), comm.Get_size()
    if size > 2**args.J_time + 1:
        print('Too many ranks!')
        sys.exit('1')
    if rank == 0:
        print('\n\nCreating mesh with %d time refines and %d space refines.'
              % (args.J_time, args.J_space))
        print('GPU ranks: %d ' % size)
        print('Arguments: %s' % args)
    return comm, rank, size


def report_construction(heat):
    print('N = %d. M = %d.' % (heat.N, heat.M))
    print('Constructed bilinear forms in %s s.' % heat.setup_time)
    print('Device memory after construction: %smb.' % device_mb())


def counters(op, **more):
    record = {'time_applies': op.time_applies,
              'time_communication': op.time_communication,
              'num_applies': op.num_applies}
    record.update(more)
    return record


def seeded_vector(heat, vector_type, seed=128):
    """The timing driver's input: uniform random numbers, drawn per GLOBAL time
    row (seed + t) so that every rank count sees the same global vector (the
    reference seeds 128 and draws the local block)."""
    dd = heat.dofs_distr
    vec = vector_type(dd)
    for t in range(dd.t_begin, dd.t_end):
        row = np.random.RandomState(seed + t).rand(heat.M)
        vec.X_loc[t - dd.t_begin] = torch.from_numpy(row).to(vec.buf.device)
    return vec


def time_operator(comm, op, vec, iters):
    """`iters` applies of op to vec, the halo re-exchanged each time; one untimed
    apply first (plans, workspaces).  Returns the operator's record."""
    op @ vec
    op.num_applies = op.time_applies = op.time_communication = 0
    began = MPI.Wtime()
    per_apply, per_exchange = [], []
    for _ in range(iters):
        before = (op.time_applies, op.time_communication)
        vec._invalidate()
        op @ vec
        per_apply.append(op.time_applies - before[0])
        per_exchange.append(op.time_communication - before[1])
        comm.Barrier()
    return counters(op, time_applies_iter=per_apply,
                    time_communication_iter=per_exchange,
                    time_total=MPI.Wtime() - began)


def take_options(args, options, wanted):
    """(the parsed command line without the flags of the table `options`, those options -- or
    None where none of the flags `wanted` is given): what the drivers print and record stays
    what it was."""
    taken = argparse.Namespace(**{flag: vars(args).pop(flag) for flag, _, _, _ in options})
    return args, (taken if any(getattr(taken, flag) for flag in wanted) else None)


# what a solve driver can do with its solution: (name, options, the flags that ask for it)
POST_OPTIONS = (SAMPLE_OPTIONS + TRACK_OPTIONS + HISTORY_OPTIONS + CURVES_OPTIONS + SOLID_OPTIONS + ISO_OPTIONS
                + NESTED_OPTIONS)
_POST = (('sample', SAMPLE_OPTIONS, ('sample_out', 'error_norms')), ('track', TRACK_OPTIONS, ('track_out',)),
         ('history', HISTORY_OPTIONS, ('history_out',)), ('curves', CURVES_OPTIONS, ('curves_out',)),
         ('solid', SOLID_OPTIONS, ('solid_out',)), ('iso', ISO_OPTIONS, ('iso_out',)),
         ('nested', NESTED_OPTIONS, ('nested',)))


def take_post_options(args):
    """(the parsed command line without POST_OPTIONS -- never constructor arguments --, asked):
    asked[name] = the options of 'sample', 'track', 'history', 'curves', 'solid', 'iso', 'nested',
    None where the command line does not ask for it.  --solid_out without --solid_threshold,
    --iso_out without --iso_threshold or with an --iso_every below 1, and a negative --nested
    end the run as an argument error does, before anything is built."""
    asked = {}
    for name, options, wanted in _POST:
        args, asked[name] = take_options(args, options, wanted)
    if asked['solid'] is not None and asked['solid'].solid_threshold is None:
        raise SystemExit('--solid_out needs --solid_threshold: the maps are those of one threshold')
    if asked['iso'] is not None and asked['iso'].iso_threshold is None:
        raise SystemExit('--iso_out needs --iso_threshold: the isotherms are those of one threshold')
    if asked['iso'] is not None and asked['iso'].iso_every < 1:
        raise SystemExit('--iso_every must be at least 1')
    if asked['nested'] is not None and asked['nested'].nested < 0:
        raise SystemExit('--nested must be at least 0')
    if asked['nested'] is not None and asked['nested'].nested_rhs not in ('own', 'restricted'):
        raise SystemExit('--nested_rhs must be own or restricted, not %r' % asked['nested'].nested_rhs)
    return args, asked


def nested_levels(J_time, J_space, nested, size=1):
    """[(J_time - l, J_space - l) for l = nested .. 1]: the coarser problems of --nested, the
    coarsest first.  Ends the run, before anything is built, where a level cannot be built:
    a negative number of refines, or fewer time nodes than ranks."""
    levels = [(J_time - l, J_space - l) for l in range(int(nested), 0, -1)]
    for jt, js in levels:
        if jt < 0 or js < 0:
            raise SystemExit('--nested %d: there is no level (J_time = %d, J_space = %d)' % (nested, jt, js))
        if 2**jt + 1 < size:
            raise SystemExit('--nested %d: the level J_time = %d has %d time nodes, fewer than the %d ranks'
                             % (nested, jt, 2**jt + 1, size))
    return levels


def solve_nested(heat, build, levels, rank=0, rhs=None, **solve_arguments):
    """Nested iteration: ``build(J_time, J_space)`` makes the driver object of each of `levels`
    (nested_levels: the coarsest first); every level is solved from the prolonged solution of
    the one before it (heat.prolong_from, solve(x0=)), the coarsest from zero, `heat` last.
    `rhs`: a functional on `heat`'s trial space (what ``sample_along_adjoint`` returned, heat.f
    itself) in place of every level's own f -- a coarser level solves for
    ``heat.restrict_to(level, rhs)``, `heat` for ``solve(rhs=rhs, x0=...)``.  Rank 0 prints one
    line with the iterations per level, and with `rhs` which right-hand side the level used.
    `solve_arguments` (callback, history, ...) go to the LAST solve.  Returns (u, iterations) of
    `heat`, and the list of (J_time, J_space, iterations) of all levels; collective."""
    if rhs is None and heat.f is None:  # before a coarser problem is built
        raise SystemExit('--nested: solve() is the path of a problem with forcing; this problem has none')
    before, u, counts = None, None, []
    for number, level in enumerate(list(levels) + [None]):
        this = heat if level is None else build(*level)
        x0 = None if before is None else this.prolong_from(before, u)
        if rhs is None:
            u, iters = this.solve(x0=x0, **(solve_arguments if level is None else {}))
            said = ''
        elif level is None:
            u, iters = this.solve(rhs=rhs, x0=x0, **solve_arguments)
            said = ', for the given right-hand side'
        else:
            u, iters = this.solve(rhs=heat.restrict_to(this, rhs), x0=x0)
            said = ', for the restricted right-hand side'
        mesh_space, mesh_time = this._sample_meshes
        counts.append((int(mesh_time.N_el).bit_length() - 1, mesh_space.J - 1, iters))
        if rank == 0:
            print('\nNested level %d of %d (J_time = %d, J_space = %d): %d PCG steps%s%s.'
                  % ((number, len(levels)) + counts[-1] + ('' if x0 is not None else ', from zero', said)))
        before = this
    return u, iters, counts


def run_post(heat, solution, asked, rank=0):
    """After the solve, what `asked` (take_post_options) asks for, in the fixed order sample,
    track, history, curves, solid, iso, error norms; every step is collective.  Returns the record
    of the error norms, None where there is none."""
    for name, write in (('sample', write_samples), ('track', write_track), ('history', write_history),
                        ('curves', write_curves), ('solid', write_solid), ('iso', write_isotherms)):
        if asked[name] is not None and getattr(asked[name], name + '_out'):
            write(heat, solution, asked[name], rank)
    if asked['sample'] is not None and asked['sample'].error_norms:
        return report_error_norms(heat, solution, rank)
    return None


def report_error_norms(heat, solution, rank=0):
    """--error_norms: one line with the four norms of u - u_h and the relative errors
    (heat.error_norms, collective; works for both solve drivers), and the dict for the
    record (arrays as lists).  A problem without data['exact'] says so and returns None."""
    if heat._exact[0] is None:
        if rank == 0:
            print('Error norms: this problem has no exact solution; nothing to compare with.')
        return None
    n = heat.error_norms(solution)
    if rank == 0:
        line = 'Error norms: L2(L2) %.6e (relative %.4e)' % (n['l2_l2'], n['l2_l2'] / n['exact_l2_l2'])
        if n['l2_h1'] is not None:
            line += ', L2(H1) %.6e (relative %.4e)' % (n['l2_h1'], n['l2_h1'] / n['exact_l2_h1'])
        line += ', L2 at T %.6e; exact: L2(L2) %.6e' % (n['l2_at'][-1], n['exact_l2_l2'])
        if n['l2_h1'] is not None:
            line += ', L2(H1) %.6e' % n['exact_l2_h1']
        print(line)
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in n.items()}


def _write_npz(path, rank, **arrays):
    """Rank 0 writes `arrays` -- device tensors copied out, the rest as it is -- to `path`."""
    if rank == 0:
        with open(path, 'wb') as f:  # the name as given: np.savez appends .npz to a path
            np.savez(f, **{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in arrays.items()})


def write_samples(heat, solution, args, rank=0):
    """--sample_out: the solution on a raster of sample_raster^d points over the bounding
    box at sample_times equally spaced times from 0 to T, written by rank 0 as an .npz with
    times (K,), points (R^d, d), inside (R^d,) and values (K, R^d).  Collective
    (heat.sample); works for both solve drivers."""
    from .sampling import raster
    mesh_space, mesh_time = heat._sample_meshes
    times = np.linspace(0.0, mesh_time.T, args.sample_times)
    points = raster(mesh_space, args.sample_raster)
    values = heat.sample(solution, times, points)
    located = heat.sample_plan.locate(points)
    _write_npz(args.sample_out, rank, times=times, points=points, inside=located.inside, values=values)
    return values


def write_history(heat, solution, args, rank=0):
    """--history_out: the history maps of the solution on a raster of history_raster^d points
    over the bounding box, written by rank 0 as an .npz with points (R^d, d), inside (R^d,) and
    one (R^d,) array per field (heat.history_maps with points; the three threshold fields only
    with --history_threshold).  Collective; works for both solve drivers."""
    from .sampling import raster
    points = raster(heat._sample_meshes[0], args.history_raster)
    got = heat.history_maps(solution, threshold=args.history_threshold, points=points)
    _write_npz(args.history_out, rank, points=points, **got)
    return got


def write_curves(heat, solution, args, rank=0):
    """--curves_out: the time curves of the solution, written by rank 0 as an .npz with times
    (N,) and one array per field of heat.time_curves (the five zone fields only with
    --curves_threshold).  Collective; works for both solve drivers."""
    got = heat.time_curves(solution, threshold=args.curves_threshold)
    mesh_time = heat._sample_meshes[1]
    times = np.array([float(k) * float(mesh_time.h) for k in range(mesh_time.nv)])
    _write_npz(args.curves_out, rank, times=times, **got)
    return got


def write_solid(heat, solution, args, rank=0):
    """--solid_out: the solidification maps of the solution, written by rank 0 as an .npz with
    centroids (nc, d) -- the mean of a cell's vertices, in the mesh's cell order --, threshold
    and one array per field of heat.solidification_maps.  Collective; works for both solve
    drivers."""
    got = heat.solidification_maps(solution, threshold=args.solid_threshold)
    mesh = heat._sample_meshes[0]
    centroids = np.asarray(mesh.points, dtype=np.float64)[np.asarray(mesh.cells, dtype=np.int64)].mean(axis=1)
    _write_npz(args.solid_out, rank, centroids=centroids, threshold=float(args.solid_threshold), **got)
    return got


def write_isotherms(heat, solution, args, rank=0):
    """--iso_out: the isotherm {u_h = iso_threshold} of the solution at every iso_every-th time
    node from 0, written by rank 0 as an .npz with threshold and one array per entry of
    heat.isotherms.  Collective; works for both solve drivers."""
    nodes = list(range(0, heat._sample_meshes[1].nv, args.iso_every))
    got = heat.isotherms(solution, threshold=args.iso_threshold, nodes=nodes)
    _write_npz(args.iso_out, rank, threshold=float(args.iso_threshold), **got)
    return got


def require_path(heat, args):
    """Ends the run with a message where --track_out cannot be served: the drivers ask
    before they solve."""
    if getattr(heat, 'path', None) is None:
        raise SystemExit('--track_out: this problem has no path to follow (square_moving_source has one)')
    if args.track_points < 1:
        raise SystemExit('--track_points must be at least 1')


def write_track(heat, solution, args, rank=0):
    """--track_out: u_h, d/dt u_h and grad u_h along the path c(t) of the problem
    (heat.path = data['path']) at track_points equally spaced times from 0 to T, written by
    rank 0 as an .npz with times (K,), points (K, d), inside (K,), u (K,), dt (K,) and grad
    (d, K).  Collective (heat.sample_along); works for both solve drivers."""
    require_path(heat, args)
    _, mesh_time = heat._sample_meshes
    times = np.linspace(0.0, mesh_time.T, args.track_points)
    points = np.ascontiguousarray(np.asarray(heat.path(times), dtype=np.float64))
    assert points.ndim == 2 and points.shape[0] == len(times), points.shape
    got = heat.sample_along(solution, times, points, fields=('u', 'dt', 'grad'))
    _write_npz(args.track_out, rank, times=times, points=points, **{k: got[k] for k in ('inside', 'u', 'dt', 'grad')})
    return got


def publish(comm, record):
    """Gathers the per-rank records on rank 0 and prints them as the reference's
    `data:` line, base64(zlib(pickle))."""
    everyone = comm.gather(record, root=0)
    if comm.Get_rank() == 0:
        blob = base64.b64encode(zlib.compress(pickle.dumps(everyone)))
        print('\ndata: %s' % str(blob, 'ascii'))
    return everyone
