"""Model problems (counterpart of reference source/problem.py:7-41).

``square``: u(t,x,y) = exp(-2 pi^2 t) sin(pi x) sin(pi y) on [0,1]^2, no forcing
(problem.py:7-19).  ``lshape`` is not in the reference (anything but square /
cube asserts there, problem.py:35-41); BASELINE.json config 4 names it, so it
is defined here with the same data on the L-shaped domain.  ``cube``:
u = exp(-3 pi^2 t) sin(pi x) sin(pi y) sin(pi z) on [0,1]^3 (problem.py:21-32).

``square_forced`` / ``cube_forced``: manufactured solutions with a right-hand side,
in the reference's shape for it (problem.py:13-17: ``data['g']`` is a list of
separable pairs ``(g_t, g_x)`` of pointwise functions, g = sum g_t(t) g_x(x)).  With
s_kl = sin(k pi x) sin(l pi y),
    square:  u = exp(-t) s_11 + t s_21,   g = (2 pi^2 - 1) exp(-t) s_11 + (1 + 5 pi^2 t) s_21,
    cube:    u = exp(-t) s_111 + t s_211, g = (3 pi^2 - 1) exp(-t) s_111 + (1 + 6 pi^2 t) s_211,
u(0) = s_11 (s_111): two pairs whose space factors differ.  ``data['exact']`` is u
as a function (t, x, y[, z]) of arrays -- NumPy arrays or torch tensors that broadcast --
and ``data['exact_grad']`` its spatial gradient, a tuple of d arrays: what
``error_norms`` (source/error_norms.py) integrates against.  All four manufactured
problems (these two and the two ``*_nonseparable`` ones) carry both.  ``exact`` of the
forced problems evaluates HOST tensors with NumPy (detached; the doubles of the NumPy
call) and device tensors with torch on the device, whose sin and exp may differ from
NumPy's in the last place.

An entry of ``data['g']`` may also be a CALLABLE g(t, x, y[, z]): a pointwise function of
float64 arrays that broadcast, for right-hand sides that are no short separable sum.
The drivers evaluate it on the device with torch tensors (assembly.fill_test_space_slab;
it is the user's coefficient function, as u0 is); the functions below take NumPy arrays
as well, which is what the tests and ``exact`` use.
``square_nonseparable`` / ``cube_nonseparable``: u = s E with s = sin(pi x) sin(pi y)
[sin(pi z)] and E = exp(-t (1 + x)), which couples t and x:
    g = E [(d pi^2 - (1 + x) - t^2) s + 2 t pi cos(pi x) sin(pi y) [sin(pi z)]],  u(0) = s.
``square_moving_source``: u(0) = 0 and a Gaussian heat source of width 0.1 on a circle,
    g = exp(-|x - c(t)|^2 / (2 0.1^2)),  c(t) = (0.5 + 0.25 cos 2 pi t, 0.5 + 0.25 sin 2 pi t);
no exact solution; ``data['path']`` is the callable c(t) (times (K,) -> points (K, 2)) that
the drivers' --track_out follows.
"""
import sys

import numpy as np

from .mesh import (construct_2d_lshape_mesh, construct_2d_square_mesh,
                   construct_3d_cube_mesh, construct_interval)


def _time_mesh(J_space, J_time):
    if not J_time:
        J_time = J_space
    return construct_interval(N=2**int(J_time + 0.5))


def _u0(x, y):
    return np.sin(np.pi * x) * np.sin(np.pi * y)


def square(J_space, J_time=None):
    mesh_space, bc = construct_2d_square_mesh(nrefines=J_space)
    data = {'g': [], 'u0': _u0}
    return mesh_space, bc, _time_mesh(J_space, J_time), data, "square"


def lshape(J_space, J_time=None):
    mesh_space, bc = construct_2d_lshape_mesh(nrefines=J_space)
    data = {'g': [], 'u0': _u0}
    return mesh_space, bc, _time_mesh(J_space, J_time), data, "lshape"


def jitter(mesh, rel=0.2, seed=0):
    """Moves every interior vertex by up to `rel` times the shortest edge (seeded):
    the triangulation keeps its topology and hierarchy, but no two elements are
    congruent any more, so no two entries of M_x or A_x repeat -- an "unstructured
    mesh, irregular CSR" in the sense of BASELINE.json config 4 for the kernels
    that otherwise live on repeated values (dictionary form of the Kronecker
    apply)."""
    pts, tris = mesh.points, mesh.tris
    e = np.concatenate([pts[tris[:, a]] - pts[tris[:, b]] for a, b in ((0, 1), (1, 2), (2, 0))])
    h = np.sqrt((e * e).sum(axis=1)).min()
    rng = np.random.RandomState(seed)
    move = rel * h * (2.0 * rng.rand(*pts.shape) - 1.0)
    move[mesh.boundary] = 0.0
    mesh.points = pts + move
    return mesh


def lshape_jitter(J_space, J_time=None):
    mesh_space, bc, mesh_time, data, _ = lshape(J_space, J_time)
    return jitter(mesh_space), bc, mesh_time, data, "lshape_jitter"


def _u0_3d(x, y, z):
    return np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)


def cube(J_space, J_time=None):
    mesh_space, bc = construct_3d_cube_mesh(nrefines=J_space)
    data = {'g': [], 'u0': _u0_3d}
    return mesh_space, bc, _time_mesh(J_space, J_time), data, "cube"


def _s21(x, y):
    return np.sin(2 * np.pi * x) * np.sin(np.pi * y)


def _s211(x, y, z):
    return np.sin(2 * np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z)


def _array_module(*args):
    """torch if any argument is a torch tensor (subclasses included), else NumPy; torch
    is not imported for NumPy callers -- a tensor cannot exist before its module."""
    torch = sys.modules.get('torch')
    if torch is not None and any(isinstance(a, torch.Tensor) for a in args):
        return torch
    return np


def _as_array(xp, v):
    return np.asarray(v, dtype=np.float64) if xp is np else xp.as_tensor(v, dtype=xp.float64)


def _sine_product(xp, ks, x, cos_at=None):
    """prod_c sin(k_c pi x_c) from the left, in the doubles of _u0 / _s21; with cos_at = j
    the factor of axis j is replaced by its derivative k_j pi cos(k_j pi x_j)."""
    out = None
    for axis, (k, c) in enumerate(zip(ks, x)):
        arg = np.pi * c if k == 1 else k * np.pi * c
        factor = k * np.pi * xp.cos(arg) if axis == cos_at else xp.sin(arg)
        out = factor if out is None else out * factor
    return out


def _forced_data(d, first, second):
    """u = exp(-t) first + t second on [0,1]^d, where -laplace first = d pi^2 first
    and -laplace second = (d + 3) pi^2 second: g = u_t - laplace u.  ``exact`` and
    ``exact_grad`` take NumPy arrays or torch tensors (_array_module); on NumPy arrays
    ``exact`` is the expression exp(-t) first(x) + t second(x) it always was, and host
    tensors get those doubles; device tensors are evaluated by torch on the device."""
    pi2 = np.pi**2
    g = [(lambda t: (d * pi2 - 1.0) * np.exp(-t), first),
         (lambda t: 1.0 + (d + 3.0) * pi2 * t, second)]
    k_first, k_second = (1,) * d, (2,) + (1,) * (d - 1)

    def exact(t, *x):
        xp = _array_module(t, *x)
        if xp is np:
            return np.exp(-t) * first(*x) + t * second(*x)
        t, x = _as_array(xp, t), [_as_array(xp, c) for c in x]
        if not t.is_cuda and not any(c.is_cuda for c in x):
            # host tensors: NumPy's sin and exp, so that the host has ONE set of doubles
            # whichever array type carries them (torch's CPU kernels round some arguments
            # one unit in the last place differently)
            return xp.from_numpy(np.asarray(exact(t.detach().numpy(), *[c.detach().numpy() for c in x])))
        return xp.exp(-t) * _sine_product(xp, k_first, x) + t * _sine_product(xp, k_second, x)

    def exact_grad(t, *x):
        xp = _array_module(t, *x)
        t, x = _as_array(xp, t), [_as_array(xp, c) for c in x]
        return tuple(xp.exp(-t) * _sine_product(xp, k_first, x, j) + t * _sine_product(xp, k_second, x, j)
                     for j in range(d))

    return {'g': g, 'u0': first, 'exact': exact, 'exact_grad': exact_grad}


def square_forced(J_space, J_time=None):
    mesh_space, bc = construct_2d_square_mesh(nrefines=J_space)
    return mesh_space, bc, _time_mesh(J_space, J_time), _forced_data(2, _u0, _s21), "square_forced"


def cube_forced(J_space, J_time=None):
    mesh_space, bc = construct_3d_cube_mesh(nrefines=J_space)
    return mesh_space, bc, _time_mesh(J_space, J_time), _forced_data(3, _u0_3d, _s211), "cube_forced"


def _nonseparable_data(d):
    """u = s E on [0,1]^d: u_t = -(1 + x) u, laplace u = E laplace s + 2 grad s . grad E
    + s laplace E with grad E = (-t E, 0[, 0]) and laplace E = t^2 E."""
    def parts(t, x):
        xp = _array_module(t, *x)
        t, x = _as_array(xp, t), [_as_array(xp, c) for c in x]
        s, rest = xp.sin(np.pi * x[0]), 1.0  # s in the order of u0's product
        for c in x[1:]:
            s, rest = s * xp.sin(np.pi * c), rest * xp.sin(np.pi * c)
        return xp, t, x[0], s, rest, xp.exp(-t * (1.0 + x[0]))

    def exact(t, *x):
        xp, t, x0, s, rest, E = parts(t, x)
        return s * E

    def g(t, *x):
        xp, t, x0, s, rest, E = parts(t, x)
        return E * ((d * np.pi**2 - (1.0 + x0) - t * t) * s + 2.0 * t * np.pi * xp.cos(np.pi * x0) * rest)

    def exact_grad(t, *x):
        """grad u = E grad s + s grad E with grad E = (-t E, 0[, 0])."""
        xp, t, x0, s, rest, E = parts(t, x)
        x = [_as_array(xp, c) for c in x]
        ks = (1,) * d
        return tuple(E * (_sine_product(xp, ks, x, j) - t * s) if j == 0 else E * _sine_product(xp, ks, x, j)
                     for j in range(d))

    return {'g': [g], 'u0': _u0 if d == 2 else _u0_3d, 'exact': exact, 'exact_grad': exact_grad}


def square_nonseparable(J_space, J_time=None):
    mesh_space, bc = construct_2d_square_mesh(nrefines=J_space)
    return mesh_space, bc, _time_mesh(J_space, J_time), _nonseparable_data(2), "square_nonseparable"


def cube_nonseparable(J_space, J_time=None):
    mesh_space, bc = construct_3d_cube_mesh(nrefines=J_space)
    return mesh_space, bc, _time_mesh(J_space, J_time), _nonseparable_data(3), "cube_nonseparable"


def _moving_source_centre(xp, t):
    return 0.5 + 0.25 * xp.cos(2.0 * np.pi * t), 0.5 + 0.25 * xp.sin(2.0 * np.pi * t)


def _moving_source(t, x, y):
    xp = _array_module(t, x, y)
    t, x, y = _as_array(xp, t), _as_array(xp, x), _as_array(xp, y)
    cx, cy = _moving_source_centre(xp, t)
    return xp.exp(-((x - cx)**2 + (y - cy)**2) / (2.0 * 0.1**2))


def _moving_source_path(t):
    """c(t), the centre of the source: times (K,) -> points (K, 2), NumPy arrays or torch
    tensors."""
    xp = _array_module(t)
    return xp.stack(_moving_source_centre(xp, _as_array(xp, t)), -1)


def square_moving_source(J_space, J_time=None):
    mesh_space, bc = construct_2d_square_mesh(nrefines=J_space)
    data = {'g': [_moving_source], 'u0': lambda x, y: np.zeros_like(x), 'path': _moving_source_path}
    return mesh_space, bc, _time_mesh(J_space, J_time), data, "square_moving_source"


def problem_helper(problem, J_space, J_time=None):
    if problem == 'square':
        return square(J_space, J_time)
    elif problem == 'lshape':
        return lshape(J_space, J_time)
    elif problem == 'lshape_jitter':
        return lshape_jitter(J_space, J_time)
    elif problem == 'cube':
        return cube(J_space, J_time)
    elif problem == 'square_forced':
        return square_forced(J_space, J_time)
    elif problem == 'cube_forced':
        return cube_forced(J_space, J_time)
    elif problem == 'square_nonseparable':
        return square_nonseparable(J_space, J_time)
    elif problem == 'cube_nonseparable':
        return cube_nonseparable(J_space, J_time)
    elif problem == 'square_moving_source':
        return square_moving_source(J_space, J_time)
    else:
        assert (False)
