"""What the two solve drivers share after the solve (source/postprocess.py) and what the plans
of the error norms, the time curves and the solidification maps open with (csrc/p1_mesh.h:
p1_plan_open), the parts that need no GPU: a refused argument is refused before a vector is
uploaded or a plan is built, and the three plan creators refuse alike.

The mesh is the 3 x 3-vertex square (8 triangles, 1 free vertex): the smallest with both a
boundary and a free vertex."""
import ctypes

import numpy as np
import pytest

from source.assembly import free_dofs
from source.postprocess import PostProcessing
from source.problem import problem_helper

PLANS = ('sample_plan', 'error_plan', 'curves_plan', 'solid_plan')


@pytest.fixture(scope='module')
def square():
    mesh = problem_helper('square', J_space=0, J_time=1)[0]
    assert np.asarray(mesh.points).shape == (9, 2) and np.asarray(mesh.cells).shape == (8, 3)
    assert len(free_dofs(mesh)) == 1
    return mesh


class _Recorder(PostProcessing):
    """A driver of nothing but its hooks, which record that they ran."""
    def __init__(self, mesh):
        self._init_postprocessing(mesh, None, {})
        self.ran = []

    def _trial_vector(self, u, who):
        self.ran.append(('_trial_vector', who))
        return u

    def _adjoint_target(self, out):
        self.ran.append(('_adjoint_target',))
        return None, out


REFUSED = {
    'history, NaN threshold': (lambda h, u: h.history_maps(u, threshold=float('nan')), 'threshold is NaN'),
    'history, points of one axis': (lambda h, u: h.history_maps(u, points=np.zeros(5)), r'points of shape \(5,\)'),
    'history, field without its threshold': (lambda h, u: h.history_maps(u, fields=('time_above',)), 'needs a threshold'),
    'curves, NaN threshold': (lambda h, u: h.time_curves(u, threshold=float('nan')), 'threshold is NaN'),
    'solid, no threshold': (lambda h, u: h.solidification_maps(u, None), 'needs a threshold'),
    'solid, 3-d points on a 2-d mesh': (lambda h, u: h.solidification_maps(u, 0.5, points=np.zeros((5, 3))),
                                        r'points of shape \(5, 3\)'),
    'adjoint, unknown field': (lambda h, u: h.sample_along_adjoint(np.ones(2), np.zeros(2), np.zeros((2, 2)), field='flux'),
                               "not 'flux'"),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_a_refused_argument_runs_no_hook_and_builds_no_plan(square, case):
    """For both drivers at once: the ValueError comes before `u` is looked at (the serial
    driver would upload it there) and before any plan is built."""
    call, text = REFUSED[case]
    heat = _Recorder(square)
    assert all(getattr(heat, name) is None for name in PLANS)
    with pytest.raises(ValueError, match=text):
        call(heat, 'no vector at all')
    assert heat.ran == []
    assert all(getattr(heat, name) is None for name in PLANS)


# the phrases of the three creators before p1_plan_open became their one opening, taken from a
# build of that commit on this mesh
PHRASES = {'d = 4': 'bad arguments', 'nc = 0': 'bad arguments', 'null cells': 'bad arguments',
           'a cell names vertex nv': 'cell 7 names vertex 9',
           'a free vertex named twice': 'free dof 1 is vertex 8 (out of range or named twice)'}


@pytest.mark.parametrize('create', ['stk_err_plan_create', 'stk_curves_plan_create', 'stk_solid_plan_create'])
def test_the_plan_creators_refuse_alike(square, create):
    """Every one of these is refused before the first HIP call: no GPU needed."""
    from source import _lib
    lib = _lib.lib()
    pts = np.ascontiguousarray(square.points, dtype=np.float64)
    cells = np.ascontiguousarray(square.cells, dtype=np.int64)
    fd = np.ascontiguousarray(free_dofs(square), dtype=np.int64)
    assert fd.tolist() == [8]
    bad_cells = cells.copy()
    bad_cells[-1, 2] = len(pts)
    good = dict(d=2, nc=len(cells), cells=cells.ctypes.data, fd=fd)
    cases = {'d = 4': dict(d=4), 'nc = 0': dict(nc=0), 'null cells': dict(cells=None),
             'a cell names vertex nv': dict(cells=bad_cells.ctypes.data),
             'a free vertex named twice': dict(fd=np.array([8, 8], dtype=np.int64))}
    assert sorted(cases) == sorted(PHRASES)
    for case, change in cases.items():
        a = dict(good, **change)
        plan = ctypes.c_void_p()
        rc = getattr(lib, create)(a['d'], len(pts), a['nc'], pts.ctypes.data, a['cells'], len(a['fd']),
                                  a['fd'].ctypes.data, ctypes.byref(plan))
        assert rc != 0 and not plan.value, case
        assert lib.stk_last_error().decode() == '%s: %s' % (create, PHRASES[case]), case
