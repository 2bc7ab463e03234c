"""tests/c_host/solid_host.c: the host routines of the solidification plan -- the Z-curve
order of the cells and the tiles' row lists -- from plain C99 on a grid whose cells come in a
scattered order, checked inside the program.  No GPU is touched: it runs in the CPU suite."""
import os
import subprocess

import pytest

from conftest import REPO
from test_c_host import _build

SRC = os.path.join(REPO, 'tests', 'c_host', 'solid_host.c')


@pytest.mark.parametrize('side', [1, 11, 16, 64])
def test_c_host_runs_the_solidification_plan_routines(tmp_path, side):
    exe = _build(str(tmp_path / 'solid_host'), SRC)
    res = subprocess.run([exe, str(side)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'solid_host ok' in res.stdout, res.stdout + res.stderr
    assert '%d cells' % (2 * side * side) in res.stdout and '%d free dofs' % ((side - 1) ** 2) in res.stdout
