"""tests/c_host/restrict_host.c: the host routine of the restriction plan -- the transposed
parents table of stk_transfer_children -- from plain C99 on a refined grid in the hierarchical
numbering, checked inside the program.  No GPU is touched: it runs in the CPU suite."""
import os
import subprocess

import pytest

from conftest import REPO
from test_c_host import _build

SRC = os.path.join(REPO, 'tests', 'c_host', 'restrict_host.c')


@pytest.mark.parametrize('side', [1, 2, 9, 100])
def test_c_host_runs_the_children_builder(tmp_path, side):
    exe = _build(str(tmp_path / 'restrict_host'), SRC)
    res = subprocess.run([exe, str(side)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'restrict_host ok' in res.stdout, res.stdout + res.stderr
    assert '%d fine rows, %d coarse rows' % ((2 * side - 1) ** 2, (side - 1) ** 2) in res.stdout
