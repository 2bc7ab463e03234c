"""Worker of tests/test_forcing_gpu.py: square_forced (J_time = 3, J_space = 5) on the
ranks torch.distributed.run started (gloo, sharing the box's GPU); rank 0 writes what the
forcing adds -- B u, B^T K g, f, the solve with its history, both error numbers -- to
STK_FORCING_OUT for the test to compare with its one-rank run."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'spacetime-fullgrid-parallel_amd'))

from source.comm import MPI  # noqa: E402
from test_forcing_gpu import _forced_run  # noqa: E402


def main():
    comm = MPI.COMM_WORLD
    assert comm.Get_size() > 1
    got = _forced_run(comm, 3, 5)
    comm.Barrier()
    if comm.Get_rank() == 0:
        np.savez(os.environ['STK_FORCING_OUT'], **got)
        print('mp_forcing_worker ok: %d ranks, %d iterations' % (comm.Get_size(), got['iters']))


if __name__ == '__main__':
    main()
