import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, 'tests', 'golden')

# The CPU results the golden fixtures pin depend on the intra-op thread count (it sets the reduction split of the CPU
# convolutions, and the tiny networks amplify the fp32 round-off); the fixtures agree with 8 threads.  Every test process,
# and the worker processes the tests start, uses 8 whatever the machine has.
CPU_THREADS = 8
os.environ['OMP_NUM_THREADS'] = str(CPU_THREADS)
torch.set_num_threads(CPU_THREADS)


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs a real MI355X (run with -m gpu on the GPU box)')


@pytest.fixture(scope='session')
def golden():
    import numpy as np

    class G:
        def __getitem__(self, name):
            return np.load(os.path.join(GOLDEN, name + '.npz'))
    return G()
