import os
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'x-transformers-rl_amd'))
os.environ.setdefault('TQDM_DISABLE', '1')


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs an MI355X (runs through the HIP C-ABI library)')


class Golden(dict):
    """The arrays of one fixture by key, with np.load's ``files`` list."""

    @property
    def files(self):
        return list(self)


@pytest.fixture(scope='session')
def golden():
    import numpy as np
    here = REPO / 'tests' / 'golden'

    def load(name):
        """tests/golden/<name>.npz, or its parts <name>.part1.npz, <name>.part2.npz, ... (a fixture
        over the size limit of a committed file is stored in parts, make_golden.save)."""
        one = here / f'{name}.npz'
        paths = [one] if one.exists() else sorted(here.glob(f'{name}.part*.npz'),
                                                  key=lambda p: int(p.name[len(name) + 5:-4]))
        assert paths, f'no golden fixture {name}'
        out = Golden()
        for p in paths:
            with np.load(p, allow_pickle=False) as z:
                out.update({k: z[k] for k in z.files})
        return out
    return load
