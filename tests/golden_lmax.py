"""The lmax 3 step golden (tools/make_golden_lmax.py): singa_L<L>_B3.npz keeps everything but the element-wise gradient
samples, which live in singa_L<L>_B3_grad_samples.npz (together the two would pass the size limit of a committed file).
`golden` reads such a pair as one archive, and every other golden as tests.helpers.golden does; `reads_split_goldens` makes the
test bodies of other modules, which the odd-degree tests call with their own criteria, read through it."""
import os

import numpy as np

from tests import helpers

ODD = (3,)


class GoldenPair:
    def __init__(self, *archives):
        self._archives = archives
        self.files = [k for z in archives for k in z.files]

    def __getitem__(self, key):
        for z in self._archives:
            if key in z.files:
                return z[key]
        raise KeyError(key)


def golden(name):
    main = helpers.golden(name)
    extra = os.path.join(helpers.GOLDEN, name[:-len(".npz")] + "_grad_samples.npz")
    return GoldenPair(main, np.load(extra)) if os.path.exists(extra) else main


def reads_split_goldens(monkeypatch, *modules):
    for m in modules:
        monkeypatch.setattr(m, "golden", golden)
