"""What the tests of a bank of templates share (tests/test_match_bank_host.py, tests/test_match_bank_gpu.py,
tests/test_match_bank_cli_gpu.py): the class of two exemplars of the planted syllable and the threshold fixed on the float64 model
(test_match_bank_host.py asserts the gap it lies in); the random banks the identity tests run."""
import numpy as np

import match_cases as mc

EXEMPLAR_SEEDS = (1, 4)   # the second planted syllable of each
THRESHOLD = 0.77          # over seeds 2 and 3 the class scores at least 0.885 within a frame of every planted syllable and at most
#                           0.671 more than 12 frames from all of them (float64 model)
SEPARATION = mc.SEPARATION


def exemplar_of(seed, which=1):
    cols, frames = mc.columns64(seed), mc.planted(seed)[1]
    return cols[frames[which]:frames[which] + mc.N].astype(np.float32)


def exemplars():
    """[2, 12, 29] float32: one class"""
    return np.stack([exemplar_of(seed) for seed in EXEMPLAR_SEEDS])


def random_templates(rng, K, n, bins):
    t = (rng.standard_normal((K, n, bins)) * 2).astype(np.float32)
    assert (t < 0).any()
    return t
