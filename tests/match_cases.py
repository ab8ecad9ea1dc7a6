"""What the matching tests share (tests/test_match_host.py, tests/test_match_gpu.py, tests/test_match_cli_gpu.py): the exemplar cut
from one planted recording, the planted recordings it is matched against, and the threshold and separation at which every
planted syllable is found once and nothing else is."""
import numpy as np

import pyoracle as po
import train_cases
import util

N = 12                    # frames of the exemplar: the planted syllable's (train_cases.planted_channel)
THRESHOLD = 0.77          # every planted syllable of seeds 2 to 5 scores at least 0.870 near its position, nothing else above 0.665
SEPARATION = 12
SEEDS = (2, 3)

_cache = {}


def planted(seed):
    """-> (samples float32, the planted syllables' first frames: their first samples / hop, to the nearest frame)"""
    if seed not in _cache:
        x, pos = train_cases.planted_channel(seed)
        _cache[seed] = (x, np.rint(pos / 132.0).astype(np.int64))
    return _cache[seed]


def columns64(seed):
    key = ("cols", seed)
    if key not in _cache:
        _cache[key] = util.oracle_for(util.sample_net()).spectrogram(planted(seed)[0], po.F64)
    return _cache[key]


def exemplar():
    """the 12 frames of seed 1's second planted syllable, float32 [12, 29]"""
    cols, frames = columns64(1), planted(1)[1]
    return cols[frames[1]:frames[1] + N].astype(np.float32)


def found_once(positions, frames, n_positions):
    """does every planted syllable whose window lies inside the recording have exactly one match within 1 frame, and is there no
    other match?"""
    want = [f for f in frames if f + N <= n_positions + N - 1]
    left = list(int(p) for p in positions)
    for f in want:
        near = [p for p in left if abs(p - int(f)) <= 1]
        if len(near) != 1:
            return False
        left.remove(near[0])
    return not left
