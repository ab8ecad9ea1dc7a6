"""What the tests of a ragged bank share (tests/test_match_ragged_host.py, tests/test_match_ragged_gpu.py,
tests/test_match_ragged_cli_gpu.py): the random ragged banks, and the class of two exemplars of DIFFERENT lengths of the planted
syllable whose anchors mark the same frame of the syllable, with the threshold fixed on the float64 model
(test_match_ragged_host.py asserts the gap it lies in)."""
import numpy as np

import match_cases as mc

LENGTHS = (1, 12, 17, 5, 12)
CLASSES = (0, 0, 1, 0, 2)
ANCHORS = (0, 3, 16, 4, 0)

# the chain: exemplar 0 is all 12 frames of seed 1's second planted syllable, anchored at its last frame; exemplar 1 the last 10
# frames of seed 4's second planted syllable, anchored at ITS last frame: both anchors are frame 11 of the syllable
EXEMPLARS = ((1, 0, 12), (4, 2, 12))     # (seed, first frame within the syllable, end frame within the syllable)
MARK = 11                                # the frame of the syllable an event names
THRESHOLD = 0.77                         # over seeds 2 and 3 (float64 model) the class scores at least 0.876 within a frame of every planted
#                                          syllable's frame 11 and at most 0.674 more than 12 frames from all of them
SEPARATION = mc.SEPARATION


def exemplars():
    """-> (a list of two float32 arrays [12, 29] and [10, 29], their anchors)"""
    out, anchors = [], []
    for seed, lo, hi in EXEMPLARS:
        cols, frames = mc.columns64(seed), mc.planted(seed)[1]
        out.append(cols[frames[1] + lo:frames[1] + hi].astype(np.float32))
        anchors.append(MARK - lo)
    return out, anchors


def random_templates(rng, lengths, bins):
    t = [(rng.standard_normal((n, bins)) * 2).astype(np.float32) for n in lengths]
    assert any((x < 0).any() for x in t)
    return t


def found_once(frames_found, planted_frames, n_frames):
    """does every planted syllable whose 12 frames lie inside the recording have exactly one event within 1 frame of its frame
    MARK, and is there no other event?"""
    want = [int(f) + MARK for f in planted_frames if f + mc.N <= n_frames]
    left = [int(p) for p in frames_found]
    for f in want:
        near = [p for p in left if abs(p - f) <= 1]
        if len(near) != 1:
            return False
        left.remove(near[0])
    return not left
