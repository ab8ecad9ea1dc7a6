"""The fold kernel's evaluation stage after its exact trims (kernels_fused_s.hip): the row statistics read as pairs where the form
uses no more, the output map multiplied by an exact reciprocal where the gain is a power of two (csrc/exact_reciprocal.hpp).
Neither may change a bit, of an output or of the decision `Double(output) >= threshold`.

Two shapes on the reference's sample network (hop 132: the instantiation with the compile-time hop), small enough for seconds:
    2 channels x (132 * 47 + 256) samples    48 frames, 39 evaluations a channel; the launcher cuts so short a channel into wave
                                             segments of one tile each (fused_plan.cpp, fused_segmentation), so every tile is a
                                             segment's first and last
    3 channels x (132 * 600 + 256) samples   601 frames, 592 evaluations a channel, in wave segments of three tiles: seams between
                                             segments, carried rows between a segment's tiles, a ragged last tile
Each is held against the oracle (1e-5, flags equal), against a dump of outputs and flags the PARENT commit's build wrote for the
same inputs (tests/golden/fold_eval_parent.npz: byte for byte), and, with the threshold put on, beside and between values the
kernel itself produced and at +-inf and NaN, against `Double(output) >= threshold` on its own outputs at every evaluation.
The output map: a gain of 0.5 and of 2^-126 (multiplied by 2 and by 2^126), and of 3 (no power of two: divided)."""
import hashlib
import os

import numpy as np
import pytest

import pyoracle as po
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import nets, synth

pytestmark = pytest.mark.gpu

SHAPES = {"one_tile_segments": (2, 132 * 47 + 256), "three_tile_segments": (3, 132 * 600 + 256)}
FORM = (2, (4, 0, 1, 8, 0, 1, 1, 0, 0, 0))                # the twice-folded example-class form on eight waves, one network
PARENT_DUMP = os.path.join(util.GOLD, "fold_eval_parent.npz")


def _torch():
    import torch
    return torch


def inputs(name):
    """The shape's audio: planted syllables on the even channels (flags fire), other audio at another level on the odd ones."""
    C, S = SHAPES[name]
    return np.stack([synth.syllable_channel(S, util.template(), seed=210 + c) if c % 2 == 0 else synth.channel(S, 220 + c) * 0.4
                     for c in range(C)]).astype(np.float32)


def run_fold(cfg, x):
    """-> (outputs [C, E, n_out] float32, flags [C, E] uint8) of one batch call, which must be the fold kernel's in FORM."""
    torch = _torch()
    with sd.SyllableDetector(cfg, channels=x.shape[0]) as det:
        det.profile(True)
        out, fl = det.run(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        assert util.launched(det) == ["fused_s_kernel"]
        assert det.lastFusedForm() == FORM
        return out.cpu().numpy(), fl.cpu().numpy()


_CACHE = {}


def _base(name):
    """The shape's inputs, the sample network's outputs and flags on them, the oracle's fp64 outputs and flags: computed once."""
    if name not in _CACHE:
        cfg = util.sample_net()
        assert cfg.windowLength - cfg.windowOverlap == 132
        x = inputs(name)
        out, fl = run_fold(cfg, x)
        o = util.oracle_for(cfg)
        runs = [o.run(x[c], po.F64, cfg.rule) for c in range(x.shape[0])]
        _CACHE[name] = (cfg, x, out, fl, np.stack([r[2] for r in runs]), np.stack([np.asarray(r[1]) for r in runs]))
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_against_the_oracle(name):
    cfg, x, out, fl, w64, wfl = _base(name)
    assert out.shape == w64.shape and out.shape[1] == (x.shape[1] - 256) // 132 + 1 - (cfg.timeRange - 1)
    util.assert_outputs_close(out, w64, util.TOL)
    # flags EQUAL: no fp64 output of these inputs lies within the bar of the threshold, so no fp32 result within 1e-5 may decide otherwise
    thr = float(cfg.thresholds[0])
    assert (np.abs(w64[..., 0] - thr) > 2 * util.TOL * np.maximum(1.0, np.abs(w64[..., 0]))).all()
    assert np.array_equal(fl.astype(bool), wfl.astype(bool).reshape(fl.shape))
    assert int(fl.sum()) < fl.size and (int(fl.sum()) > 0) == (name == "three_tile_segments")      # (48 frames are too few for a syllable)
    util.assert_flags_follow_outputs(fl, out, cfg.thresholds, cfg.rule)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_same_bits_as_the_parent_build(name):
    """Outputs and flags byte for byte what the parent commit's library wrote for the same inputs."""
    _, x, out, fl, _, _ = _base(name)
    z = np.load(PARENT_DUMP)
    assert z[name + "_samples_sha256"].item() == hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
    assert out.dtype == np.float32 and z[name + "_outputs"].dtype == np.uint32 and fl.dtype == z[name + "_flags"].dtype == np.uint8
    assert np.array_equal(out.view(np.uint32), z[name + "_outputs"])
    assert np.array_equal(fl, z[name + "_flags"])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_threshold_edge(name):
    """The threshold on three values the kernel produced, one double above and below each, strictly between each and the next
    float, and at +inf, -inf and NaN: the flags are `Double(output) >= threshold` of the kernel's own outputs, everywhere."""
    cfg, x, out, _, _, _ = _base(name)
    vals = np.unique(out[0, :, 0][np.isfinite(out[0, :, 0])])
    assert len(vals) >= 3
    picks = [vals[0], vals[len(vals) // 2], vals[-1]]
    thrs = [np.inf, -np.inf, np.nan]
    for v in picks:
        d, nxt = np.float64(v), np.float64(np.nextafter(v, np.float32(np.inf)))
        between = d + (nxt - d) * 0.375
        assert d < between < nxt
        thrs += [float(d), float(np.nextafter(d, np.inf)), float(np.nextafter(d, -np.inf)), float(between)]
    seen = set()
    for thr in thrs:
        o2, f2 = run_fold(nets.variant(cfg, thresholds=[thr]), x)
        assert np.array_equal(o2.view(np.uint32), out.view(np.uint32)), "the threshold %r moved output values" % thr
        util.assert_flags_follow_outputs(f2, o2, [thr], cfg.rule)
        seen.add((int(f2.sum()) > 0, int(f2.sum()) < f2.size))
    assert seen == {(True, True), (True, False), (False, True)}          # some thresholds split the values, -inf passes all, +inf and NaN none


def _with_gain(cfg, gain, thr):
    c = nets.variant(cfg, thresholds=[thr])
    fn = c.net.outputProcessing
    assert len(fn) == 1 and fn[0].function == "mapminmax" and np.asarray(fn[0].gains).shape == (1,)
    fn[0].gains = np.array([gain], np.float32)
    return c


@pytest.mark.parametrize("gain", [0.5, 3.0, 2.0 ** -126], ids=["half", "three", "two_to_minus_126"])
def test_output_gain(gain):
    """The reverse output map (y - y0) / gain + x0 under a gain whose reciprocal is exact (0.5; 2^-126, the smallest normal float:
    outputs of up to 2^127) and under one that has to be divided by (3): against the oracle, and the decision on the CPU."""
    cfg0, x, _, _, w64_0, _ = _base("three_tile_segments")
    assert float(np.asarray(cfg0.net.outputProcessing[0].gains)[0]) == 2.0     # (the sample network's own gain is a power of two)
    # a threshold in the middle of channel 0's outputs under this gain: x0 + (y - y0) / gain of the base run's median
    f0 = cfg0.net.outputProcessing[0]
    y_med = (np.median(w64_0[0, :, 0]) - float(np.asarray(f0.xOffsets)[0])) * 2.0 + float(f0.y)
    thr = float(np.asarray(f0.xOffsets)[0]) + (y_med - float(f0.y)) / float(np.float32(gain))
    cfg = _with_gain(cfg0, gain, thr)
    out, fl = run_fold(cfg, x)
    o = util.oracle_for(cfg)
    w64 = np.stack([o.run(x[c], po.F64, cfg.rule)[2] for c in range(x.shape[0])])
    assert np.isfinite(out).all() and np.isfinite(w64).all()
    if gain >= 0.5:
        util.assert_outputs_close(out, w64, util.TOL)
    else:
        # 2^-126: the map's slope is 2^126, and it scales whatever error the network's output y carries exactly (a power of two,
        # x0 == 0): the project's bar of 1e-5 is for values at the network's scale, so it is held THERE -- both sides times the
        # gain, which is exact in fp32 and fp64 -- instead of relative to outputs of 1e35 that are differences y - y0 of nearly equal
        # numbers (the plain bar measured 0.031 here: the cancellation in y - y0, not the map).  The bits are not tied to the gain-0.5
        # run's: so steep a map sends evaluations to the exact recomputation behind the kernel (the precision guard's bound
        # divides by the gain), whose values are other floats within the bar.
        assert float(np.asarray(f0.xOffsets)[0]) == 0.0
        util.assert_outputs_close(out.astype(np.float64) * gain, w64 * gain, util.TOL)
    util.assert_flags_follow_outputs(fl, out, cfg.thresholds, cfg.rule)
    assert 0 < int(fl[0].sum()) < fl[0].size
