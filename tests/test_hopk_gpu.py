"""The fold kernel's compile-time hop (kernels_fused_s.hip, HOP = 132: the ring schedule as constants of the instruction stream)
against the run-time hop it replaces (SYLDET_FUSED_HOPK=0 keeps that one): the same instructions on the same values, so every
case is held to EQUALITY -- outputs bit for bit (NaN included), flags, the precision guard's work -- between a handle created
under the switch and one created without it, on the same samples.  The oracle is the rest of the suite's business (its hop-132
cases run the compile-time form by default)."""
import numpy as np
import pytest

import fused_forms as ff
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import nets, synth

pytestmark = pytest.mark.gpu

TILE = 16                                                 # frames per wave and tile (kFusedSTileFrames)


def _torch():
    import torch
    return torch


def _bits(t):
    return t.contiguous().view(_torch().int32)


def _both(monkeypatch, create, run, want_form=None):
    """-> [(outputs, flags, fixupStats, per-call extras)] of a handle created under SYLDET_FUSED_HOPK=0 and of one created without it."""
    torch = _torch()
    res = []
    for switch in ("0", None):
        if switch is None:
            monkeypatch.delenv("SYLDET_FUSED_HOPK", raising=False)
        else:
            monkeypatch.setenv("SYLDET_FUSED_HOPK", switch)
        with create() as det:
            det.profile(True)
            out, fl = run(det)
            torch.cuda.synchronize()
            assert util.launched(det) == ["fused_s_kernel"]
            if want_form is not None:
                assert det.lastFusedForm() == want_form
            res.append((out, fl, det.fixupStats()))
    monkeypatch.delenv("SYLDET_FUSED_HOPK", raising=False)
    return res


def _assert_same(a, b):
    torch = _torch()
    (a_out, a_fl, a_fix), (b_out, b_fl, b_fix) = a, b
    assert a_out.shape == b_out.shape and a_fl.shape == b_fl.shape
    same = (_bits(a_out) == _bits(b_out)).reshape(a_out.shape[0], -1).all(dim=1)
    assert bool(same.all()), "outputs differ on channels %s" % torch.nonzero(~same).flatten().tolist()[:8]
    assert torch.equal(a_fl, b_fl)
    assert a_fix == b_fix


def _form(gen, mn=0):
    return (2, (4, gen, 1, 8, 0, 1, 1, 0, mn, 0))


def _gen_cfg(seed):
    """256-point frames at hop 132 with a network whose class is run-time facts (LogSig hidden layer, mapstd, two outputs)."""
    return ff.make(seed, 256, 256, 132, 12, 29, 8, 3, n_out=2, rule=1, **ff.RUNTIME)


def _audio(C, S, seed0):
    return np.stack([synth.syllable_channel(S, util.template(), seed=seed0 + c) if c % 2 == 0 else synth.channel(S, seed0 + c)
                     for c in range(C)]).astype(np.float32)


def test_sample_network_bitwise(monkeypatch):
    """The reference's sample network (hop 132) on seeded audio with planted syllables: some flags fire, every bit agrees."""
    torch = _torch()
    cfg = util.sample_net()
    assert cfg.windowLength - cfg.windowOverlap == 132
    x = torch.from_numpy(_audio(5, 44100 * 2 + 77, 40)).cuda()
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector(cfg, channels=5), lambda det: det.run(x), _form(0))
    _assert_same(a, b)
    assert int(b[1].sum()) > 0


@pytest.mark.parametrize("tiles", [1, 2, 3, 4, 5, 8, 9])
def test_segment_lengths(monkeypatch, tiles):
    """Wave segments of 1 .. 9 tiles: shorter than the ring's period of four tiles, one period, two, and each remainder.  With
    2048 channels a channel is cut into one workgroup's eight wave segments (fused_plan.cpp, fused_segmentation), whose stride is
    16 k - (timeRange - 1) evaluations for k tiles: seven segments of k whole tiles and a last one that ends in a ragged tile."""
    torch = _torch()
    cfg = util.sample_net()
    T, C = cfg.timeRange, 2048
    seg = TILE * tiles - (T - 1)
    E = 8 * seg - 5
    S = ff.samples_for(cfg, E + T - 1)
    g = torch.Generator(device="cuda").manual_seed(900 + tiles)
    x = torch.rand((C, S), generator=g, device="cuda", dtype=torch.float32) - 0.5
    x *= torch.logspace(-3, 0, C, device="cuda").reshape(C, 1)          # (channels at levels 60 dB apart)

    def run(det):
        assert det.countEvaluations(S) == E and det.segmentEvaluations(S) == seg
        return det.run(x)
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector(cfg, channels=C), run, _form(0))
    _assert_same(a, b)


def test_gen_form(monkeypatch):
    """The instantiation that takes the network's class as run-time facts."""
    torch = _torch()
    cfg = _gen_cfg(9101)
    x = torch.from_numpy(_audio(4, 132 * 16 * 21 + 300, 60)).cuda()
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector(cfg, channels=4), lambda det: det.run(x), _form(1))
    _assert_same(a, b)


@pytest.mark.parametrize("gen", [0, 1])
def test_multi_network_twins(monkeypatch, gen):
    """A bank of three networks, a network per channel: the multi-network twins of both instantiations."""
    torch = _torch()
    if gen:
        cfgs = [_gen_cfg(9201 + k) for k in range(3)]
    else:
        base = util.sample_net()
        cfgs = [base] + [nets.perturbed(base, 9300 + k) for k in range(1, 3)]
    channel_net = [(2 * c + 1) % 3 for c in range(7)]
    x = torch.from_numpy(_audio(7, 132 * 16 * 13 + 500, 80)).cuda()
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector.multi(cfgs, channel_net), lambda det: det.run(x), _form(gen, 1))
    _assert_same(a, b)


def test_click_over_quiet_cage(monkeypatch):
    """Full-scale clicks over quiet cages: the precision guard appends work items (a branch the compile-time form keeps), and the
    two handles recompute the same evaluations.  Every frame carries its own scale on this kernel, so a click 120 dB over its cage
    (channel 1) is held on the grid; the guard speaks where a window's frames are more than 2^45 apart (channel 0: the cage at
    1e-15) and for what no grid holds (channel 2: the click is an infinite sample)."""
    torch = _torch()
    cfg = util.sample_net()
    S = 132 * 16 * 19 + 400
    xh = np.stack([synth.channel(S, 70 + c) * q for c, q in enumerate((1e-15, 1e-6, 1e-6))]).astype(np.float32)
    xh[0, 9000] = 1.0
    xh[1, 20011] = -1.0
    xh[2, 132 * 16 * 8 + 3] = np.inf
    x = torch.from_numpy(xh).cuda()
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector(cfg, channels=3), lambda det: det.run(x), _form(0))
    _assert_same(a, b)
    assert b[2][0] > 0 and b[2][1] == 0
