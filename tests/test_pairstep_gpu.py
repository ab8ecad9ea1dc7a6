"""The fold kernel's progress words (kernels_fused_s.hip at hop 132; csrc/pair_progress.hpp): the two waves of a SIMD tell each
other which tile they are on, and the one behind runs at the higher priority.  Priority moves WHEN instructions issue, never what
they compute, so every case is held to EQUALITY -- outputs bit for bit (NaN included), flags, the precision guard's work, the
form reported -- between a handle created under SYLDET_FUSED_PAIRSTEP=0 and one created without it, on the same samples.  The
cases are the ones where a partner is absent, shorter, or about to finish: nothing may wait for a word nobody writes."""
import numpy as np
import pytest

import fused_forms as ff
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import nets, synth

pytestmark = pytest.mark.gpu

TILE = 16                                                 # frames per wave and tile (kFusedSTileFrames)
WAVES = 8                                                 # waves a workgroup of the form; wave w shares its SIMD with wave w ^ 4


def _torch():
    import torch
    return torch


def _bits(t):
    return t.contiguous().view(_torch().int32)


def _both(monkeypatch, create, run, want_form):
    """-> [(outputs, flags, fixupStats)] of a handle created under SYLDET_FUSED_PAIRSTEP=0 and of one created without it."""
    torch = _torch()
    res = []
    for switch in ("0", None):
        if switch is None:
            monkeypatch.delenv("SYLDET_FUSED_PAIRSTEP", raising=False)
        else:
            monkeypatch.setenv("SYLDET_FUSED_PAIRSTEP", switch)
        with create() as det:
            det.profile(True)
            out, fl = run(det)
            torch.cuda.synchronize()
            assert util.launched(det) == ["fused_s_kernel"]
            assert det.lastFusedForm() == want_form
            res.append((out, fl, det.fixupStats()))
    monkeypatch.delenv("SYLDET_FUSED_PAIRSTEP", raising=False)
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
    x = torch.from_numpy(_audio(5, 44100 * 2 + 77, 140)).cuda()
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector(cfg, channels=5), lambda det: det.run(x), _form(0))
    _assert_same(a, b)
    assert int(b[1].sum()) > 0


def _wave_tiles(det, cfg, E):
    """Tiles of each wave of a one-channel batch of E evaluations (kernels_fused_s.hip: wave w of workgroup b takes evaluations
    [(8 b + w) seg, +seg), and T - 1 + its evaluations frames in tiles of 16), from the library's own segment length."""
    T = cfg.timeRange
    S = ff.samples_for(cfg, E + T - 1)
    if det.countEvaluations(S) != E:
        return S, None
    seg = det.segmentEvaluations(S)
    lens = [min(seg, E - w * seg) for w in range((E + seg - 1) // seg)]
    return S, [(n + T - 1 + TILE - 1) // TILE for n in lens]


def _find(det, cfg, want):
    for E in range(1, 1200):
        S, tiles = _wave_tiles(det, cfg, E)
        if tiles is not None and len(tiles) <= WAVES and want(tiles):
            return E, S, tiles
    raise AssertionError("no batch length of one workgroup has the wanted wave segments")


PARTNERS = {
    # one wave, one tile: waves 1 .. 7 have no segment; wave 0 reads a word nobody ever writes
    "one_wave_one_tile": lambda t: t == [1],
    # five of the eight waves: wave 0's partner (wave 4) has a single tile against wave 0's several, wave 1's partner has none
    "five_waves": lambda t: len(t) == 5 and t[4] == 1 and t[0] >= 2,
    # all eight: the last wave has one tile against its partner's (wave 3's) full segment
    "short_last_wave": lambda t: len(t) == 8 and t[7] == 1 and t[3] >= 2 and t[3] == t[0],
}


@pytest.mark.parametrize("case", sorted(PARTNERS))
def test_unequal_and_absent_partners(monkeypatch, case):
    """One channel, one workgroup, its length found from segmentEvaluations so that the partners of a SIMD are unequal or absent."""
    torch = _torch()
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=1) as probe:
        E, S, tiles = _find(probe, cfg, PARTNERS[case])
    if case == "one_wave_one_tile":
        assert E == 1
    x = torch.from_numpy(_audio(1, S, 150 + len(tiles))).cuda()

    def run(det):
        assert det.countEvaluations(S) == E
        return det.run(x)
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector(cfg, channels=1), run, _form(0))
    assert b[0].shape[1] == E
    _assert_same(a, b)


def test_gen_form(monkeypatch):
    """The instantiation that takes the network's class as run-time facts."""
    torch = _torch()
    cfg = _gen_cfg(9401)
    x = torch.from_numpy(_audio(3, 132 * 16 * 21 + 300, 160)).cuda()
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector(cfg, channels=3), lambda det: det.run(x), _form(1))
    _assert_same(a, b)


@pytest.mark.parametrize("gen", [0, 1])
def test_two_network_bank(monkeypatch, gen):
    """A bank of two networks (syldet_create_multi), three channels: the multi-network twins of both instantiations."""
    torch = _torch()
    if gen:
        cfgs = [_gen_cfg(9501 + k) for k in range(2)]
    else:
        base = util.sample_net()
        cfgs = [base, nets.perturbed(base, 9601)]
    channel_net = [0, 1, 1]
    x = torch.from_numpy(_audio(3, 132 * 16 * 13 + 500, 170)).cuda()
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector.multi(cfgs, channel_net), lambda det: det.run(x), _form(gen, 1))
    _assert_same(a, b)


def test_same_handle_twice(monkeypatch):
    """The same handle on the same samples twice: the same bits, whichever wave of a pair happened to lead."""
    torch = _torch()
    monkeypatch.delenv("SYLDET_FUSED_PAIRSTEP", raising=False)
    cfg = util.sample_net()
    x = torch.from_numpy(_audio(5, 44100 * 2 + 77, 180)).cuda()
    with sd.SyllableDetector(cfg, channels=5) as det:
        det.profile(True)
        res = []
        for _ in range(2):
            out, fl = det.run(x)
            torch.cuda.synchronize()
            assert util.launched(det) == ["fused_s_kernel"]
            res.append((out.clone(), fl.clone(), det.fixupStats()))
    _assert_same(res[0], res[1])


def test_forty_tiles_a_wave(monkeypatch):
    """Segments of 40 tiles: the priority has changed hands many times by the end.  256 channels make a channel one workgroup of
    eight full wave segments (fused_plan.cpp, fused_segmentation)."""
    torch = _torch()
    cfg = util.sample_net()
    T, C, tiles = cfg.timeRange, 256, 40
    seg = TILE * tiles - (T - 1)
    E = WAVES * seg
    S = ff.samples_for(cfg, E + T - 1)
    g = torch.Generator(device="cuda").manual_seed(4040)
    x = torch.rand((C, S), generator=g, device="cuda", dtype=torch.float32) - 0.5
    x *= torch.logspace(-3, 0, C, device="cuda").reshape(C, 1)          # (channels at levels 60 dB apart)

    def run(det):
        assert det.countEvaluations(S) == E and det.segmentEvaluations(S) == seg
        return det.run(x)
    a, b = _both(monkeypatch, lambda: sd.SyllableDetector(cfg, channels=C), run, _form(0))
    _assert_same(a, b)
