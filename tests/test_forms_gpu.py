"""Every compiled instantiation of the three fused kernels against the fp64 anchor (tests/fused_forms.py has the table, and
tests/test_forms_host.py proves it complete): each case runs its configuration, asks the library which instantiation ran
(syldet_last_fused_form) and holds every channel to its own network's anchor under the suite's one rule
(util.check_with_evidence: the contract's 1e-5, evidence beyond it, flags that follow the outputs, NaN where the anchor has NaN).
The fold kernel's network leaves also run as a bank of two networks (the multi-network twin), the 16-bit leaves on int16 rows,
the spectrogram leaves through syldet_spectrogram_device.  Two batch lengths a case: a partial first tile, and one that spans
more wave segments than a workgroup has waves and ends in a ragged tile."""
import numpy as np
import pytest

import fused_forms as ff
import pyoracle as po
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import nets, synth

pytestmark = pytest.mark.gpu

CHANNELS = 3
NET_OF = [0, 1, 0]


def _inputs(cfg, frames):
    """Three channels: planted syllables, the same with a x0.004 level step in the middle of a 16-frame tile and three evaluation
    windows of exact silence (0/0 in l2normalize / normalizestd, a constant window in normalize), and noise."""
    gap, hop = ff.geometry(cfg)
    S = ff.samples_for(cfg, frames)
    x = np.stack([synth.syllable_channel(S, util.template(), seed=31, hop=hop), synth.syllable_channel(S, util.template(), seed=32, hop=hop),
                  synth.channel(S, 5)]).astype(np.float32)
    step = gap + (16 * (frames // 24) + 5) * hop + hop // 2 + 3
    x[1, step:] *= np.float32(0.004)
    quiet = 3 * ((cfg.timeRange - 1) * hop + cfg.windowLength)
    x[1, S // 5: S // 5 + quiet] = 0.0
    return x


def _with_thresholds(cfg, o, x):
    """Thresholds inside the range the network produces on x, so that flags of both values occur.  Rule 0 looks at output 0 alone:
    its median.  Rule 1 fires when ANY output reaches its threshold: with each at its output's 1 - 1 / (2 n_out) quantile at least
    1 / (2 n_out) and at most half of the evaluations fire, however the outputs move against each other (medians of two outputs in
    antiphase would fire on every evaluation)."""
    w64 = o.run(x, po.F64, cfg.rule)[2]
    ok = np.isfinite(w64).all(axis=1)
    q = 0.5 if cfg.rule == 0 else 1.0 - 0.5 / w64.shape[1]
    return nets.variant(cfg, thresholds=[float(t) for t in np.quantile(w64[ok], q, axis=0)])


class Reference:
    """The anchors of one case, computed once on the long batch (the short one is its first samples: an evaluation depends on
    its own window alone) and left unchanged."""

    def __init__(self, cfgs, x, net_of):
        self.x = x
        self.cfgs = [_with_thresholds(c, util.oracle_for(c), x[net_of.index(k)]) for k, c in enumerate(cfgs)]
        self.oracles = [util.oracle_for(c) for c in self.cfgs]
        self.net_of = net_of
        self.w64, self.w32 = [], []
        for c in range(x.shape[0]):
            o, cfg = self.oracles[net_of[c]], self.cfgs[net_of[c]]
            self.w64.append(o.run(x[c], po.F64, cfg.rule)[2])
            self.w32.append(o.run(x[c], po.F32, cfg.rule)[0])

    def check(self, out, fl, S):
        E = out.shape[1]
        both = False
        for c in range(self.x.shape[0]):
            o, cfg = self.oracles[self.net_of[c]], self.cfgs[self.net_of[c]]
            assert E == o.count_evals(S)
            err, wide = util.check_with_evidence(o, cfg, self.x[c, :S], out[c], fl[c], w64=self.w64[c][:E], w32=self.w32[c][:E])
            print("  channel %d: %d evaluations, worst error %.3g%s" % (c, E, err, ", widened %s" % wide if wide else ""))
            both |= bool(0 < fl[c].sum() < fl[c].size)
        return both


def _spans(det, leaf, S, frames):
    """The long batch really spans more wave segments than a workgroup has waves (the fold kernel; two passes' segments for the
    older kernels) and ends in a ragged tile -- from the library's own segmenting rule."""
    E, seg = det.countEvaluations(S), det.segmentEvaluations(S)
    assert seg > 0
    segments = -(-E // seg)
    assert segments >= (leaf[1][ff.S_NW] + 1 if leaf[0] == 2 else 2), (E, seg, segments)
    assert frames % 16 != 0 and det.countFrames(S) == frames


def _run_network_case(case, cfgs, net_of, leaf, monkeypatch):
    import torch
    ff.apply_env(monkeypatch, case.env)
    fa, fb = ff.sizes(case.cfg, case.leaf)
    x = _inputs(case.cfg, fb)
    if case.s16:
        x16 = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
        x = x16.astype(np.float32) * np.float32(2.0 ** -15)                  # what a 16-bit sample means, exactly
    ref = Reference(cfgs, x, net_of)
    make = (lambda: sd.SyllableDetector(ref.cfgs[0], channels=CHANNELS)) if len(cfgs) == 1 else (lambda: sd.SyllableDetector.multi(ref.cfgs, net_of))
    both = False
    with make() as det:
        for frames in (fa, fb):
            S = ff.samples_for(case.cfg, frames)
            S -= S & 1 if case.s16 else 0                                    # (int16 rows of whole words)
            if case.s16:
                out, fl = det.runPCM16(torch.from_numpy(np.ascontiguousarray(x16[:, :S])).cuda())
            else:
                out, fl = det.run(torch.from_numpy(np.ascontiguousarray(x[:, :S])).cuda())
            torch.cuda.synchronize()
            assert det.lastFusedForm() == leaf, "prediction and launch disagree"
            out, fl = out.cpu().numpy(), fl.cpu().numpy()
            if frames == fb:
                _spans(det, leaf, S, frames)
            both |= ref.check(out, fl, S)
            if case.s16:
                # ... and the fp32 path's bits on the widened samples (tests/test_pcm16_gpu.py's rule)
                o32, f32 = det.run(torch.from_numpy(np.ascontiguousarray(x[:, :S])).cuda())
                torch.cuda.synchronize()
                p = list(leaf[1])
                p[ff.S_S16] = 0
                assert det.lastFusedForm() == (2, tuple(p))
                assert np.array_equal(out.view(np.uint32), o32.cpu().numpy().view(np.uint32)) and np.array_equal(fl, f32.cpu().numpy())
    assert both, "no channel has flags of both values: the thresholds are outside the produced range"


NETWORK_CASES = [c for c in ff.CASES if not c.spect]
SPECT_CASES = [c for c in ff.CASES if c.spect]
FOLD_NETWORK_CASES = [c for c in NETWORK_CASES if c.leaf[0] == 2]


@pytest.mark.parametrize("case", NETWORK_CASES, ids=[c.name for c in NETWORK_CASES])
def test_leaf_against_the_anchor(oracle_lib, case, monkeypatch):
    _run_network_case(case, [case.cfg], [0, 0, 0], case.leaf, monkeypatch)


@pytest.mark.parametrize("case", FOLD_NETWORK_CASES, ids=[c.name for c in FOLD_NETWORK_CASES])
def test_multi_network_twin_against_the_anchors(oracle_lib, case, monkeypatch):
    """The same case as a bank of two networks of its class, channels alternating: the leaf's MN = 1 twin, every channel held to
    its own network's anchor."""
    p = list(case.leaf[1])
    p[ff.S_MN] = 1
    _run_network_case(case, [case.cfg, ff.sibling(case, 99)], NET_OF, (2, tuple(p)), monkeypatch)


def _check_columns(det, cfg, x, leaf):
    import torch
    cols = det.spectrogram(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    torch.cuda.synchronize()
    assert det.lastFusedForm() == leaf, "prediction and launch disagree"
    cols = cols.cpu().numpy()
    o = util.oracle_for(cfg)
    for c in range(x.shape[0]):
        want = o.spectrogram(x[c], po.F64)
        print("  channel %d: %d frames, worst column error %.3g" % (c, want.shape[0], float((np.abs(cols[c] - want) / util.column_scale(want)).max())))
        util.assert_columns_close(cols[c], want)


@pytest.mark.parametrize("case", SPECT_CASES, ids=[c.name for c in SPECT_CASES])
def test_spectrogram_leaf_against_the_anchor(oracle_lib, case, monkeypatch):
    ff.apply_env(monkeypatch, case.env)
    fa, fb = ff.sizes(case.cfg, case.leaf)
    x = _inputs(case.cfg, fb)
    with sd.SyllableDetector(case.cfg, channels=CHANNELS) as det:
        for frames in (fa, fb):
            _check_columns(det, case.cfg, x[:, :ff.samples_for(case.cfg, frames)], case.leaf)


@pytest.mark.parametrize("b", ff.BAND_CASES, ids=[b.name for b in ff.BAND_CASES])
def test_band_edges_of_the_fold_kernels_tables(oracle_lib, b, monkeypatch):
    """fused_plan.cpp builds the folded bases, the parity offsets, the lone-sample row and the DC row on the host, in tiles of
    sixteen rows: DC inside the band, odd and even first bins, 1 .. 64 bins, a band that ends at N/2 - 1 -- as a network
    (3 hidden units, timeRange 2) and, where the fold kernel has a spectrogram form for the shape, the columns themselves."""
    import torch
    from syllable_detector_swift_amd.config import frequencyIndexRange
    r = frequencyIndexRange(b.cfg.fourierLength, b.cfg.samplingRate, *b.cfg.freqRange)
    assert (r[0], r[1] - r[0]) == (b.f0, b.F)
    ff.apply_env(monkeypatch, {})
    fa, fb = ff.sizes(b.cfg, b.leaf)
    x = _inputs(b.cfg, fb)
    ref = Reference([b.cfg], x, [0, 0, 0])
    try:
        spect_leaf = sd.fusedFormOfConfig(b.cfg, CHANNELS, x.shape[1], spectrogram=True)
    except sd.SyllableDetectorError:
        spect_leaf = None
    assert (spect_leaf is not None and spect_leaf[0] == 2) == (b.cfg.fourierLength == 256 and b.F <= 32)
    with sd.SyllableDetector(ref.cfgs[0], channels=CHANNELS) as det:
        for frames in (fa, fb):
            S = ff.samples_for(b.cfg, frames)
            out, fl = det.run(torch.from_numpy(np.ascontiguousarray(x[:, :S])).cuda())
            torch.cuda.synchronize()
            assert det.lastFusedForm() == b.leaf
            ref.check(out.cpu().numpy(), fl.cpu().numpy(), S)
        if spect_leaf is not None and spect_leaf[0] == 2:
            _check_columns(det, b.cfg, x, spect_leaf)


def test_a_failed_dry_run_leaves_the_next_launch_real(oracle_lib, monkeypatch):
    """syldet_fused_form_of_config on a configuration it refuses, then a real batch on the same thread: it reaches the device."""
    import torch
    ff.apply_env(monkeypatch, {})
    case = next(c for c in ff.CASES if c.name == "s_f2_exact")
    with pytest.raises(sd.SyllableDetectorError):
        sd.fusedFormOfConfig(nets.variant(case.cfg, windowLength=1024), CHANNELS, 40000)
    x = _inputs(case.cfg, 40)
    ref = Reference([case.cfg], x, [0, 0, 0])
    with sd.SyllableDetector(ref.cfgs[0], channels=CHANNELS) as det:
        with pytest.raises(sd.SyllableDetectorError):
            det.lastFusedForm()                                              # (no call through this handle yet)
        out, fl = det.run(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        assert det.lastFusedForm() == case.leaf
        ref.check(out.cpu().numpy(), fl.cpu().numpy(), x.shape[1])
