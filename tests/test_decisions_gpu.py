"""The decision itself, on every kernel and host path that writes or moves a flag: the flag is the reference's comparison
`Double(output) >= threshold` (SyllableDetector.swift:27-31; any output against its own threshold: TrackDetector.swift:72-77)
applied to the float the engine ITSELF produced -- a pure function of that float and a double, so every check here is exact
and no evaluation is excluded (util.assert_flags_follow_outputs).

Every case runs twice.  Pass 1 with arbitrary thresholds gives the engine's outputs; pass 2 puts a threshold exactly ON a
value output k produced on channel 0 ("at": must fire) or one double above it ("above": a double no float holds, so a kernel
that rounds the threshold to float, or compares with `>`, decides differently), every other output's threshold at 1e30.
Thresholds must not move values: pass 2's outputs are pass 1's, bit for bit."""
import numpy as np
import pytest

import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth
from syllable_detector_swift_amd.bank import ShardedSyllableDetectorBank
from syllable_detector_swift_amd.config import SyllableDetectorConfig, frequencyIndexRange

pytestmark = pytest.mark.gpu

FAR = 1e30                     # a threshold no output reaches


def _torch():
    import torch
    return torch


def _np(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


def _input(C, S, hop=132, nan_in=None):
    """Channel 0 with planted syllables (outputs spread), the others other audio at other levels (no two channels share
    values); `nan_in`: a channel that gets one NaN sample."""
    rows = [synth.syllable_channel(S, util.template(), seed=4, hop=hop)]
    for c in range(1, C):
        rows.append((synth.syllable_channel(S, util.template(), seed=4 + c, hop=hop) if c % 2 else synth.channel(S, 30 + c))
                    * (0.37 if c % 2 else 2.5))
    x = np.stack(rows).astype(np.float32)
    if nan_in is not None:
        x[nan_in, S // 2] = np.nan
    return x


def _same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32
    same = a.view(np.uint32) == b.view(np.uint32)
    assert same.all(), "thresholds moved %d output values, first at %s" % ((~same).sum(), np.argwhere(~same)[0])


def _once(open_det, thr, xd, call, expect):
    with open_det(thr) as det:
        det.profile(True)
        out, fl = call(det, xd)
        _torch().cuda.synchronize()
        expect(det)
        return _np(out), _np(fl)


def _value(col, pick=None):
    """A value the output really produced, at about the 80th percentile of the finite ones -- of the DISTINCT ones, so that a
    saturating output layer's ties cannot put it on the largest value: both flag values occur."""
    ok = np.isfinite(col) if pick is None else (np.isfinite(col) & pick)
    cand = np.unique(col[ok])
    assert cand.size >= 10, cand.size
    return cand[int(0.8 * (cand.size - 1))]


def _edges(open_det, x, n_out, rule, expect, call=None, chan_thr=None, own=None, base=None, pick=None, want_nan=False):
    """The two passes (module docstring).  open_det(thresholds of channel 0's network) -> a detector; expect(det) asserts the
    kernel that ran; call(det, samples on the device) -> (outputs, flags); chan_thr(thresholds) -> what the helper gets
    ([n_out], or [C, n_out] where channels have networks of their own); own: the rows that share channel 0's thresholds;
    pick(pass 1's outputs) -> the evaluations of channel 0 a threshold may be taken from."""
    xd = _torch().from_numpy(x).cuda()
    call = call or (lambda det, xd: det.run(xd))
    chan_thr = chan_thr or (lambda thr: np.asarray(thr, np.float64))
    base = list(base) if base is not None else [0.1 + 0.05 * k for k in range(n_out)]
    out1, fl1 = _once(open_det, base, xd, call, expect)
    assert out1.shape[0] == x.shape[0] and out1.shape[2] == n_out and out1.dtype == np.float32
    own = slice(None) if own is None else own
    util.assert_flags_follow_outputs(fl1, out1, chan_thr(base), rule)
    assert bool(np.isnan(out1).any()) == want_nan
    mask = None if pick is None else pick(out1)
    vs = [_value(out1[0, :, k], mask) for k in range(n_out)]
    for k in range(n_out):
        v = vs[k]
        nxt = np.nextafter(v, np.float32(np.inf))
        assert nxt.dtype == np.float32
        for kind in ("at", "above"):
            thr = [FAR] * n_out
            thr[k] = float(v) if kind == "at" else float(np.nextafter(np.float64(v), np.inf))
            assert np.float64(np.float32(thr[k])) != thr[k] or kind == "at"           # (above: no float holds it)
            out2, fl2 = _once(open_det, thr, xd, call, expect)
            _same_bits(out1, out2)                                                     # (a)
            util.assert_flags_follow_outputs(fl2, out2, chan_thr(thr), rule)           # (b): every evaluation of every channel
            col = out2[0, :, k]
            at = col.view(np.uint32) == v.view(np.uint32)                              # (c)
            assert at.any(), (k, kind)
            with np.errstate(invalid="ignore"):
                hi = col >= nxt
            if rule == 1 or k == 0:
                assert hi.any() and fl2[0][hi].all(), (k, kind)
                if kind == "at":
                    assert fl2[0][at].all(), (k, kind)
                    assert fl2.min() == 0 and fl2.max() == 1, (k, kind)
                else:
                    assert not fl2[0][at].any(), (k, kind)
            else:
                # rule "first": output k crosses its threshold and no flag fires
                assert (col.astype(np.float64) >= thr[k]).any() and not fl2[own].any(), (k, kind)
    if n_out > 1:
        thr = [float(v) for v in vs]                                                   # every output at a value of its own
        out2, fl2 = _once(open_det, thr, xd, call, expect)
        _same_bits(out1, out2)
        util.assert_flags_follow_outputs(fl2, out2, chan_thr(thr), rule)
        at0 = out2[0, :, 0].view(np.uint32) == vs[0].view(np.uint32)
        assert at0.any() and fl2[0][at0].all() and fl2.max() == 1
    return out1


def _names_are(*names):
    def expect(det):
        assert util.launched(det) == list(names), util.launched(det)
    return expect


def _plain(cfg, C, engine=_abi.ENGINE_AUTO):
    return lambda thr: sd.SyllableDetector(nets.variant(cfg, thresholds=list(thr)), channels=C, engine=engine)


def _fused_s_size(hop):
    return 64 * hop * 3 + 999                      # three tiles and a ragged tail


# ---- the fused kernels ------------------------------------------------------------------------------------------------------
def test_fold_kernel_example_network(monkeypatch):
    """fused_s_kernel, the reference's example network (the form without the general output stage), one output."""
    util.select_fused(monkeypatch, "fused_s_kernel")
    cfg = util.sample_net()
    _edges(_plain(cfg, 3), _input(3, _fused_s_size(132)), 1, 0, _names_are("fused_s_kernel"))


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("H,n_out,hop,chain", [(4, 2, 132, ("l2normalize", "mapminmax")), (8, 3, 132, ("l2normalize", "mapminmax")),
                                               (12, 4, 132, ("l2normalize", "mapstd")), (16, 4, 64, ()),
                                               (4, 3, 64, ("l2normalize", "mapminmax")), (7, 2, 100, ("l2normalize",))])
def test_fold_kernel_general_output_stage(monkeypatch, H, n_out, hop, chain, rule):
    """fused_s_kernel's general form: each output's threshold in its lane group (or read back from the table of lane-group
    constants, 5 .. 8 hidden units on eight waves), `counts` for the rule, the hits merged across lane groups.  Hidden widths
    of one to four quads, a hop that is a multiple of 64 and hops that are not."""
    util.select_fused(monkeypatch, "fused_s_kernel")
    rng = np.random.default_rng(1000 * H + n_out)
    net = nets.random_net(rng, 290, (H,), n_out, transfer=("TanSig", "TanSig") if not chain else ("TanSig", "PureLin"),
                          in_fns=chain, out_fns=("mapminmax",) if H % 2 == 0 else ())
    cfg = nets.variant(util.sample_net(), net=net, windowOverlap=256 - hop, rule=rule)
    _edges(_plain(cfg, 2), _input(2, _fused_s_size(hop), hop=hop) * np.float32(1.0 if chain else 0.05), n_out, rule, _names_are("fused_s_kernel"))


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("n_out", [1, 4])
@pytest.mark.parametrize("kernel", ["fused_r_kernel", "fused_kernel"])
def test_older_fused_kernels(monkeypatch, kernel, n_out, rule):
    """fused_r_kernel (SYLDET_FUSED_NOFOLD=1) and fused_kernel (SYLDET_FUSED_CLASSIC=1) take the example class with one and
    with four outputs; n_out = 1 is the example network itself (the form without the general output stage)."""
    util.select_fused(monkeypatch, kernel)
    base = util.sample_net()
    if n_out == 1:
        cfg = nets.variant(base, rule=rule)
    else:
        net = nets.random_net(np.random.default_rng(40 + n_out), 290, (4,), n_out, in_fns=("l2normalize", "mapminmax"), out_fns=("mapstd",))
        cfg = nets.variant(base, net=net, rule=rule)
    _edges(_plain(cfg, 2), _input(2, _fused_s_size(132)), n_out, rule, _names_are(kernel))


# ---- the single-output kernels of the generic engine's fast forms --------------------------------------------------------
def _framed(N, hop, lo, hi, T, H, window=_abi.WINDOW_HAMMING, seed=0):
    f0, f1 = frequencyIndexRange(N, 44100.0, lo, hi)
    net = nets.random_net(np.random.default_rng(seed + N + T), (f1 - f0) * T, (H,), 1, in_fns=("l2normalize", "mapminmax"), out_fns=("mapminmax",))
    return SyllableDetectorConfig(44100.0, N, N, N - hop, (lo, hi), T, "linear", [0.4], net, window=window)


@pytest.mark.parametrize("which", ["fft1k", "bdft four hops", "bdft two hops", "mlp_mfma"])
def test_single_output_matrix_core_kernels(monkeypatch, which):
    """fft1k_net_kernel (BASELINE configs[2] with the block transform switched off), bdft_net_kernel on frames of four and of
    two hops, mlp_mfma_kernel behind the FFT: each reads thresholds[0] itself."""
    monkeypatch.delenv("SYLDET_NO_BDFT", raising=False)
    monkeypatch.delenv("SYLDET_NO_FFT1K", raising=False)
    if which == "fft1k":
        monkeypatch.setenv("SYLDET_NO_BDFT", "1")
        cfg, names = nets.config3(), ["fft1k_net_kernel"]
    elif which == "bdft four hops":
        cfg, names = _framed(1024, 256, 2000.0, 7000.0, 10, 4, window=_abi.WINDOW_HANNING), ["bdft_net_kernel"]
    elif which == "bdft two hops":
        cfg, names = _framed(512, 256, 2000.0, 7000.0, 10, 4), ["bdft_net_kernel"]
    else:
        cfg, names = _framed(256, 64, 500.0, 7300.0, 12, 2), None
    hop = cfg.windowLength - cfg.windowOverlap
    S = cfg.windowLength + hop * 700 + 37
    x = _input(3, S, nan_in=2 if which != "fft1k" else None)

    def expect(det):
        got = util.launched(det)
        assert (got == names) if names else (got[-1] == "mlp_mfma_kernel"), got
    _edges(_plain(cfg, 3), x, 1, 0, expect, want_nan=which != "fft1k")


# ---- the generic engine's interpretive kernels ------------------------------------------------------------------------------
def _interpretive_kernel(cfg):
    """Which of its three kernels launch_mlp_generic (kernels_generic.hip) starts for `cfg` -- syldet_timings lists all three as
    "mlp_generic_kernel", so the test restates the rule for the shapes it uses: a normaliser first, at most two layers and eight
    outputs, <= 320 inputs and <= 8 hidden units -> the register-resident kernels; of those, [l2normalize,] one affine map, two
    layers, at most two outputs and one output map -> mlp_chain_kernel, else mlp_small_kernel; anything else mlp_generic_kernel."""
    net = cfg.net
    fns = [f.function for f in net.inputProcessing]
    normalised = bool(fns) and fns[0] in ("l2normalize", "normalize", "normalizestd")
    L = net.layers
    if not (normalised and len(L) <= 2 and L[-1].outputs <= 8 and L[0].inputs <= 320 and L[0].outputs <= 8):
        return "mlp_generic_kernel"
    affine_last = fns[-1] in ("mapminmax", "mapstd")
    chain = len(L) == 2 and L[-1].outputs <= 2 and len(net.outputProcessing) <= 1 and affine_last and \
        (fns[:-1] == ["l2normalize"] or len(fns) == 1)
    return "mlp_chain_kernel" if chain else "mlp_small_kernel"


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("kernel,n_out", [("mlp_chain_kernel", 1), ("mlp_chain_kernel", 2), ("mlp_small_kernel", 1), ("mlp_small_kernel", 3),
                                          ("mlp_generic_kernel", 1), ("mlp_generic_kernel", 3)])
def test_interpretive_kernels_of_the_generic_engine(kernel, n_out, rule):
    """SYLDET_ENGINE_GENERIC: mlp_chain_kernel (the training script's chain; it holds at most two outputs), mlp_small_kernel
    (three outputs, or a normalize chain), mlp_generic_kernel via mlp_eval_wave (no normaliser) -- net_thresholds(n, c) with
    `lim = rule == 0 ? 1 : n_out` and its restatements."""
    rng = np.random.default_rng(7 * n_out + len(kernel))
    chain = {"mlp_chain_kernel": ("l2normalize", "mapminmax"),
             "mlp_small_kernel": ("l2normalize", "mapminmax") if n_out == 3 else ("normalize", "mapminmax"),
             "mlp_generic_kernel": ("mapminmax",)}[kernel]
    cfg = nets.variant(util.sample_net(), net=nets.random_net(rng, 290, (4,), n_out, in_fns=chain, out_fns=("mapminmax",)), rule=rule)
    assert _interpretive_kernel(cfg) == kernel

    def expect(det):
        assert det.geometry.engine == _abi.ENGINE_GENERIC and util.launched(det)[-1] == "mlp_generic_kernel", util.launched(det)
    _edges(_plain(cfg, 3, engine=_abi.ENGINE_GENERIC), _input(3, 132 * 1500 + 333, nan_in=1), n_out, rule, expect, want_nan=True)


# ---- the wide engine ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,rule", [("config5", 0), ("config5_shape32", 0), ("config5_m32", 0), ("H96_3out_logsig", 0), ("H96_3out_logsig", 1)])
def test_wide_gemm_kernels(monkeypatch, shape, rule):
    """wide_gemm16_kernel (one output and three), wide_gemm_kernel (SYLDET_WIDE_SHAPE32=1), wide_gemm32s_kernel
    (SYLDET_WIDE_M32=1): the opt-in bf16 engine's epilogues."""
    for name in ("SYLDET_WIDE_SHAPE32", "SYLDET_WIDE_M32", "SYLDET_WIDE_TANH_POLY", "SYLDET_WIDE_NO_FRONT"):
        monkeypatch.delenv(name, raising=False)
    base = nets.from_npz()
    gemm = "wide_gemm16_kernel"
    if shape == "config5_shape32":
        monkeypatch.setenv("SYLDET_WIDE_SHAPE32", "1")
        gemm = "wide_gemm_kernel"
    if shape == "config5_m32":
        monkeypatch.setenv("SYLDET_WIDE_M32", "1")
        gemm = "wide_gemm32s_kernel"
    if shape.startswith("config5"):
        cfg, n_out = nets.wide_mlp(base), 1
    else:
        net = nets.random_net(np.random.default_rng(3), 290, (96,), 3, transfer=("LogSig", "TanSig"))
        cfg, n_out = nets.variant(base, net=net, rule=rule), 3

    def expect(det):
        assert det.geometry.engine == _abi.ENGINE_WIDE_BF16
        assert [k for k in util.launched(det) if k.startswith("wide_gemm")] == [gemm], util.launched(det)
    _edges(_plain(cfg, 3, engine=_abi.ENGINE_WIDE_BF16), _input(3, 70000), n_out, rule, expect)


# ---- the exact recomputation ---------------------------------------------------------------------------------------------------
def test_exact_recomputation_behind_the_fold_kernel(monkeypatch):
    """fixup_kernel (mlp_eval_wave): a recording ten times full scale through a network without a normaliser.  The thresholds
    sit on evaluations the recomputation REWROTE: those whose output differs from a run of the same input with the guard off
    (SYLDET_NO_GUARD=1)."""
    torch = _torch()
    util.select_fused(monkeypatch, "fused_s_kernel")
    cfg = nets.variant(util.sample_net(), net=nets.random_net(np.random.default_rng(3), 290, (4,), 1, in_fns=()))
    S = 132 * 700 + 256
    x = (synth.channels(2, S, first=1) * np.array([[10.0], [3.0]])).astype(np.float32)
    monkeypatch.setenv("SYLDET_NO_GUARD", "1")
    with sd.SyllableDetector(cfg, channels=2) as det:
        raw, _ = det.run(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        assert det.fixupStats()[0] == 0
        raw = raw.cpu().numpy()
    monkeypatch.delenv("SYLDET_NO_GUARD")

    def expect(det):
        assert [n for n, _ in det.lastTimings()] == ["fused_s_kernel", "fixup_kernel"], det.lastTimings()
        assert det.fixupStats()[0] > 0 and det.fixupStats()[1] == 0

    def rewritten(out1):
        diff = out1[0, :, 0].view(np.uint32) != raw[0, :, 0].view(np.uint32)
        assert diff.sum() >= 10, diff.sum()
        return diff
    _edges(_plain(cfg, 2), x, 1, 0, expect, pick=rewritten)


# ---- a network per channel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["fold", "generic"])
def test_multi_network_bank(engine):
    """syldet_create_multi, three networks with different thresholds, channels interleaved, channel 0 on network 1: the edge
    threshold goes into network 1 only, the helper gets each channel's own network's thresholds -- and the same flags against
    network 0's thresholds for every channel must FAIL.  The fold kernel (SD_NET(thresholds)), and the generic engine on a
    three-output network (mlp_small_kernel's net_thresholds(n, c)), both rules."""
    C = 5
    channel_net = np.array([1, 0, 2, 1, 0])
    if engine == "fold":
        base, n_out, rules, eng = util.sample_net(), 1, (0,), _abi.ENGINE_AUTO
        S, expect = _fused_s_size(132), _names_are("fused_s_kernel")
    else:
        net = nets.random_net(np.random.default_rng(11), 290, (4,), 3, in_fns=("l2normalize", "mapminmax"), out_fns=("mapminmax",))
        base, n_out, rules, eng = nets.variant(util.sample_net(), net=net), 3, (0, 1), _abi.ENGINE_GENERIC
        assert _interpretive_kernel(base) == "mlp_small_kernel"
        S = 132 * 1200 + 333

        def expect(det):
            assert det.geometry.engine == _abi.ENGINE_GENERIC and util.launched(det)[-1] == "mlp_generic_kernel", util.launched(det)
    others = {0: [-1e6] * n_out, 2: [0.1 + 0.05 * k for k in range(n_out)]}
    x = _input(C, S, nan_in=4)
    for rule in rules:
        def cfgs_for(thr):
            return [nets.variant(nets.perturbed(base, 50 + k) if k else base, thresholds=list(thr) if k == 1 else others[k], rule=rule)
                    for k in range(3)]

        def chan_thr(thr):
            return np.asarray([list(thr) if k == 1 else others[k] for k in channel_net], np.float64)
        seen = []

        def call(det, xd):
            out, fl = det.run(xd)
            seen.append((out, fl))
            return out, fl
        _edges(lambda thr: sd.SyllableDetector.multi(cfgs_for(thr), channel_net, engine=eng), x, n_out, rule, expect, call=call,
               chan_thr=chan_thr, own=np.nonzero(channel_net == 1)[0], base=[0.2] * n_out, want_nan=True)
        # the last variant's flags against network 0's thresholds on every channel: must not pass
        out, fl = (_np(t) for t in seen[-1])
        with pytest.raises(AssertionError, match="do not follow"):
            util.assert_flags_follow_outputs(fl, out, np.asarray([others[0]] * C, np.float64), rule)


def _with_band(base, lo, hi, fourier_length=None, hidden=4, seed=0, in_fns=("l2normalize", "mapminmax"), **changes):
    N = fourier_length or base.fourierLength
    f0, f1 = sd.frequencyIndexRange(N, base.samplingRate, lo, hi)
    net = nets.random_net(np.random.default_rng(seed), (f1 - f0) * base.timeRange, (hidden,), 1, in_fns=in_fns)
    return nets.variant(base, fourierLength=N, freqRange=(lo, hi), net=net, thresholds=[0.1], **changes)


@pytest.mark.parametrize("first", ["fold class", "generic class"])
def test_mixed_bank(first):
    """syldet_create_mixed, two classes (the example network on the fold kernel; 512-point frames with log columns behind
    normalize on the generic engine), channels interleaved: each class launch writes the bank's rows through row_of.  Channel 0
    -- whose network gets the edge threshold -- once on the fold class, once on the generic one."""
    base = util.sample_net()
    wide512 = _with_band(base, 1000.0, 9000.0, fourier_length=512, hidden=8, seed=2, in_fns=("normalize", "mapminmax"), spectrogramScaling="log")
    cfgs = [base, wide512] if first == "fold class" else [wide512, base]
    channel_net = np.array([0, 1, 0, 1, 1])
    C = len(channel_net)
    other = [0.3]

    def expect(det):
        names = util.launched(det)
        assert names.count("fused_s_kernel") == 1 and "mlp_generic_kernel" in names, names
        engines = [det.channelGeometry(c).engine for c in range(C)]
        fold = 0 if first == "fold class" else 1
        assert engines == [_abi.ENGINE_FUSED if k == fold else _abi.ENGINE_GENERIC for k in channel_net], engines
    _edges(lambda thr: sd.SyllableDetector.mixed([nets.variant(cfgs[0], thresholds=list(thr)), nets.variant(cfgs[1], thresholds=other)], channel_net),
           _input(C, 132 * 900 + 311), 1, 0, expect,
           chan_thr=lambda thr: np.asarray([list(thr) if k == 0 else other for k in channel_net], np.float64),
           own=np.nonzero(channel_net == 0)[0])


# ---- other inputs -----------------------------------------------------------------------------------------------------------------
def test_pcm16_input_on_the_fold_kernel(monkeypatch):
    """run with int16 samples, read natively by the fold kernel (rows of whole words: an even length)."""
    torch = _torch()
    util.select_fused(monkeypatch, "fused_s_kernel")
    x = _input(2, _fused_s_size(132) + 1)
    x16 = np.clip(np.rint(x / np.abs(x).max() * 20000.0), -32768, 32767).astype(np.int16)
    xd16 = torch.from_numpy(x16).cuda()
    _edges(_plain(util.sample_net(), 2), x, 1, 0, _names_are("fused_s_kernel"), call=lambda det, xd: det.runPCM16(xd16))


def test_a_nan_sample_on_the_fold_kernel(monkeypatch):
    """Flags are 0 exactly where outputs are NaN (the helper's rule: a NaN never hits), whatever the threshold."""
    util.select_fused(monkeypatch, "fused_s_kernel")
    out = _edges(_plain(util.sample_net(), 2), _input(2, _fused_s_size(132), nan_in=1), 1, 0, _names_are("fused_s_kernel"), want_nan=True)
    assert 0 < np.isnan(out[1]).sum() < 40 and not np.isnan(out[0]).any()


@pytest.mark.parametrize("engine", [_abi.ENGINE_AUTO, _abi.ENGINE_GENERIC])
def test_non_finite_thresholds(monkeypatch, engine):
    """-inf, +inf and NaN thresholds pass through the C struct as they are and give what Double >= Double gives: every
    evaluation that is not NaN fires; none fires; none fires.  No layer of the library refuses them (the reference does not)."""
    torch = _torch()
    util.select_fused(monkeypatch, "fused_s_kernel")
    x = _input(2, _fused_s_size(132), nan_in=1)
    xd = torch.from_numpy(x).cuda()
    for thr in (-np.inf, np.inf, np.nan):
        cfg = nets.variant(util.sample_net(), thresholds=[thr])
        c_abi, keep = cfg.to_abi()
        got = c_abi.thresholds[0]
        assert np.float64(got).tobytes() == np.float64(thr).tobytes()
        del keep
        with sd.SyllableDetector(cfg, channels=2, engine=engine) as det:
            det.profile(True)
            out, fl = det.run(xd)
            torch.cuda.synchronize()
            assert util.launched(det)[-1] == ("fused_s_kernel" if engine == _abi.ENGINE_AUTO else "mlp_generic_kernel")
            out, fl = out.cpu().numpy(), fl.cpu().numpy()
        nan = np.isnan(out[..., 0])
        assert nan.any() and not nan.all()
        util.assert_flags_follow_outputs(fl, out, [thr], 0)
        assert np.array_equal(fl, (~nan).astype(np.uint8) if thr == -np.inf else np.zeros_like(fl))


# ---- entry points: the example network on the fold kernel ---------------------------------------------------------------------
def _edge_thresholds(cfg, x):
    """(v_0, [(kind, threshold)], outputs of the device run): thresholds on and one double above a value channel 0 produced."""
    torch = _torch()
    with sd.SyllableDetector(cfg, channels=x.shape[0]) as det:
        det.profile(True)
        out, _ = det.run(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        assert util.launched(det) == ["fused_s_kernel"]
        out = out.cpu().numpy()
    v = _value(out[0, :, 0])
    return v, [("at", float(v)), ("above", float(np.nextafter(np.float64(v), np.inf)))], out


def _device_run(cfg, x):
    torch = _torch()
    with sd.SyllableDetector(cfg, channels=x.shape[0]) as det:
        out, fl = det.run(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        return out.cpu().numpy(), fl.cpu().numpy()


def _check_entry(out, fl, want_out, want_fl, thr, v, kind, what):
    _same_bits(want_out, np.ascontiguousarray(out))
    util.assert_flags_follow_outputs(fl, out, [thr], 0)
    assert np.array_equal(fl, want_fl), what
    at = out[0, :, 0].view(np.uint32) == v.view(np.uint32)
    assert at.any() and (fl[0][at] == (1 if kind == "at" else 0)).all(), what
    assert fl.min() == 0 and fl.max() == 1, what


def test_host_and_interleaved_entry_points(monkeypatch):
    """run on host buffers with the pipeline cut into several stages (SYLDET_HOST_CHUNK_BYTES) and runInterleaved (device and
    host): flags follow their own outputs and are the device run's, seams included."""
    torch = _torch()
    util.select_fused(monkeypatch, "fused_s_kernel")
    base = util.sample_net()
    C, hop = 3, 132
    x = _input(C, 256 + 1300 * hop + 77)
    v, edges, _ = _edge_thresholds(base, x)
    for kind, thr in edges:
        cfg = nets.variant(base, thresholds=[thr])
        want_out, want_fl = _device_run(cfg, x)
        monkeypatch.setenv("SYLDET_HOST_CHUNK_BYTES", str(C * 4 * hop * 300))
        with sd.SyllableDetector(cfg, channels=C) as det:
            out, fl = det.runHost(x)
            _check_entry(out, fl, want_out, want_fl, thr, v, kind, "pipelined host call")
        monkeypatch.delenv("SYLDET_HOST_CHUNK_BYTES")
        with sd.SyllableDetector(cfg, channels=C) as det:
            frames = np.ascontiguousarray(x.T)
            out, fl = det.runInterleaved(torch.from_numpy(frames).cuda())
            torch.cuda.synchronize()
            _check_entry(out.cpu().numpy(), fl.cpu().numpy(), want_out, want_fl, thr, v, kind, "runInterleaved")
            out, fl = det.runInterleavedHost(frames)
            _check_entry(out, fl, want_out, want_fl, thr, v, kind, "runInterleavedHost")


@pytest.mark.parametrize("channels,devices,ranks", [(5, [0, 0, 0], 0), (5, [0], 1), (2, [0, 0, 0], 0)])
def test_sharded_banks(monkeypatch, channels, devices, ranks):
    """The sharded bank's pack -> exchange -> unpack of flags: ragged channel blocks over three shards with the copy exchange,
    one RCCL rank, and the time-axis split (two channels over three shards: flags stitched across the seams).  Every shard's
    own flags against its own outputs, the gathered flags on every device against the outputs put together, all equal to the
    plain bank's."""
    util.select_fused(monkeypatch, "fused_s_kernel")
    base = util.sample_net()
    x = _input(channels, 256 + 900 * 132 + 77)
    S = x.shape[1]
    v, edges, _ = _edge_thresholds(base, x)
    for kind, thr in edges:
        cfg = nets.variant(base, thresholds=[thr])
        want_out, want_fl = _device_run(cfg, x)
        with ShardedSyllableDetectorBank(cfg, channels, devices) as bank:
            outs, fls, alls = bank.run(bank.scatter(x), S)
            bank.synchronize()
            assert bank.rcclRanks == ranks
            whole = np.full_like(want_out, np.nan)
            for i, s in enumerate(bank.shards):
                _, _, e0, cnt = bank.ranges(i, S)
                o, f = outs[i].cpu().numpy(), fls[i].cpu().numpy()
                util.assert_flags_follow_outputs(f, o, [thr], 0)
                whole[s.first_channel:s.first_channel + s.channels, e0:e0 + cnt] = o
            for i in range(len(bank.shards)):
                _check_entry(whole, alls[i].cpu().numpy(), want_out, want_fl, thr, v, kind, "gathered flags on shard %d's device" % i)
            out, fl = bank.runHost(x)
            _check_entry(out, fl, want_out, want_fl, thr, v, kind, "the bank's host call")


def test_streaming_decisions(monkeypatch):
    """appendAudioData in uneven chunks, then processNewValue (behind processAll on every other chunk, on its own on the
    others): after EVERY evaluation lastDetected is the rule on lastOutputs against the threshold; the steps that land on v_0
    report 1 with the threshold on it and 0 with the threshold one double above.  Channel 1's last third goes through
    seenSyllable: the OR over exactly the evaluations it consumed."""
    util.select_fused(monkeypatch, "fused_s_kernel")
    base = util.sample_net()
    C = 2
    x = _input(C, 132 * 400 + 256)
    S = x.shape[1]
    v, edges, _ = _edge_thresholds(base, x)
    for kind, thr in edges:
        cfg = nets.variant(base, thresholds=[thr])
        want_out, want_fl = _device_run(cfg, x)
        on_v = int((want_out[0, :, 0].view(np.uint32) == v.view(np.uint32)).sum())
        assert on_v > 0
        with sd.SyllableDetector(cfg, channels=C) as det:
            rng = np.random.default_rng(1)
            done = [0, 0]
            on_edge = 0
            pos, chunk = 0, 0
            while pos < S:
                n = min(int(rng.integers(1, 3000)), S - pos)
                for c in range(C):
                    det.appendAudioData(x[c, pos:pos + n], c)
                pos += n
                chunk += 1
                if chunk % 2:
                    det.processAll()
                for c in range(C):
                    if c == 1 and pos > 2 * S // 3:
                        e1 = max(det.countEvaluations(pos), 0)
                        assert det.seenSyllable(c) == bool(want_fl[c, done[c]:e1].any()), (done[c], e1)
                        assert det.pendingEvaluations(c) == 0
                        done[c] = e1
                        continue
                    while det.processNewValue(c):
                        last = np.asarray(det.lastOutputsFor(c), np.float32)
                        e = done[c]
                        assert last.view(np.uint32)[0] == want_out[c, e].view(np.uint32)[0], (c, e)
                        hit = int(det.lastDetectedFor(c))
                        assert hit == int(util.flags_from_outputs(last[None, :], [thr], 0)[0]) == int(want_fl[c, e]), (c, e)
                        if c == 0 and last.view(np.uint32)[0] == v.view(np.uint32):
                            assert hit == (1 if kind == "at" else 0)
                            on_edge += 1
                        done[c] += 1
            assert done[0] == done[1] == want_out.shape[1] > 0
            assert on_edge == on_v
