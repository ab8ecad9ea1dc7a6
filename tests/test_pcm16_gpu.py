"""16-bit PCM on the device: every *_s16 entry point against its fp32 twin on the same handle, fed float(x) * 2^-15 with the
same strides.  The conversion is exact and every engine runs the fp32 kernels on the converted samples, so the contract is
EQUALITY: outputs as bit patterns (NaN included), flags, detections and the exact recomputation's work items."""
import os
import subprocess

import numpy as np
import pytest

import util
import wavutil
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth
from syllable_detector_swift_amd.bank import PinnedArray

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
WIDEN = "widen_s16_kernel"


def _torch():
    import torch
    return torch


def _bits(t):
    torch = _torch()
    if isinstance(t, np.ndarray):
        return t.view(np.int32) if t.dtype == np.float32 else t
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _to_f32(x16):
    """what the fp32 entry points are given for 16-bit PCM: float(x) * 2^-15 (exact)"""
    if isinstance(x16, np.ndarray):
        return x16.astype(np.float32) * np.float32(2.0 ** -15)
    return x16.float() * (2.0 ** -15)


def _pcm(C, S, seed=0, cfg=None):
    """C rows of 16-bit PCM, one kind a row in turn: planted syllables (flags fire), noise, silence, alternating full scale,
    isolated clicks."""
    rng = np.random.default_rng(seed)
    cfg = cfg or util.sample_net()
    rows = []
    for c in range(C):
        kind = c % 5
        if kind == 0:
            r = np.clip(np.round(synth.syllable_channel(S, util.template(), seed=seed + c) * 32768.0), -32768, 32767)
        elif kind == 1:
            r = rng.integers(-32768, 32768, S)
        elif kind == 2:
            r = np.zeros(S)
        elif kind == 3:
            r = np.where(np.arange(S) % 2 == 0, 32767, -32768)
        else:
            r = np.zeros(S)
            r[rng.integers(0, S, max(1, S // 3000))] = rng.choice([32767, -32768, 20000, -1], max(1, S // 3000))
        rows.append(r.astype(np.int16))
    return np.stack(rows)


def _assert_same(o16, f16, o32, f32):
    torch = _torch()
    if isinstance(o16, np.ndarray):
        assert np.array_equal(_bits(o16), _bits(o32)) and np.array_equal(f16, f32)
    else:
        assert torch.equal(_bits(o16), _bits(o32)) and torch.equal(f16, f32)


def _compare_device(det, x16, x32, native):
    """runPCM16 against run on the same handle: equal bits, flags, detections, work items.  native: the s16 call's kernels are
    the fp32 call's, fused_s_kernel among them and no widening pass (the fold kernel's s16 form); otherwise the widening pass and
    then the fp32 call's kernels.  Returns (the fp32 call's kernels, its work items, flags)."""
    torch = _torch()
    det.profile(True)
    o32, f32 = det.run(x32)
    torch.cuda.synchronize()
    items32 = det.fixupStats()
    names32 = util.launched(det)
    o16, f16 = det.runPCM16(x16)
    torch.cuda.synchronize()
    items16 = det.fixupStats()
    names16 = util.launched(det)
    _assert_same(o16, f16, o32, f32)
    assert items16 == items32 and items32[1] == 0
    if native:
        assert names16 == names32 and "fused_s_kernel" in names16 and WIDEN not in names16, (names16, names32)
    else:
        assert names16 == [WIDEN] + names32, (names16, names32)
    i16, c16 = det.detections(f16)
    i32, c32 = det.detections(f32)
    torch.cuda.synchronize()
    assert torch.equal(c16, c32)
    for c in range(c32.shape[0]):                               # (the first counts[c] entries of a row are written)
        n = min(int(c32[c]), i32.shape[1])
        assert torch.equal(i16[c, :n], i32[c, :n]), c
    return names32, items32[0], f32


def _single(cfg, x16np, native, engine=_abi.ENGINE_AUTO):
    torch = _torch()
    x16 = torch.from_numpy(x16np).cuda()
    with sd.SyllableDetector(cfg, channels=x16np.shape[0], engine=engine) as det:
        return _compare_device(det, x16, _to_f32(x16), native)


def _gen_chain(base, n_out=2, seed=3):
    F = base.net.inputs // base.timeRange
    net = nets.random_net(np.random.default_rng(seed), F * base.timeRange, (4,), n_out, transfer=("LogSig", "TanSig"),
                          in_fns=("l2normalize", "mapstd"))
    return nets.variant(base, net=net, thresholds=[0.3] * n_out)


def _three_classes():
    """test_mixed_gpu's set: sample.txt, a narrower band, 512-point frames behind normalize with log columns, a second network
    of sample.txt's class"""
    base = util.sample_net()

    def band(lo, hi, N=None, hidden=4, seed=0, in_fns=("l2normalize", "mapminmax"), **kw):
        N = N or base.fourierLength
        f0, f1 = sd.frequencyIndexRange(N, base.samplingRate, lo, hi)
        net = nets.random_net(np.random.default_rng(seed), (f1 - f0) * base.timeRange, (hidden,), 1, in_fns=in_fns)
        return nets.variant(base, fourierLength=N, freqRange=(lo, hi), net=net, thresholds=[0.1], **kw)
    return [base, band(2000.0, 5000.0, seed=1),
            band(1000.0, 9000.0, N=512, hidden=8, seed=2, in_fns=("normalize", "mapminmax"), spectrogramScaling="log"),
            nets.perturbed(base, 5)]


S_SHORT = 132 * 600 + 256


def test_sample_net_on_the_fold_kernel():
    names, _, fl = _single(util.sample_net(), _pcm(5, S_SHORT, seed=1), native=True)
    assert names == ["fused_s_kernel"]
    assert int(fl[0].sum()) > 0                                # the planted syllables fire


def test_gen_chain_with_two_outputs_on_the_fold_kernel():
    names, _, _ = _single(_gen_chain(util.sample_net()), _pcm(5, S_SHORT, seed=2), native=True)
    assert names == ["fused_s_kernel"]


def test_multi_network_bank():
    torch = _torch()
    base = util.sample_net()
    x16 = torch.from_numpy(_pcm(5, S_SHORT, seed=3)).cuda()
    with sd.SyllableDetector.multi([base, nets.perturbed(base, 5)], [0, 1, 0, 1, 1]) as det:
        names, _, _ = _compare_device(det, x16, _to_f32(x16), native=True)
    assert names == ["fused_s_kernel"]
    gen = _gen_chain(base)                                      # (the GEN chain's multi-network form)
    with sd.SyllableDetector.multi([gen, nets.perturbed(gen, 6)], [1, 0, 0, 1, 0]) as det:
        names, _, _ = _compare_device(det, x16, _to_f32(x16), native=True)
    assert names == ["fused_s_kernel"]


def test_mixed_bank_widens_once_for_all_classes():
    torch = _torch()
    cfgs = _three_classes()
    x16 = torch.from_numpy(_pcm(6, S_SHORT, seed=4)).cuda()
    x32 = _to_f32(x16)
    with sd.SyllableDetector.mixed(cfgs, [0, 1, 2, 3, 0, 2]) as det:
        det.profile(True)
        o32, f32 = det.run(x32)
        torch.cuda.synchronize()
        items32, names32 = det.fixupStats(), util.launched(det)
        o16, f16 = det.runPCM16(x16)
        torch.cuda.synchronize()
        items16, names16 = det.fixupStats(), util.launched(det)
    _assert_same(o16, f16, o32, f32)
    assert items16 == items32
    # the two fold-kernel classes read the int16 rows in place; the 512-point class reads the one widened copy
    assert names16.count(WIDEN) == 1 and [n for n in names16 if n != WIDEN] == names32, (names16, names32)
    assert names32.count("fused_s_kernel") == 2 and len(names32) >= 3, names32


def test_exact_recomputation_gives_the_same_items_and_bits():
    """No normaliser and a first layer scaled up: full-scale int16 sends windows to fixup_kernel on the fp32 path; the s16 call
    recomputes the same items and writes the same bits."""
    base = util.sample_net()
    net = nets.random_net(np.random.default_rng(3), base.net.inputs, (4,), 1, in_fns=())
    net.layers[0].weights = (net.layers[0].weights * np.float32(64.0)).astype(np.float32)
    cfg = nets.variant(base, net=net)
    x = _pcm(5, 132 * 2000 + 256, seed=5)
    x[1] = (x[1] // 256).astype(np.int16)                       # a quiet row ...
    x[1, 100000:100400] = 32767                                 # ... with a loud stretch inside
    names, items, _ = _single(cfg, x, native=True)            # (fixup_kernel reads the int16 rows too)
    assert names == ["fused_s_kernel"] and items > 0


@pytest.mark.parametrize("case", ["hop128", "hop64", "hop192", "window128", "hop131", "frames1024", "wide_bf16"])
def test_each_engine(case):
    base = util.sample_net()
    rng = np.random.default_rng(7)
    engine, C, S = _abi.ENGINE_AUTO, 5, S_SHORT
    if case == "hop128":
        cfg = nets.variant(base, windowOverlap=128)
    elif case == "hop64":
        cfg = nets.variant(base, windowOverlap=256 - 64)
    elif case == "hop192":                                      # (a multiple of 64 where the padding does not fit: the plain ring)
        cfg = nets.variant(base, windowOverlap=256 - 192)
    elif case == "window128":
        F = base.net.inputs // base.timeRange
        f0, f1 = sd.frequencyIndexRange(128, base.samplingRate, *base.freqRange)
        cfg = nets.variant(base, fourierLength=128, windowLength=128, windowOverlap=64,
                           net=nets.random_net(rng, (f1 - f0) * base.timeRange, (4,), 1))
        del F
    elif case == "hop131":
        cfg = nets.variant(base, windowOverlap=256 - 131)
    elif case == "frames1024":
        cfg, C, S = nets.config3(), 3, 1024 + 256 * 300
    else:
        F = base.net.inputs // base.timeRange
        cfg = nets.variant(base, net=nets.random_net(rng, F * base.timeRange, (40,), 1, transfer=("SatLin", "PureLin"),
                                                     in_fns=("normalize",), out_fns=()))
        engine, C = _abi.ENGINE_WIDE_BF16, 3
    names, _, _ = _single(cfg, _pcm(C, S, seed=8), case == "hop192", engine)
    if case in ("hop128", "hop64", "hop192", "window128"):      # widened: CS8, the padded ring, K2 = 2; hop 192 reads int16
        assert names == ["fused_s_kernel"], names
    elif case == "hop131":                                      # the generic engine
        assert names[0] in ("stft_lanes_kernel", "stft_generic_kernel") and not any(n.startswith("fused") for n in names), names
    elif case == "frames1024":
        assert names in (["bdft_net_kernel"], ["fft1k_net_kernel"]), names
    else:
        assert names[-1].startswith("wide_gemm"), names


@pytest.mark.parametrize("layout", ["wide_stride", "odd_stride", "offset_base"])
def test_layouts(layout):
    torch = _torch()
    C, S = 5, S_SHORT
    pad = {"wide_stride": 64, "odd_stride": 1, "offset_base": 8}[layout]
    big16 = torch.from_numpy(_pcm(C, S + pad, seed=9)).cuda()
    big32 = _to_f32(big16)
    off = 1 if layout == "offset_base" else 0
    x16, x32 = big16[:, off:off + S], big32[:, off:off + S]
    assert x16.stride(0) == S + pad and x32.stride(0) == S + pad
    for k, cfg in enumerate((util.sample_net(), nets.variant(util.sample_net(), windowOverlap=256 - 131), nets.config3())):
        # (the fold kernel's s16 form wants rows of whole 4-byte words: an even stride and a 4-byte aligned base)
        with sd.SyllableDetector(cfg, channels=C) as det:
            _compare_device(det, x16, x32, native=(k == 0 and layout == "wide_stride"))


def test_host_pipeline_and_interleaved(monkeypatch):
    torch = _torch()
    C, S = 4, 132 * 1500 + 256
    cfgs = [util.sample_net(), _three_classes()[2]]
    x16 = _pcm(C, S, seed=10)
    x32 = _to_f32(x16)
    monkeypatch.setenv("SYLDET_HOST_CHUNK_BYTES", str(C * S * 4 // 4))     # >= 3 stages (read at create)
    for k, cfg in enumerate(cfgs):
        with sd.SyllableDetector(cfg, channels=C) as det:
            det.profile(True)
            E = det.countEvaluations(S)
            o32, f32 = det.runHost(x32)
            det.profile(True, history=8)                        # (drops what the fp32 call recorded)
            o16, f16 = det.runPCM16Host(x16)
            _assert_same(o16, f16, o32, f32)
            # each stage is a profiled call: at least three of them, each natively (sample.txt) or through the widening pass
            stages = [det.timingsOf(i) for i in range(8)]
            stages = [[n for n, _ in st] for st in stages if st]
            assert 3 <= len(stages) < 8, stages
            for st in stages:
                assert (WIDEN in st) == (k == 1) and ("fused_s_kernel" in st) == (k == 0), st
            # page-locked input and results
            px = PinnedArray(x16.shape, np.int16)
            px.array[...] = x16
            po_, pf = PinnedArray((C, E, det.geometry.outputs), np.float32), PinnedArray((C, E), np.uint8)
            det.runPCM16Host(px.array, po_.array, pf.array)
            _assert_same(po_.array.copy(), pf.array.copy(), o32, f32)
            px.free(); po_.free(); pf.free()
            # interleaved, host and device
            fr16 = np.ascontiguousarray(x16.T)
            fr32 = np.ascontiguousarray(x32.T)
            io32, if32 = det.runInterleavedHost(fr32)
            io16, if16 = det.runInterleavedPCM16Host(fr16)
            _assert_same(io16, if16, io32, if32)
            do32, df32 = det.runInterleaved(torch.from_numpy(fr32).cuda())
            do16, df16 = det.runInterleavedPCM16(torch.from_numpy(fr16).cuda())
            torch.cuda.synchronize()
            _assert_same(do16, df16, do32, df32)
            assert (WIDEN in util.launched(det)) == (k == 1)


def test_streaming_appends():
    C = 3
    cfg = util.sample_net()
    x16 = _pcm(C, 132 * 300 + 256, seed=11)
    x32 = _to_f32(x16)
    S = x16.shape[1]
    results = []
    for pcm in (False, True):
        got = [[] for _ in range(C)]
        seen = []
        with sd.SyllableDetector(cfg, channels=C) as det:
            rng = np.random.default_rng(12)
            pos = 0
            while pos < S:
                n = int(rng.integers(1, 4000))
                blk = slice(pos, min(S, pos + n))
                if rng.integers(0, 2):
                    if pcm:
                        det.appendInterleavedDataPCM16(np.ascontiguousarray(x16[:, blk].T))
                    else:
                        det.appendInterleavedData(np.ascontiguousarray(x32[:, blk].T))
                else:
                    for c in range(C):
                        if pcm:
                            det.appendAudioDataPCM16(x16[c, blk], c)
                        else:
                            det.appendAudioData(x32[c, blk], c)
                pos = blk.stop
                det.processAll()
                for c in range(C):
                    while det.processNewValue(c):
                        got[c].append(np.asarray(det.lastOutputsFor(c), np.float32))
            for c in range(C):
                seen.append(det.seenSyllable(c))
        results.append(([np.stack(g) if g else np.zeros((0, 1), np.float32) for g in got], seen))
    (g32, s32), (g16, s16) = results
    for c in range(C):
        assert g16[c].shape == g32[c].shape and g32[c].shape[0] > 0
        assert np.array_equal(g16[c].view(np.int32), g32[c].view(np.int32)), c
    assert s16 == s32
    # the ring-full rule counts fp32 samples, as for the fp32 appends
    with sd.SyllableDetector(cfg, channels=1) as det:
        big16 = np.zeros(409600 // 4 + 1, np.int16)
        with pytest.raises(sd.SyllableDetectorError) as ei:
            det.appendAudioDataPCM16(big16, 0)
        assert ei.value.status == _abi.ERR_BUFFER_FULL
        with pytest.raises(sd.SyllableDetectorError) as ei:
            det.appendAudioData(big16.astype(np.float32), 0)
        assert ei.value.status == _abi.ERR_BUFFER_FULL


def test_refusals_touch_nothing():
    """The fp32 twins' argument checks and statuses, before any launch."""
    import ctypes as C
    torch = _torch()
    lib = _abi.lib
    x16 = torch.zeros((2, 4096), dtype=torch.int16, device="cuda")
    out = torch.zeros(4096 * 4, dtype=torch.float32, device="cuda")
    fl = torch.zeros(4096 * 4, dtype=torch.uint8, device="cuda")
    host = np.zeros(2 * 4096, np.int16)
    hp = host.ctypes.data_as(_abi.c_int16_p)
    bad = _abi.ERR_INVALID_ARGUMENT
    with sd.SyllableDetector(util.sample_net(), channels=2) as det:
        det.profile(True)
        h = det._h
        assert lib.syldet_run_device_s16(h, None, 4096, 4096, out.data_ptr(), fl.data_ptr(), None) == bad
        assert lib.syldet_run_device_s16(h, x16.data_ptr(), -1, 4096, out.data_ptr(), fl.data_ptr(), None) == bad
        assert lib.syldet_run_device_s16(h, x16.data_ptr(), 4096, 4095, out.data_ptr(), fl.data_ptr(), None) == bad
        assert lib.syldet_run_s16(h, None, 4096, 4096, None, None) == bad
        assert lib.syldet_run_s16(h, hp, -1, 4096, None, None) == bad
        assert lib.syldet_run_s16(h, hp, 4096, 100, None, None) == bad
        for total in (1, 3):
            assert lib.syldet_run_interleaved_device_s16(h, x16.data_ptr(), 2048, total, out.data_ptr(), fl.data_ptr(), None) == bad
            assert lib.syldet_run_interleaved_s16(h, hp, 2048, total, None, None) == bad
            assert lib.syldet_append_interleaved_s16(h, hp, 16, total) == bad
        assert lib.syldet_run_interleaved_device_s16(h, x16.data_ptr(), -1, 2, out.data_ptr(), fl.data_ptr(), None) == bad
        assert lib.syldet_run_interleaved_s16(h, None, 4096, 2, None, None) == bad
        for ch in (-1, 2):
            assert lib.syldet_append_s16(h, ch, hp, 16) == bad
        assert lib.syldet_append_s16(h, 0, None, 16) == bad
        assert lib.syldet_append_s16(h, 0, hp, -1) == bad
        assert lib.syldet_append_interleaved_s16(h, None, 16, 2) == bad
        torch.cuda.synchronize()
        ms = (C.c_double * 8)()
        names = (C.c_char_p * 8)()
        n = C.c_int32()
        lib.syldet_last_timings(h, ms, names, 8, C.byref(n))
        assert n.value == 0                                     # no batch call got as far as a launch
        assert det.pendingEvaluations(0) == 0
        with pytest.raises(ValueError):
            det.runPCM16(x16.float())
        with pytest.raises(ValueError):
            det.run(x16)                                        # run() still refuses anything but float32


def test_cli_16_bit_wav_equals_float_wav(tmp_path):
    cfg = util.sample_net()
    net = tmp_path / "net.txt"
    net.write_text(cfg.toText())
    x16 = _pcm(5, 44100 * 2, seed=13)
    x16[3] = x16[0][::-1]
    frames = np.ascontiguousarray(x16.T)
    p16, p32 = tmp_path / "a16.wav", tmp_path / "a32.wav"
    wavutil.write_wav(str(p16), frames, 44100, "pcm16")
    wavutil.write_wav(str(p32), frames.astype(np.float32) * np.float32(2.0 ** -15), 44100, "float32")

    def lines(p):
        r = subprocess.run([CLI, "-n", str(net), "-a", str(p)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    a, b = lines(p16), lines(p32)
    assert a == b and len(a) > 0
