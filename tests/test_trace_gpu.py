"""The Simulator's output track on the device (syldet_trace*; kernels_trace.hip).  The outputs come from the library's own,
separately tested run(); the expansion is what is under test, so every comparison with tests/trace_ref.py is EXACT: the bit
patterns of the fp32 trace (NaN at the same places), the int16 values."""
import numpy as np
import pytest

import pyoracle as po
import trace_ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d differences, first at %s: %s != %s" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def _net_for(base, outputs=1, seed=0, **changes):
    """`base`'s front end with `changes` (the band stays) and a random network that fits it"""
    cfg = nets.variant(base, **changes)
    cfg.net = nets.random_net(np.random.default_rng(seed), base.geometry().bins * cfg.timeRange, (4,), outputs)
    cfg.thresholds = [0.3 + 0.2 * i for i in range(outputs)]
    return cfg


def _shapes():
    base = util.sample_net()
    return {"example (hop 132)": (base, 0),
            "hop 128": (nets.variant(base, windowOverlap=128), 0),
            "hop 131": (nets.variant(base, windowOverlap=125), 0),
            "gap 20": (nets.variant(base, windowOverlap=-20), 0),
            "timeRange 1": (_net_for(base, seed=3, timeRange=1), 0),
            "window 128": (nets.variant(base, windowLength=128, windowOverlap=40), 0),
            "three outputs": (_net_for(base, outputs=3, seed=4), 2)}


def _audio(C, S, seed=0):
    x = np.stack([synth.channel(S, seed + c) for c in range(C)]).astype(np.float32)
    if C:
        x[0] = synth.syllable_channel(S, util.template(), seed=11 + seed)[:S]
    return x


def _want(det, outputs, thresholds, n, k=0):
    g = det.geometry
    return trace_ref.closed_form_bank(np.asarray(outputs), thresholds, g.first_index, g.hop, n, k)


@pytest.mark.parametrize("shape", list(_shapes()))
@pytest.mark.parametrize("C", [1, 5, 64])
def test_planar_traces_equal_the_closed_form(shape, C):
    torch = _torch()
    cfg, k = _shapes()[shape]
    S = 23003 if C < 64 else 9001                                   # (neither a multiple of 8)
    x = torch.from_numpy(_audio(C, S)).cuda()
    with sd.SyllableDetector(cfg, channels=C) as det:
        out, _ = det.run(x)
        g = det.geometry
        assert g.hop == cfg.windowLength - cfg.windowOverlap and out.shape[1] > 10
        t32 = det.trace(out, S, output=k)
        t16 = det.trace(out, S, output=k, dtype=np.int16)
        torch.cuda.synchronize()
        want = _want(det, out.cpu().numpy(), cfg.thresholds, S, k)
    _same_bits(t32.cpu().numpy(), want)
    _same_bits(t16.cpu().numpy(), trace_ref.to_s16(want))
    assert want.max() > 0 and not want[:, :g.first_index].any()


def _filled(shape, dtype, device):
    torch = _torch()
    t = torch.empty(shape, dtype=torch.int16 if dtype == np.int16 else torch.float32, device=device)
    if dtype == np.int16:
        t.fill_(-21846)                                              # 0xAAAA
    else:
        t.view(torch.int32).fill_(0x7FC0BEEF)                        # a NaN with a payload: any write shows
    return t


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_layouts_and_lengths(dtype):
    """wider and odd strides, a base one element past a 16-byte line, lengths that are no multiple of 8, below D, 0; fewer
    evaluations than the recording has, none at all; the elements between n_samples and the stride keep their bytes"""
    torch = _torch()
    cfg = util.sample_net()
    C, S = 3, 20011
    x = torch.from_numpy(_audio(C, S, 5)).cuda()
    fill = _filled((1,), dtype, "cuda").cpu().numpy()[0]
    conv = (lambda w: trace_ref.to_s16(w)) if dtype == np.int16 else (lambda w: w)
    with sd.SyllableDetector(cfg, channels=C) as det:
        out, _ = det.run(x)
        out_np = out.cpu().numpy()
        E, D, hop = out.shape[1], det.geometry.first_index, det.geometry.hop
        cases = [(S, S + 8, 0, out), (S, S + 13, 0, out), (S, S + 5, 1, out), (S, S + 2, 3, out), (S - 3, S, 0, out),
                 (D - 1, D + 6, 0, out), (D + 1, D + 1, 1, out), (7, 9, 1, out), (S, S + 4, 0, out[:, :E - 3].contiguous()),
                 (S, S, 0, out[:, :0].contiguous()), (S + 1000, S + 1000, 0, out)]
        for n, stride, shift, o in cases:
            flat = _filled((C * stride + 16,), dtype, x.device)
            rows = flat[shift:shift + C * stride].view(C, stride)
            got = det.trace(o, n, dtype=dtype, out=rows[:, :n])
            torch.cuda.synchronize()
            assert got.data_ptr() == rows.data_ptr()
            want = conv(_want(det, out_np[:, :o.shape[1]], cfg.thresholds, n))
            case = "n %d stride %d shift %d evals %d" % (n, stride, shift, o.shape[1])
            _same_bits(rows[:, :n].cpu().numpy(), want)
            rest = flat.cpu().numpy().copy()
            body = rest[shift:shift + C * stride].reshape(C, stride)
            body[:, :n] = fill
            same = (rest.view(np.int32) == fill.view(np.int32)) if dtype == np.float32 else (rest == fill)
            assert same.all(), case + ": bytes outside the first n_samples of a row were written"
            if n <= D or o.shape[1] == 0:
                assert not want.any()
            if o.shape[1] == E - 3:
                assert not want[:, D + (E - 3) * hop:].any()             # zeros behind the last hold
        # nothing to write
        assert det.trace(out, 0, dtype=dtype).shape == (C, 0)
        torch.cuda.synchronize()


def _hand_made(thr):
    """outputs that meet every branch for threshold thr: NaN, the infinities, negative values, values above the threshold, the
    threshold itself, exact ties of v * 32767 at .5 (v = (m + 0.5) / 32767 cannot be hit exactly through a division in general,
    so the ties are looked for: quotients whose product with 32767 is m + 0.5 exactly), zeros of both signs"""
    t = np.float32(thr)
    vals = [np.nan, np.inf, -np.inf, -1.0, -1e-30, -0.0, 0.0, 1e-30, float(t), float(t) * 2, 3.0e38, -3.0e38,
            float(np.nextafter(t, np.float32(np.inf))), float(np.nextafter(t, np.float32(-np.inf)))]
    rng = np.random.default_rng(7)
    vals += list((rng.random(600) * 1.3 - 0.15) * float(t))
    with np.errstate(all="ignore"):
        # ties: v = (2 m + 1) / 65534 for m with an exactly representable product; out = v * t, kept if the division gives v back
        for m in (0, 1, 2, 3, 100, 16383, 16384, 32765, 32766):
            v = np.float32((2 * m + 1) / 65534.0)
            if np.float32(v * np.float32(32767)) == np.float32(m + 0.5):
                o = np.float32(v * t)
                for cand in (o, np.nextafter(o, np.float32(0)), np.nextafter(o, np.float32(2) * o)):
                    if np.float32(cand / t) == v:
                        vals.append(float(cand))
                        break
    return np.array(vals, np.float32)


@pytest.mark.parametrize("thr", [0.4424, -0.5, 0.0, 0.1, 1.0 / 3.0, 1e-3 + 1e-11, 3.0])
def test_hand_made_values(thr):
    """thresholds that are negative, zero and not representable in fp32 (0.1, 1/3: the Double is rounded to Float first)"""
    torch = _torch()
    cfg = nets.variant(util.sample_net(), thresholds=[thr])
    vals = _hand_made(thr)
    E = len(vals)
    with sd.SyllableDetector(cfg, channels=2) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        out = np.stack([vals, vals[::-1]]).reshape(2, E, 1).copy()
        n = D + E * hop + 77
        t32 = det.trace(torch.from_numpy(out).cuda(), n)
        t16 = det.trace(torch.from_numpy(out).cuda(), n, dtype=np.int16)
        fr = det.trace(torch.from_numpy(out).cuda(), n, dtype=np.int16, interleaved=True)
        torch.cuda.synchronize()
        want = _want(det, out, [thr], n)
    if thr == 0.4424:
        v = trace_ref.values(out[0], [thr])
        ties = np.float32(v * np.float32(32767)) % 1 == 0.5
        assert np.isnan(v).any() and (v == 1).any() and (v == 0).any() and ties.sum() >= 2, ties.sum()
    _same_bits(t32.cpu().numpy(), want)
    _same_bits(t16.cpu().numpy(), trace_ref.to_s16(want))
    _same_bits(fr.cpu().numpy(), trace_ref.to_s16(want).T)


def test_denormal_quotients():
    """Quotients (and outputs) below the smallest normal fp32 number: numpy's division keeps denormals; the device's
    v_div_scale / v_div_fmas / v_div_fixup sequence is held to the same bits."""
    torch = _torch()
    cfg = nets.variant(util.sample_net(), thresholds=[4.0])
    vals = np.array([1e-38, 1.5e-38, 1e-39, 4e-45, 2e-44, -1e-39, 4.7e-38], np.float32)
    with sd.SyllableDetector(cfg, channels=1) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        out = vals.reshape(1, -1, 1).copy()
        n = D + len(vals) * hop
        t32 = det.trace(torch.from_numpy(out).cuda(), n).cpu().numpy()
        want = _want(det, out, [4.0], n)
    got_v, want_v = t32[0, D::hop], want[0, D::hop]
    print("denormal quotients: device", [hex(int(b)) for b in got_v.view(np.uint32)], "numpy", [hex(int(b)) for b in want_v.view(np.uint32)])
    assert (want_v[:5] > 0).all() and (want_v[:5] < np.finfo(np.float32).tiny).all()
    _same_bits(t32, want)


@pytest.mark.parametrize("C,n", [(1, 10007), (3, 10007), (33, 5003), (64, 4999), (70, 2777)])
def test_interleaved_is_the_planar_trace_transposed(C, n):
    torch = _torch()
    cfg = util.sample_net()
    x = torch.from_numpy(_audio(C, n, 2)).cuda()
    with sd.SyllableDetector(cfg, channels=C) as det:
        out, _ = det.run(x)
        planar = det.trace(out, n, dtype=np.int16)
        frames = _filled((n + 8, C), np.int16, x.device)
        got = det.trace(out, n, dtype=np.int16, interleaved=True, out=frames[:n])
        short = det.trace(out, det.geometry.first_index - 2, dtype=np.int16, interleaved=True)
        torch.cuda.synchronize()
        want = trace_ref.to_s16(_want(det, out.cpu().numpy(), cfg.thresholds, n))
    assert got.shape == (n, C) and not short.cpu().numpy().any()
    _same_bits(planar.cpu().numpy(), want)
    _same_bits(got.cpu().numpy(), want.T)
    assert (frames[n:].cpu().numpy() == -21846).all()                # nothing behind the last frame
    assert want.max() > 0


def test_short_hops_on_hand_made_outputs():
    """holds shorter than a 16-byte group (hop 1, 3, 5): the sample-by-sample walk of both kernels"""
    torch = _torch()
    base = util.sample_net()
    rng = np.random.default_rng(3)
    for hop in (1, 3, 5):
        cfg = nets.variant(base, windowOverlap=base.windowLength - hop)
        with sd.SyllableDetector(cfg, channels=3) as det:
            D = det.geometry.first_index
            assert det.geometry.hop == hop
            E = 9000
            out = (rng.random((3, E, 1)) * 0.7).astype(np.float32)
            n = D + E * hop + 5
            o = torch.from_numpy(out).cuda()
            t32, t16 = det.trace(o, n), det.trace(o, n, dtype=np.int16)
            fr = det.trace(o, n, dtype=np.int16, interleaved=True)
            torch.cuda.synchronize()
            want = _want(det, out, cfg.thresholds, n)
        _same_bits(t32.cpu().numpy(), want)
        _same_bits(t16.cpu().numpy(), trace_ref.to_s16(want))
        _same_bits(fr.cpu().numpy(), trace_ref.to_s16(want).T)


@pytest.mark.parametrize("kind", ["multi", "mixed"])
def test_every_channel_divides_by_its_own_networks_threshold(kind):
    torch = _torch()
    base = util.sample_net()
    if kind == "multi":
        cfgs = [base, nets.perturbed(base, 5), nets.perturbed(base, 6)]
        for i, c in enumerate(cfgs):
            c.thresholds = [0.4424 + 0.21 * i]
        net_of = [0, 1, 2, 1, 0]
        det = sd.SyllableDetector.multi(cfgs, net_of)
    else:
        f0, f1 = sd.frequencyIndexRange(base.fourierLength, base.samplingRate, 2000.0, 5000.0)
        narrow = nets.variant(base, freqRange=(2000.0, 5000.0), thresholds=[0.1],
                              net=nets.random_net(np.random.default_rng(1), (f1 - f0) * base.timeRange, (4,), 1))
        cfgs = [base, narrow, nets.perturbed(base, 5)]
        net_of = [1, 0, 2, 1, 0, 2]
        det = sd.SyllableDetector.mixed(cfgs, net_of)
    C, S = len(net_of), 15013
    thr = [cfgs[i].thresholds for i in net_of]
    assert len({t[0] for t in thr}) == 3
    with det:
        out, _ = det.run(torch.from_numpy(_audio(C, S, 9)).cuda())
        t32 = det.trace(out, S)
        t16 = det.trace(out, S, dtype=np.int16)
        fr = det.trace(out, S, dtype=np.int16, interleaved=True)
        torch.cuda.synchronize()
        want = _want(det, out.cpu().numpy(), thr, S)
        host = det.traceHost(out.cpu().numpy(), S)
    _same_bits(t32.cpu().numpy(), want)
    _same_bits(t16.cpu().numpy(), trace_ref.to_s16(want))
    _same_bits(fr.cpu().numpy(), trace_ref.to_s16(want).T)
    _same_bits(host, want)
    # (the thresholds matter: every channel under channel 0's would differ)
    assert not np.array_equal(want, _want(det, out.cpu().numpy(), thr[0], S))


def test_simulate_is_run_then_trace_and_the_host_forms_agree():
    torch = _torch()
    cfg = util.sample_net()
    C, S = 4, 30001
    x = _audio(C, S, 4)
    with sd.SyllableDetector(cfg, channels=C) as det:
        xd = torch.from_numpy(x).cuda()
        out, fl = det.run(xd)
        tr, out2, fl2 = det.simulate(xd)
        tr32, _, _ = det.simulate(xd, dtype=np.float32)
        torch.cuda.synchronize()
        assert tr.dtype == torch.int16 and tr.shape == (C, S)
        _same_bits(out2.cpu().numpy(), out.cpu().numpy())
        assert torch.equal(fl, fl2)
        _same_bits(tr.cpu().numpy(), det.trace(out, S, dtype=np.int16).cpu().numpy())
        _same_bits(tr32.cpu().numpy(), det.trace(out, S).cpu().numpy())
        h32 = det.traceHost(out.cpu().numpy(), S)
        h16 = det.traceHost(out.cpu().numpy(), S, dtype=np.int16)
        _same_bits(h32, tr32.cpu().numpy())
        _same_bits(h16, tr.cpu().numpy())
        assert det.traceHost(out.cpu().numpy()[:, :0], 500).shape == (C, 500) and not det.traceHost(out.cpu().numpy()[:, :0], 500).any()
        assert det.traceHost(out.cpu().numpy(), 0).shape == (C, 0)


def test_argument_statuses_with_a_live_handle():
    torch = _torch()
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=2) as det:
        o = torch.zeros((2, 10, 1), device="cuda")
        t = torch.full((2, 4000), 7.0, device="cuda")
        q = torch.full((2, 4000), 7, dtype=torch.int16, device="cuda")
        lib, bad = _abi.lib, _abi.ERR_INVALID_ARGUMENT
        for k in (-1, 1, 5):
            assert lib.syldet_trace_device(det._h, o.data_ptr(), 10, k, t.data_ptr(), 4000, 4000, None) == bad
            assert lib.syldet_trace_device_s16(det._h, o.data_ptr(), 10, k, q.data_ptr(), 4000, 4000, None) == bad
            assert lib.syldet_trace_interleaved_device_s16(det._h, o.data_ptr(), 10, k, q.data_ptr(), 4000, None) == bad
        assert "output" in _abi.last_error()
        assert lib.syldet_trace_device(det._h, o.data_ptr(), -1, 0, t.data_ptr(), 4000, 4000, None) == bad
        assert lib.syldet_trace_device(det._h, o.data_ptr(), 10, 0, t.data_ptr(), -1, 4000, None) == bad
        assert lib.syldet_trace_device(det._h, o.data_ptr(), 10, 0, t.data_ptr(), 4000, 3999, None) == bad
        assert lib.syldet_trace_device_s16(det._h, o.data_ptr(), 10, 0, q.data_ptr(), 4000, 3999, None) == bad
        assert lib.syldet_trace_device(det._h, None, 10, 0, t.data_ptr(), 4000, 4000, None) == bad
        assert lib.syldet_trace_device(det._h, o.data_ptr(), 10, 0, None, 4000, 4000, None) == bad
        assert lib.syldet_trace_interleaved_device_s16(det._h, o.data_ptr(), 10, 0, None, 4000, None) == bad
        h = np.zeros((2, 10, 1), np.float32)
        ht = np.zeros((2, 100), np.float32)
        assert lib.syldet_trace(det._h, h.ctypes.data_as(_abi.c_float_p), 10, 0, ht.ctypes.data_as(_abi.c_float_p), 100, 99) == bad
        assert lib.syldet_trace(det._h, h.ctypes.data_as(_abi.c_float_p), 10, 1, ht.ctypes.data_as(_abi.c_float_p), 100, 100) == bad
        torch.cuda.synchronize()
        assert (t == 7.0).all() and (q == 7).all()                   # refused before the device was touched
        with pytest.raises(ValueError):
            det.trace(o, 100, interleaved=True)                      # frames are int16
        with pytest.raises(ValueError):
            det.trace(o, 100, dtype=np.float64)
        with pytest.raises(ValueError):
            det.simulate(torch.zeros((2, 5000), device="cuda"), dtype=np.int32)
        with pytest.raises(ValueError):
            det.trace(o, 100, out=torch.zeros((2, 99), device="cuda"))


def test_the_launch_is_listed_under_profiling():
    torch = _torch()
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=3) as det:
        det.profile(True)
        out, _ = det.run(torch.from_numpy(_audio(3, 9000)).cuda())
        det.trace(out, 9000)
        torch.cuda.synchronize()
        assert util.launched(det) == ["trace_kernel"]
        det.trace(out, 9000, dtype=np.int16)
        torch.cuda.synchronize()
        assert util.launched(det) == ["trace_kernel"]
        det.trace(out, 9000, dtype=np.int16, interleaved=True)
        torch.cuda.synchronize()
        names = det.lastTimings()
        assert [n for n, _ in names] == ["trace_interleaved_s16_kernel"] and names[0][1] > 0


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_end_to_end_against_the_oracle(seed):
    """The trace of the oracle's fp64 outputs against the library's fp32 trace: within 1e-5 / |Float(thr)| + 2^-23 wherever
    neither is clamped (the 1e-5 output contract carried through one division), and the flag of evaluation e set exactly when
    trace[D + e hop] == 1.0 over the evaluations whose output 0 is further than 1e-4 |thr| from the threshold (the flag compares
    in Double, the trace divides in Float)."""
    torch = _torch()
    cfg = util.sample_net()
    x = synth.syllable_channel(44100, util.template(), seed=seed)
    thr = cfg.thresholds[0]
    with sd.SyllableDetector(cfg, channels=1) as det:
        out, fl = det.run(torch.from_numpy(x[None]).cuda())
        tr = det.trace(out, len(x))
        torch.cuda.synchronize()
        D, hop = det.geometry.first_index, det.geometry.hop
        out, fl, tr = out.cpu().numpy()[0], fl.cpu().numpy()[0], tr.cpu().numpy()[0]
    _, _, w64 = util.oracle_for(cfg).run(x, po.F64)
    E = w64.shape[0]
    assert out.shape[0] == E
    want = trace_ref.closed_form(w64, cfg.thresholds, D, hop, len(x))
    free = (want > 0) & (want < 1) & (tr > 0) & (tr < 1)
    bar = 1e-5 / abs(float(np.float32(thr))) + 2.0 ** -23
    err = np.abs(tr.astype(np.float64) - want.astype(np.float64))[free]
    print("seed %d: %d evaluations, %d flags, %d unclamped samples, worst |trace - oracle| %.3g (bar %.3g)" %
          (seed, E, int(fl.sum()), int(free.sum()), float(err.max()), bar))
    assert free.sum() > 10 * hop and err.max() <= bar
    assert (want == 1).any()                                         # the clamp at the threshold is exercised
    band = np.abs(out[:, 0].astype(np.float64) - thr) <= 1e-4 * abs(thr)
    assert fl.sum() >= 1 and band.sum() <= 0.01 * E
    at = tr[D + np.arange(E) * hop]
    assert np.array_equal((at == 1.0)[~band], fl.astype(bool)[~band])
