"""Mixed banks on the device (syldet_create_mixed): one handle whose networks share the evaluation clock and differ in band,
FFT size, chain and widths.  Each class of compatible networks runs exactly as a handle of that class's networks would, so every
case is held to EQUALITY with the class's own handle (syldet_create_multi, or syldet_create for one network) over the class's
channels on the same samples -- outputs bit for bit (NaN included), flags, detections, the exact recomputation's work -- and the
fold kernel's channels also to the fp64 oracle of each channel's own network."""
import numpy as np
import pytest

import pyoracle as po
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth

pytestmark = pytest.mark.gpu

def _torch():
    import torch
    return torch


def _bits(t):
    return t.contiguous().view(_torch().int32) if t.dtype == _torch().float32 else t


def _with_band(base, lo, hi, fourier_length=None, hidden=4, seed=0, in_fns=("l2normalize", "mapminmax"), **changes):
    N = fourier_length or base.fourierLength
    f0, f1 = sd.frequencyIndexRange(N, base.samplingRate, lo, hi)
    net = nets.random_net(np.random.default_rng(seed), (f1 - f0) * base.timeRange, (hidden,), 1, in_fns=in_fns)
    return nets.variant(base, fourierLength=N, freqRange=(lo, hi), net=net, thresholds=[0.1], **changes)


def _three_classes():
    """[sample.txt, a narrower band, 512-point frames with 8 hidden units and log columns behind normalize, a second network
    of sample.txt's class]: classes {0, 3}, {1}, {2}"""
    base = util.sample_net()
    narrow = _with_band(base, 2000.0, 5000.0, seed=1)
    wide512 = _with_band(base, 1000.0, 9000.0, fourier_length=512, hidden=8, seed=2, in_fns=("normalize", "mapminmax"),
                         spectrogramScaling="log")
    cfgs = [base, narrow, wide512, nets.perturbed(base, 5)]
    assert narrow.geometry().bins != base.geometry().bins and wide512.geometry().bins not in (base.geometry().bins, narrow.geometry().bins)
    return cfgs


def _class_sets(cfgs, channel_net):
    """[(network indices of the class, the class's channels)] by syldet_config_compatible"""
    reps, members = [], []
    for i, c in enumerate(cfgs):
        for k, r in enumerate(reps):
            if sd.configsCompatible(cfgs[r], c)[0]:
                members[k].append(i)
                break
        else:
            reps.append(i)
            members.append([i])
    net = np.asarray(channel_net)
    out = []
    for m in members:
        rows = np.nonzero(np.isin(net, m))[0]
        if rows.size:
            out.append((m, rows))
    return out


def _class_handle(cfgs, members, channel_net, rows, engine=_abi.ENGINE_AUTO):
    local = [members.index(int(channel_net[r])) for r in rows]
    if len(members) == 1:
        return sd.SyllableDetector(cfgs[members[0]], channels=len(rows), engine=engine)
    return sd.SyllableDetector.multi([cfgs[m] for m in members], local, engine=engine)


def _run_classes(cfgs, channel_net, x, engine=_abi.ENGINE_AUTO):
    """Each class's own handle over the class's channels (the same segmentation as the mixed bank's class launch); the
    results scattered back to the bank's rows.  Returns (outputs, flags, [names of each class's kernels], items)."""
    torch = _torch()
    out = fl = None
    names, items = [], 0
    for members, rows in _class_sets(cfgs, channel_net):
        r = torch.from_numpy(rows).to(x.device)
        with _class_handle(cfgs, members, channel_net, rows, engine) as det:
            det.profile(True)
            o, f = det.run(x[r].contiguous())
            torch.cuda.synchronize()
            names.append(util.launched(det))
            items += det.fixupStats()[0]
        if out is None:
            out = torch.empty((x.shape[0],) + tuple(o.shape[1:]), dtype=o.dtype, device=x.device)
            fl = torch.empty((x.shape[0],) + tuple(f.shape[1:]), dtype=f.dtype, device=x.device)
        out[r] = o
        fl[r] = f
    return out, fl, names, items


def _assert_equal(a_out, a_fl, b_out, b_fl):
    torch = _torch()
    a_out, b_out, a_fl, b_fl = (torch.as_tensor(v) for v in (a_out, b_out, a_fl, b_fl))
    assert a_out.shape == b_out.shape and a_fl.shape == b_fl.shape
    same = (_bits(a_out) == _bits(b_out)).all(dim=-1).all(dim=-1)
    assert bool(same.all()), "outputs differ on channels %s" % torch.nonzero(~same).flatten().tolist()[:8]
    assert torch.equal(a_fl, b_fl)


def _input(C, S, seed0=300):
    return np.stack([synth.syllable_channel(S, util.template(), seed=seed0 + c) if c % 3 == 0 else synth.channel(S, seed0 + c)
                     for c in range(C)]).astype(np.float32)


def test_three_interleaved_classes_equal_their_own_handles(oracle_lib):
    torch = _torch()
    cfgs = _three_classes()
    C = 12
    channel_net = [c % 4 for c in range(C)]
    S = 44100 * 2 + 77
    xh = _input(C, S)
    x = torch.from_numpy(xh).cuda()
    with sd.SyllableDetector.mixed(cfgs, channel_net) as det:
        det.profile(True)
        out, fl = det.run(x)
        torch.cuda.synchronize()
        names = util.launched(det)
        items = det.fixupStats()[0]
        g = det.geometry
        own = [c.geometry() for c in cfgs]
        for field in ("f0", "f1", "bins", "inputs"):         # (-1 where the classes differ)
            vals = {getattr(o, field) for o in own}
            assert getattr(g, field) == (vals.pop() if len(vals) == 1 else -1), field
        assert g.bins == -1 and g.inputs == -1 and g.engine == -1
        assert g.hop == cfgs[0].geometry().hop and g.outputs == 1
        for c in range(C):
            cg = det.channelGeometry(c)
            own = cfgs[channel_net[c]].geometry()
            assert (cg.bins, cg.inputs, cg.f0, cg.f1) == (own.bins, own.inputs, own.f0, own.f1)
            assert cg.engine == (_abi.ENGINE_GENERIC if channel_net[c] == 2 else _abi.ENGINE_FUSED)
    # one call: the fold kernel for the two fold classes and the generic engine for the third
    assert names.count("fused_s_kernel") == 2 and "mlp_generic_kernel" in names, names
    c_out, c_fl, c_names, c_items = _run_classes(cfgs, channel_net, x)
    # the 512-point class: AUTO keeps it on the generic engine (asserted, not assumed), the others on the fold kernel
    assert c_names[0] == ["fused_s_kernel"] and c_names[1] == ["fused_s_kernel"], c_names
    assert c_names[2] and not any(n.startswith("fused") for n in c_names[2]) and "mlp_generic_kernel" in c_names[2], c_names
    _assert_equal(out, fl, c_out, c_fl)
    assert items == c_items
    out, fl = out.cpu().numpy(), fl.cpu().numpy()
    assert fl.sum() > 0
    oracles = {k: util.oracle_for(cfgs[k]) for k in (0, 1, 3)}
    for c in range(C):
        k = channel_net[c]
        if k == 2:
            continue
        _, _, w64 = oracles[k].run(xh[c], po.F64)
        util.assert_outputs_close(out[c], w64)
        util.assert_flags_exact(fl[c], w64, cfgs[k].thresholds, cfgs[k].rule)


def test_host_pointer_run_split_into_stages_and_interleaved(monkeypatch):
    torch = _torch()
    cfgs = _three_classes()
    C = 7
    channel_net = [2, 0, 1, 3, 1, 2, 0]
    S = 132 * 3000 + 256
    xh = synth.channels(C, S, first=30)
    x = torch.from_numpy(xh).cuda()
    with sd.SyllableDetector.mixed(cfgs, channel_net) as det:
        out, fl = det.run(x)
        io, ifl = det.runInterleaved(torch.from_numpy(np.ascontiguousarray(xh.T)).cuda())
        torch.cuda.synchronize()
        out, fl, io, ifl = out.cpu(), fl.cpu(), io.cpu(), ifl.cpu()
        ho, hfl = det.runInterleavedHost(np.ascontiguousarray(xh.T))
        _assert_equal(io, ifl, out, fl)
        _assert_equal(ho, hfl, out, fl)
    # a stage of about a third of the recording: the pipelined host call cuts it into stages
    monkeypatch.setenv("SYLDET_HOST_CHUNK_BYTES", str(C * S * 4 // 3))
    with sd.SyllableDetector.mixed(cfgs, channel_net) as det:
        po_, pf = det.runHost(xh)
    _assert_equal(po_, pf, out, fl)
    c_out, c_fl, _, _ = _run_classes(cfgs, channel_net, x)
    _assert_equal(out, fl, c_out.cpu(), c_fl.cpu())


def test_streaming_equals_batch_one_round_trip_per_group():
    """Ragged interleaved appends, then process_all: every channel's evaluations bit for bit the batch call's, each channel
    against its own network's threshold; each drain is ONE profiled call that holds every class's launches (one H2D copy,
    the launches, one D2H copy and one synchronisation per evaluation group -- not a round trip per class)."""
    torch = _torch()
    base = util.sample_net()
    cfgs = _three_classes()
    cfgs[0] = nets.variant(base, thresholds=[-1e6])          # (always detects)
    cfgs[3] = nets.variant(nets.perturbed(base, 6), thresholds=[1e6])   # (never does)
    C = 8
    channel_net = [3, 0, 1, 2, 2, 0, 1, 3]
    S = 132 * 400 + 256
    x = synth.channels(C, S, first=50)
    with sd.SyllableDetector.mixed(cfgs, channel_net) as det:
        out, fl = det.run(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        out, fl = out.cpu().numpy(), fl.cpu().numpy()
        det.profile(True, history=4)
        got = [[] for _ in range(C)]
        det_flags = [[] for _ in range(C)]
        pos = 0
        rng = np.random.default_rng(2)
        drains = 0
        while pos < S:
            n = int(rng.integers(1, 6000))
            det.appendInterleavedData(np.ascontiguousarray(x[:, pos:pos + n].T))
            pos += n
            if det.processAll() > 0:
                drains += 1
                names = [nm for nm, _ in det.lastTimings()]
                assert names.count("fused_s_kernel") == 2 and "mlp_generic_kernel" in names, names
            for c in range(C):
                while det.processNewValue(c):
                    got[c].append(det.lastOutputsFor(c))
                    det_flags[c].append(det.lastDetectedFor(c))
        assert drains > 3
        for c in range(C):
            g = np.asarray(got[c], np.float32)
            assert g.shape == out[c].shape
            assert np.array_equal(g.view(np.int32), out[c].view(np.int32)), c
            thr = cfgs[channel_net[c]].thresholds[0]
            assert det_flags[c] == [bool(v >= thr) for v in g[:, 0]]
            assert np.array_equal(np.asarray(det_flags[c], np.uint8), fl[c])
        assert all(all(det_flags[c]) for c in range(C) if channel_net[c] == 0)
        assert not any(any(det_flags[c]) for c in range(C) if channel_net[c] == 3)
        for c in range(C):
            det.appendAudioData(x[c, :132 * 20], c)
            seen = det.seenSyllable(c)
            if channel_net[c] in (0, 3):
                assert seen == (channel_net[c] == 0), c
            assert det.pendingEvaluations(c) == 0


def test_exact_recomputation_uses_each_rows_network():
    """A chain without a normaliser through a loud recording sends windows to fixup_kernel; the recomputed evaluations are
    each row's own network's, written to its own row -- bit for bit the class handles' -- and the work the sum of theirs."""
    torch = _torch()
    base = util.sample_net()
    loud = nets.variant(base, net=nets.random_net(np.random.default_rng(3), 290, (4,), 1, in_fns=()))
    cfgs = _three_classes()
    cfgs = [cfgs[2], loud, nets.perturbed(loud, 71), cfgs[1]]
    S = 132 * 2000 + 256
    a, b = synth.channels(2, S, first=1) * np.float32(10.0)
    x = torch.from_numpy(np.stack([a, a, b, b, a, b]).astype(np.float32)).cuda()
    channel_net = [0, 1, 2, 3, 2, 1]
    with sd.SyllableDetector.mixed(cfgs, channel_net) as det:
        det.profile(True)
        out, fl = det.run(x)
        torch.cuda.synchronize()
        items, over = det.fixupStats()
    c_out, c_fl, _, c_items = _run_classes(cfgs, channel_net, x)
    assert over == 0 and c_items > 0 and items == c_items
    _assert_equal(out, fl, c_out, c_fl)
    assert not bool((_bits(out[1]) == _bits(out[4])).all())     # (the same audio, two networks)


def test_detections_per_channel():
    torch = _torch()
    cfgs = _three_classes()
    C = 8
    channel_net = [1, 3, 0, 2, 0, 1, 3, 2]
    S = 44100 * 3
    x = torch.from_numpy(np.stack([synth.syllable_channel(S, util.template(), seed=600 + c) for c in range(C)])).cuda()
    with sd.SyllableDetector.mixed(cfgs, channel_net) as det:
        _, fl = det.run(x)
        idx, cnt = det.detections(fl, debounce=0.1)
        torch.cuda.synchronize()
    for members, rows in _class_sets(cfgs, channel_net):
        r = torch.from_numpy(rows).cuda()
        with _class_handle(cfgs, members, channel_net, rows) as det:
            _, f = det.run(x[r].contiguous())
            i2, c2 = det.detections(f, debounce=0.1)
            torch.cuda.synchronize()
        assert torch.equal(fl[r], f)
        for j, c in enumerate(rows):
            assert int(cnt[c]) == int(c2[j])
            assert torch.equal(idx[c, :int(cnt[c])], i2[j, :int(c2[j])])
    assert int(cnt.sum()) > 0


def test_all_compatible_is_a_multi_handle_and_one_network_a_plain_one():
    torch = _torch()
    base = util.sample_net()
    cfgs = [base, nets.perturbed(base, 1), nets.perturbed(base, 2)]
    x = torch.from_numpy(synth.channels(5, 132 * 500 + 256, first=2)).cuda()
    with sd.SyllableDetector.mixed(cfgs, [2, 0, 1, 1, 0]) as det:
        assert det.geometry.bins == base.geometry().bins and det.geometry.engine == _abi.ENGINE_FUSED
        out, fl = det.run(x)
    with sd.SyllableDetector.multi(cfgs, [2, 0, 1, 1, 0]) as det:
        o, f = det.run(x)
    torch.cuda.synchronize()
    _assert_equal(out, fl, o, f)
    with sd.SyllableDetector.mixed([base], [0, 0, 0, 0, 0]) as det:
        out, fl = det.run(x)
        cols = det.spectrogram(x)                             # (a plain handle: the spectrogram is there)
    with sd.SyllableDetector(base, channels=5) as det:
        o, f = det.run(x)
        c2 = det.spectrogram(x)
    torch.cuda.synchronize()
    _assert_equal(out, fl, o, f)
    assert torch.equal(_bits(cols), _bits(c2))


def test_refusals_and_geometry_on_a_device():
    torch = _torch()
    cfgs = _three_classes()
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.SyllableDetector.mixed(cfgs, [0, 1, 2, 3], engine=_abi.ENGINE_FUSED)
    assert ei.value.status == _abi.ERR_UNSUPPORTED
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.SyllableDetector.mixed(cfgs, [0, 1, 2, 3], engine=_abi.ENGINE_WIDE_BF16)
    assert ei.value.status == _abi.ERR_UNSUPPORTED
    x = torch.from_numpy(synth.channels(4, 132 * 300 + 256, first=4)).cuda()
    with sd.SyllableDetector.mixed(cfgs, [0, 1, 2, 3]) as det:
        with pytest.raises(sd.SyllableDetectorError) as ei:
            det.spectrogram(x)
        assert ei.value.status == _abi.ERR_UNSUPPORTED
        with pytest.raises(sd.SyllableDetectorError) as ei:
            det.spectrogramHost(x.cpu().numpy())
        assert ei.value.status == _abi.ERR_UNSUPPORTED
        with pytest.raises(sd.SyllableDetectorError):
            det.channelGeometry(4)
    # FUSED where every class takes the fold kernel: the fold kernel for all of them
    with sd.SyllableDetector.mixed([cfgs[0], cfgs[1]], [1, 0, 1], engine=_abi.ENGINE_FUSED) as det:
        det.profile(True)
        det.run(x[:3].contiguous())
        torch.cuda.synchronize()
        assert util.launched(det) == ["fused_s_kernel", "fused_s_kernel"]
        assert [det.channelGeometry(c).bins for c in range(3)] == [cfgs[1].geometry().bins, cfgs[0].geometry().bins, cfgs[1].geometry().bins]


def test_cli_one_network_per_track(tmp_path):
    """`-n a -n b`: track t of a two-track file runs network t through one mixed bank.  Each track's lines equal a one-network
    run of that track's network on the same file, restricted to that track; a file with another number of tracks is refused."""
    import os
    import subprocess
    import wavutil
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "syllable_detector_swift_amd", "lib",
                       "syllable-detector-cli")
    base = util.sample_net()
    narrow = _with_band(base, 2000.0, 5000.0, seed=1)
    paths = []
    for k, cfg in enumerate((base, narrow)):
        p = tmp_path / ("net%d.txt" % k)
        p.write_text(cfg.toText())
        paths.append(str(p))
    n = 5 * 44100
    q = np.stack([np.clip(np.round(synth.syllable_channel(n, util.template(), seed=40 + c) * 32768.0), -32768, 32767)
                  for c in range(2)], axis=1).astype(np.int16)
    wav = str(tmp_path / "two.wav")
    wavutil.write_wav(wav, q, 44100, "pcm16")

    def run(*args, ok=True):
        r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=600)
        assert (r.returncode == 0) == ok, r.stderr
        return r.stdout.splitlines()
    both = run("-n", paths[0], "-n", paths[1], "-a", wav, "--chunk", "0")
    assert both
    for t in range(2):
        own = [ln for ln in run("-n", paths[t], "-a", wav, "--chunk", "0") if ln.split(",")[0] == str(t)]
        mine = [ln for ln in both if ln.split(",")[0] == str(t)]
        assert mine == own, t
    mono = str(tmp_path / "mono.wav")
    wavutil.write_wav(mono, q[:, :1], 44100, "pcm16")
    r = subprocess.run([cli, "-n", paths[0], "-n", paths[1], "-a", mono], capture_output=True, text=True, timeout=600)
    assert not r.stdout.strip() and "2 networks" in r.stderr      # (skipped, as an unreadable file is)
