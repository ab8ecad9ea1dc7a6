"""Multi-network banks on the device (syldet_create_multi): one handle, a network per channel.  Per channel the arithmetic is
exactly that of a handle of the channel's own network, so every case is held to EQUALITY with single-network handles made from
the same configuration on the same samples -- outputs bit for bit (NaN included), flags, detections, the exact recomputation's
work -- and the hot path also to the fp64 oracle of each channel's own network."""
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


def _run_multi(cfgs, channel_net, x, engine=_abi.ENGINE_AUTO):
    torch = _torch()
    with sd.SyllableDetector.multi(cfgs, channel_net, engine=engine) as det:
        det.profile(True)
        out, fl = det.run(x)
        torch.cuda.synchronize()
        return out, fl, util.launched(det), det.fixupStats(), det.geometry.engine


def _run_singles(cfgs, channel_net, x, engine=_abi.ENGINE_AUTO, mask=True):
    """Network k's own handle over the whole batch (the same segmentation as the multi handle's), with the channels of the
    other networks silenced when `mask` (so that its exact-recomputation items are its channels' alone).  Returns its rows."""
    torch = _torch()
    C = x.shape[0]
    net = np.asarray(channel_net)
    out = fl = None
    names, items = [], 0
    for k, cfg in enumerate(cfgs):
        rows = np.nonzero(net == k)[0]
        if rows.size == 0:
            continue
        xk = x
        if mask:
            xk = x.clone()
            other = torch.from_numpy(np.nonzero(net != k)[0]).to(x.device)
            xk[other] = 0.0
        with sd.SyllableDetector(cfg, channels=C, engine=engine) as det:
            det.profile(True)
            o, f = det.run(xk)
            torch.cuda.synchronize()
            names.append(util.launched(det))
            items += det.fixupStats()[0]
        if out is None:
            out, fl = torch.empty_like(o), torch.empty_like(f)
        r = torch.from_numpy(rows).to(x.device)
        out[r] = o[r]
        fl[r] = f[r]
        del o, f, xk
    return out, fl, names, items


def _assert_equal(a_out, a_fl, b_out, b_fl):
    torch = _torch()
    assert a_out.shape == b_out.shape and a_fl.shape == b_fl.shape
    same = (_bits(a_out) == _bits(b_out)).all(dim=-1).all(dim=-1)
    assert bool(same.all()), "outputs differ on channels %s" % torch.nonzero(~same).flatten().tolist()[:8]
    assert torch.equal(a_fl, b_fl)


def _variants(base, K, seed0=100):
    return [base] + [nets.perturbed(base, seed0 + k) for k in range(1, K)]


def test_hot_path_eight_networks_interleaved(oracle_lib):
    """The reference's example class with K = 8 networks and channel c on network (5 c) mod 8: one launch of the fold kernel,
    every channel equal to its own network's handle and within the flat 1e-5 of that network's fp64 oracle."""
    torch = _torch()
    base = util.sample_net()
    cfgs = _variants(base, 8)
    C = 64
    channel_net = [(5 * c) % 8 for c in range(C)]
    S = 44100 * 2 + 77
    xh = np.stack([synth.syllable_channel(S, util.template(), seed=200 + c) if c % 3 == 0 else synth.channel(S, c)
                   for c in range(C)]).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    out, fl, names, fix, engine = _run_multi(cfgs, channel_net, x)
    assert engine == _abi.ENGINE_FUSED and names == ["fused_s_kernel"]
    s_out, s_fl, s_names, s_items = _run_singles(cfgs, channel_net, x)
    assert all(n == ["fused_s_kernel"] for n in s_names)
    _assert_equal(out, fl, s_out, s_fl)
    assert fix[0] == s_items
    out, fl = out.cpu().numpy(), fl.cpu().numpy()
    assert fl.sum() > 0
    oracles = [util.oracle_for(c) for c in cfgs]
    for c in range(C):
        cfg = cfgs[channel_net[c]]
        _, _, w64 = oracles[channel_net[c]].run(xh[c], po.F64)
        util.assert_outputs_close(out[c], w64)
        util.assert_flags_exact(fl[c], w64, cfg.thresholds, cfg.rule)


def test_hot_path_at_full_size():
    """64 channels x 2^24 samples (the benchmark's batch), eight networks: equal to the eight single handles."""
    torch = _torch()
    base = util.sample_net()
    cfgs = _variants(base, 8, seed0=300)
    C, S = 64, 1 << 24
    channel_net = [(5 * c) % 8 for c in range(C)]
    x = synth.channels_on_device(C, S, torch.device("cuda", 0), fs=base.samplingRate)
    out, fl, names, _, _ = _run_multi(cfgs, channel_net, x)
    assert names == ["fused_s_kernel"]
    s_out, s_fl, s_names, _ = _run_singles(cfgs, channel_net, x, mask=False)
    assert all(n == ["fused_s_kernel"] for n in s_names)
    _assert_equal(out, fl, s_out, s_fl)
    assert int(fl.sum()) > 0


def _class_case(cfg, x, K=3, channel_net=None):
    torch = _torch()
    cfgs = _variants(cfg, K, seed0=17)
    C = x.shape[0]
    channel_net = channel_net or [(2 * c + 1) % K for c in range(C)]
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out, fl, names, fix, _ = _run_multi(cfgs, channel_net, xd)
    assert names == ["fused_s_kernel"], names
    s_out, s_fl, s_names, s_items = _run_singles(cfgs, channel_net, xd)
    assert all(n == ["fused_s_kernel"] for n in s_names), s_names
    _assert_equal(out, fl, s_out, s_fl)
    assert fix[0] == s_items


def _class_input(S, C=6, hop=132, level_step=True):
    x = np.stack([synth.syllable_channel(S, util.template(), seed=60 + c, hop=hop) if c % 2 else synth.channel(S, 40 + c)
                  for c in range(C)]).astype(np.float32)
    if level_step:
        x[1, S // 2:] *= np.float32(0.004)
        x[2, 3000:3000 + 4 * 256] = 0.0
    return x


@pytest.mark.parametrize("H", [4, 8, 16])
@pytest.mark.parametrize("n_out", [1, 2, 4])
def test_fold_kernel_hidden_widths_and_outputs(H, n_out):
    rng = np.random.default_rng(10 * H + n_out)
    base = util.sample_net()
    net = nets.random_net(rng, 290, (H,), n_out, in_fns=("l2normalize", "mapminmax"), out_fns=("mapminmax",))
    cfg = nets.variant(base, net=net, thresholds=[float(t) for t in rng.uniform(-0.2, 0.3, n_out)], rule=n_out % 2)
    _class_case(cfg, _class_input(132 * 900 + 311))


@pytest.mark.parametrize("chain", [("l2normalize", "mapminmax"), ("normalize", "mapminmax"), ("normalizestd", "mapstd"), ("mapminmax",)])
def test_fold_kernel_every_normaliser_and_none(chain):
    rng = np.random.default_rng(len(chain) + 7 * len(chain[0]))
    base = util.sample_net()
    cfg = nets.variant(base, net=nets.random_net(rng, 290, (4,), 1, in_fns=chain, out_fns=("mapminmax",)), thresholds=[0.1])
    _class_case(cfg, _class_input(132 * 700 + 256))


@pytest.mark.parametrize("scaling", ["log", "db"])
def test_fold_kernel_log_and_db_behind_l2normalize(scaling):
    rng = np.random.default_rng(5)
    base = util.sample_net()
    cfg = nets.variant(base, net=nets.random_net(rng, 290, (4,), 1, in_fns=("l2normalize", "mapminmax"), out_fns=("mapminmax",)),
                       spectrogramScaling=scaling, thresholds=[0.1])
    _class_case(cfg, _class_input(132 * 700 + 256))


def test_fold_kernel_hop_128_staggered_chunks():
    rng = np.random.default_rng(128)
    base = util.sample_net()
    cfg = nets.variant(base, windowOverlap=128, net=nets.random_net(rng, 290, (4,), 1), thresholds=[0.1])
    _class_case(cfg, _class_input(128 * 1500 + 300, hop=128))


def test_fold_kernel_64_bin_band():
    rng = np.random.default_rng(64)
    base = util.sample_net()
    F = 61                                                     # (500 .. 11000 Hz under 256-point frames: bins 3 .. 63)
    cfg = nets.variant(base, freqRange=(500.0, 11000.0), net=nets.random_net(rng, F * 10, (4,), 1), thresholds=[0.1])
    assert cfg.geometry().bins == F
    _class_case(cfg, _class_input(132 * 700 + 256))


@pytest.mark.parametrize("which", ["log_behind_normalize", "1024_point_frames"])
def test_generic_engine_where_auto_keeps_it(which):
    """Structures AUTO keeps off the fold kernel: the multi handle's AUTO and GENERIC both run the generic engine exactly as a
    handle created with SYLDET_ENGINE_GENERIC does (FFT + the interpretive network kernels, per channel its own parameters)."""
    torch = _torch()
    base = util.sample_net()
    rng = np.random.default_rng(3)
    if which == "log_behind_normalize":
        cfg = nets.variant(base, net=nets.random_net(rng, 290, (4,), 1, in_fns=("normalize", "mapminmax"), out_fns=("mapminmax",)),
                           spectrogramScaling="log", thresholds=[0.0])
        S = 132 * 600 + 256
    else:
        cfg = nets.config3()
        S = 256 * 500 + 1024
    cfgs = _variants(cfg, 3, seed0=40)
    C = 5
    channel_net = [2, 0, 1, 0, 2]
    x = torch.from_numpy(synth.channels(C, S, first=9)).cuda()
    s_out, s_fl, s_names, _ = _run_singles(cfgs, channel_net, x, engine=_abi.ENGINE_GENERIC)
    for engine in (_abi.ENGINE_AUTO, _abi.ENGINE_GENERIC):
        out, fl, names, _, geom_engine = _run_multi(cfgs, channel_net, x, engine=engine)
        assert geom_engine == _abi.ENGINE_GENERIC
        assert names and not any(n.startswith("fused") for n in names), names
        assert names == s_names[0], (names, s_names[0])
        _assert_equal(out, fl, s_out, s_fl)


def test_exact_recomputation_uses_each_channels_network():
    """A chain without a normaliser through a loud recording: the fold kernel hands windows to the exact recomputation
    (fixup_kernel).  The two channels that carry the same audio run different networks; the recomputed evaluations must be
    each channel's own network's -- bit for bit the single handles' -- and the work the sum of theirs."""
    torch = _torch()
    base = util.sample_net()
    cfg = nets.variant(base, net=nets.random_net(np.random.default_rng(3), 290, (4,), 1, in_fns=()))
    cfgs = _variants(cfg, 2, seed0=70)
    S = 132 * 2000 + 256
    a, b = synth.channels(2, S, first=1) * np.float32(10.0)
    x = torch.from_numpy(np.stack([a, a, b, b]).astype(np.float32)).cuda()
    channel_net = [0, 1, 1, 0]
    out, fl, names, (items, over), _ = _run_multi(cfgs, channel_net, x)
    assert names == ["fused_s_kernel"] and over == 0
    s_out, s_fl, _, s_items = _run_singles(cfgs, channel_net, x)
    assert s_items > 0 and items == s_items
    _assert_equal(out, fl, s_out, s_fl)
    # the same audio through the two networks: different results (the networks really differ where the recomputation ran)
    assert not bool((_bits(out[0]) == _bits(out[1])).all())


def test_streaming_equals_batch_and_each_channel_keeps_its_threshold():
    """append_interleaved + process_all + process_new_value on a multi handle: every channel's evaluations bit for bit the batch
    call's, handed out in order; last_detected / seen_syllable against the channel's own network's threshold."""
    torch = _torch()
    base = util.sample_net()
    cfgs = [nets.variant(base, thresholds=[-1e6]), nets.perturbed(base, 5), nets.variant(nets.perturbed(base, 6), thresholds=[1e6])]
    C = 6
    channel_net = [2, 0, 1, 1, 0, 2]
    S = 132 * 300 + 256
    x = synth.channels(C, S, first=20)
    with sd.SyllableDetector.multi(cfgs, channel_net) as det:
        out, fl = det.run(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        out, fl = out.cpu().numpy(), fl.cpu().numpy()
        got = [[] for _ in range(C)]
        det_flags = [[] for _ in range(C)]
        pos = 0
        rng = np.random.default_rng(1)
        while pos < S:
            n = int(rng.integers(1, 5000))
            det.appendInterleavedData(np.ascontiguousarray(x[:, pos:pos + n].T))
            pos += n
            det.processAll()
            for c in range(C):
                while det.processNewValue(c):
                    got[c].append(det.lastOutputsFor(c))
                    det_flags[c].append(det.lastDetectedFor(c))
        for c in range(C):
            g = np.asarray(got[c], np.float32)
            assert g.shape == out[c].shape
            assert np.array_equal(g.view(np.int32), out[c].view(np.int32)), c
            thr = cfgs[channel_net[c]].thresholds[0]
            assert det_flags[c] == [bool(v >= thr) for v in g[:, 0]]
            assert np.array_equal(np.asarray(det_flags[c], np.uint8), fl[c])
        assert all(all(det_flags[c]) for c in range(C) if channel_net[c] == 0)
        assert not any(any(det_flags[c]) for c in range(C) if channel_net[c] == 2)
        # seenSyllable drains what is pending against the channel's own threshold: always on network 0, never on network 2
        for c in range(C):
            det.appendAudioData(x[c, :132 * 20], c)
            seen = det.seenSyllable(c)
            if channel_net[c] != 1:
                assert seen == (channel_net[c] == 0), c
            assert det.pendingEvaluations(c) == 0


def test_detections_per_channel():
    torch = _torch()
    base = util.sample_net()
    cfgs = _variants(base, 4, seed0=90)
    C = 8
    channel_net = [3, 1, 0, 2, 1, 3, 0, 2]
    S = 44100 * 3
    x = torch.from_numpy(np.stack([synth.syllable_channel(S, util.template(), seed=500 + c) for c in range(C)])).cuda()
    with sd.SyllableDetector.multi(cfgs, channel_net) as det:
        _, fl = det.run(x)
        idx, cnt = det.detections(fl, debounce=0.1)
        torch.cuda.synchronize()
    _, s_fl, _, _ = _run_singles(cfgs, channel_net, x, mask=False)
    assert torch.equal(fl, s_fl)
    net = np.asarray(channel_net)
    for k, cfg in enumerate(cfgs):
        with sd.SyllableDetector(cfg, channels=C) as det:
            _, f = det.run(x)
            i2, c2 = det.detections(f, debounce=0.1)
            torch.cuda.synchronize()
        for c in np.nonzero(net == k)[0]:
            assert int(cnt[c]) == int(c2[c])
            assert torch.equal(idx[c, :int(cnt[c])], i2[c, :int(c2[c])])
    assert int(cnt.sum()) > 0


def test_one_network_is_a_plain_handle():
    torch = _torch()
    base = util.sample_net()
    x = torch.from_numpy(synth.channels(3, 132 * 500 + 256, first=2)).cuda()
    with sd.SyllableDetector.multi([base], [0, 0, 0]) as det:
        out, fl = det.run(x)
    with sd.SyllableDetector(base, channels=3) as det:
        o, f = det.run(x)
    torch.cuda.synchronize()
    _assert_equal(out, fl, o, f)


def test_refusals_on_a_device():
    base = util.sample_net()
    c3 = nets.config3()
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.SyllableDetector.multi([c3, nets.perturbed(c3, 1)], [0, 1], engine=_abi.ENGINE_FUSED)
    assert ei.value.status == _abi.ERR_UNSUPPORTED
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.SyllableDetector.multi([base, nets.perturbed(base, 1)], [0, 1], engine=_abi.ENGINE_WIDE_BF16)
    assert ei.value.status == _abi.ERR_UNSUPPORTED
    # ... and on request the fold kernel where it takes the shape
    with sd.SyllableDetector.multi([base, nets.perturbed(base, 1)], [1, 0], engine=_abi.ENGINE_FUSED) as det:
        assert det.geometry.engine == _abi.ENGINE_FUSED
