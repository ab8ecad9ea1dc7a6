"""Mixed banks on the host (no GPU): which configurations share the evaluation clock (syldet_config_same_clock), and the
argument checks of syldet_create_mixed, which all run before a device is touched."""
import copy
import ctypes as C

import numpy as np
import pytest

import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets


def _with_band(base, lo, hi, fourier_length=None, hidden=4, seed=0, **changes):
    """base's framing with another band (and FFT size): a first layer sized for the bins that band gives"""
    N = fourier_length or base.fourierLength
    f0, f1 = sd.frequencyIndexRange(N, base.samplingRate, lo, hi)
    net = nets.random_net(np.random.default_rng(seed), (f1 - f0) * base.timeRange, (hidden,), 1)
    return nets.variant(base, fourierLength=N, freqRange=(lo, hi), net=net, thresholds=[0.1], **changes)


def _clock_changes(base):
    """(field the library names, a configuration that differs from base in that clock field alone)"""
    out = []
    r = 48000.0 / base.samplingRate                        # (the band moved with the rate so that it keeps its bins)
    out.append(("sampling_rate", nets.variant(base, samplingRate=48000.0, freqRange=(base.freqRange[0] * r, base.freqRange[1] * r))))
    out.append(("window_length", nets.variant(base, windowLength=192, windowOverlap=60)))
    out.append(("window_overlap", nets.variant(base, windowOverlap=128)))
    c = nets.variant(base, timeRange=base.timeRange - 1)
    F = base.net.inputs // base.timeRange
    c.net = nets.random_net(np.random.default_rng(1), F * c.timeRange, (4,), 1)
    out.append(("time_range", c))
    c = copy.deepcopy(base)
    rng = np.random.default_rng(2)
    L1 = c.net.layers[1]
    c.net.layers[1] = sd.NeuralNetLayer(4, 2, rng.standard_normal((2, 4)).astype(np.float32), np.zeros(2, np.float32), "PureLin")
    f = c.net.outputProcessing[0]
    c.net.outputProcessing[0] = sd.ProcessingFunction("mapminmax", np.repeat(np.asarray(f.xOffsets), 2), np.repeat(np.asarray(f.gains), 2), f.y)
    c.thresholds = [0.5, 0.5]
    assert L1.outputs == 1
    out.append(("n_thresholds", c))
    return out


def _free_changes(base):
    """configurations that share base's clock but not its band, FFT size, chain or widths (each valid on its own)"""
    rng = np.random.default_rng(4)
    F = base.net.inputs // base.timeRange
    out = [
        _with_band(base, 2000.0, 5000.0),                                            # a narrower band: other bins and inputs
        _with_band(base, 1000.0, 9000.0, fourier_length=512, hidden=8, spectrogramScaling="log"),   # 512-point frames
        nets.variant(base, net=nets.random_net(rng, F * base.timeRange, (16,), 1)),  # a wider hidden layer
        nets.variant(base, net=nets.random_net(rng, F * base.timeRange, (6, 3), 1, transfer=("LogSig", "TanSig", "PureLin"),
                                               in_fns=("normalize", "mapminmax"), out_fns=())),   # another chain, three layers
        nets.variant(base, window=_abi.WINDOW_HANNING, spectrum=_abi.SPECTRUM_MAGNITUDE, rule=_abi.RULE_ANY),
    ]
    return out


def test_each_clock_field_is_named():
    base = util.sample_net()
    for field, other in _clock_changes(base):
        other.geometry()                                   # (each is a valid configuration of its own)
        assert sd.configsShareClock(base, other) == (False, field), field
        assert sd.configsShareClock(other, base) == (False, field), field


def test_band_fft_size_chain_and_widths_may_differ():
    base = util.sample_net()
    for other in _free_changes(base):
        other.geometry()
        assert sd.configsShareClock(base, other) == (True, None)
        assert sd.configsShareClock(other, base) == (True, None)
        assert sd.configsCompatible(base, other)[0] is False       # (what syldet_create_multi would refuse)
    assert sd.configsShareClock(base, nets.perturbed(base, 3)) == (True, None)


def test_same_clock_rejects_null_and_invalid():
    base = util.sample_net()
    ca, keep = base.to_abi()
    field = C.c_char_p()
    assert _abi.lib.syldet_config_same_clock(None, C.byref(ca), C.byref(field)) == _abi.ERR_INVALID_ARGUMENT
    assert _abi.lib.syldet_config_same_clock(C.byref(ca), None, None) == _abi.ERR_INVALID_ARGUMENT
    bad = nets.variant(base, thresholds=[0.5, 0.5])        # threshold count != outputs: what syldet_create refuses
    cb, keep2 = bad.to_abi()
    assert _abi.lib.syldet_config_same_clock(C.byref(ca), C.byref(cb), C.byref(field)) == _abi.ERR_THRESHOLD_MISMATCH
    del keep, keep2


def _create_mixed(cfgs, channel_net, engine=_abi.ENGINE_AUTO, n_nets=None, null_cfg=False, null_map=False):
    abi = [c.to_abi() for c in cfgs]
    ptrs = (_abi.Config_p * max(1, len(abi)))(*[C.pointer(c) for c, _ in abi])
    cn = np.ascontiguousarray(channel_net, np.int32)
    h = _abi.Handle()
    st = _abi.lib.syldet_create_mixed(None if null_cfg else ptrs, len(abi) if n_nets is None else n_nets,
                                      None if null_map else cn.ctypes.data_as(_abi.c_int32_p), cn.size, 0, engine, C.byref(h))
    assert not h.value, "no handle may come back from a refused call"
    return st, _abi.last_error()


def test_create_mixed_argument_errors_need_no_device():
    base = util.sample_net()
    narrow = _with_band(base, 2000.0, 5000.0)
    mixed = [base, narrow]
    assert _create_mixed(mixed, [0, 2])[0] == _abi.ERR_INVALID_ARGUMENT          # index outside [0, n_nets)
    assert _create_mixed(mixed, [0, -1])[0] == _abi.ERR_INVALID_ARGUMENT
    assert _create_mixed(mixed, [0, 1], null_cfg=True)[0] == _abi.ERR_INVALID_ARGUMENT
    assert _create_mixed(mixed, [0, 1], null_map=True)[0] == _abi.ERR_INVALID_ARGUMENT
    assert _create_mixed(mixed, [0, 0], n_nets=0)[0] == _abi.ERR_INVALID_ARGUMENT
    assert _create_mixed(mixed, [0, 1], engine=7)[0] == _abi.ERR_INVALID_ARGUMENT
    # a clock mismatch names the field -- even on a network nobody uses
    for field, other in _clock_changes(base):
        st, msg = _create_mixed([base, narrow, other], [0, 1, 0])
        assert st == _abi.ERR_UNSUPPORTED and field in msg, (field, msg)
        st, msg = _create_mixed([base, other], [0, 0])
        assert st == _abi.ERR_UNSUPPORTED and field in msg, (field, msg)
    # a configuration syldet_create refuses: the same status as there
    st, _ = _create_mixed([base, nets.variant(base, thresholds=[0.5, 0.5])], [0, 1])
    assert st == _abi.ERR_THRESHOLD_MISMATCH
    assert _create_mixed(mixed, [0, 1], engine=_abi.ENGINE_WIDE_BF16)[0] == _abi.ERR_UNSUPPORTED
    # FUSED with a class the fold kernel does not take (512-point frames): refused before the device
    gen = _with_band(base, 1000.0, 9000.0, fourier_length=512, hidden=8, spectrogramScaling="log")
    st, msg = _create_mixed([base, gen], [0, 1], engine=_abi.ENGINE_FUSED)
    assert st == _abi.ERR_UNSUPPORTED and "fold kernel" in msg, msg
    # a NULL entry in the list
    abi = [base.to_abi()]
    ptrs = (_abi.Config_p * 2)(C.pointer(abi[0][0]), None)
    cn = np.zeros(2, np.int32)
    h = _abi.Handle()
    assert _abi.lib.syldet_create_mixed(ptrs, 2, cn.ctypes.data_as(_abi.c_int32_p), 2, 0, 0, C.byref(h)) == _abi.ERR_INVALID_ARGUMENT
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.SyllableDetector.mixed(mixed, [0, 3])
    assert ei.value.status == _abi.ERR_INVALID_ARGUMENT
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.SyllableDetector.mixed([base, nets.variant(base, windowOverlap=128)], [0, 1])
    assert ei.value.status == _abi.ERR_UNSUPPORTED


def test_channel_geometry_argument_checks():
    assert _abi.lib.syldet_channel_geometry(None, 0, None) == _abi.ERR_INVALID_ARGUMENT
