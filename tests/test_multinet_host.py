"""Multi-network banks on the host (no GPU): which configurations may share a handle (syldet_config_compatible), and the
argument checks of syldet_create_multi, which all run before a device is touched."""
import copy
import ctypes as C

import numpy as np
import pytest

import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets


def _base():
    return util.sample_net()


def _structural_changes(base):
    """(field the library names, a configuration that differs from base there and nowhere else in its shape)"""
    out = []
    # (the band moved with the framing so that it keeps its bins and the network its inputs)
    r = 48000.0 / base.samplingRate
    out.append(("sampling_rate", nets.variant(base, samplingRate=48000.0, freqRange=(base.freqRange[0] * r, base.freqRange[1] * r))))
    out.append(("fourier_length", nets.variant(base, fourierLength=512, freqRange=(base.freqRange[0] / 2, base.freqRange[1] / 2))))
    out.append(("window_length", nets.variant(base, windowLength=192, windowOverlap=60)))
    out.append(("window_overlap", nets.variant(base, windowOverlap=128)))
    c = nets.variant(base, timeRange=base.timeRange - 1)                  # (the first layer must keep matching the inputs)
    F = base.net.inputs // base.timeRange
    c.net.layers[0] = sd.NeuralNetLayer(F * c.timeRange, 4, np.asarray(base.net.layers[0].weights)[:, :F * c.timeRange],
                                        base.net.layers[0].biases, "TanSig")
    c.net.inputProcessing = [sd.ProcessingFunction("l2normalize"),
                             sd.ProcessingFunction("mapminmax", np.asarray(base.net.inputProcessing[1].xOffsets)[:F * c.timeRange],
                                                   np.asarray(base.net.inputProcessing[1].gains)[:F * c.timeRange],
                                                   base.net.inputProcessing[1].y)]
    out.append(("time_range", c))
    out.append(("scaling", nets.variant(base, spectrogramScaling="log")))
    out.append(("window", nets.variant(base, window=_abi.WINDOW_HANNING)))
    out.append(("spectrum", nets.variant(base, spectrum=_abi.SPECTRUM_MAGNITUDE)))
    out.append(("rule", nets.variant(base, rule=_abi.RULE_ANY)))
    c = copy.deepcopy(base)
    c.net.inputProcessing = c.net.inputProcessing[1:]
    out.append(("n_input_fns", c))
    c = copy.deepcopy(base)
    c.net.inputProcessing[0] = sd.ProcessingFunction("normalize")
    out.append(("input_fns.kind", c))
    c = copy.deepcopy(base)
    c.net.outputProcessing = []
    out.append(("n_output_fns", c))
    c = copy.deepcopy(base)
    f = c.net.outputProcessing[0]
    c.net.outputProcessing[0] = sd.ProcessingFunction("mapstd", f.xOffsets, f.gains, f.y)
    out.append(("output_fns.kind", c))
    c = copy.deepcopy(base)
    L0, L1 = c.net.layers
    c.net.layers = [L0, sd.NeuralNetLayer(4, 4, np.eye(4, dtype=np.float32), np.zeros(4, np.float32), "TanSig"), L1]
    out.append(("n_layers", c))
    c = copy.deepcopy(base)
    rng = np.random.default_rng(3)
    c.net.layers[0] = sd.NeuralNetLayer(L0.inputs, 6, rng.standard_normal((6, L0.inputs)).astype(np.float32) * 0.05,
                                        np.zeros(6, np.float32), "TanSig")
    c.net.layers[1] = sd.NeuralNetLayer(6, 1, rng.standard_normal((1, 6)).astype(np.float32), np.zeros(1, np.float32), "PureLin")
    out.append(("layers.outputs", c))
    c = copy.deepcopy(base)
    c.net.layers[0].transferFunction = "LogSig"
    out.append(("layers.transfer", c))
    c = copy.deepcopy(base)
    c.net.layers[1] = sd.NeuralNetLayer(4, 2, rng.standard_normal((2, 4)).astype(np.float32), np.zeros(2, np.float32), "PureLin")
    f = c.net.outputProcessing[0]
    c.net.outputProcessing[0] = sd.ProcessingFunction("mapminmax", np.repeat(np.asarray(f.xOffsets), 2), np.repeat(np.asarray(f.gains), 2), f.y)
    c.thresholds = [0.5, 0.5]
    out.append(("layers.outputs", c))
    return out


def test_structural_differences_are_named():
    base = _base()
    for field, other in _structural_changes(base):
        other.geometry()                                   # (each is a valid configuration of its own)
        ok, got = sd.configsCompatible(base, other)
        assert (ok, got) == (False, field), "%s: got %s" % (field, (ok, got))
        ok, got = sd.configsCompatible(other, base)
        assert (ok, got) == (False, field)


def test_band_is_compared_not_the_frequencies():
    base = _base()
    f0, f1 = base.geometry().f0, base.geometry().f1
    fs, N = base.samplingRate, base.fourierLength
    # freq_lo moved by a fraction of a bin: the same band -> compatible
    same = nets.variant(base, freqRange=(base.freqRange[0] + 0.25 * fs / N, base.freqRange[1]))
    assert (same.geometry().f0, same.geometry().f1) == (f0, f1)
    assert sd.configsCompatible(base, same) == (True, None)
    # a band one bin lower and wider: the first layer would have to change too, so keep the inputs and move the whole band
    moved = nets.variant(base, freqRange=(base.freqRange[0] - fs / N, base.freqRange[1] - fs / N))
    assert (moved.geometry().f0, moved.geometry().f1) != (f0, f1)
    assert sd.configsCompatible(base, moved) == (False, "band")


def test_parameters_may_differ():
    base = _base()
    for seed in range(4):
        other = nets.perturbed(base, seed)
        assert not np.array_equal(other.net.layers[0].weights, base.net.layers[0].weights)
        assert other.thresholds != base.thresholds
        assert sd.configsCompatible(base, other) == (True, None)
    # each kind of parameter alone
    c = copy.deepcopy(base)
    c.net.layers[1].biases = np.asarray(c.net.layers[1].biases) + 1.0
    assert sd.configsCompatible(base, c) == (True, None)
    c = copy.deepcopy(base)
    c.net.inputProcessing[1].gains = np.asarray(c.net.inputProcessing[1].gains) * 2.0
    c.net.outputProcessing[0].y = 0.5
    assert sd.configsCompatible(base, c) == (True, None)
    c = nets.variant(base, thresholds=[0.9])
    assert sd.configsCompatible(base, c) == (True, None)


def test_compatible_rejects_null_and_invalid():
    base = _base()
    ca, keep = base.to_abi()
    field = C.c_char_p()
    assert _abi.lib.syldet_config_compatible(None, C.byref(ca), C.byref(field)) == _abi.ERR_INVALID_ARGUMENT
    bad = nets.variant(base, thresholds=[0.5, 0.5])        # threshold count != outputs: what syldet_create refuses
    cb, keep2 = bad.to_abi()
    assert _abi.lib.syldet_config_compatible(C.byref(ca), C.byref(cb), C.byref(field)) == _abi.ERR_THRESHOLD_MISMATCH
    del keep, keep2


def _create_multi(cfgs, channel_net, engine=_abi.ENGINE_AUTO, n_nets=None, null_cfg=False):
    abi = [c.to_abi() for c in cfgs]
    ptrs = (_abi.Config_p * max(1, len(abi)))(*[C.pointer(c) for c, _ in abi])
    cn = np.ascontiguousarray(channel_net, np.int32)
    h = _abi.Handle()
    st = _abi.lib.syldet_create_multi(None if null_cfg else ptrs, len(abi) if n_nets is None else n_nets,
                                      cn.ctypes.data_as(_abi.c_int32_p), cn.size, 0, engine, C.byref(h))
    assert not h.value, "no handle may come back from a refused call"
    return st, _abi.last_error()


def test_create_multi_argument_errors_need_no_device():
    base = _base()
    nets2 = [base, nets.perturbed(base, 1)]
    assert _create_multi(nets2, [0, 2])[0] == _abi.ERR_INVALID_ARGUMENT          # index outside [0, n_nets)
    assert _create_multi(nets2, [0, -1])[0] == _abi.ERR_INVALID_ARGUMENT
    assert _create_multi(nets2, [0, 1], null_cfg=True)[0] == _abi.ERR_INVALID_ARGUMENT
    assert _create_multi(nets2, [0, 0], n_nets=0)[0] == _abi.ERR_INVALID_ARGUMENT
    st, msg = _create_multi([base, nets.variant(base, rule=_abi.RULE_ANY)], [0, 1])
    assert st == _abi.ERR_UNSUPPORTED and "rule" in msg
    st, msg = _create_multi([base, nets.variant(base, windowOverlap=128)], [0, 0])   # (even a network nobody uses must fit)
    assert st == _abi.ERR_UNSUPPORTED and "window_overlap" in msg
    assert _create_multi(nets2, [0, 1], engine=_abi.ENGINE_WIDE_BF16)[0] == _abi.ERR_UNSUPPORTED
    assert _create_multi(nets2, [0, 1], engine=7)[0] == _abi.ERR_INVALID_ARGUMENT
    # a NULL entry in the list
    abi = [base.to_abi()]
    ptrs = (_abi.Config_p * 2)(C.pointer(abi[0][0]), None)
    cn = np.zeros(2, np.int32)
    h = _abi.Handle()
    assert _abi.lib.syldet_create_multi(ptrs, 2, cn.ctypes.data_as(_abi.c_int32_p), 2, 0, 0, C.byref(h)) == _abi.ERR_INVALID_ARGUMENT
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.SyllableDetector.multi(nets2, [0, 3])
    assert ei.value.status == _abi.ERR_INVALID_ARGUMENT
