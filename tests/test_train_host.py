"""Training, the host side (no GPU): the numpy model of tests/train_ref.py against central finite differences in float64 for every
transfer function and input chain; csrc/train_targets.hpp alone under ASan and UBSan (a program of its own,
tests/cpp/train_targets_test.cpp); syldet_train_targets_host against the Python-integer model, bit for bit;
syldet_train_param_count; the entry points under ABI 1; and every status that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import train_cases as cases
import train_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = _abi.lib
NEW = ("syldet_trainer_create", "syldet_trainer_destroy", "syldet_trainer_shape", "syldet_train_param_count", "syldet_train_targets_device",
       "syldet_train_targets_host", "syldet_train_gradient_device")
CHAINS = [(), ("l2normalize",), ("normalize",), ("normalizestd",), ("mapminmax",), ("mapstd",), ("l2normalize", "mapminmax"),
          ("normalizestd", "mapstd"), ("mapstd", "normalize", "mapminmax")]


def _loss64(net, cols, theta, t, w):
    """the loss alone, in float64, of float64 parameters (the model's forward)"""
    sel = np.nonzero(w > 0)[0]
    W1, b1, W2, b2 = ref.split(net, theta)
    x = ref.inputs(net, cols, sel, np.float64)
    a1 = x @ W1.T + b1
    h1 = ref._transfer(net.tf0, a1)
    a2 = h1 @ W2.T + b2
    y = ref._transfer(net.tf1, a2)
    for xo, g, yk in net.out_fns:
        y = (y - np.float64(yk)) / g.astype(np.float64) + xo.astype(np.float64)
    return float((w[sel].astype(np.float64) * ((y - t[sel]) ** 2).sum(axis=1)).sum()), a1, a2


@pytest.mark.parametrize("chain", CHAINS, ids=lambda c: "+".join(c) or "none")
@pytest.mark.parametrize("tf", ["TanSig", "LogSig", "PureLin", "SatLin"])
def test_the_models_gradient_is_the_finite_difference(tf, chain):
    scaling = ("linear", "log", "db")[len(chain) % 3]
    for seed in range(20):                             # (SatLin: a draw whose sums stay away from the kinks at 0 and 1)
        cfg = cases.small_net(tf0=tf, tf1=tf, in_fns=chain, out_fns=("mapminmax", "mapstd"), scaling=scaling, seed=100 + seed)
        net = ref.net_of(cfg, cases.SMALL_BINS)
        rng = np.random.default_rng(seed)
        E = 9
        cols = cases.columns(rng, E + net.T - 1, net.F)
        theta = cases.theta_of(cfg).astype(np.float64)
        if tf == "SatLin":
            theta[net.H * net.I:net.H * net.I + net.H] += 0.5
        t = rng.integers(0, 2, (E, net.O)).astype(np.float32)
        w = rng.uniform(0.1, 1.0, E).astype(np.float32)
        w[[2, 5]] = (0.0, np.nan)                      # unselected, whatever the columns hold
        _, a1, a2 = _loss64(net, cols, theta, t, np.nan_to_num(w))
        near = min(np.abs(a1).min(), np.abs(a1 - 1).min(), np.abs(a2).min(), np.abs(a2 - 1).min())
        if tf != "SatLin" or near > 1e-3:
            break
    else:
        pytest.fail("no draw away from the SatLin kinks")
    L, Ws, g, A = ref.gradient(net, cols, theta.astype(np.float32), t, w, np.float64)
    # (the model rounds theta to float32 first; so does this)
    theta = theta.astype(np.float32).astype(np.float64)
    wz = np.nan_to_num(w)
    assert L == pytest.approx(_loss64(net, cols, theta, t, wz)[0], rel=1e-12) and Ws == pytest.approx(float(wz[wz > 0].astype(np.float64).sum()), rel=1e-12)
    fd = np.zeros(net.P)
    for p in range(net.P):
        step = 1e-6 * max(1.0, abs(theta[p]))
        hi, lo = theta.copy(), theta.copy()
        hi[p] += step
        lo[p] -= step
        fd[p] = (_loss64(net, cols, hi, t, wz)[0] - _loss64(net, cols, lo, t, wz)[0]) / (hi[p] - lo[p])
    scale = np.maximum(A, 1e-12)
    assert (np.abs(fd - g) <= 1e-6 * scale + 1e-9).all(), float((np.abs(fd - g) / scale).max())
    assert (A >= np.abs(g) * (1 - 1e-12)).all()
    # the float32 model is the same function: it agrees to float32's precision of the term sums
    r = ref.bars(net, cols, theta.astype(np.float32), t, w)
    assert r[4] < 1e-4 and r[5] < 1e-4, r[4:]


def test_the_targets_rule_alone_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "train_targets_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "train_targets_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_symbols_exist_and_the_abi_is_still_1():
    with open(os.path.join(ROOT, "include", "syldet.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _abi.SIGNATURES and getattr(LIB, name).argtypes == _abi.SIGNATURES[name][1]
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert LIB.syldet_abi_version() == 1 == _abi.ABI_VERSION and "#define SYLDET_ABI_VERSION 1" in header
    section = header[header.index("---- training: loss and gradient"):]
    for word in ('"train_targets_kernel"', '"train_gradient_kernel"', '"train_combine_kernel"', "train_targets.hpp", "layer0.weights [H][I]",
                 "SELECTED iff", "no float atomics"):
        assert word in section, word
    assert re.search(r"#define SYLDET_TRAIN_MAX_HIDDEN +16\b", header) and _abi.TRAIN_MAX_HIDDEN == 16
    assert re.search(r"#define SYLDET_TRAIN_MAX_OUTPUTS +4\b", header) and _abi.TRAIN_MAX_OUTPUTS == 4
    assert callable(sd.SyllableDetector.trainer) and callable(sd.Recordings.trainer)
    for name in ("params", "configWith", "targets", "gradient", "fit", "fitInputMap"):
        assert callable(getattr(sd.Trainer, name)), name
    assert callable(sd.trainTargetsHost) and callable(sd.trainParamCount)


@pytest.mark.parametrize("hop", [132, 131])
def test_the_host_targets_equal_the_integer_model(hop):
    first = 9 * hop + 256
    rng = np.random.default_rng(hop)
    seen_pos = seen_neg = seen_two = 0
    for E in (0, 1, 2, 77, 300):
        end = first + E * hop
        for n_out in (1, 2, 4):
            for n_labels in (0, 1, 7, 40):
                labels = np.sort(rng.integers(-2000, end + 2001, n_labels))
                if n_labels >= 7:
                    labels[1] = labels[0]                                  # a repeated label, and two closer than any half width but 0
                    labels[6] = labels[5] + 3
                    labels = np.sort(labels)
                outs = rng.integers(0, n_out, n_labels).astype(np.int32)
                for hw in (0, 1, hop, 5 * hop):
                    for lo in (None, outs):
                        for wp, wn in ((0.25, 0.125), (0.5 / 7, 0.0), (0.0, 1.0 / 3)):
                            want_t, want_w = ref.targets(labels, lo, E, hw, wp, wn, first, hop, n_out)
                            got_t, got_w = sd.trainTargetsHost(labels, E, hw, wp, wn, first, hop, outputs=n_out, labelOutputs=lo)
                            assert got_t.tobytes() == want_t.tobytes() and got_w.tobytes() == want_w.tobytes(), (E, n_out, n_labels, hw)
                        seen_pos += int((want_t.sum(axis=1) > 0).sum())
                        seen_neg += int((want_t.sum(axis=1) == 0).sum())
                        seen_two += int((want_t.sum(axis=1) > 1).sum())
    assert seen_pos > 0 and seen_neg > 0 and seen_two > 0
    # a half width of 0 selects exactly the evaluation whose sample number a label is
    t, w = sd.trainTargetsHost([first + 5 * hop, first + 5 * hop + 1], 10, 0, 1.0, 0.0, first, hop)
    assert t[:, 0].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0] and np.array_equal(w, t[:, 0])


def test_the_parameter_count():
    assert sd.trainParamCount(util.sample_net()) == 290 * 4 + 4 + 4 + 1 == 1169
    assert sd.trainParamCount(nets.config3()) == 1160 * 4 + 4 + 4 + 1
    assert sd.trainParamCount(cases.small_net()) == 21 * 3 + 3 + 2 * 3 + 2
    assert sd.trainParamCount(cases.sample_wide()) == 290 * 16 + 16 + 4 * 16 + 4
    one = cases.small_net()
    one.net.layers = one.net.layers[:1]
    with pytest.raises(sd.SyllableDetectorError) as e:
        sd.trainParamCount(one)
    assert e.value.status == _abi.ERR_UNSUPPORTED
    n = C.c_int64()
    c, keep = util.sample_net().to_abi()
    assert LIB.syldet_train_param_count(None, C.byref(n)) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_train_param_count(C.byref(c), None) == _abi.ERR_INVALID_ARGUMENT


def test_the_statuses_that_need_no_device():
    labels = np.array([100, 200, 300], np.int64)
    outs = np.array([0, 1, 0], np.int32)
    t, w = np.zeros((5, 2), np.float32), np.zeros(5, np.float32)
    lp, op, tp, wp = labels.ctypes.data_as(_abi.c_int64_p), outs.ctypes.data_as(_abi.c_int32_p), t.ctypes.data_as(_abi.c_float_p), w.ctypes.data_as(_abi.c_float_p)
    names = (("labels", lp), ("n_labels", 3), ("outs", op), ("n_out", 2), ("hw", 10), ("wp", 0.5), ("wn", 0.25), ("first", 1444), ("hop", 132), ("n_evals", 5),
             ("targets", tp), ("weights", wp))
    call = lambda **kw: LIB.syldet_train_targets_host(*[kw.get(k, v) for k, v in names])
    assert call() == 0 and call(outs=None) == 0 and call(n_labels=0, labels=None) == 0 and call(n_evals=0, targets=None, weights=None) == 0
    assert call(wp=0.0, wn=0.0) == 0 and call(hw=0) == 0 and call(hw=2 ** 40) == 0
    before = (t.copy(), w.copy())
    unsorted = np.array([100, 99, 300], np.int64)
    for bad in (dict(labels=None), dict(targets=None), dict(weights=None), dict(n_labels=-1), dict(n_evals=-1), dict(n_out=0), dict(n_out=5), dict(hw=-1),
                dict(hw=2 ** 40 + 1), dict(wp=float("nan")), dict(wn=float("nan")), dict(wp=-0.5), dict(wn=-1e-9), dict(hop=0), dict(hop=2 ** 30 + 1),
                dict(n_out=1), dict(labels=unsorted.ctypes.data_as(_abi.c_int64_p)), dict(first=2 ** 61), dict(first=-2 ** 61)):
        assert call(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        assert np.array_equal(t, before[0]) and np.array_equal(w, before[1]), bad
    outs[1] = -1
    assert call() == _abi.ERR_INVALID_ARGUMENT and "label_output[1]" in _abi.last_error()
    # the calls on handles: NULL before anything else
    h = _abi.Handle()
    begin = np.zeros(2, np.int64)
    bp = begin.ctypes.data_as(_abi.c_int64_p)
    assert LIB.syldet_trainer_create(None, None, C.byref(h)) == _abi.ERR_INVALID_ARGUMENT and not h
    assert LIB.syldet_trainer_create(None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_trainer_shape(None, None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_train_targets_device(None, None, bp, None, 0, 1.0, 1.0, 0, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_train_gradient_device(None, None, 0, 0, None, None, None, 0, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_trainer_destroy(None) == 0
    # the bindings: a sharded bank has no trainer; the Python layer's own argument errors
    with pytest.raises(sd.SyllableDetectorError) as e:
        sd.ShardedSyllableDetectorBank.trainer(object())
    assert e.value.status == _abi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        sd.trainTargetsHost([1, 2], 4, 0, 1.0, 1.0, 0, 1, outputs=2, labelOutputs=[0])
    with pytest.raises(sd.SyllableDetectorError):
        sd.trainTargetsHost([1, 2], 4, -1, 1.0, 1.0, 0, 1)
