"""Training from the tool without a GPU (include/syldet.h, "training from the tool"): syldet_train_adam_host, syldet_train_init_host
and syldet_train_input_map_host against the numpy model of tests/train_adam_ref.py, bit for bit; csrc/train_adam.hpp alone under
ASan and UBSan (a program of its own, tests/cpp/train_adam_test.cpp); syldet_config_save_text against toText(), byte for byte;
syldet_train_config_with; the entry points under ABI 1; and every usage error of --train through the tool, before any device."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import train_adam_ref as aref
import train_cases as cases
import util
import wavutil
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = _abi.lib
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
NEW = ["syldet_train_input_range_device", "syldet_train_input_map_host", "syldet_trainer_set_input_map", "syldet_trainer_input_map",
       "syldet_train_adam_device", "syldet_train_adam_host", "syldet_train_fit_device", "syldet_train_init_host", "syldet_train_config_with",
       "syldet_config_save_text"]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def test_symbols_exist_and_the_abi_is_still_1():
    with open(os.path.join(ROOT, "include", "syldet.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _abi.SIGNATURES and getattr(LIB, name).argtypes == _abi.SIGNATURES[name][1]
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert LIB.syldet_abi_version() == 1 == _abi.ABI_VERSION
    for name in ("inputRange", "setInputMap", "inputMap", "adamStep", "fitDevice", "fit", "fitInputMap"):
        assert callable(getattr(sd.Trainer, name)), name
    assert callable(sd.trainAdamHost) and callable(sd.trainInitHost) and callable(sd.trainInputMapHost) and callable(sd.SyllableDetectorConfig.saveText)


@pytest.mark.parametrize("P", [74, 1169])
def test_the_host_step_equals_the_model_to_the_bit(P):
    rng = np.random.default_rng(P)
    p = rng.standard_normal(P).astype(np.float32)
    # NaN and Inf in the moments in front of step 1: not read
    m = np.full(P, np.nan, np.float32)
    v = np.full(P, np.inf, np.float32)
    mp, mm, mv = p.copy(), m.copy(), v.copy()
    for t in range(1, 6):
        grad = (rng.standard_normal(P) * 10.0 ** rng.uniform(-6, 0, P)).astype(np.float32)
        grad[::17] = 0.0
        loss = (float(rng.uniform(0.1, 2.0)), 0.0 if t == 3 else float(rng.uniform(0.2, 3.0)))
        before = p.copy()
        p, m, v, mean = sd.trainAdamHost(p, m, v, grad, loss, t, lr=0.01)
        mp, mm, mv, mmean = aref.adam_step(mp, mm, mv, grad, loss, t, lr=0.01)
        assert _bits(p) == _bits(mp) and _bits(m) == _bits(mm) and _bits(v) == _bits(mv), t
        assert mean == mmean and (mean == 0.0) == (t == 3)
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
        assert (_bits(p) == _bits(before)) == (t == 3)                 # Wsum = 0: the parameters keep their bits
    # other hyperparameters than the defaults
    a = sd.trainAdamHost(p, m, v, grad, (1.0, 0.5), 7, lr=0.003, beta1=0.8, beta2=0.99, eps=1e-6)
    b = aref.adam_step(p, m, v, grad, (1.0, 0.5), 7, lr=0.003, beta1=0.8, beta2=0.99, eps=1e-6)
    assert all(_bits(x) == _bits(y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] == 2.0


def test_the_host_step_refuses_what_the_header_names():
    p = np.zeros(3, np.float32)
    for bad in (dict(step=0), dict(step=-1), dict(lr=float("nan")), dict(lr=float("inf")), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1.0), dict(eps=float("nan"))):
        kw = dict(step=1)
        kw.update(bad)
        with pytest.raises(sd.SyllableDetectorError) as e:
            sd.trainAdamHost(p, p, p, p, (1.0, 1.0), **kw)
        assert e.value.status == _abi.ERR_INVALID_ARGUMENT, bad


@pytest.mark.parametrize("shape", [(21, 3, 2), (290, 4, 1)])
def test_the_seeded_start_equals_the_model_to_the_bit(shape):
    I, H, O = shape
    for seed in (0, 1, 2 ** 63 + 12345):
        theta = sd.trainInitHost(seed, I, H, O)
        assert theta.size == H * I + H + O * H + O and _bits(theta) == _bits(aref.init(seed, I, H, O)), seed
        assert np.abs(theta[:H * I]).max() <= np.float32(np.sqrt(3.0 / I)) and not theta[-O:].any() and theta[:H * I].std() > 0.4 * np.sqrt(3.0 / I)
    assert _bits(sd.trainInitHost(0, I, H, O)) != _bits(sd.trainInitHost(1, I, H, O))
    with pytest.raises(sd.SyllableDetectorError):
        sd.trainInitHost(0, 0, H, O)


def test_the_input_map_of_a_range_equals_the_model_to_the_bit():
    rng = np.random.default_rng(3)
    lo = (rng.standard_normal(290) * 10.0 ** rng.uniform(-3, 2, 290)).astype(np.float32)
    hi = (lo + np.abs(rng.standard_normal(290)).astype(np.float32) * np.float32(3)).astype(np.float32)
    hi[7] = lo[7]                                      # a position that never moves: gain 1
    hi[9], lo[9] = np.float32(0.0), np.float32(0.0)
    xo, g = sd.trainInputMapHost(np.stack([lo, hi]))
    mxo, mg = aref.input_map(np.stack([lo, hi]))
    assert _bits(xo) == _bits(mxo) == _bits(lo) and _bits(g) == _bits(mg)
    assert g[7] == 1.0 and g[9] == 1.0 and (g > 0).all()
    # the least maps to -1 and the greatest to +1
    moving = hi > lo
    assert np.allclose(((hi - xo) * g - 1)[moving], 1.0, atol=1e-5)


def _networks(tmp):
    """the sample network, a small one with every kind of function, configuration 3, and every network under tests/golden"""
    out = [("sample", util.sample_net()), ("small", cases.small_net("LogSig", "SatLin", ("normalizestd", "mapstd"), ("mapminmax", "mapstd"), "db", seed=4)),
           ("config3", nets.config3())]
    for name in util.case_names():
        z = np.load(os.path.join(util.GOLD, name + ".npz"))
        path = tmp / ("cfg_%s.npz" % name)
        np.savez(path, **{k[4:]: z[k] for k in z.files if k.startswith("cfg_")})
        out.append((name, nets.from_npz(str(path))))
    return out


def test_the_text_writer_gives_toTexts_bytes_and_the_file_loads_again(tmp_path):
    seen = 0
    for name, cfg in _networks(tmp_path):
        path = tmp_path / ("%s.txt" % name)
        cfg.saveText(path)
        assert path.read_bytes() == cfg.toText().encode(), name
        again = sd.SyllableDetectorConfig.fromTextFile(str(path))
        assert again.spectrogramScaling == cfg.spectrogramScaling and list(again.thresholds) == [float(v) for v in cfg.thresholds]
        for a, b in zip(again.net.layers, cfg.net.layers):
            assert np.array_equal(np.asarray(a.weights, np.float32), np.asarray(b.weights, np.float32)) and np.array_equal(a.biases, np.asarray(b.biases, np.float32))
            assert a.transferFunction == b.transferFunction
        for fa, fb in zip(list(again.net.inputProcessing) + list(again.net.outputProcessing), list(cfg.net.inputProcessing) + list(cfg.net.outputProcessing)):
            assert fa.function == fb.function
            if fb.function in ("mapminmax", "mapstd"):
                assert np.array_equal(fa.xOffsets, np.asarray(fb.xOffsets, np.float32)) and np.array_equal(fa.gains, np.asarray(fb.gains, np.float32)) and fa.y == np.float32(fb.y)
        seen += 1
    assert seen >= 3 + len(util.case_names()) > 3
    c, keep = util.sample_net().to_abi()
    assert LIB.syldet_config_save_text(None, b"x") == _abi.ERR_INVALID_ARGUMENT and LIB.syldet_config_save_text(C.byref(c), None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_config_save_text(C.byref(c), str(tmp_path / "no" / "such" / "dir.txt").encode()) == _abi.ERR_PARSE_OPEN


def test_config_with_replaces_the_layers_and_the_map_and_checks_sizes(tmp_path):
    cfg = util.sample_net()
    c, keep = cfg.to_abi()
    P = sd.trainParamCount(cfg)
    theta = sd.trainInitHost(5, 290, 4, 1)
    xo = np.arange(290, dtype=np.float32)
    g = np.full(290, 0.5, np.float32)
    fp = lambda a: a.ctypes.data_as(_abi.c_float_p)
    out = _abi.Config_p()
    for n in (P - 1, P + 1, 0, -1):
        assert LIB.syldet_train_config_with(C.byref(c), fp(theta), n, None, None, 0.0, C.byref(out)) == _abi.ERR_INVALID_ARGUMENT and not out
    assert LIB.syldet_train_config_with(None, fp(theta), P, None, None, 0.0, C.byref(out)) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_train_config_with(C.byref(c), None, P, None, None, 0.0, C.byref(out)) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_train_config_with(C.byref(c), fp(theta), P, fp(xo), None, 0.0, C.byref(out)) == _abi.ERR_INVALID_ARGUMENT
    three = cases.small_net()
    three.net.layers = three.net.layers[:1]
    three.thresholds = [0.5] * 3
    c3, keep3 = three.to_abi()
    assert LIB.syldet_train_config_with(C.byref(c3), fp(theta), P, None, None, 0.0, C.byref(out)) == _abi.ERR_UNSUPPORTED
    nomap = cases.small_net(in_fns=("l2normalize",))
    cn, keepn = nomap.to_abi()
    small_theta = np.zeros(sd.trainParamCount(nomap), np.float32)
    assert LIB.syldet_train_config_with(C.byref(cn), fp(small_theta), small_theta.size, fp(xo), fp(g), -1.0, C.byref(out)) == _abi.ERR_UNSUPPORTED
    for with_map in (False, True):
        assert LIB.syldet_train_config_with(C.byref(c), fp(theta), P, fp(xo) if with_map else None, fp(g) if with_map else None, -0.5, C.byref(out)) == 0 and out
        path = tmp_path / ("with_%d.txt" % with_map)
        assert LIB.syldet_config_save_text(out, str(path).encode()) == 0
        LIB.syldet_config_free(out)
        out = _abi.Config_p()
        got = sd.SyllableDetectorConfig.fromTextFile(str(path))
        assert _bits(cases.theta_of(got)) == _bits(theta)
        m, was = got.net.inputProcessing[1], cfg.net.inputProcessing[1]
        assert m.function == "mapminmax"
        if with_map:
            assert np.array_equal(m.xOffsets, xo) and np.array_equal(m.gains, g) and m.y == -0.5
        else:
            assert np.array_equal(m.xOffsets, np.asarray(was.xOffsets, np.float32)) and np.array_equal(m.gains, np.asarray(was.gains, np.float32)) and m.y == was.y
        assert got.net.outputProcessing[0].function == cfg.net.outputProcessing[0].function and got.samplingRate == cfg.samplingRate


def test_the_step_alone_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "train_adam_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "train_adam_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


# ---- the tool's usage errors: all reported before a device is opened ----
def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_cli")
    net = d / "net.txt"
    net.write_text(util.sample_net().toText())
    three = cases.small_net()
    three.net.layers = [three.net.layers[0], sd.NeuralNetLayer(3, 3, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), "TanSig"), three.net.layers[1]]
    deep = d / "deep.txt"
    deep.write_text(three.toText())
    wide = d / "wide.txt"
    wide.write_text(cases.sample_wide(17, 1, "TanSig").toText())
    nomap = d / "nomap.txt"
    nomap.write_text(cases.small_net(in_fns=("l2normalize",)).toText())
    wav = d / "a.wav"
    wavutil.write_wav(str(wav), np.zeros((3000, 1)), 44100, "pcm16", False)
    labels = d / "labels.tsv"
    labels.write_text("%s\t0\t2000\n" % wav)
    return dict(dir=d, net=str(net), deep=str(deep), wide=str(wide), nomap=str(nomap), wav=str(wav), labels=str(labels))


def _usage(r, text):
    assert r.returncode == 64 and text in r.stderr and "Path to trained network file." in r.stdout, (r.returncode, r.stderr)


def test_train_needs_batch_and_an_output(files):
    out = str(files["dir"] / "out.txt")
    _usage(_cli("-n", files["net"], "-a", files["wav"], "--train", files["labels"], "--train-out", out), "--train needs --batch.")
    _usage(_cli("-n", files["net"], "-a", files["wav"], "--batch", "--train", files["labels"]), "--train <labels.tsv> needs --train-out <net.txt>.")
    assert not os.path.exists(out)


def test_train_takes_one_network_the_trainer_takes(files):
    out = str(files["dir"] / "out2.txt")
    common = ["-a", files["wav"], "--batch", "--train", files["labels"], "--train-out", out]
    _usage(_cli("-n", files["net"], "-n", files["net"], *common), "--train takes one network (-n).")
    _usage(_cli("-n", files["deep"], *common), "--train: the trainer does not take this network")
    _usage(_cli("-n", files["wide"], *common), "--train: the trainer does not take this network")
    _usage(_cli("-n", files["nomap"], *common, "--train-fit-map"), "--train-fit-map: the network has no mapminmax input function.")
    _usage(_cli("-n", files["net"], *common, "--train-output", "1"), "--train-output 1: the network has 1 output(s).")
    assert not os.path.exists(out)


@pytest.mark.parametrize("option", [["--train-out", "x.txt"], ["--train-steps", "5"], ["--train-rate", "0.01"], ["--train-width", "0.003"], ["--train-seed", "0"],
                                    ["--train-fit-map"], ["--train-output", "0"], ["--train-log", "log.tsv"]], ids=lambda o: o[0])
def test_the_dependent_options_need_train(files, option):
    _usage(_cli("-n", files["net"], "-a", files["wav"], "--batch", *option), "need --train <labels.tsv>.")


@pytest.mark.parametrize("option,text", [(["--train-steps", "-1"], "--train-steps takes a number of steps, 0 or more."), (["--train-steps", "x"], "--train-steps takes"),
                                         (["--train-rate", "nan"], "--train-rate takes a positive number."), (["--train-rate", "0"], "--train-rate takes a positive number."),
                                         (["--train-width", "-1"], "--train-width takes a number of seconds, 0 or more."),
                                         (["--train-seed", "-3"], "--train-seed takes a whole number, 0 or more."),
                                         (["--train-output", "-1"], "--train-output takes the number of a network output, 0 or more.")], ids=lambda o: " ".join(o) if isinstance(o, list) else None)
def test_the_train_options_values(files, option, text):
    _usage(_cli("-n", files["net"], "-a", files["wav"], "--batch", "--train", files["labels"], "--train-out", str(files["dir"] / "o.txt"), *option), text)


def test_the_usage_text_names_the_options():
    r = _cli("-h")
    for name in ("--train <labels.tsv>", "--train-out <net.txt>", "--train-steps <n>", "--train-rate <lr>", "--train-width <seconds>", "--train-seed <s>", "--train-fit-map",
                 "--train-output <k>", "--train-log <log.tsv>"):
        assert name in r.stdout, name
