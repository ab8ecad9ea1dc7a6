"""Training from the tool on the GPU (include/syldet.h, "training from the tool"): the input range, the Adam step, the fit.

The range without a function in front of the map is numpy's min / max over the contributing windows, bit for bit.  Behind
normalisers the bar is |dev - m64| <= 8 max(e32, 2^-24 a): m64 and m32 are the ranges of tests/train_ref.py's inputs() in float64 and
in float32 on the same case, e32 = max |m32 - m64|, a = max |m64| -- the float32 model's own error with the margin of 8 that
tests/test_train_gpu.py gives the gradient (another summation order, fused multiply-adds, a log a few ulp from libm's); never
anything the device produced.  Each case prints its worst ratio.  The packed plan's range is the elementwise min / max of its
recordings' own ranges, bit for bit, whatever lies between them.  The Adam step is syldet_train_adam_host's bits; the fit is the
bits of as many gradient + step calls, three launches a step, and a refused call leaves the parameters alone."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import train_cases as cases
import train_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

pytestmark = pytest.mark.gpu

LENGTHS = [5000, 12001, 7000]


def _front(cfg, bins):
    """(the model's net of the functions in front of cfg's first mapminmax, that function's index)"""
    fns = cfg.net.inputProcessing
    at = next(k for k, f in enumerate(fns) if f.function == "mapminmax")
    front = copy.deepcopy(cfg)
    front.net.inputProcessing = fns[:at]
    return ref.net_of(front, bins), at


def _model_range(net, cols, w, dtype):
    """min / max [2, I] and the count over the contributing evaluations of every row: weight > 0 and all I values finite"""
    lo, hi, count = np.full(net.I, np.inf), np.full(net.I, -np.inf), 0
    for c in range(cols.shape[0]):
        with np.errstate(all="ignore"):
            sel = np.nonzero(w[c] > 0)[0]
            x = ref.inputs(net, cols[c], sel, dtype)
        x = x[np.isfinite(x).all(axis=1)]
        count += x.shape[0]
        if x.shape[0]:
            lo, hi = np.minimum(lo, x.min(axis=0)), np.maximum(hi, x.max(axis=0))
    return np.stack([lo, hi]), count


def _device_range(tr, cols, w):
    rng, count = tr.inputRange(torch.from_numpy(cols).cuda(), torch.from_numpy(w).cuda())
    torch.cuda.synchronize()
    return rng.cpu().numpy(), int(count.cpu())


def _third(rng, shape):
    """weights with one evaluation in three selected, by a seeded draw"""
    return np.where(rng.integers(0, 3, shape) == 0, rng.uniform(0.2, 1.0, shape), 0.0).astype(np.float32)


# ---- the range, exact ----
def test_the_range_in_front_of_a_bare_map_is_numpys_min_and_max_to_the_bit():
    cfg = cases.small_net(in_fns=("mapminmax",))
    with sd.SyllableDetector(cfg, channels=2) as det, det.trainer() as tr:
        tile, T, F = tr.tile, cfg.timeRange, det.geometry.bins
        E = tile + 37                                  # one full tile and one ragged tile a row
        rng = np.random.default_rng(21)
        cols = cases.columns(rng, E + T - 1, F, rows=2)
        w = _third(rng, (2, E))
        w[1, tile:] = 0.0                              # row 1's second tile: no selected evaluation
        w[0, 5] = np.nan                               # a NaN weight does not contribute
        w[0, 40:43] = 0.0                              # frame 42 is read by the evaluations 40, 41, 42 alone: all unselected
        cols[0, 42, 3] = np.nan
        w[0, tile + 10:tile + 13] = 0.5                # frame tile + 12 is read by three selected evaluations
        cols[0, tile + 12, 1] = np.inf
        with np.errstate(invalid="ignore"):
            selected = int((w > 0).sum())
        want, count = _model_range(_front(cfg, F)[0], cols, w, np.float32)
        assert count == selected - 3 and (w[1, :tile] > 0).any()
        want = (want + 0.0).astype(np.float32)         # (zeros by value: -0.0 + 0.0 is +0.0)
        got, n = _device_range(tr, cols, w)
        assert n == count
        assert got.tobytes() == want.tobytes() and np.isfinite(got).all()
        # the same call again: the same bits, launches only
        det.profile(True)
        try:
            again, n2 = _device_range(tr, cols, w)
            assert again.tobytes() == got.tobytes() and n2 == n
            names = det.lastTimings()
            assert [k for k, _ in names] == ["train_range_kernel", "train_range_combine_kernel"] and all(ms > 0 for _, ms in names)
        finally:
            det.profile(False)
        # zeros are written as +0.0
        z = np.zeros_like(cols)
        z[:, ::2] = -0.0
        got, n = _device_range(tr, z, np.ones((2, E), np.float32))
        assert n == 2 * E and got.tobytes() == np.zeros((2, 21), np.float32).tobytes()
        # no contributing evaluation: {+inf, -inf} and 0
        got, n = _device_range(tr, cols, np.zeros((2, E), np.float32))
        assert n == 0 and (got[0] == np.inf).all() and (got[1] == -np.inf).all()


# ---- the range behind normalisers ----
def _hold_range(name, cfg, rows, E_of, seed):
    with sd.SyllableDetector(cfg, channels=rows) as det, det.trainer() as tr:
        F, T = det.geometry.bins, cfg.timeRange
        E = E_of(tr.tile)
        rng = np.random.default_rng(seed)
        cols = cases.columns(rng, E + T - 1, F, rows=rows)
        w = _third(rng, (rows, E))
        w[:, tr.tile - 1:tr.tile + 1] = 0.75           # the evaluations on both sides of the tile boundary
        net, at = _front(cfg, F)
        m64, count = _model_range(net, cols, w, np.float64)
        m32, count32 = _model_range(net, cols, w, np.float32)
        got, n = _device_range(tr, cols, w)
        xo, g, y, index = tr.inputMap()
        assert index == at and n == count == count32 == int((w > 0).sum())
        e32, a = float(np.abs(m32 - m64).max()), float(np.abs(m64).max())
        bar = 8 * max(e32, 2.0 ** -24 * a)
        worst = float(np.abs(got.astype(np.float64) - m64).max())
        print("%s: %d evaluations of %d contribute; e32 %.3g, a %.3g, device %.3g, ratio %.3g of the bar" % (name, n, rows * E, e32, a, worst, worst / bar))
        assert worst <= bar, "%s: |dev - m64| = %.3g against a bar of %.3g" % (name, worst, bar)
        assert (got[0] <= got[1]).all()


def test_the_range_behind_l2normalize():
    _hold_range("7 bins, l2normalize", cases.small_net(in_fns=("l2normalize", "mapminmax")), 2, lambda tile: tile + 37, 22)


def test_the_range_behind_normalizestd_in_db():
    _hold_range("7 bins, normalizestd, dB", cases.small_net(in_fns=("normalizestd", "mapminmax"), scaling="db"), 2, lambda tile: tile + 37, 23)


def test_the_range_of_the_sample_network():
    _hold_range("sample network", util.sample_net(), 1, lambda tile: tile + 5, 24)


def test_the_range_of_config_3s_geometry_one_evaluation_over_a_tile():
    cfg = nets.config3()
    assert cfg.net.inputs == 1160                      # the form whose workgroup holds more than 64 KB
    _hold_range("1160 inputs", cfg, 1, lambda tile: tile + 1, 25)


def test_a_bank_without_a_mapminmax_input_function_is_unsupported():
    cfg = cases.small_net(in_fns=("l2normalize",))
    with sd.SyllableDetector(cfg, channels=1) as det, det.trainer() as tr:
        cols = torch.ones((1, 12, 7), device="cuda")
        with pytest.raises(sd.SyllableDetectorError) as e:
            tr.inputRange(cols, torch.ones((1, 10), device="cuda"))
        assert e.value.status == _abi.ERR_UNSUPPORTED
        with pytest.raises(sd.SyllableDetectorError) as e:
            tr.setInputMap(np.zeros(21), np.ones(21))
        assert e.value.status == _abi.ERR_UNSUPPORTED


# ---- the range of a packed plan ----
def _packed():
    """3 recordings of noise on 2 rows of the sample network"""
    cfg = util.sample_net()
    audio = [(np.random.default_rng(40 + k).standard_normal(n) * 0.1).astype(np.float32) for k, n in enumerate(LENGTHS)]
    offsets = np.cumsum([0] + [x.size for x in audio])[:-1]
    det = sd.SyllableDetector(cfg, channels=2)
    rec = det.recordings(LENGTHS)
    cols = rec.spectrogram(rec.load(torch.from_numpy(np.concatenate(audio)).cuda(), offsets))
    torch.cuda.synchronize()
    return cfg, det, rec, cols


def test_the_packed_plans_range_is_its_recordings_own_and_what_lies_between_them_never_contributes():
    cfg, det, rec, cols = _packed()
    with det, rec, rec.trainer() as tr:
        slots = rec.slots
        T, E = cfg.timeRange, rec.rowEvaluations
        assert len(slots) == 3 and len({s[0] for s in slots}) == 2 and all(s[3] > 0 for s in slots)
        _, w = tr.targets([np.array([], np.int64)] * 3, 0, 1.0, 0.5)          # every evaluation of a recording 0.5, everything else 0
        host = cols.cpu().numpy()
        mine = np.zeros(host.shape[:2], bool)
        for s in slots:
            mine[s[0], s[2]:s[2] + s[3] + T - 1] = True
        assert (~mine).sum() > 0 and int((w > 0).sum()) == sum(s[3] for s in slots)
        rng, count = tr.inputRange(cols, w)
        junk = np.where((np.arange(host.size) % 2 == 0).reshape(host.shape), np.float32(np.nan), np.float32(np.inf))
        planted = torch.from_numpy(np.where(mine[:, :, None], host, junk).astype(np.float32)).cuda()
        rng2, count2 = tr.inputRange(planted, w)
        torch.cuda.synchronize()
        rng, rng2 = rng.cpu().numpy(), rng2.cpu().numpy()
        assert rng2.tobytes() == rng.tobytes() and int(count2) == int(count)
    lo, hi, total = np.full(290, np.inf, np.float32), np.full(290, -np.inf, np.float32), 0
    with sd.SyllableDetector(cfg, channels=1) as one, one.trainer() as tr1:
        for s in slots:
            own = np.ascontiguousarray(host[s[0], s[2]:s[2] + s[3] + T - 1])[None]
            r, n = _device_range(tr1, own, np.ones((1, s[3]), np.float32))
            lo, hi, total = np.minimum(lo, r[0]), np.maximum(hi, r[1]), total + n
    assert int(count) == total == sum(s[3] for s in slots)
    assert rng.tobytes() == np.stack([lo, hi]).tobytes()


def test_a_new_input_map_is_what_later_calls_use():
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=1) as det, det.trainer() as tr:
        E = 40
        rng = np.random.default_rng(31)
        cols = cases.columns(rng, E + 9, 29, rows=1)
        w = rng.uniform(0.2, 1.0, (1, E)).astype(np.float32)
        t = rng.integers(0, 2, (1, E, 1)).astype(np.float32)
        r, n = _device_range(tr, cols, w)
        xo, g = sd.trainInputMapHost(r)
        was = tr.inputMap()
        assert np.array_equal(was[0], cfg.net.inputProcessing[1].xOffsets) and was[2] == np.float32(cfg.net.inputProcessing[1].y) and was[3] == 1
        theta = torch.from_numpy(cases.theta_of(cfg)).cuda()
        d = [torch.from_numpy(a).cuda() for a in (cols, t, w)]
        before = tr.gradient(d[0], theta, d[1], d[2])[2].cpu().numpy()
        tr.setInputMap(xo, g, -1.0)
        got = tr.inputMap()
        assert got[0].tobytes() == xo.tobytes() and got[1].tobytes() == g.tobytes() and got[2] == -1.0
        loss, wsum, grad = tr.gradient(d[0], theta, d[1], d[2])
        fitted = copy.deepcopy(cfg)
        fitted.net.inputProcessing[1].xOffsets, fitted.net.inputProcessing[1].gains, fitted.net.inputProcessing[1].y = xo, g, -1.0
    # ... the gradient of a bank made with that map, bit for bit; the range does not depend on the map
    with sd.SyllableDetector(fitted, channels=1) as det2, det2.trainer() as tr2:
        loss2, wsum2, grad2 = tr2.gradient(d[0], theta, d[1], d[2])
        assert grad2.cpu().numpy().tobytes() == grad.cpu().numpy().tobytes() != before.tobytes() and float(loss2) == float(loss)
        assert _device_range(tr2, cols, w)[0].tobytes() == r.tobytes()


# ---- the Adam step ----
@pytest.mark.parametrize("which", ["small", "sample"])
def test_the_device_step_is_the_host_steps_bits(which):
    cfg = cases.small_net() if which == "small" else util.sample_net()
    with sd.SyllableDetector(cfg, channels=1) as det, det.trainer() as tr:
        P = tr.paramCount
        assert P == (74 if which == "small" else 1169)
        rng = np.random.default_rng(P)
        p = rng.standard_normal(P).astype(np.float32)
        hp, hm, hv = p.copy(), np.full(P, np.nan, np.float32), np.full(P, np.nan, np.float32)
        dp = torch.from_numpy(p).cuda()
        det.profile(True)
        try:
            for step in (1, 2, 3):
                grad = (rng.standard_normal(P) * 10.0 ** rng.uniform(-5, 0, P)).astype(np.float32)
                loss = np.array([rng.uniform(0.1, 2.0), rng.uniform(0.2, 3.0)])
                mean = tr.adamStep(dp, torch.from_numpy(loss).cuda(), torch.from_numpy(grad).cuda(), step, lr=0.02)
                torch.cuda.synchronize()
                assert util.launched(det) == ["train_adam_kernel"]
                hp, hm, hv, hmean = sd.trainAdamHost(hp, hm, hv, grad, loss, step, lr=0.02)
                assert dp.cpu().numpy().tobytes() == hp.tobytes(), step
                assert float(mean) == hmean == loss[0] / loss[1]
        finally:
            det.profile(False)
        # a weight sum of 0: the parameters keep their bits, the mean loss is 0
        mean = tr.adamStep(dp, torch.tensor([3.0, 0.0], dtype=torch.float64, device="cuda"), torch.from_numpy(grad).cuda(), 4, lr=0.02)
        torch.cuda.synchronize()
        assert dp.cpu().numpy().tobytes() == hp.tobytes() and float(mean) == 0.0
        # refusals leave them alone too
        for bad in (dict(step=0), dict(lr=float("nan")), dict(beta1=1.0), dict(eps=-1.0)):
            kw = dict(step=5)
            kw.update(bad)
            with pytest.raises(sd.SyllableDetectorError) as e:
                tr.adamStep(dp, torch.tensor([3.0, 1.0], dtype=torch.float64, device="cuda"), torch.from_numpy(grad).cuda(), **kw)
            assert e.value.status == _abi.ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert dp.cpu().numpy().tobytes() == hp.tobytes()


# ---- the fit ----
def test_the_fit_is_as_many_gradient_and_step_calls_to_the_bit_and_three_launches_a_step():
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=2) as det, det.trainer() as tr:
        E = tr.tile + 9
        rng = np.random.default_rng(33)
        cols = torch.from_numpy(cases.columns(rng, E + 9, 29, rows=2)).cuda()
        t = torch.from_numpy(rng.integers(0, 2, (2, E, 1)).astype(np.float32)).cuda()
        w = torch.from_numpy(_third(rng, (2, E))).cuda()
        r, _ = tr.inputRange(cols, w)
        tr.setInputMap(*sd.trainInputMapHost(r.cpu().numpy()))
        start = torch.from_numpy(sd.trainInitHost(0, 290, 4, 1)).cuda()
        # five separate calls
        p = start.clone()
        out = (torch.empty(2, dtype=torch.float64, device="cuda"), torch.empty(1169, device="cuda"))
        means = []
        for step in range(1, 6):
            tr.gradient(cols, p, t, w, out=out)
            means.append(tr.adamStep(p, out[0], out[1], step, lr=0.01))
        torch.cuda.synchronize()
        means = np.array([float(m) for m in means])
        det.profile(True, history=5)
        try:
            fitted, history = tr.fitDevice(cols, t, w, start, steps=5, lr=0.01)
            torch.cuda.synchronize()
            names = [k for back in range(4, -1, -1) for k, _ in det.timingsOf(back)]
        finally:
            det.profile(False)
        assert names == ["train_gradient_kernel", "train_combine_kernel", "train_adam_kernel"] * 5
        assert fitted.cpu().numpy().tobytes() == p.cpu().numpy().tobytes() != start.cpu().numpy().tobytes()
        assert history.cpu().numpy().tobytes() == means.tobytes() and (means > 0).all()
        assert start.cpu().numpy().tobytes() == sd.trainInitHost(0, 290, 4, 1).tobytes()
        # steps = 0: the parameters as they were, an empty history
        same, none = tr.fitDevice(cols, t, w, start, steps=0)
        assert same.cpu().numpy().tobytes() == start.cpu().numpy().tobytes() and none.numel() == 0
        # a refused call leaves the parameters as they were
        lib = _abi.lib
        keep = fitted.clone()
        hist = torch.zeros(5, dtype=torch.float64, device="cuda")
        names = (("t", tr._h), ("cols", cols.data_ptr()), ("J", int(cols.shape[1])), ("stride", 0), ("tg", t.data_ptr()), ("w", w.data_ptr()), ("E", E),
                 ("p", fitted.data_ptr()), ("steps", 5), ("lr", 0.01), ("b1", 0.9), ("b2", 0.999), ("eps", 1e-8), ("hist", hist.data_ptr()), ("stream", None))
        call = lambda **kw: lib.syldet_train_fit_device(*[kw.get(k, v) for k, v in names])
        for bad in (dict(E=E + 1), dict(E=-1), dict(steps=-1), dict(lr=float("nan")), dict(b1=1.0), dict(b2=-0.5), dict(eps=float("inf")), dict(p=None), dict(hist=None),
                    dict(cols=None), dict(tg=None), dict(w=None), dict(t=None), dict(stride=1)):
            assert call(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        torch.cuda.synchronize()
        assert fitted.cpu().numpy().tobytes() == keep.cpu().numpy().tobytes() and not hist.cpu().numpy().any()


# ---- the gradient kernel keeps its bits ----
def _gradient_case(cfg, rows, extra, seed):
    with sd.SyllableDetector(cfg, channels=rows) as det, det.trainer() as tr:
        E = tr.tile + extra
        rng = np.random.default_rng(seed)
        cols = cases.columns(rng, E + cfg.timeRange - 1, det.geometry.bins, rows=rows)
        t = rng.integers(0, 2, (rows, E, tr.outputs)).astype(np.float32)
        w = rng.uniform(0.2, 1.0, (rows, E)).astype(np.float32)
        w[:, ::3] = 0
        loss, wsum, grad = tr.gradient(*[torch.from_numpy(a).cuda() for a in (cols, cases.theta_of(cfg), t, w)])
        torch.cuda.synchronize()
        return np.array([float(loss), float(wsum)]), grad.cpu().numpy()


GRADIENT_CASES = {
    "sample": lambda: (util.sample_net(), 3, 40, 1),
    "small_l2": lambda: (cases.small_net(), 2, 37, 2),
    "small_std_db": lambda: (cases.small_net("LogSig", "LogSig", ("normalizestd", "mapstd"), ("mapminmax",), "db", seed=4), 1, 5, 3),
    "small_norm_log": lambda: (cases.small_net("SatLin", "TanSig", ("normalize",), ("mapstd", "mapminmax"), "log", seed=6), 2, 5, 4),
    "small_map_l2": lambda: (cases.small_net("SatLin", "TanSig", ("mapminmax", "l2normalize"), ("mapstd", "mapminmax"), "log", seed=6), 2, 5, 5),
    "wide16": lambda: (cases.sample_wide(16, 4, "SatLin", "PureLin"), 1, 7, 6),
    "wide8": lambda: (cases.sample_wide(8, 2, "TanSig", "PureLin"), 1, 7, 7),
    "config3": lambda: (nets.config3(), 1, 1, 8),
}


@pytest.mark.parametrize("name", sorted(GRADIENT_CASES))
def test_the_gradient_kernel_gives_the_bits_it_gave_before_its_chain_was_shared(name):
    """tests/golden/train_gradient_parent.npz holds loss, weight sum and gradient of these cases as train_gradient_kernel gave them on
    an MI355X while the input chain's statistics and values were written inside it: every instantiation, every kind of input
    function, the three scalings.  Sharing that text with the range kernel must not move a bit."""
    gold = np.load(os.path.join(util.GOLD, "train_gradient_parent.npz"))
    loss, grad = _gradient_case(*GRADIENT_CASES[name]())
    assert loss.tobytes() == gold[name + "_loss"].tobytes() and grad.tobytes() == gold[name + "_grad"].tobytes()
