"""Training a network per channel on the GPU (syldet_trainer_create_multi; include/syldet.h "training a network per channel").

The contract is bit identity: network n's loss, weight sum, gradient, range, count, Adam step and fit history from the multi trainer
are compared, as integer views (bytes), with a PLAIN trainer on a PLAIN bank of that network's configuration over that network's rows
gathered contiguously (r = NULL).  No tolerance anywhere but in (1), where network 0 is ALSO held to the float64 numpy model of
tests/train_ref.py with the bar of tests/test_train_gpu.py -- |g_dev - g64| <= 8 max(r32, 2^-24) A_p, r32 from the same model in
float32, never from the device -- so that correctness does not rest on the plain kernel alone."""
import ctypes

import numpy as np
import pytest
import torch

import train_cases as cases
import train_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
LENGTHS = [5000, 1000, 12001, 3000, 7000]
NETWORKS = [0, 1, 0, 1, 1]


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _bytes(x):
    return np.ascontiguousarray(x.detach().cpu().numpy()).tobytes()


def _weights(rng, shape):
    return rng.uniform(0.2, 1.0, shape).astype(np.float32)


def _rows_of(channel_net, n):
    return [r for r, k in enumerate(channel_net) if k == n]


def _thetas(cfgs):
    return np.stack([cases.theta_of(c) for c in cfgs])


def _plain_gradient(cfg, rows, cols, theta, t, w, prepare=None):
    """a plain trainer on a plain bank of cfg over the gathered rows -> (loss bytes, wsum bytes, gradient bytes)"""
    with sd.SyllableDetector(cfg, channels=len(rows)) as det, det.trainer() as tr:
        if prepare is not None:
            prepare(tr)
        loss, wsum, grad = tr.gradient(*_cuda(cols[rows], theta, t[rows], w[rows]))
        torch.cuda.synchronize()
        return _bytes(loss), _bytes(wsum), _bytes(grad)


def _multi_gradient(mt, cols, thetas, t, w):
    loss, wsum, grad = mt.gradient(*_cuda(cols, thetas, t, w))
    torch.cuda.synchronize()
    return loss, wsum, grad


def _equal_per_network(cfgs, channel_net, got, cols, thetas, t, w):
    loss, wsum, grad = got
    for n, cfg in enumerate(cfgs):
        want = _plain_gradient(cfg, _rows_of(channel_net, n), cols, thetas[n], t, w)
        assert (_bytes(loss[n]), _bytes(wsum[n]), _bytes(grad[n])) == want, "network %d" % n


# ---- (1) interleaved rows ----
def test_1_interleaved_rows_a_ragged_tile_an_unselected_tile_a_nan_weight_and_an_idle_network():
    base = cases.small_net()
    cfgs = [base, nets.perturbed(base, 1), nets.perturbed(base, 2)]
    for other in cfgs[1:]:
        for f, g in zip(other.net.inputProcessing + other.net.outputProcessing, base.net.inputProcessing + base.net.outputProcessing):
            if f.function == "mapminmax":
                assert not np.array_equal(f.xOffsets, g.xOffsets) and not np.array_equal(f.gains, g.gains) and f.y != g.y
    channel_net = [0, 2, 0, 1, 2]
    with sd.SyllableDetector.multi(cfgs, channel_net) as det, det.multiTrainer() as mt:
        tile = mt.tile
        E = 2 * tile + 3
        assert mt.networks == 3 and mt.rowNetwork.tolist() == channel_net and mt.shape == (5, 3, 74, 2)
        assert mt.groups(E).tolist() == [6, 3, 6]
        net = ref.net_of(base, det.geometry.bins)
        rng = np.random.default_rng(21)
        cols = cases.columns(rng, E + net.T - 1, net.F, rows=5)
        t = rng.integers(0, 2, (5, E, 2)).astype(np.float32)
        w = _weights(rng, (5, E))
        w[2, tile:2 * tile] = 0.0                      # one whole tile unselected
        w[0, 5] = np.nan                               # a NaN weight is not selected
        w[3] = 0.0                                     # network 1's only row: nothing selected, whatever its columns hold
        cols[3] = np.nan
        thetas = _thetas(cfgs)
        got = _multi_gradient(mt, cols, thetas, t, w)
    _equal_per_network(cfgs, channel_net, got, cols, thetas, t, w)
    loss, wsum, grad = (x.cpu().numpy() for x in got)
    assert loss[1] == 0.0 and wsum[1] == 0.0 and not grad[1].any() and grad[1].tobytes() == bytes(grad[1].nbytes)
    assert loss[0] > 0 and loss[2] > 0 and grad[0].tobytes() != grad[2].tobytes()
    # network 0 against the float64 model, the bar of tests/test_train_gpu.py
    rows = _rows_of(channel_net, 0)
    L = Ws = 0.0
    g, A = np.zeros(net.P), np.zeros(net.P)
    L32, g32 = np.float32(0), np.zeros(net.P, np.float32)
    for c in rows:
        l, ws, gc, ac = ref.gradient(net, cols[c], thetas[0], t[c], w[c], np.float64)
        L, Ws, g, A = L + l, Ws + ws, g + gc, A + ac
        l32, _, gc32, _ = ref.gradient(net, cols[c], thetas[0], t[c], w[c], np.float32)
        L32, g32 = np.float32(L32 + l32), (g32 + gc32).astype(np.float32)
    nz = A > 0
    r32 = float((np.abs(g32.astype(np.float64) - g)[nz] / A[nz]).max())
    rl32 = abs(float(L32) - L) / L
    ok, ratio = ref.within(grad[0], g, A, r32)
    okl, ratiol = ref.within([loss[0]], [L], [L], rl32)
    print("(1) network 0: r32 %.3g, device %.3g (gradient); r32 %.3g, device %.3g (loss)" % (r32, ratio, rl32, ratiol))
    assert ok, "gradient ratio %.3g against a bar of %.3g" % (ratio, 8 * max(r32, 2.0 ** -24))
    assert okl, "loss ratio %.3g against a bar of %.3g" % (ratiol, 8 * max(rl32, 2.0 ** -24))
    assert abs(wsum[0] - Ws) <= 1e-12 * max(Ws, 1.0) and np.isfinite(grad[0]).all()


# ---- (2) more tiles than groups for one network only ----
def test_2_one_network_has_more_tiles_than_workgroups_and_the_other_has_not():
    base = cases.small_net()
    cfgs = [base, nets.perturbed(base, 3)]
    channel_net = [0, 1, 0]
    with sd.SyllableDetector.multi(cfgs, channel_net) as det, det.multiTrainer() as mt:
        tile, per_row = mt.tile, 600
        E = per_row * tile - 5
        groups = mt.groups(E).tolist()
        bound = groups[0]
        assert groups == [bound, 600] and 600 < bound < 1200          # network 0: 1200 tiles on `bound` workgroups; network 1: a tile each
        net = ref.net_of(base, det.geometry.bins)
        rng = np.random.default_rng(22)
        cols = cases.columns(rng, E + net.T - 1, net.F, rows=3)
        t = rng.integers(0, 2, (3, E, 2)).astype(np.float32)
        w = _weights(rng, (3, E))
        w[:, ::3] = 0.0
        w[0, :100 * tile] = 0.0                        # skipped, then worked
        second = bound - per_row                       # row 2's tile `second` + g is workgroup g's second tile
        w[2, (second + 120) * tile:(second + 151) * tile] = 0.0       # worked, then skipped
        cols[0, :100 * tile] = np.nan
        thetas = _thetas(cfgs)
        got = _multi_gradient(mt, cols, thetas, t, w)
    _equal_per_network(cfgs, channel_net, got, cols, thetas, t, w)
    assert float(got[0][0]) > 0 and float(got[0][1]) > 0


# ---- (3) every instantiation ----
def _instantiation(which):
    if which == "sample":
        return util.sample_net(), (290, 4, 1)
    if which == "eight":
        return cases.sample_wide(8, 1, "TanSig"), (290, 8, 1)
    if which == "sixteen":
        return cases.sample_wide(16, 4, "SatLin", "PureLin"), (290, 16, 4)
    return nets.config3(), (1160, 4, 1)


@pytest.mark.parametrize("which", ["sample", "eight", "sixteen", "config3"])
def test_3_every_instantiation_of_the_multi_kernel(which):
    base, (I, H, O) = _instantiation(which)
    cfgs = [base, nets.perturbed(base, 4)]
    channel_net = [1, 0, 1]
    with sd.SyllableDetector.multi(cfgs, channel_net) as det, det.multiTrainer() as mt:
        assert mt.shape == (3, 2, H * I + H + O * H + O, O)
        E = mt.tile + 1
        assert mt.groups(E).tolist() == [2, 4]
        net = ref.net_of(base, det.geometry.bins)
        assert net.I == I
        rng = np.random.default_rng(23)
        cols = cases.columns(rng, E + net.T - 1, net.F, rows=3)
        t = rng.integers(0, 2, (3, E, O)).astype(np.float32)
        w = _weights(rng, (3, E))
        w[:, ::5] = 0.0
        thetas = _thetas(cfgs)
        got = _multi_gradient(mt, cols, thetas, t, w)
    _equal_per_network(cfgs, channel_net, got, cols, thetas, t, w)
    assert got[2].cpu().numpy().any() and np.isfinite(got[2].cpu().numpy()).all()


# ---- (4) N = 1 ----
def test_4_one_network_on_a_plain_bank_is_the_plain_trainer():
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=2) as det, det.trainer() as tr, det.multiTrainer() as mt:
        assert mt.networks == 1 and mt.rowNetwork.tolist() == [0, 0] and mt.shape == (2, 1, 1169, 1)
        E = tr.tile + 9
        rng = np.random.default_rng(24)
        cols, t, w = _cuda(cases.columns(rng, E + 9, 29, rows=2), rng.integers(0, 2, (2, E, 1)).astype(np.float32), _weights(rng, (2, E)))
        theta = torch.from_numpy(sd.trainInitHost(4, 290, 4, 1)).cuda()
        assert mt.groups(E).tolist() == [4]
        loss, wsum, grad = tr.gradient(cols, theta, t, w)
        mloss, mwsum, mgrad = mt.gradient(cols, theta[None], t, w)
        torch.cuda.synchronize()
        assert (_bytes(mloss[0]), _bytes(mwsum[0]), _bytes(mgrad[0])) == (_bytes(loss), _bytes(wsum), _bytes(grad)) and float(wsum) > 0
        p, history = tr.fitDevice(cols, t, w, theta, steps=3)
        mp, mhistory = mt.fitDevice(cols, t, w, theta[None], steps=3)
        torch.cuda.synchronize()
        assert mhistory.shape == (3, 1) and _bytes(mp[0]) == _bytes(p) != _bytes(theta) and _bytes(mhistory[:, 0]) == _bytes(history)


# ---- (5) the fit ----
def test_5_the_fit_and_the_step_per_network_and_an_idle_network_keeps_its_bits():
    base = util.sample_net()
    cfgs = [base, nets.perturbed(base, 5), nets.perturbed(base, 6)]
    channel_net = [0, 1, 2, 0]
    with sd.SyllableDetector.multi(cfgs, channel_net) as det, det.multiTrainer() as mt:
        E = mt.tile + 9
        rng = np.random.default_rng(25)
        h_cols, h_t, h_w = cases.columns(rng, E + 9, 29, rows=4), rng.integers(0, 2, (4, E, 1)).astype(np.float32), _weights(rng, (4, E))
        h_w[:, ::3] = 0.0
        h_w[2] = 0.0                                   # network 2 has a row and no selected evaluation
        cols, t, w = _cuda(h_cols, h_t, h_w)
        start = np.stack([sd.trainInitHost(n, 290, 4, 1) for n in range(3)])
        rng_dev, count = mt.inputRange(cols, w)
        torch.cuda.synchronize()
        assert count.cpu().tolist()[2] == 0
        maps = [sd.trainInputMapHost(rng_dev[n].cpu().numpy()) for n in range(2)]
        for n in range(2):
            mt.setInputMap(n, *maps[n])
        fitted, history = mt.fitDevice(cols, t, w, torch.from_numpy(start).cuda(), steps=5, lr=0.01)
        torch.cuda.synchronize()
        assert fitted.shape == (3, 1169) and history.shape == (5, 3)
        # the step alone, per network, against the host's text
        out = (torch.empty((3, 2), dtype=torch.float64, device="cuda"), torch.empty((3, 1169), device="cuda"))
        mt.gradient(cols, fitted, t, w, out=out)
        stepped = fitted.clone()
        means = mt.adamStep(stepped, out[0], out[1], 1, lr=0.02)
        torch.cuda.synchronize()
        for n in range(3):
            hp, _, _, hmean = sd.trainAdamHost(fitted[n].cpu().numpy(), np.full(1169, np.nan, np.float32), np.full(1169, np.nan, np.float32),
                                               out[1][n].cpu().numpy(), out[0][n].cpu().numpy(), 1, lr=0.02)
            assert _bytes(stepped[n]) == hp.tobytes() and float(means[n]) == hmean, n
        assert _bytes(stepped[2]) == _bytes(fitted[2]) and float(means[2]) == 0.0
    for n in range(2):
        rows = _rows_of(channel_net, n)
        with sd.SyllableDetector(cfgs[n], channels=len(rows)) as det, det.trainer() as tr:
            tr.setInputMap(*maps[n])
            p, h = tr.fitDevice(cols[rows].contiguous(), t[rows].contiguous(), w[rows].contiguous(), torch.from_numpy(start[n]).cuda(), steps=5, lr=0.01)
            torch.cuda.synchronize()
            assert _bytes(fitted[n]) == _bytes(p) != start[n].tobytes(), n
            assert _bytes(history[:, n]) == _bytes(h) and (h > 0).all(), n
    assert _bytes(fitted[2]) == start[2].tobytes() and not history[:, 2].cpu().numpy().any()


# ---- (6) the range and the map ----
def test_6_the_input_range_per_network_and_a_map_set_for_one_network_alone():
    base = cases.small_net()
    cfgs = [base, nets.perturbed(base, 7)]
    channel_net = [0, 1, 1]
    with sd.SyllableDetector.multi(cfgs, channel_net) as det, det.multiTrainer() as mt:
        E = mt.tile + 40
        rng = np.random.default_rng(26)
        h_cols, h_t, h_w = cases.columns(rng, E + 2, 7, rows=3), rng.integers(0, 2, (3, E, 2)).astype(np.float32), _weights(rng, (3, E))
        h_w[:, ::4] = 0.0
        cols, t, w = _cuda(h_cols, h_t, h_w)
        h_cols[1, 50] = np.inf                         # (the range's columns alone) three evaluations of network 1 are not whole
        cols_r, = _cuda(h_cols)
        thetas = torch.from_numpy(_thetas(cfgs)).cuda()
        r, count = mt.inputRange(cols_r, w)
        before = mt.gradient(cols, thetas, t, w)
        torch.cuda.synchronize()
        before = [(_bytes(before[0][n]), _bytes(before[1][n]), _bytes(before[2][n])) for n in range(2)]
        assert r.shape == (2, 2, 21) and count.shape == (2,)
        for n in range(2):
            xo, g, y, at = mt.inputMap(n)
            f = cfgs[n].net.inputProcessing[1]
            assert at == 1 and xo.tobytes() == np.asarray(f.xOffsets, np.float32).tobytes() and g.tobytes() == np.asarray(f.gains, np.float32).tobytes()
            assert y == np.float32(f.y)
        xo1, g1 = sd.trainInputMapHost(r[1].cpu().numpy())
        mt.setInputMap(1, xo1, g1, -0.75)
        xo, g, y, at = mt.inputMap(1)
        assert xo.tobytes() == xo1.tobytes() and g.tobytes() == g1.tobytes() and y == -0.75 and at == 1
        assert mt.inputMap(0)[0].tobytes() == np.asarray(cfgs[0].net.inputProcessing[1].xOffsets, np.float32).tobytes()
        after = mt.gradient(cols, thetas, t, w)
        torch.cuda.synchronize()
        after = [(_bytes(after[0][n]), _bytes(after[1][n]), _bytes(after[2][n])) for n in range(2)]
        assert after[0] == before[0] and after[1][2] != before[1][2] and after[1][0] != before[1][0]
        made = mt.configsWith(thetas)
        assert len(made) == 2 and np.asarray(made[1].net.inputProcessing[1].xOffsets, np.float32).tobytes() == xo1.tobytes() and made[1].net.inputProcessing[1].y == -0.75
        assert cases.theta_of(made[0]).tobytes() == cases.theta_of(cfgs[0]).tobytes() and mt.params(made).cpu().numpy().tobytes() == _bytes(thetas)
    for n in range(2):
        rows = _rows_of(channel_net, n)
        with sd.SyllableDetector(cfgs[n], channels=len(rows)) as det, det.trainer() as tr:
            pr, pc = tr.inputRange(cols_r[rows].contiguous(), w[rows].contiguous())
            torch.cuda.synchronize()
            assert _bytes(r[n]) == _bytes(pr) and int(count[n]) == int(pc) > 0, n
            if n == 1:
                assert int(pc) == int((h_w[rows] > 0).sum()) - 2       # (frame 50 is in three windows; one of them has weight 0)
                tr.setInputMap(xo1, g1, -0.75)
            loss, wsum, grad = tr.gradient(cols[rows].contiguous(), thetas[n], t[rows].contiguous(), w[rows].contiguous())
            torch.cuda.synchronize()
            assert (_bytes(loss), _bytes(wsum), _bytes(grad)) == after[n], n


# ---- (7) packed recordings ----
def _packed(cfgs, channel_net):
    audio = [(np.random.default_rng(60 + k).standard_normal(n) * 0.1).astype(np.float32) for k, n in enumerate(LENGTHS)]
    offsets = np.cumsum([0] + [x.size for x in audio])[:-1]
    det = sd.SyllableDetector.multi(cfgs, channel_net)
    rec = det.recordings(LENGTHS, networks=NETWORKS)
    cols = rec.spectrogram(rec.load(torch.from_numpy(np.concatenate(audio)).cuda(), offsets))
    torch.cuda.synchronize()
    return det, rec, cols


def test_7_packed_recordings_train_the_network_of_their_row():
    base = util.sample_net()
    cfgs = [base, nets.perturbed(base, 8)]
    channel_net = [1, 0, 1]
    det, rec, cols = _packed(cfgs, channel_net)
    with det, rec, rec.multiTrainer() as mt:
        assert mt.shape == (5, 2, 1169, 1) and mt.rowNetwork.tolist() == channel_net
        slots = rec.slots
        hop, first, T, E = det.geometry.hop, det.geometry.first_index, base.timeRange, rec.rowEvaluations
        assert all(channel_net[s[0]] == NETWORKS[k] for k, s in enumerate(slots)) and slots[1][3] == 0
        rng = np.random.default_rng(27)
        labels = [np.sort(rng.integers(-500, n + 500, 6)) for n in LENGTHS]
        t, w = mt.targets(labels, 2 * hop, 0.5, 1.0 / 64)
        torch.cuda.synchronize()
        want_t, want_w = np.zeros((3, E, 1), np.float32), np.zeros((3, E), np.float32)
        for k, s in enumerate(slots):
            kt, kw = sd.trainTargetsHost(labels[k], s[3], 2 * hop, 0.5, 1.0 / 64, first, hop, 1)
            want_t[s[0], s[2]:s[2] + s[3]], want_w[s[0], s[2]:s[2] + s[3]] = kt, kw
        assert _bytes(t) == want_t.tobytes() and _bytes(w) == want_w.tobytes() and (want_w == 0).any() and (want_w == 0.5).any()
        # NaN and +Inf, alternating, in every frame that belongs to no recording's evaluations
        host = cols.cpu().numpy()
        mine = np.zeros(host.shape[:2], bool)
        for s in slots:
            if s[3] > 0:
                mine[s[0], s[2]:s[2] + s[3] + T - 1] = True
        assert (~mine).sum() > 0
        junk = np.where((np.arange(host.size) % 2 == 0).reshape(host.shape), np.float32(np.nan), np.float32(np.inf))
        planted = np.where(mine[:, :, None], host, junk).astype(np.float32)
        thetas = _thetas(cfgs)
        clean = mt.gradient(cols, torch.from_numpy(thetas).cuda(), t, w)
        got = mt.gradient(torch.from_numpy(planted).cuda(), torch.from_numpy(thetas).cuda(), t, w)
        torch.cuda.synchronize()
        assert [_bytes(x) for x in clean] == [_bytes(x) for x in got] and np.isfinite(got[2].cpu().numpy()).all() and (got[1].cpu().numpy() > 0).all()
    _equal_per_network(cfgs, channel_net, got, planted, thetas, want_t, want_w)


# ---- (8) repeatability and the launch rule ----
def test_8_the_same_arrays_give_the_same_bits_and_a_repeated_call_is_launches_only():
    base = util.sample_net()
    cfgs = [base, nets.perturbed(base, 9)]
    with sd.SyllableDetector.multi(cfgs, [0, 1, 0]) as det, det.multiTrainer() as mt:
        E = mt.tile + 40
        rng = np.random.default_rng(28)
        cols, t, w, other = _cuda(cases.columns(rng, E + 9, 29, rows=3), rng.integers(0, 2, (3, E, 1)).astype(np.float32), _weights(rng, (3, E)),
                                  _weights(rng, (3, E)))
        thetas = torch.from_numpy(_thetas(cfgs)).cuda()
        bits = lambda r: tuple(_bytes(x) for x in r)
        first = bits(mt.gradient(cols, thetas, t, w))
        for _ in range(2):
            assert bits(mt.gradient(cols, thetas, t, w)) == first
        assert bits(mt.gradient(cols, thetas, t, other)) != first and bits(mt.gradient(cols, thetas, t, w)) == first
        det.profile(True)
        try:
            out = (torch.empty((2, 2), dtype=torch.float64, device="cuda"), torch.empty((2, 1169), device="cuda"))
            for _ in range(2):
                mt.gradient(cols, thetas, t, w, out=out)
            torch.cuda.synchronize()
            names = det.lastTimings()
            assert [n for n, _ in names] == ["train_gradient_kernel", "train_combine_kernel"] and all(ms > 0 for _, ms in names)
            labels = [np.array([2000, 9000]), np.array([], np.int64), np.array([5000])]
            for _ in range(2):
                mt.targets(labels, 132, 0.5, 0.5, n_evals=E)
            torch.cuda.synchronize()
            assert util.launched(det) == ["train_targets_kernel"]
        finally:
            det.profile(False)


# ---- (9) the statuses ----
def test_9_every_refusal_leaves_the_results_alone():
    lib = _abi.lib
    base = util.sample_net()
    h = _abi.Handle()
    with sd.SyllableDetector.mixed([base, cases.sample_wide(8, 1, "TanSig")], [0, 1]) as det:
        assert lib.syldet_trainer_create_multi(det._h, None, ctypes.byref(h)) == _abi.ERR_UNSUPPORTED and not h
    three = cases.small_net()
    three.net.layers = [three.net.layers[0], sd.NeuralNetLayer(3, 3, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), "TanSig"), three.net.layers[1]]
    wide = cases.sample_wide(17, 1, "TanSig")
    for bad in (three, wide):
        with sd.SyllableDetector.multi([bad, nets.perturbed(bad, 1)], [0, 1]) as det:
            assert lib.syldet_trainer_create_multi(det._h, None, ctypes.byref(h)) == _abi.ERR_UNSUPPORTED and not h
    cfgs = [base, nets.perturbed(base, 8)]
    det, rec, cols = _packed(cfgs, [1, 0, 1])
    with det, rec, rec.multiTrainer() as mt:
        E, J, P = rec.rowEvaluations, int(cols.shape[1]), 1169
        loss = torch.full((2, 2), SENTINEL, dtype=torch.float64, device="cuda")
        grad = torch.full((2, P), SENTINEL, device="cuda")
        theta = torch.zeros((2, P), device="cuda")
        t, w = torch.zeros((3, E, 1), device="cuda"), torch.ones((3, E), device="cuda")
        names = (("t", mt._h), ("cols", cols.data_ptr()), ("J", J), ("stride", 0), ("theta", theta.data_ptr()), ("tg", t.data_ptr()), ("w", w.data_ptr()),
                 ("E", E), ("loss", loss.data_ptr()), ("grad", grad.data_ptr()), ("stream", None))
        call = lambda **kw: lib.syldet_train_gradient_device(*[kw.get(k, v) for k, v in names])
        for bad in (dict(t=None), dict(cols=None), dict(theta=None), dict(tg=None), dict(w=None), dict(loss=None), dict(grad=None), dict(E=E - 1), dict(E=E + 1),
                    dict(J=J - 1), dict(J=J + 1), dict(E=-1), dict(J=-1), dict(stride=J * 29 - 1)):
            assert call(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        # the range, the step and the fit
        rng_out = torch.full((2, 2, 290), SENTINEL, device="cuda")
        count = torch.full((2,), 77, dtype=torch.int64, device="cuda")
        for bad in (dict(E=E - 1), dict(J=J + 1), dict(cols=None), dict(w=None), dict(rng=None), dict(count=None)):
            kw = dict(cols=cols.data_ptr(), J=J, w=w.data_ptr(), E=E, rng=rng_out.data_ptr(), count=count.data_ptr())
            kw.update(bad)
            assert lib.syldet_train_input_range_device(mt._h, kw["cols"], kw["J"], 0, kw["w"], kw["E"], kw["rng"], kw["count"], None) == _abi.ERR_INVALID_ARGUMENT, bad
        assert lib.syldet_train_adam_device(mt._h, None, loss.data_ptr(), grad.data_ptr(), 1, 0.01, 0.9, 0.999, 1e-8, None, None) == _abi.ERR_INVALID_ARGUMENT
        assert lib.syldet_train_adam_device(mt._h, theta.data_ptr(), loss.data_ptr(), grad.data_ptr(), 0, 0.01, 0.9, 0.999, 1e-8, None, None) == _abi.ERR_INVALID_ARGUMENT
        history = torch.full((2, 2), SENTINEL, dtype=torch.float64, device="cuda")
        for bad in (dict(E=E + 1), dict(J=J - 1), dict(theta=None), dict(history=None), dict(cols=None)):
            kw = dict(cols=cols.data_ptr(), J=J, E=E, theta=theta.data_ptr(), history=history.data_ptr())
            kw.update(bad)
            assert lib.syldet_train_fit_device(mt._h, kw["cols"], kw["J"], 0, t.data_ptr(), w.data_ptr(), kw["E"], kw["theta"], 2, 0.01, 0.9, 0.999, 1e-8,
                                               kw["history"], None) == _abi.ERR_INVALID_ARGUMENT, bad
        # a network outside [0, N)
        x = np.full(290, SENTINEL, np.float32)
        fp = x.ctypes.data_as(_abi.c_float_p)
        kept = mt.inputMap(1)
        for net in (-1, 2, 1 << 20):
            assert lib.syldet_trainer_set_input_map_of(mt._h, net, fp, fp, -1.0) == _abi.ERR_INVALID_ARGUMENT, net
            assert lib.syldet_trainer_input_map_of(mt._h, net, None, fp, fp, None) == _abi.ERR_INVALID_ARGUMENT and (x == SENTINEL).all(), net
        assert lib.syldet_trainer_set_input_map_of(mt._h, 1, None, fp, -1.0) == _abi.ERR_INVALID_ARGUMENT
        assert lib.syldet_trainer_set_input_map_of(mt._h, 1, fp, fp, float("nan")) == _abi.ERR_INVALID_ARGUMENT
        assert mt.inputMap(1)[0].tobytes() == kept[0].tobytes() and mt.inputMap(1)[2] == kept[2]
        groups = np.full(2, 77, np.int32)
        assert lib.syldet_trainer_groups(mt._h, -1, groups.ctypes.data_as(_abi.c_int32_p)) == _abi.ERR_INVALID_ARGUMENT and (groups == 77).all()
        assert lib.syldet_trainer_groups(mt._h, E, None) == _abi.ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert (loss == SENTINEL).all() and (grad == SENTINEL).all() and (rng_out == SENTINEL).all() and (count == 77).all() and (history == SENTINEL).all()
        assert not theta.cpu().numpy().any()
        assert call() == 0
        torch.cuda.synchronize()
        assert not (loss == SENTINEL).any() and not (grad == SENTINEL).any()
