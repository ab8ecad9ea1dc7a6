"""Training on the GPU (syldet_train_targets_device, syldet_train_gradient_device; include/syldet.h "training").

The gradient bar: for every parameter |g_dev - g64| <= 8 max(r32, 2^-24) A_p, where g64 and A_p (the sum of the absolute
per-evaluation contributions) come from the float64 numpy model of tests/train_ref.py and r32 is the worst ratio |g32 - g64| / A_p of
the SAME model run with every array and operation in float32 on the same case -- never anything the device produced.  The margin of
8 is for the device's other summation order, fused multiply-adds, a tanh a few ulp from libm's and the one fp64 -> fp32 rounding of
the combine.  Where A_p is 0 the device's entry is exactly 0.  The loss is held the same way with A = L64.  Each case prints r32 and
the device's worst ratio.  The cases on the sample network use spectrogram columns of planted syllables or of noise and a mapminmax
fitted to them (train_cases.fit_map), as training does: on columns its map was not made for the stock network saturates every tanh
unit, 1 - h^2 cancels in float32 and r32 is 1e-3, a bar that would not notice a dropped evaluation.

The targets are bit identity with the Python-integer model; the packed plan's gradient ignores, bit for bit, NaN and +Inf planted in
every frame that is no recording's; a workgroup that owns several tiles, skips one and works the next adds them up; the same arrays
give the same bits call after call; a repeated call is launches only; every refusal leaves the results alone."""
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
LENGTHS = [5000, 1000, 12001, 3000, 7000]              # (1000 samples: shorter than one evaluation of the sample network)


def _model(net, cols, theta, t, w, orders=("matmul",)):
    """the rows' models added up: (L64, Wsum64, g64, A, r32 of the gradient, r32 of the loss); the float32 sums run row after row.
    orders: the float32 model's first-layer summation orders (train_ref.gradient); r32 is the worst over them"""
    L = Ws = 0.0
    g, A = np.zeros(net.P), np.zeros(net.P)
    for c in range(cols.shape[0]):
        l, ws, gc, ac = ref.gradient(net, cols[c], theta, t[c], w[c], np.float64)
        L, Ws, g, A = L + l, Ws + ws, g + gc, A + ac
    nz = A > 0
    r = rl = 0.0
    for order in orders:
        L32, g32 = np.float32(0), np.zeros(net.P, np.float32)
        for c in range(cols.shape[0]):
            l32, _, gc32, _ = ref.gradient(net, cols[c], theta, t[c], w[c], np.float32, order)
            L32, g32 = np.float32(L32 + l32), (g32 + gc32).astype(np.float32)
        r = max(r, float((np.abs(g32.astype(np.float64) - g)[nz] / A[nz]).max()) if nz.any() else 0.0)
        rl = max(rl, abs(float(L32) - L) / L if L > 0 else 0.0)
    return L, Ws, g, A, r, rl


def _device(tr, cols, theta, t, w):
    loss, wsum, grad = tr.gradient(torch.from_numpy(cols).cuda(), torch.from_numpy(theta).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(w).cuda())
    torch.cuda.synchronize()
    return float(loss.cpu()), float(wsum.cpu()), grad.cpu().numpy()


def _hold(name, dev, want):
    L, Ws, g, A, r, rl = want
    ok, ratio = ref.within(dev[2], g, A, r)
    okl, ratiol = ref.within([dev[0]], [L], [L], rl)
    print("%s: r32 %.3g, device %.3g (gradient); r32 %.3g, device %.3g (loss)" % (name, r, ratio, rl, ratiol))
    assert ok, "%s: gradient ratio %.3g against a bar of %.3g" % (name, ratio, 8 * max(r, 2.0 ** -24))
    assert okl, "%s: loss ratio %.3g against a bar of %.3g" % (name, ratiol, 8 * max(rl, 2.0 ** -24))
    assert abs(dev[1] - Ws) <= 1e-12 * max(Ws, 1.0)    # (fp64 sums of float32 weights, in another order)
    assert np.isfinite(dev[2]).all()


def _weights(rng, shape, every=1):
    w = rng.uniform(0.2, 1.0, shape).astype(np.float32)
    if every > 1:
        w[..., np.arange(shape[-1]) % every != 3] = 0.0
    return w


# ---- the gradient on a bank's channels ----
def _planted_columns(cfg, rows, E, seed):
    """[rows, E + T - 1, bins] float32: the bank's own spectrogram of `rows` channels of noise and planted syllables"""
    with sd.SyllableDetector(cfg, channels=rows) as det:
        n = (E + cfg.timeRange - 2) * det.geometry.hop + cfg.windowLength
        assert det.countEvaluations(n) == E
        x = np.stack([cases.planted_channel(seed + k, n=n, every=6000, jitter=1500)[0] for k in range(rows)])
        cols = det.spectrogram(torch.from_numpy(x).cuda()).cpu().numpy()
    return cols


def test_a_the_sample_network_over_a_tile_boundary_a_ragged_tile_an_empty_row_and_subsampled_negatives():
    base = util.sample_net()
    with sd.SyllableDetector(base, channels=1) as det, det.trainer() as tr:
        tile = tr.tile
    assert tile % 32 == 0 and tile >= 32
    E = 2 * tile + 3
    cols = _planted_columns(base, 3, E, 5)
    cfg = cases.fit_map(base, 29, [cols[0], cols[2]])
    with sd.SyllableDetector(cfg, channels=3) as det, det.trainer() as tr:
        assert tr.shape == (3, 1169, 1) and tr.tile == tile
        net = ref.net_of(cfg, det.geometry.bins)
        rng = np.random.default_rng(1)
        cols[1] = np.nan                               # row 1 is unselected: whatever its columns hold
        theta = cases.theta_of(cfg)
        t = rng.integers(0, 2, (3, E, 1)).astype(np.float32)
        w = np.stack([_weights(rng, (E,)), np.zeros(E, np.float32), _weights(rng, (E,), every=16)])
        w[0, 5] = np.nan                               # a NaN weight is not selected
        want = _model(net, cols, theta, t, w)
        assert want[4] < 1e-4                          # (the units are not saturated: the bar notices one evaluation of 700)
        _hold("(a) sample network, 3 rows of %d" % E, _device(tr, cols, theta, t, w), want)


def test_a2_workgroups_that_own_several_tiles_skip_one_and_work_the_next():
    # More tiles than the kernel takes workgroups (at most 1024, include/syldet.h): workgroup g owns the tiles g and g + 1024 and adds
    # both into its partial.  Row 0's first 100 tiles have no selected evaluation -- their workgroups skip a tile, then work one --
    # and 31 tiles of row 1 that are some workgroup's second have none either: worked, then skipped.
    cfg = cases.small_net()
    with sd.SyllableDetector(cfg, channels=2) as det, det.trainer() as tr:
        tile, per_row = tr.tile, 600
        E = per_row * tile - 5
        assert 1024 < 2 * per_row <= 2048
        net = ref.net_of(cfg, det.geometry.bins)
        rng = np.random.default_rng(11)
        cols = cases.columns(rng, E + net.T - 1, net.F, rows=2)
        t = rng.integers(0, 2, (2, E, 2)).astype(np.float32)
        w = _weights(rng, (2, E))
        w[:, ::3] = 0.0
        w[0, :100 * tile] = 0.0
        second = 1024 - per_row                        # row 1's tile `second` + g is workgroup g's second tile
        w[1, (second + 120) * tile:(second + 151) * tile] = 0.0
        cols[0, :100 * tile] = np.nan                  # (what a skipped tile would have read)
        theta = cases.theta_of(cfg)
        d = [torch.from_numpy(a).cuda() for a in (cols, theta, t, w)]
        first = tr.gradient(*d)
        again = tr.gradient(*d)
        torch.cuda.synchronize()
        dev = (float(first[0]), float(first[1]), first[2].cpu().numpy())
        assert np.float64(again[0].cpu()).tobytes() == np.float64(first[0].cpu()).tobytes() and again[2].cpu().numpy().tobytes() == dev[2].tobytes()
        _hold("(a2) 7 bins, %d tiles of %d on 2 rows" % (2 * per_row, tile), dev, _model(net, np.nan_to_num(cols), theta, t, w))


def test_b_the_small_logsig_network_in_db_with_normalizestd_and_mapstd():
    cfg = cases.small_net("LogSig", "LogSig", ("normalizestd", "mapstd"), ("mapminmax",), "db", seed=4)
    with sd.SyllableDetector(cfg, channels=1) as det, det.trainer() as tr:
        net = ref.net_of(cfg, det.geometry.bins)
        rng = np.random.default_rng(2)
        E = 5
        cols = cases.columns(rng, E + net.T - 1, net.F, rows=1)
        t = rng.integers(0, 2, (1, E, 2)).astype(np.float32)
        w = _weights(rng, (1, E))
        _hold("(b) 7 bins, LogSig, dB, 5 evaluations", _device(tr, cols, cases.theta_of(cfg), t, w), _model(net, cols, cases.theta_of(cfg), t, w))


@pytest.mark.parametrize("chain", [("normalize",), (), ("mapminmax", "l2normalize")], ids=lambda c: "+".join(c) or "none")
def test_b2_the_other_chains_and_transfer_functions(chain):
    cfg = cases.small_net("SatLin" if chain else "TanSig", "TanSig", chain, ("mapstd", "mapminmax"), "log" if chain else "linear", seed=6)
    with sd.SyllableDetector(cfg, channels=2) as det, det.trainer() as tr:
        net = ref.net_of(cfg, det.geometry.bins)
        rng = np.random.default_rng(3)
        E = 40
        cols = cases.columns(rng, E + net.T - 1, net.F, rows=2)
        cols[1, 10:13] = 0.25                          # a window of equal values: normalize's range 0 fills -1
        t = rng.integers(0, 2, (2, E, 2)).astype(np.float32)
        w = _weights(rng, (2, E))
        theta = cases.theta_of(cfg)
        theta[net.H * net.I:net.H * net.I + net.H] += 0.4
        _hold("(b2) 7 bins, %s" % ("+".join(chain) or "no chain"), _device(tr, cols, theta, t, w), _model(net, cols, theta, t, w))


def test_c_sixteen_satlin_hidden_units_and_four_outputs():
    # The first layer is scaled and centred, from the float64 model alone, so that every SatLin unit runs through its linear range
    # (0, 1) in most evaluations.  With the random layer as drawn a unit's sum hardly moves from one evaluation to the next (the
    # mapped inputs sit near -1), so a unit is flat throughout or leaves 0 in a single evaluation by a hair; a parameter's A_p is then
    # one term h = a of 1e-3 whose float32 rounding (1e-7 of a 290-term sum) no fp32 first layer controls, and r32 is one
    # rounding's luck, not a yardstick: the float32 model drew 1.1e-6 there and the device 3.7e-5, as did a CPU emulation of it.
    cfg = cases.sample_wide(16, 4, "SatLin", "PureLin")
    net = ref.net_of(cfg, 29)
    shares = cases.spread_first_layer(cfg, net, cases.columns(np.random.default_rng(4), 600, 29))
    assert shares.min() > 0.5
    with sd.SyllableDetector(cfg, channels=1) as det, det.trainer() as tr:
        assert tr.shape == (1, 290 * 16 + 16 + 64 + 4, 4) and det.geometry.bins == 29
        rng = np.random.default_rng(4)
        E = tr.tile + 7                                # a tile boundary and a ragged tile on the 16-unit form too
        cols = cases.columns(rng, E + net.T - 1, net.F, rows=1)
        t = rng.integers(0, 2, (1, E, 4)).astype(np.float32)
        w = _weights(rng, (1, E))
        theta = cases.theta_of(cfg)
        want = _model(net, cols, theta, t, w)
        _hold("(c) 290 -> 16 SatLin -> 4, %d evaluations" % E, _device(tr, cols, theta, t, w), want)


def test_c2_the_random_satlin_layer_as_drawn_against_float32_in_several_orders():
    # The draw test (c) does not use: the random first layer as it comes.  Its units are flat in most evaluations, and a few
    # parameters are touched by one evaluation whose unit left 0 by 1e-3; their A_p is that one term, and what the bar then measures
    # is the float32 rounding of one cancelled 290-term sum, which differs from one summation order to the next by more than the
    # margin of 8.  So here r32 is the worst of the float32 model with the first layer's products added by numpy's matmul, one after
    # another from input 0, and one after another from input 289 -- three orders that are not the device's (frame by frame, then the
    # frames).  On the CPU they gave 1.1e-6, 1.6e-5 and 4.2e-5 for this case.
    cfg = cases.sample_wide(16, 4, "SatLin", "PureLin")
    with sd.SyllableDetector(cfg, channels=1) as det, det.trainer() as tr:
        net = ref.net_of(cfg, det.geometry.bins)
        rng = np.random.default_rng(4)
        E = tr.tile + 7
        cols = cases.columns(rng, E + net.T - 1, net.F, rows=1)
        t = rng.integers(0, 2, (1, E, 4)).astype(np.float32)
        w = _weights(rng, (1, E))
        theta = cases.theta_of(cfg)
        want = _model(net, cols, theta, t, w, orders=("matmul", "forward", "reverse"))
        _hold("(c2) 290 -> 16 SatLin -> 4 as drawn, %d evaluations, three float32 orders" % E, _device(tr, cols, theta, t, w), want)


def test_d_config_3s_geometry_one_evaluation_over_a_tile():
    cfg = nets.config3()
    with sd.SyllableDetector(cfg, channels=1) as det, det.trainer() as tr:
        assert det.geometry.bins == 116 and tr.shape == (1, 1160 * 4 + 4 + 4 + 1, 1)
        E = tr.tile + 1
        net = ref.net_of(cfg, det.geometry.bins)
        rng = np.random.default_rng(5)
        cols = cases.columns(rng, E + net.T - 1, net.F, rows=1)
        t = rng.integers(0, 2, (1, E, 1)).astype(np.float32)
        w = _weights(rng, (1, E))
        _hold("(d) 1160 -> 4 -> 1, %d evaluations" % E, _device(tr, cols, cases.theta_of(cfg), t, w), _model(net, cols, cases.theta_of(cfg), t, w))


def test_e_too_few_samples_for_one_evaluation_give_exact_zeros():
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=1) as det, det.trainer() as tr:
        assert det.countEvaluations(1443) == 0
        cols = det.spectrogram(torch.zeros((1, 1443), device="cuda"))
        theta = torch.from_numpy(cases.theta_of(cfg)).cuda()
        out = (torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda"), torch.full((1169,), SENTINEL, device="cuda"))
        t, w = tr.targets([[700]], 132, 1.0, 1.0, n_evals=0)
        assert t.shape == (1, 0, 1) and w.shape == (1, 0)
        loss, wsum, grad = tr.gradient(cols, theta, t, w, out=out)
        torch.cuda.synchronize()
        assert float(loss) == 0.0 and float(wsum) == 0.0 and not grad.cpu().numpy().any()
        # ... and so does a row without a selected evaluation
        cols = torch.from_numpy(cases.columns(np.random.default_rng(0), 30, 29, rows=1)).cuda()
        out[0].fill_(SENTINEL), out[1].fill_(SENTINEL)
        loss, wsum, grad = tr.gradient(cols, theta, torch.ones((1, 21, 1), device="cuda"), torch.zeros((1, 21), device="cuda"), out=out)
        torch.cuda.synchronize()
        assert float(loss) == 0.0 and float(wsum) == 0.0 and not grad.cpu().numpy().any()


# ---- the targets ----
def test_the_targets_of_a_banks_channels_are_the_integer_model():
    cfg = cases.small_net(out_fns=())
    with sd.SyllableDetector(cfg, channels=3) as det, det.trainer() as tr:
        hop, first, E = det.geometry.hop, det.geometry.first_index, 300
        rng = np.random.default_rng(7)
        labels = [np.sort(rng.integers(-2000, first + E * hop + 2000, n)) for n in (12, 0, 30)]
        labels[0][1] = labels[0][0]
        labels[2][15] = labels[2][14]                  # two labels of different outputs at one sample, inside the detector
        outs = [rng.integers(0, 2, l.size).astype(np.int32) for l in labels]
        outs[2][14:16] = (0, 1)
        assert first < labels[2][14] < first + (E - 1) * hop
        for hw, lo in ((0, None), (hop, outs), (5 * hop, outs)):
            t, w = tr.targets(labels, hw, 0.5 / 7, 0.125, labelOutputs=lo, n_evals=E)
            torch.cuda.synchronize()
            for c in range(3):
                want_t, want_w = ref.targets(labels[c], None if lo is None else lo[c], E, hw, 0.5 / 7, 0.125, first, hop, 2)
                assert t[c].cpu().numpy().tobytes() == want_t.tobytes() and w[c].cpu().numpy().tobytes() == want_w.tobytes(), (hw, c)
            if lo is not None:
                assert (t.sum(dim=2) > 1).any() and (w == 0.125).any()


def _packed():
    """5 recordings of noise on 2 rows of the sample network, its mapminmax fitted to the recordings' own columns"""
    base = util.sample_net()
    audio = [(np.random.default_rng(40 + k).standard_normal(n) * 0.1).astype(np.float32) for k, n in enumerate(LENGTHS)]
    offsets = np.cumsum([0] + [x.size for x in audio])[:-1]

    def load(cfg):
        det = sd.SyllableDetector(cfg, channels=2)
        rec = det.recordings(LENGTHS)
        cols = rec.spectrogram(rec.load(torch.from_numpy(np.concatenate(audio)).cuda(), offsets))
        torch.cuda.synchronize()
        return det, rec, cols

    det, rec, cols = load(base)
    own = [rec.columnsView(cols, k).cpu().numpy() for k in range(len(LENGTHS))]
    rec.close()
    det.close()
    cfg = cases.fit_map(base, 29, own)
    return (cfg,) + load(cfg)


def test_the_packed_plans_targets_and_gradient_and_what_lies_between_recordings():
    cfg, det, rec, cols = _packed()
    with det, rec, rec.trainer() as tr:
        assert tr.shape == (5, 1169, 1)
        slots = rec.slots
        hop, first, T, E = det.geometry.hop, det.geometry.first_index, cfg.timeRange, rec.rowEvaluations
        assert [s[3] for s in slots][1] == 0 and len({s[0] for s in slots}) == 2
        rng = np.random.default_rng(8)
        labels = [np.sort(rng.integers(-500, n + 500, 6)) for n in LENGTHS]
        t, w = tr.targets(labels, 2 * hop, 0.5, 1.0 / 64)
        torch.cuda.synchronize()
        want_t, want_w = ref.packed_targets(slots, 2, E, labels, None, 2 * hop, 0.5, 1.0 / 64, first, hop, 1)
        assert t.cpu().numpy().tobytes() == want_t.tobytes() and w.cpu().numpy().tobytes() == want_w.tobytes()
        assert (want_w == 0).any() and (want_w == 0.5).any()            # the zeros between and behind the recordings are part of it
        # the gradient over the recordings' own evaluations
        net = ref.net_of(cfg, det.geometry.bins)
        theta = cases.theta_of(cfg)
        host = cols.cpu().numpy()
        own = [(k, s) for k, s in enumerate(slots) if s[3] > 0]
        kc = np.stack([np.pad(host[s[0], s[2]:s[2] + s[3] + T - 1], ((0, E - s[3]), (0, 0))) for _, s in own])
        kt = np.stack([np.pad(want_t[s[0], s[2]:s[2] + s[3]], ((0, E - s[3]), (0, 0))) for _, s in own])
        kw = np.stack([np.pad(want_w[s[0], s[2]:s[2] + s[3]], (0, E - s[3])) for _, s in own])
        d_theta = torch.from_numpy(theta).cuda()
        loss, wsum, grad = tr.gradient(cols, d_theta, t, w)
        torch.cuda.synchronize()
        dev = (float(loss), float(wsum), grad.cpu().numpy())
        _hold("packed plan, 5 recordings on 2 rows", dev, _model(net, kc, theta, kt, kw))
        # NaN and +Inf, alternating, in every frame that belongs to no recording's evaluations
        mine = np.zeros(host.shape[:2], bool)
        for _, s in own:
            mine[s[0], s[2]:s[2] + s[3] + T - 1] = True
        assert (~mine).sum() > 0
        junk = np.where((np.arange(host.size) % 2 == 0).reshape(host.shape), np.float32(np.nan), np.float32(np.inf))
        planted = torch.from_numpy(np.where(mine[:, :, None], host, junk).astype(np.float32)).cuda()
        loss2, wsum2, grad2 = tr.gradient(planted, d_theta, t, w)
        torch.cuda.synchronize()
        assert np.float64(loss2.cpu()).tobytes() == np.float64(loss.cpu()).tobytes() and float(wsum2) == float(wsum)
        assert grad2.cpu().numpy().tobytes() == grad.cpu().numpy().tobytes()


# ---- the launch rule ----
def test_the_same_arrays_give_the_same_bits_and_a_repeated_call_is_launches_only():
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=3) as det, det.trainer() as tr:
        E = tr.tile + 40
        rng = np.random.default_rng(9)
        cols = torch.from_numpy(cases.columns(rng, E + 9, 29, rows=3)).cuda()
        theta = torch.from_numpy(cases.theta_of(cfg)).cuda()
        t = torch.from_numpy(rng.integers(0, 2, (3, E, 1)).astype(np.float32)).cuda()
        w = torch.from_numpy(_weights(rng, (3, E))).cuda()
        other = torch.from_numpy(_weights(rng, (3, E), every=4)).cuda()
        bits = lambda r: (np.float64(r[0].cpu()).tobytes(), np.float64(r[1].cpu()).tobytes(), r[2].cpu().numpy().tobytes())
        first = bits(tr.gradient(cols, theta, t, w))
        for _ in range(2):
            assert bits(tr.gradient(cols, theta, t, w)) == first
        between = bits(tr.gradient(cols, theta, t, other))
        assert between != first and bits(tr.gradient(cols, theta, t, w)) == first
        det.profile(True)
        try:
            out = (torch.empty(2, dtype=torch.float64, device="cuda"), torch.empty(1169, device="cuda"))
            for _ in range(2):
                tr.gradient(cols, theta, t, w, out=out)
            torch.cuda.synchronize()
            names = det.lastTimings()
            assert [n for n, _ in names] == ["train_gradient_kernel", "train_combine_kernel"] and all(ms > 0 for _, ms in names)
            labels = [np.array([2000, 9000]), np.array([], np.int64), np.array([5000])]
            for _ in range(2):
                tr.targets(labels, 132, 0.5, 0.5, n_evals=E)
            torch.cuda.synchronize()
            assert util.launched(det) == ["train_targets_kernel"]
        finally:
            det.profile(False)


# ---- the statuses ----
def test_every_refusal_leaves_the_results_alone():
    lib = _abi.lib
    cfg = util.sample_net()
    h = _abi.Handle()
    # creation: anything outside the first version's limits
    three = cases.small_net()
    three.net.layers = [three.net.layers[0], sd.NeuralNetLayer(3, 3, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), "TanSig"), three.net.layers[1]]
    for bad in (three, cases.sample_wide(17, 1, "TanSig"), cases.sample_wide(4, 5, "TanSig")):
        with sd.SyllableDetector(bad, channels=1) as det:
            assert lib.syldet_trainer_create(det._h, None, ctypes.byref(h)) == _abi.ERR_UNSUPPORTED and not h
    with sd.SyllableDetector.multi([cfg, nets.perturbed(cfg, 1)], [0, 1]) as det:
        assert lib.syldet_trainer_create(det._h, None, ctypes.byref(h)) == _abi.ERR_UNSUPPORTED and not h
    with sd.SyllableDetector.mixed([cfg, cases.sample_wide(8, 1, "TanSig")], [0, 1]) as det:
        assert lib.syldet_trainer_create(det._h, None, ctypes.byref(h)) == _abi.ERR_UNSUPPORTED and not h
    cfg_d, det, rec, cols = _packed()
    with det, rec, rec.trainer() as tr, det.trainer() as plain:
        E, J, P = rec.rowEvaluations, int(cols.shape[1]), 1169
        loss = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda")
        grad = torch.full((P,), SENTINEL, device="cuda")
        theta = torch.zeros(P, device="cuda")
        t, w = torch.zeros((2, E, 1), device="cuda"), torch.ones((2, E), device="cuda")
        names = (("t", tr._h), ("cols", cols.data_ptr()), ("J", J), ("stride", 0), ("theta", theta.data_ptr()), ("tg", t.data_ptr()), ("w", w.data_ptr()),
                 ("E", E), ("loss", loss.data_ptr()), ("grad", grad.data_ptr()), ("stream", None))
        call = lambda **kw: lib.syldet_train_gradient_device(*[kw.get(k, v) for k, v in names])
        for bad in (dict(t=None), dict(cols=None), dict(theta=None), dict(tg=None), dict(w=None), dict(loss=None), dict(grad=None), dict(E=E - 1), dict(E=E + 1),
                    dict(J=J - 1), dict(J=J + 1), dict(E=-1), dict(J=-1), dict(stride=J * 29 - 1), dict(stride=1),
                    dict(t=plain._h, E=J - 8), dict(t=plain._h, E=J), dict(t=plain._h, E=10, J=18)):
            assert call(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        torch.cuda.synchronize()
        assert (loss == SENTINEL).all() and (grad == SENTINEL).all()
        # the targets
        labels = np.array([10, 20, 30, 40, 50, 60], np.int64)
        begin = np.array([0, 1, 2, 3, 4, 6], np.int64)
        outs = np.zeros(6, np.int32)
        dt = torch.full((2, E, 1), SENTINEL, device="cuda")
        dw = torch.full((2, E), SENTINEL, device="cuda")
        p64 = lambda a: a.ctypes.data_as(_abi.c_int64_p)
        names = (("t", tr._h), ("labels", p64(labels)), ("begin", p64(begin)), ("outs", outs.ctypes.data_as(_abi.c_int32_p)), ("hw", 132), ("wp", 0.5),
                 ("wn", 0.25), ("E", E), ("dt", dt.data_ptr()), ("dw", dw.data_ptr()), ("stream", None))
        call = lambda **kw: lib.syldet_train_targets_device(*[kw.get(k, v) for k, v in names])
        bad0, down, unsorted, out_of = begin.copy(), begin.copy(), labels.copy(), outs.copy()
        bad0[0] = 1
        down[3] = 1
        unsorted[5] = 45
        out_of[2] = 1
        for bad in (dict(t=None), dict(labels=None), dict(begin=None), dict(dt=None), dict(dw=None), dict(begin=p64(bad0)), dict(begin=p64(down)),
                    dict(labels=p64(unsorted)), dict(outs=out_of.ctypes.data_as(_abi.c_int32_p)), dict(hw=-1), dict(wp=float("nan")), dict(wn=float("nan")),
                    dict(wp=-1.0), dict(wn=-0.25), dict(E=E - 1), dict(E=-1)):
            assert call(**bad) == _abi.ERR_INVALID_ARGUMENT, bad
        torch.cuda.synchronize()
        assert (dt == SENTINEL).all() and (dw == SENTINEL).all()
        assert call() == 0 and call(outs=None) == 0
        torch.cuda.synchronize()
        assert not (dt == SENTINEL).any() and not (dw == SENTINEL).any()
