"""The level meters on the device (syldet_levels*, syldet_output_levels*, the streaming getters; kernels_levels.hip).  Every
comparison with tests/levels_ref.py is EXACT: the fp64 mean squares as uint64, the fp32 output readings as uint32 (NaN at the
same places); the RMS after the host's sqrt."""
import threading

import numpy as np
import pytest

import levels_ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

pytestmark = pytest.mark.gpu

S_BIG = 200003             # several workgroups a row, a short last buffer, a short last reading
LENGTHS = [8, 32, 4096]
PERIODS = [1, 5, 137, 10 ** 6]


def _torch():
    import torch
    return torch


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.view(np.uint64 if got.dtype == np.float64 else np.uint32), want.view(np.uint64 if got.dtype == np.float64 else np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%d differences, first at %s: %r != %r" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def _clock(cfg):
    return (cfg.windowLength, cfg.windowOverlap, cfg.timeRange)


def _rows(S, L, P, seed=0):
    """three channels: noise at 1e-4, full scale, and one with planted values (which depend on where the readings lie)"""
    rng = np.random.default_rng(1000 + seed)
    x = np.stack([rng.standard_normal(S) * 1e-4, rng.uniform(-1, 1, S), rng.standard_normal(S) * 0.05]).astype(np.float32)
    B = -(-S // L)
    Pe = max(1, min(P, B))
    M = -(-B // Pe)
    info = {"M": M, "sticks": None, "ignored": None}
    p = x[2]
    if S > 40:
        r1 = min(2, M - 1)
        p[min(r1 * Pe * L + 3, S - 1)] = np.nan                         # in the first buffer of reading r1: it sticks
        info["sticks"] = r1
        r2 = r1 + 2
        if Pe >= 2 and r2 < M and r2 * Pe * L + L + 1 < S:
            p[r2 * Pe * L + L + 1] = np.nan                             # in the second buffer of reading r2: ignored
            info["ignored"] = r2
        p[S // 2] = np.inf
        p[S // 3: S // 3 + min(3 * L, S // 8)] = 0.0                    # a stretch of zeros
    return x, info


_reference = {}


def _want_in(x, L, P, key=None):
    """the reference readings of rows x, computed once per key"""
    if key is not None and key in _reference:
        return _reference[key]
    want = np.stack([levels_ref.input_readings(row, L, P) for row in x]) if x.shape[1] else np.zeros((x.shape[0], 0))
    if key is not None:
        want.setflags(write=False)
        _reference[key] = want
    return want


@pytest.fixture(scope="module")
def det3():
    with sd.SyllableDetector(util.sample_net(), channels=3) as det:
        yield det


@pytest.mark.parametrize("P", PERIODS)
@pytest.mark.parametrize("L", LENGTHS)
def test_input_readings_bit_for_bit(det3, L, P):
    torch = _torch()
    x, info = _rows(S_BIG, L, P)
    want = _want_in(x, L, P, ("big", L, P))
    got = det3.levels(torch.from_numpy(x).cuda(), L, P)
    torch.cuda.synchronize()
    assert got.shape == (3, info["M"]) and got.dtype == torch.float64
    _same_bits(got.cpu().numpy(), want)
    assert np.isnan(want[2, info["sticks"]]) and not np.isnan(want[:2]).any()
    if info["ignored"] is not None:
        assert not np.isnan(want[2, info["ignored"]])
    assert np.isinf(want[2]).any() or np.isnan(want[2]).all()
    # the host form returns the RMS: the same readings after the host's sqrt
    with np.errstate(invalid="ignore"):
        _same_bits(det3.levelsHost(x, L, P), np.sqrt(want))


@pytest.mark.parametrize("S", [0, 5, 8, 33])
@pytest.mark.parametrize("L", LENGTHS)
def test_input_readings_of_short_rows(det3, L, S):
    torch = _torch()
    for P in (1, 3, 10 ** 6):
        x, info = _rows(S, L, P, seed=S)
        got = det3.levels(torch.from_numpy(x).cuda() if S else torch.zeros((3, 0), device="cuda"), L, P)
        torch.cuda.synchronize()
        assert got.shape == (3, levels_ref.levels_count(S, L, P))
        _same_bits(got.cpu().numpy(), _want_in(x, L, P))
        _same_bits(det3.levelsHost(x, L, P), np.sqrt(_want_in(x, L, P)))


@pytest.mark.parametrize("L,P", [(8, 5), (32, 137), (4096, 1), (32, 10 ** 6)])
def test_layouts_give_the_same_bits(det3, L, P):
    """the same rows with the base one element past a 16-byte line, and with an odd stride (rows on every alignment)"""
    torch = _torch()
    x, _ = _rows(S_BIG, L, P)
    want = _want_in(x, L, P, ("big", L, P))
    for lead, stride in [(1, S_BIG + 5), (0, S_BIG + 4), (3, S_BIG + 1)]:
        flat = torch.full((lead + 3 * stride + 8,), 1e30, device="cuda")          # (what lies between the rows must not be read)
        rows = flat[lead:lead + 3 * stride].view(3, stride)[:, :S_BIG]
        rows.copy_(torch.from_numpy(x))
        assert rows.data_ptr() % 16 == 4 * lead
        got = det3.levels(rows, L, P)
        torch.cuda.synchronize()
        _same_bits(got.cpu().numpy(), want)


@pytest.mark.parametrize("L,P", [(8, 1), (8, 137), (32, 137), (4096, 5), (1024, 10 ** 6)])
def test_s16_is_the_fp32_form_on_the_converted_samples(det3, L, P):
    torch = _torch()
    S = 70001
    rng = np.random.default_rng(16)
    q = rng.integers(-32768, 32768, (3, S)).astype(np.int16)
    q[0, :5] = [32767, -32767, -32768, 0, 1]
    q[1, -3:] = [-32768, 32767, -32768]
    q[2] //= 300                                                                  # a quiet row
    f = (q.astype(np.float32) * np.float32(2.0 ** -15))
    want = _want_in(f, L, P)
    ref = det3.levels(torch.from_numpy(f).cuda(), L, P)
    got = det3.levelsPCM16(torch.from_numpy(q).cuda(), L, P)                      # aligned rows? S is odd: rows 1, 2 are not
    flat = torch.zeros((3 * (S + 7),), dtype=torch.int16, device="cuda")
    rows = flat.view(3, S + 7)[:, :S]                                             # stride 70008: every row on a 16-byte line
    rows.copy_(torch.from_numpy(q))
    assert all((rows.data_ptr() + 2 * c * (S + 7)) % 16 == 0 for c in range(3))
    got_aligned = det3.levelsPCM16(rows, L, P)
    odd = torch.zeros((1 + 3 * (S + 2),), dtype=torch.int16, device="cuda")[1:].view(3, S + 2)[:, :S]
    odd.copy_(torch.from_numpy(q))
    got_odd = det3.levelsPCM16(odd, L, P)
    torch.cuda.synchronize()
    _same_bits(ref.cpu().numpy(), want)
    for g in (got, got_aligned, got_odd):
        _same_bits(g.cpu().numpy(), want)
    _same_bits(det3.levelsPCM16Host(q, L, P), np.sqrt(want))


@pytest.mark.parametrize("n", [0, 5, 4099, 70001])
def test_interleaved_is_the_planar_call_on_the_transposed_data(det3, n):
    torch = _torch()
    rng = np.random.default_rng(n)
    q = rng.integers(-32768, 32768, (n, 3)).astype(np.int16)
    f = (rng.standard_normal((n, 3)) * 0.1).astype(np.float32)
    def planar(a):                                                                # (an empty array has no row stride to speak of)
        return torch.from_numpy(np.ascontiguousarray(a.T)).cuda() if n else torch.zeros((3, 0), dtype=torch.from_numpy(a).dtype, device="cuda")

    for L, P in [(32, 137), (8, 3), (4096, 1)]:
        a = det3.levelsInterleaved(torch.from_numpy(f).cuda(), L, P)
        b = det3.levels(planar(f), L, P)
        c = det3.levelsInterleavedPCM16(torch.from_numpy(q).cuda(), L, P)
        d = det3.levelsPCM16(planar(q), L, P)
        torch.cuda.synchronize()
        _same_bits(a.cpu().numpy(), b.cpu().numpy())
        _same_bits(c.cpu().numpy(), d.cpu().numpy())
        _same_bits(a.cpu().numpy(), _want_in(np.ascontiguousarray(f.T), L, P))
        _same_bits(c.cpu().numpy(), _want_in(np.ascontiguousarray(q.T).astype(np.float32) * np.float32(2.0 ** -15), L, P))


def _plant_outputs(out, det, S, L, P, k):
    """NaN first in a range, NaN later in a range, +Inf and -Inf (and -0 in front of +0), at places the readings decide"""
    E = out.shape[1]
    ranges = [det.levelsEvalRange(S, E, m, L, P) for m in range(det.levelsCount(S, L, P))]
    big = [m for m, (_, n) in enumerate(ranges) if n >= 3]
    facts = {}
    if len(big) >= 1:
        out[0, ranges[big[0]][0], k] = np.nan                                     # first of its range: it sticks
        facts["sticks"] = (0, big[0])
    if len(big) >= 2:
        out[0, ranges[big[1]][0] + 1, k] = np.nan                                 # later in its range: ignored
        facts["ignored"] = (0, big[1])
    if len(big) >= 3:
        f = ranges[big[2]][0]
        out[1, f:f + ranges[big[2]][1], k] = -1.0
        out[1, f, k], out[1, f + 1, k] = -0.0, 0.0                                # the first of equal greatest values stays
        facts["minus_zero"] = (1, big[2])
    if E > 10:
        out[1, E // 2, k] = np.inf
        out[-1, E // 3, k] = -np.inf
        out[-1, E // 3 + 1, k] = np.nan
    return ranges, facts


def _check_outputs(det, cfg, out, S, L, P, k, n_evals=None):
    torch = _torch()
    E = out.shape[1] if n_evals is None else n_evals
    o = np.ascontiguousarray(out[:, :E])
    got = det.outputLevels(torch.from_numpy(o).cuda(), S, k, L, P)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    M = levels_ref.levels_count(S, L, P)
    ref_ranges = levels_ref.eval_ranges(S, E, L, P, _clock(cfg))
    assert [det.levelsEvalRange(S, E, m, L, P) for m in range(M)] == ref_ranges
    assert ref_ranges[0][0] == 0 and sum(n for _, n in ref_ranges) == E                       # they tile [0, n_evals)
    assert all(ref_ranges[m][0] + ref_ranges[m][1] == ref_ranges[m + 1][0] for m in range(M - 1))
    for c in range(out.shape[0]):
        want, empty = levels_ref.output_readings(o[c], k, S, L, P, _clock(cfg))
        _same_bits(got[c], want)
        assert list(empty) == [n == 0 for _, n in ref_ranges]
        assert not got[c][empty].any()                                            # the table's ?? 0.0
    _same_bits(det.outputLevelsHost(o, S, k, L, P), got)
    return got, ref_ranges


@pytest.mark.parametrize("L,P", [(32, 137), (8, 1), (8, 137), (4096, 5), (32, 10 ** 6), (64, 7)])
def test_output_readings_bit_for_bit(det3, L, P):
    torch = _torch()
    cfg = util.sample_net()
    x, _ = _rows(S_BIG, 32, 137)
    x[2] = np.nan_to_num(x[2], nan=0.0, posinf=0.0)
    out, _ = det3.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy().copy()
    assert 1400 < out.shape[1] < 1600
    ranges, facts = _plant_outputs(out, det3, S_BIG, L, P, 0)
    got, ref_ranges = _check_outputs(det3, cfg, out, S_BIG, L, P, 0)
    if "sticks" in facts:
        assert np.isnan(got[facts["sticks"]])
    if "ignored" in facts:
        assert not np.isnan(got[facts["ignored"]])
    if "minus_zero" in facts:
        assert got[facts["minus_zero"]] == 0 and np.signbit(got[facts["minus_zero"]])
    if P * L < det3.geometry.first_index:
        assert ref_ranges[0][1] == 0 and not got[:, 0].any()                      # the readings in front of the first evaluation
    # fewer evaluations than the clock's: the ranges are cut
    _check_outputs(det3, cfg, out, S_BIG, L, P, 0, n_evals=out.shape[1] // 2)
    _check_outputs(det3, cfg, out, S_BIG, L, P, 0, n_evals=0)


def test_output_readings_of_the_last_output_of_a_multi_output_golden_network():
    torch = _torch()
    names = [n for n in util.case_names() if len(util.load_case(n)[0].thresholds) > 1]
    assert names, "no golden case with more than one output"
    cfg, xg, _ = util.load_case(names[0])
    k = len(cfg.thresholds) - 1
    S = min(len(xg), 60001)
    x = np.stack([xg[:S], xg[:S][::-1]]).astype(np.float32)
    with sd.SyllableDetector(cfg, channels=2) as det:
        out, _ = det.run(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        out = out.cpu().numpy().copy()
        assert out.shape[2] == k + 1 and out.shape[1] > 50
        for L, P in [(32, 20), (256, 3)]:
            o = out.copy()
            _plant_outputs(o, det, S, L, P, k)
            got, _ = _check_outputs(det, cfg, o, S, L, P, k)
            other, _ = _check_outputs(det, cfg, o, S, L, P, 0)
            assert not np.array_equal(got.view(np.uint32), other.view(np.uint32))
        lib, bad = _abi.lib, _abi.ERR_INVALID_ARGUMENT
        d = torch.from_numpy(out).cuda()
        lv = torch.full((2, 100), 7.0, device="cuda")
        for kk in (-1, k + 1):
            assert lib.syldet_output_levels_device(det._h, d.data_ptr(), out.shape[1], kk, S, 32, 20, lv.data_ptr(), None) == bad
        torch.cuda.synchronize()
        assert (lv == 7.0).all()


def test_argument_statuses_with_a_live_handle(det3):
    torch = _torch()
    lib, bad = _abi.lib, _abi.ERR_INVALID_ARGUMENT
    x = torch.zeros((3, 4000), device="cuda")
    q = torch.zeros((3, 4000), dtype=torch.int16, device="cuda")
    ms = torch.full((3, 500), 7.0, dtype=torch.float64, device="cuda")
    h = det3._h
    for L in (0, 4, 12, 8192):
        assert lib.syldet_levels_device(h, x.data_ptr(), 4000, 4000, L, 1, ms.data_ptr(), None) == bad
        assert lib.syldet_levels_device_s16(h, q.data_ptr(), 4000, 4000, L, 1, ms.data_ptr(), None) == bad
        assert lib.syldet_levels_interleaved_device(h, x.data_ptr(), 4000, 3, L, 1, ms.data_ptr(), None) == bad
        assert lib.syldet_output_levels_device(h, x.data_ptr(), 10, 0, 4000, L, 1, ms.data_ptr(), None) == bad
    assert "power of two" in _abi.last_error()
    assert lib.syldet_levels_device(h, x.data_ptr(), 4000, 4000, 32, 0, ms.data_ptr(), None) == bad
    assert lib.syldet_levels_device(h, x.data_ptr(), -1, 4000, 32, 1, ms.data_ptr(), None) == bad
    assert lib.syldet_levels_device(h, x.data_ptr(), 4000, 3999, 32, 1, ms.data_ptr(), None) == bad
    assert lib.syldet_levels_device(h, None, 4000, 4000, 32, 1, ms.data_ptr(), None) == bad
    assert lib.syldet_levels_device(h, x.data_ptr(), 4000, 4000, 32, 1, None, None) == bad
    assert lib.syldet_levels_interleaved_device(h, x.data_ptr(), 4000, 2, 32, 1, ms.data_ptr(), None) == bad     # run_interleaved's rule
    assert lib.syldet_levels_interleaved_device_s16(h, q.data_ptr(), -1, 3, 32, 1, ms.data_ptr(), None) == bad
    assert lib.syldet_output_levels_device(h, x.data_ptr(), -1, 0, 4000, 32, 1, ms.data_ptr(), None) == bad
    assert lib.syldet_output_levels_device(h, x.data_ptr(), 10, 1, 4000, 32, 1, ms.data_ptr(), None) == bad
    first, count = _abi.C.c_int64(), _abi.C.c_int64()
    assert lib.syldet_levels_eval_range(h, 4000, 10, 32, 1, 125, _abi.C.byref(first), _abi.C.byref(count)) == bad
    assert lib.syldet_levels_eval_range(h, 4000, 10, 32, 1, 124, _abi.C.byref(first), _abi.C.byref(count)) == 0
    assert lib.syldet_levels_device(h, x.data_ptr(), 0, 0, 32, 1, ms.data_ptr(), None) == 0                        # n_samples == 0 writes nothing
    torch.cuda.synchronize()
    assert (ms == 7.0).all()
    with pytest.raises(ValueError):
        det3.levels(x, 12)
    with pytest.raises(ValueError):
        det3.levelsPCM16(x)


@pytest.mark.parametrize("kind", ["multi", "mixed"])
def test_banks(kind):
    torch = _torch()
    base = util.sample_net()
    if kind == "multi":
        cfgs = [base, nets.perturbed(base, 5), nets.perturbed(base, 6)]
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
    x = (np.random.default_rng(3).standard_normal((C, S)) * 0.05).astype(np.float32)
    with det:
        xd = torch.from_numpy(x).cuda()
        outputs, flags, ms, lv = det.monitor(xd, 32, 20)
        out2, fl2 = det.run(xd)
        torch.cuda.synchronize()
        assert torch.equal(outputs, out2) and torch.equal(flags, fl2)
        _same_bits(ms.cpu().numpy(), _want_in(x, 32, 20))
        o = outputs.cpu().numpy().copy()
        _plant_outputs(o, det, S, 32, 20, 0)
        _check_outputs(det, base, o, S, 32, 20, 0)
        _same_bits(lv.cpu().numpy(), np.stack([levels_ref.output_readings(outputs.cpu().numpy()[c], 0, S, 32, 20, _clock(base))[0] for c in range(C)]))
        # the streaming getters on a bank
        det.enableMeters()
        det.appendAudioData(x[1, :3000], 1)
        assert det.inputLevel(0) is None
        assert det.inputLevel(1) == float(np.sqrt(np.float64(levels_ref.sum_squares_tree(x[1, :3000])) / 3000.0))
        seen = []
        while det.processNewValue(1):
            seen.append(np.float64(np.float32(det.lastOutputsFor(1)[0])))
        assert len(seen) > 3 and det.outputLevel(1) == float(levels_ref.stat_max(seen)) and det.outputLevel(1) is None


def _stream(det, plan, x, q, meters):
    """feeds the plan's appends and reads; -> (outputs handed out per channel, readings [(kind, channel, value)], expected readings)"""
    C = det.channels
    stat_in, stat_out = [[] for _ in range(C)], [[] for _ in range(C)]
    outs = [[] for _ in range(C)]
    got, want = [], []
    at = [0] * C
    for step in plan:
        op, c = step[0], step[1]
        if op in ("f32", "s16"):
            n = step[2]
            if op == "f32":
                buf = x[c, at[c]:at[c] + n]
                det.appendAudioData(buf, c)
            else:
                det.appendAudioDataPCM16(q[c, at[c]:at[c] + n], c)
                buf = q[c, at[c]:at[c] + n].astype(np.float32) * np.float32(2.0 ** -15)
            at[c] += n
            stat_in[c].append(np.float64(levels_ref.sum_squares_tree(buf)) / np.float64(n))
        elif op == "all":
            det.processAll()
        elif op == "new":
            if det.processNewValue(c):
                outs[c].append(np.float32(det.lastOutputsFor(c)[0]))
                stat_out[c].append(np.float64(outs[c][-1]))
        elif op == "read":
            got.append(("in", c, det.inputLevel(c)))
            got.append(("out", c, det.outputLevel(c)))
            if meters:
                v = levels_ref.stat_max(stat_in[c])
                want.append(("in", c, None if v is None else float(np.sqrt(v))))
                want.append(("out", c, stat_out[c]))
            stat_in[c], stat_out[c] = [], []
    return outs, got, want


def test_streaming_readings_are_the_replay():
    cfg = util.sample_net()
    rng = np.random.default_rng(77)
    total = 60000
    x = (rng.standard_normal((2, total)) * 0.1).astype(np.float32)
    q = rng.integers(-32768, 32768, (2, total)).astype(np.int16)
    plan, fed = [], [0, 0]
    nan_first = nan_later = None
    while min(fed) < total - 800:
        if nan_first is None and fed[0] > 20000:                                  # a reading whose first buffer holds a NaN: it sticks
            plan += [("read", 0), ("f32", 0, 300), ("f32", 0, 200), ("read", 0)]
            nan_first = fed[0] + 5
            fed[0] += 500
        if nan_later is None and fed[1] > 30000:                                  # ... and one that meets it in its second buffer: ignored
            plan += [("read", 1), ("f32", 1, 100), ("f32", 1, 100), ("read", 1)]
            nan_later = fed[1] + 105
            fed[1] += 200
        c = int(rng.integers(0, 2))
        n = int(rng.integers(1, 701))
        if fed[c] + n > total:
            continue
        plan.append(("f32" if rng.random() < 0.5 else "s16", c, n))
        fed[c] += n
        r = rng.random()
        if r < 0.15:
            plan.append(("all", 0))
        if r < 0.3:
            for _ in range(int(rng.integers(1, 6))):
                plan.append(("new", c))
        if 0.3 < r < 0.4:
            plan.append(("read", int(rng.integers(0, 2))))
    plan += [("all", 0), ("new", 0), ("new", 1), ("read", 0), ("read", 1), ("read", 0)]
    x[0, nan_first] = x[1, nan_later] = np.nan
    with sd.SyllableDetector(cfg, channels=2) as on, sd.SyllableDetector(cfg, channels=2) as off:
        on.enableMeters()
        outs_on, got, want = _stream(on, plan, x, q, True)
        outs_off, got_off, _ = _stream(off, plan, x, q, False)
        assert all(v is None for _, _, v in got_off)                              # without syldet_meters_enable: no value
        assert [[np.float32(v).view(np.uint32) for v in ch] for ch in outs_on] == [[np.float32(v).view(np.uint32) for v in ch] for ch in outs_off]
        assert sum(len(ch) for ch in outs_on) > 100
        assert len(got) == len(want) > 20
        n_in = n_out = n_nan = 0
        for (kind, c, g), (_, _, w) in zip(got, want):
            if kind == "in":
                assert (g is None) == (w is None), (kind, c, g, w)
                if g is not None:
                    assert np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64), (c, g, w)
                    n_in += 1
                    n_nan += np.isnan(g)
            else:
                w = levels_ref.stat_max(w)
                assert (g is None) == (w is None), (kind, c, g, w)
                if g is not None:
                    assert np.float64(g).view(np.uint64) == np.float64(w).view(np.uint64), (c, g, w)
                    n_out += 1
        assert n_in > 10 and n_out > 5 and n_nan == 1
        assert got[-2][2] is None and got[-1][2] is None                          # read and reset: nothing since the last read


def test_seen_syllable_writes_every_drained_evaluation():
    cfg = util.sample_net()
    x = (np.random.default_rng(5).standard_normal(20000) * 0.1).astype(np.float32)
    with sd.SyllableDetector(cfg, channels=2) as a, sd.SyllableDetector(cfg, channels=2) as b:
        for det in (a, b):
            det.enableMeters()
            det.appendAudioData(x, 1)
        vals = []
        while a.processNewValue(1):
            vals.append(np.float64(np.float32(a.lastOutputsFor(1)[0])))
        b.seenSyllable(1)
        assert len(vals) > 50
        assert b.outputLevel(1) == a.outputLevel(1) == float(levels_ref.stat_max(vals))
        assert a.outputLevel(0) is None and b.inputLevel(0) is None


def test_no_value_is_lost_between_two_threads():
    cfg = util.sample_net()
    rng = np.random.default_rng(9)
    bufs = (rng.standard_normal((2000, 16)) * rng.uniform(0.01, 1.0, (2000, 1))).astype(np.float32)
    want = max(np.float64(levels_ref.sum_squares_tree(b)) / 16.0 for b in bufs)
    with sd.SyllableDetector(cfg, channels=2) as det:
        det.enableMeters()
        done = threading.Event()
        readings = []

        def reader():
            while not done.is_set():
                v = det.inputLevel(0)
                if v is not None:
                    readings.append(v)

        t = threading.Thread(target=reader)
        t.start()
        try:
            for b in bufs:
                det.appendAudioData(b, 0)
        finally:
            done.set()
            t.join()
        v = det.inputLevel(0)
        if v is not None:
            readings.append(v)
        assert det.inputLevel(0) is None and det.inputLevel(1) is None
    assert readings and max(readings) == float(np.sqrt(want))


def test_python_surface_and_defaults():
    torch = _torch()
    cfg = util.sample_net()
    S = 30001
    x = (np.random.default_rng(2).standard_normal((2, S)) * 0.1).astype(np.float32)
    with sd.SyllableDetector(cfg, channels=2) as det:
        P = det.defaultBuffersPerReading(32)
        assert P == max(1, int(0.1 * cfg.samplingRate / 32)) and det.defaultBuffersPerReading(4096) == max(1, int(0.1 * cfg.samplingRate / 4096))
        xd = torch.from_numpy(x).cuda()
        outputs, flags, ms, lv = det.monitor(xd)
        torch.cuda.synchronize()
        M = levels_ref.levels_count(S, 32, P)
        assert det.levelsCount(S) == M and ms.shape == (2, M) and lv.shape == (2, M) and lv.dtype == torch.float32
        _same_bits(ms.cpu().numpy(), _want_in(x, 32, P))
        _same_bits(det.levels(xd).cpu().numpy(), ms.cpu().numpy())
        _same_bits(lv.cpu().numpy(), np.stack([levels_ref.output_readings(outputs.cpu().numpy()[c], 0, S, 32, P, _clock(cfg))[0] for c in range(2)]))
        assert det.inputLevel(0) is None and det.outputLevel(0) is None           # the meters are off
        det.enableMeters()
        assert det.inputLevel(0) is None and det.outputLevel(1) is None           # nothing appended
        det.appendAudioData(x[0, :100], 0)
        assert det.inputLevel(0) is not None and det.inputLevel(0) is None
        det.enableMeters(False)
        det.appendAudioData(x[0, 100:200], 0)
        assert det.inputLevel(0) is None


def test_syldet_timings_lists_the_kernels(det3):
    torch = _torch()
    x, _ = _rows(S_BIG, 32, 137)
    xd = torch.from_numpy(np.nan_to_num(x, nan=0.0, posinf=0.0)).cuda()
    det3.profile(True)
    try:
        det3.levels(xd, 32, 137)
        torch.cuda.synchronize()
        t = det3.lastTimings()
        assert [n for n, _ in t] == ["levels_in_kernel", "levels_fold_kernel"] and all(ms > 0 for _, ms in t)
        det3.levels(xd, 32, 1)                                                    # every workgroup holds whole readings
        torch.cuda.synchronize()
        assert util.launched(det3) == ["levels_in_kernel"]
        det3.levelsPCM16(torch.zeros((3, 9000), dtype=torch.int16, device="cuda"), 4096, 10 ** 6)   # two workgroups? no: one
        torch.cuda.synchronize()
        assert util.launched(det3) == ["levels_in_kernel"]
        det3.levelsInterleaved(torch.zeros((S_BIG, 3), device="cuda"), 32, 137)
        torch.cuda.synchronize()
        assert util.launched(det3) == ["deinterleave_kernel", "levels_in_kernel", "levels_fold_kernel"]
        out, _ = det3.run(xd)
        det3.outputLevels(out, S_BIG)
        torch.cuda.synchronize()
        assert util.launched(det3) == ["levels_out_kernel"]
    finally:
        det3.profile(False)
