"""Packed recordings' per-sample tracks on the GPU (syldet_recordings_trace_device*, syldet_recordings_trigger*_device*): every
recording's output track, trigger track and onsets out of the packed results are, bit for bit, what the calls for one recording
(syldet_trace_device*, syldet_trigger_device*, syldet_trigger_onsets_device) give on that recording alone through a one-channel
handle, and what the numpy model (recordings_tracks_ref.py) gives; nothing but the recordings' own elements of the destination is
written; the launch rule; the statuses."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import recordings_ref as ref
import recordings_tracks_ref as tref
import trigger_ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth

pytestmark = pytest.mark.gpu

C = 3
LONGEST = 40013            # at L = 8 more than two scan chunks of 2048 buffers: the scan's carry is crossed twice


def _hop131(base):
    return nets.variant(base, windowOverlap=base.windowLength - 131)


def _lengths(cfg):
    """K = 12: none; shorter than first_index; shorter than one evaluation; exactly one evaluation; a multiple of hop; odd
    lengths; the longest; and two long ones that fill the other rows, so that short recordings follow the longest in its row"""
    hop, need, T, D = ref.clock(cfg)
    one = need + (T - 1) * hop
    return [0, D - 5, one - 1, one, 40 * hop, 7777, 1575, 12001, 333, LONGEST, 30001, 29999]


def _audio(n, k):
    if n >= 5000:
        return synth.syllable_channel(n, util.template(), seed=60 + k, every=4000)
    return synth.channel(n, 60 + k)


def _pack(make_bank, make_one, cfg, networks=None):
    """A real packed run: (bank, one-channel handles by network, rec, outputs, flags)"""
    lengths = _lengths(cfg)
    recs = [_audio(n, k) for k, n in enumerate(lengths)]
    offsets = np.cumsum([0] + [x.size + 3 for x in recs])[:-1]
    src = np.zeros(int(offsets[-1]) + recs[-1].size + 8, np.float32)
    for o, x in zip(offsets, recs):
        src[o:o + x.size] = x
    det = make_bank()
    rec = det.recordings(lengths, networks)
    out, fl = det.run(rec.load(torch.from_numpy(src).cuda(), offsets))
    torch.cuda.synchronize()
    hop, _, _, D = ref.clock(cfg)
    ones = {net: make_one(net) for net in sorted(set(networks or [0]))}
    return SimpleNamespace(cfg=cfg, det=det, ones=ones, rec=rec, out=out, fl=fl, outh=out.cpu().numpy(), flh=fl.cpu().numpy(), hop=hop, D=D,
                           lengths=lengths, networks=networks or [0] * len(lengths), K=len(lengths))


def _close(p):
    p.rec.close()
    p.det.close()
    for d in p.ones.values():
        d.close()


_BANKS = {}


def _bank(hop):
    """the base case packed and run once per hop, shared by the tests of this module"""
    if hop not in _BANKS:
        cfg = util.sample_net() if hop == 132 else _hop131(util.sample_net())
        assert ref.clock(cfg)[0] == hop
        _BANKS[hop] = _pack(lambda: sd.SyllableDetector(cfg, channels=C), lambda net: sd.SyllableDetector(cfg, channels=1), cfg)
    return _BANKS[hop]


@pytest.fixture(scope="module", autouse=True)
def _banks_closed_at_the_end():
    yield
    for p in _BANKS.values():
        _close(p)
    _BANKS.clear()


@pytest.fixture(params=[132, 131])
def packed(request):
    return _bank(request.param)


@pytest.fixture
def packed132():
    return _bank(132)


def _follower(p):
    """the recording with an evaluation that follows the longest in its row"""
    slots = p.rec.slots
    long_k = p.lengths.index(LONGEST)
    after = [k for k, s in enumerate(slots) if s[0] == slots[long_k][0] and s[1] > slots[long_k][1] and s[3] > 0]
    assert after, "no recording with an evaluation follows the longest in its row: the plan changed, choose other lengths"
    return long_k, min(after, key=lambda k: slots[k][1])


def test_the_base_case_is_what_it_says(packed132):
    p = packed132
    n_evals = [s[3] for s in p.rec.slots]
    assert p.K == 12 and n_evals[:4] == [0, 0, 0, 1] and p.lengths[4] % p.hop == 0 and p.lengths[1] < p.D
    long_k, nxt = _follower(p)
    assert p.rec.slots[nxt][1] == -(-LONGEST // p.hop) * p.hop                   # right behind it
    assert (LONGEST + 7) // 8 > 2 * 2048
    assert sum(int(tref.own(p.rec.slots, p.flh, k).sum()) for k in range(p.K)) >= 5   # the run fires


# ---- destination layouts ----
def _planar(lengths, line):
    """step 1; recording k starts 0, 1 or 7 elements behind a 16-byte line (of `line` elements) in turn"""
    offsets, pos = [], 0
    for k, n in enumerate(lengths):
        at = (pos + line - 1) // line * line + (0, 1, 7)[k % 3]
        offsets.append(at)
        pos = at + n + 3
    return np.asarray(offsets, np.int64), np.ones(len(lengths), np.int32), pos + 9


def _framed(lengths, step):
    """step > 1; the recordings in groups of `step` that share frames: offsets base + t, as the tracks of a file"""
    offsets, pos = [], 0
    for g in range(0, len(lengths), step):
        group = lengths[g:g + step]
        offsets += [pos + t for t in range(len(group))]
        pos += step * max(group) + 5
    return np.asarray(offsets, np.int64), np.full(len(lengths), step, np.int32), pos + 9


def _layout(name, lengths, itemsize):
    return _planar(lengths, 16 // itemsize) if name == "planar" else _framed(lengths, int(name[-1]))


SENTINEL = -7                  # no value of either track


def _dest(total, dtype):
    return torch.full((total,), SENTINEL, dtype=torch.float32 if dtype == np.float32 else torch.int16, device="cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _assert_same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, "%s: %d of %d elements differ, the first at %d: got %r (bits %#x), want %r (bits %#x)" % (
        what, bad.size, g.size, bad[0], got[bad[0]], g[bad[0]], want[bad[0]], w[bad[0]])


def _expect(per_recording, offsets, steps, total, dtype):
    return tref.scatter(np.full(total, SENTINEL, dtype), per_recording, offsets, steps)[0]


def _trace_alone(p, outputs, dtype, output=0, ones=None):
    """syldet_trace_device* on every recording alone: its n_evals outputs, a one-channel handle of its network"""
    got = []
    for k, s in enumerate(p.rec.slots):
        one = (ones or p.ones)[p.networks[k]]
        own = p.rec.view(outputs, k).contiguous()[None]
        got.append(one.trace(own, s[4], output=output, dtype=dtype)[0].cpu().numpy())
    return got


def _check_trace(p, outputs, thresholds_of_row, dtype, layout, ones=None):
    offsets, steps, total = _layout(layout, p.lengths, np.dtype(dtype).itemsize)
    dst = _dest(total, dtype)
    got = p.rec.trace(outputs, 0, dtype, offsets, steps, out=dst)
    assert got is dst
    alone = _trace_alone(p, outputs, dtype, ones=ones)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    _assert_same_bits(got, _expect(alone, offsets, steps, total, dtype), "against syldet_trace_device* alone")
    model = tref.trace_each(p.rec.slots, outputs.cpu().numpy(), thresholds_of_row, p.D, p.hop, 0, dtype == np.int16)
    assert np.array_equal(got, _expect(model, offsets, steps, total, dtype), equal_nan=True), "differs from the model"
    return got


@pytest.mark.parametrize("layout", ["planar", "step2", "step3"])
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_trace_of_a_real_run(packed, dtype, layout):
    p = packed
    got = _check_trace(p, p.out, [p.cfg.thresholds] * C, dtype, layout)
    assert (got != SENTINEL).sum() == sum(p.lengths) and (got > 0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
@pytest.mark.parametrize("thr", [None, 0.0])
def test_trace_of_synthetic_outputs(packed132, dtype, thr):
    """NaN, negative values, values above the threshold; thr 0.0: a zero threshold (x / 0 and 0 / 0)"""
    p = packed132
    rng = np.random.default_rng(17)
    t = float(p.cfg.thresholds[0]) if thr is None else 1.0
    o = (rng.standard_normal(p.outh.shape) * 1.5 * t).astype(np.float32)
    o[rng.random(o.shape) < 0.05] = np.nan
    o[rng.random(o.shape) < 0.05] = 0.0
    o[rng.random(o.shape) < 0.02] = np.inf
    outputs = torch.from_numpy(o).cuda()
    if thr is None:
        _check_trace(p, outputs, [p.cfg.thresholds] * C, dtype, "planar")
        return
    cfg0 = nets.variant(p.cfg, thresholds=[0.0])
    with sd.SyllableDetector(cfg0, channels=C) as det, sd.SyllableDetector(cfg0, channels=1) as one, det.recordings(p.lengths) as rec:
        assert rec.slots == p.rec.slots
        q = SimpleNamespace(**{**vars(p), "rec": rec, "det": det})
        got = _check_trace(q, outputs, [[0.0]] * C, dtype, "planar", ones={0: one})
        if dtype == np.float32:
            assert np.isnan(got).any() and (got == 1.0).any()


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_trace_on_a_mixed_bank_divides_by_the_rows_threshold(dtype):
    base = util.sample_net()
    f0, f1 = sd.frequencyIndexRange(512, base.samplingRate, 1000.0, 9000.0)
    net = nets.random_net(np.random.default_rng(2), (f1 - f0) * base.timeRange, (8,), 1, in_fns=("normalize", "mapminmax"))
    other = nets.variant(base, fourierLength=512, freqRange=(1000.0, 9000.0), net=net, thresholds=[0.1], spectrogramScaling="log")
    cfgs = [nets.variant(base, thresholds=[0.7]), other]
    channel_net = [0, 1, 0]
    networks = [k % 2 for k in range(12)]
    p = _pack(lambda: sd.SyllableDetector.mixed(cfgs, channel_net), lambda n: sd.SyllableDetector(cfgs[n], channels=1), cfgs[0], networks)
    try:
        assert {p.rec.slots[k][0] for k in range(p.K) if networks[k] == 1} == {1}
        got = _check_trace(p, p.out, [cfgs[n].thresholds for n in channel_net], dtype, "planar")
        assert (got > 0).any()
    finally:
        _close(p)


# ---- the trigger track ----
def _flags(p, pattern):
    """synthetic flags [C, rowEvaluations]; every row evaluation outside the recordings is SET in the patterns that compare
    against a recording alone with few flags: were one read, a pulse would show"""
    E = p.rec.rowEvaluations
    rng = np.random.default_rng(23)
    inside = np.zeros((C, E), bool)
    for row, _, first, n_evals, _ in p.rec.slots:
        inside[row, first:first + n_evals] = True
    if pattern == "none":
        f = np.zeros((C, E), np.uint8)
    elif pattern == "all":
        f = np.ones((C, E), np.uint8)
    elif pattern == "random":
        f = (rng.random((C, E)) < 0.03).astype(np.uint8)
    else:                                                  # "last": the last evaluation of every recording
        f = np.zeros((C, E), np.uint8)
        for row, _, first, n_evals, _ in p.rec.slots:
            if n_evals > 0:
                f[row, first + n_evals - 1] = 1
    if pattern in ("none", "random", "last"):
        f[~inside] = 1
    assert (~inside).any()
    return torch.from_numpy(f).cuda(), f


def _trigger_alone(p, fl, L, N, lat, dtype):
    got = []
    for k, s in enumerate(p.rec.slots):
        own = p.rec.view(fl, k).contiguous()[None]
        got.append(p.ones[0].triggerTrack(own, s[4], L, N, lat, dtype=dtype)[0].cpu().numpy())
    return got


@pytest.mark.parametrize("L", [8, 32, 4096])
@pytest.mark.parametrize("pattern", ["none", "all", "random", "last"])
def test_trigger_track(packed132, pattern, L):
    _check_trigger(packed132, pattern, L)


def test_trigger_track_at_hop_131():
    _check_trigger(_bank(131), "random", 8)


def _check_trigger(p, pattern, L):
    fl, flh = _flags(p, pattern)
    long_k, nxt = _follower(p)
    for dtype in (np.float32, np.int16):
        layout = "planar" if dtype == np.int16 else "step2"
        offsets, steps, total = _layout(layout, p.lengths, np.dtype(dtype).itemsize)
        for N in (1, 44, L, LONGEST + 1000):
            for lat in (0, 221, 2000):                      # 2000: longer than the recordings of 333 and 1575 samples
                dst = _dest(total, dtype)
                got = p.rec.triggerTrack(fl, L, N, lat, dtype, offsets, steps, out=dst)
                alone = _trigger_alone(p, fl, L, N, lat, dtype)
                torch.cuda.synchronize()
                got = got.cpu().numpy()
                what = "%s L %d N %d latency %d %s" % (pattern, L, N, lat, np.dtype(dtype).name)
                _assert_same_bits(got, _expect(alone, offsets, steps, total, dtype), what + ", against syldet_trigger_device* alone")
                model = tref.trigger_each(p.rec.slots, flh, p.D, p.hop, L, N, lat, dtype == np.int16)
                assert np.array_equal(got, _expect(model, offsets, steps, total, dtype)), what + ": differs from the model"
                # the recording behind the longest starts low, whatever the longest's last pulse was about to do
                mine = p.rec.trackView(got, nxt, offsets, steps)
                assert mine.size == p.lengths[nxt] and not mine[:min(L + lat, mine.size)].any()
                if pattern == "last" and N > L and lat == 0 and L <= 32:
                    # ... and that pulse, armed in the longest's last buffers, is cut at its end
                    tail = p.rec.trackView(got, long_k, offsets, steps)
                    assert tail[-1] != 0


@pytest.mark.parametrize("L", [8, 32, 4096])
def test_onsets(packed132, L):
    _check_onsets(packed132, L, ("all", "random", "last"))


def test_onsets_at_hop_131():
    _check_onsets(_bank(131), 8, ("random",))


def _check_onsets(p, L, patterns):
    for pattern in patterns:
        fl, flh = _flags(p, pattern)
        for N in (1, 44, L, LONGEST + 1000):
            for lat in (0, 221, 2000):
                idx, cnt = p.rec.triggerOnsets(fl, L, N, lat)
                track = p.rec.triggerTrack(fl, L, N, lat)
                alone = []
                for k, s in enumerate(p.rec.slots):
                    i1, c1 = p.ones[0].triggerOnsets(p.rec.view(fl, k).contiguous()[None], s[4], L, N, lat)
                    alone.append((i1, c1))
                torch.cuda.synchronize()
                idx, cnt, track = idx.cpu().numpy(), cnt.cpu().numpy(), track.cpu().numpy()
                model = tref.onsets_each(p.rec.slots, flh, p.D, p.hop, L, N, lat)
                for k in range(p.K):
                    n = int(cnt[k])
                    i1, c1 = alone[k][0].cpu().numpy(), alone[k][1].cpu().numpy()
                    assert n == int(c1[0]) and n <= idx.shape[1] and np.array_equal(idx[k, :n], i1[0, :n])
                    assert np.array_equal(idx[k, :n], model[k])
                    assert np.array_equal(idx[k, :n], trigger_ref.rising_edges(p.rec.trackView(track, k) != 0))
                if pattern == "all" and N == 1 and lat == 0:
                    full = cnt.copy()
                    assert full.max() >= 3
                    small, cnt2 = p.rec.triggerOnsets(fl, L, N, lat, capacity=2)      # below the greatest count
                    torch.cuda.synchronize()
                    assert tuple(small.shape) == (p.K, 2) and np.array_equal(cnt2.cpu().numpy(), full)
                    small = small.cpu().numpy()
                    for k in range(p.K):
                        assert np.array_equal(small[k, :min(2, full[k])], idx[k, :min(2, full[k])])
                    none, cnt0 = p.rec.triggerOnsets(fl, L, N, lat, capacity=0)       # counts only: no index to read
                    torch.cuda.synchronize()
                    assert tuple(none.shape) == (p.K, 0) and np.array_equal(cnt0.cpu().numpy(), full)


# ---- the launch rule ----
def test_the_same_layout_again_is_launches_only(packed132):
    p = packed132
    fl, flh = _flags(p, "random")
    det, rec = p.det, p.rec
    a_off, a_steps, a_total = _layout("planar", p.lengths, 2)
    b_off, b_steps, b_total = _layout("step3", p.lengths, 2)
    det.profile(True)
    try:
        for _ in range(2):
            a = rec.trace(p.out, 0, np.int16, a_off, a_steps, out=_dest(a_total, np.int16))
        torch.cuda.synchronize()
        assert util.launched(det) == ["recordings_trace_kernel"]
        for _ in range(2):
            rec.triggerTrack(fl, 32, 44, 0, np.int16, a_off, a_steps, out=_dest(a_total, np.int16))
        torch.cuda.synchronize()
        names = det.lastTimings()
        assert [n for n, _ in names] == ["recordings_trigger_scan_kernel", "recordings_trigger_kernel"] and all(ms > 0 for _, ms in names)
        rec.triggerOnsets(fl, 32, 44, 0)
        torch.cuda.synchronize()
        assert util.launched(det) == ["recordings_trigger_scan_kernel", "recordings_trigger_onsets_kernel"]
    finally:
        det.profile(False)
    # a changed layout gives the new layout's results; trace and trigger calls, each with a layout of its own, take turns
    want_a = _expect(tref.trace_each(rec.slots, p.outh, [p.cfg.thresholds] * C, p.D, p.hop, 0, True), a_off, a_steps, a_total, np.int16)
    want_b = _expect(tref.trigger_each(rec.slots, flh, p.D, p.hop, 8, 44, 0, True), b_off, b_steps, b_total, np.int16)
    assert np.array_equal(a.cpu().numpy(), want_a)
    for _ in range(2):
        b = rec.triggerTrack(fl, 8, 44, 0, np.int16, b_off, b_steps, out=_dest(b_total, np.int16))
        a = rec.trace(p.out, 0, np.int16, a_off, a_steps, out=_dest(a_total, np.int16))
        torch.cuda.synchronize()
        assert np.array_equal(b.cpu().numpy(), want_b) and np.array_equal(a.cpu().numpy(), want_a)
    # the default destination: trackLayout, zero between the recordings
    d = rec.trace(p.out).cpu().numpy()
    offsets, total = rec.trackLayout()
    assert d.size == total and np.array_equal(d, tref.scatter(np.zeros(total, np.int16), tref.trace_each(rec.slots, p.outh, [p.cfg.thresholds] * C, p.D,
                                                                                                      p.hop, 0, True), offsets)[0])


# ---- the statuses ----
def test_every_refusal_leaves_the_destination_alone(packed132):
    p = packed132
    rec, lib, K = p.rec, _abi.lib, p.K
    fl, _ = _flags(p, "all")
    off, steps, total = _layout("planar", p.lengths, 2)
    dst = _dest(total, np.int16)
    dstf = _dest(total, np.float32)
    idx = torch.full((K, 4), SENTINEL, dtype=torch.int64, device="cuda")
    cnt = torch.full((K,), SENTINEL, dtype=torch.int64, device="cuda")
    o, f, d, df = p.out.data_ptr(), fl.data_ptr(), dst.data_ptr(), dstf.data_ptr()

    def i64(a):
        a = np.ascontiguousarray(a, np.int64)
        return a, a.ctypes.data_as(_abi.c_int64_p)

    def i32(a):
        a = np.ascontiguousarray(a, np.int32)
        return a, a.ctypes.data_as(_abi.c_int32_p)

    keep = []

    def offs(change=None):
        a = off.copy()
        if change:
            a[change[0]] = change[1]
        keep.append(i64(a))
        return keep[-1][1]

    def stps(change=None):
        a = steps.copy()
        if change:
            a[change[0]] = change[1]
        keep.append(i32(a))
        return keep[-1][1]

    long_k = p.lengths.index(LONGEST)
    over = total - LONGEST + 1                              # the longest from here ends one element behind the destination
    refused = [
        lambda: lib.syldet_recordings_trace_device_s16(None, o, 0, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, None, 0, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, o, 0, None, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, o, 0, d, total, None, stps(), None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, o, -1, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, o, 1, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trace_device(rec._h, o, 1, df, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, o, 0, d, total, offs((3, -1)), stps(), None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, o, 0, d, total, offs(), stps((3, 0)), None),
        lambda: lib.syldet_recordings_trace_device(rec._h, o, 0, df, total, offs((long_k, over)), None, None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, o, 0, d, total, offs((long_k, over)), None, None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, o, 0, d, total, offs(), stps((long_k, 4)), None),
        lambda: lib.syldet_recordings_trace_device_s16(rec._h, o, 0, d, -1, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(None, f, 32, 44, 0, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, None, 32, 44, 0, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 32, 44, 0, None, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 32, 44, 0, d, total, None, stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 4, 44, 0, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 48, 44, 0, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 8192, 44, 0, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 32, 0, 0, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 32, (1 << 24) + 1, 0, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 32, 44, -1, d, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device(rec._h, f, 32, 44, (1 << 24) + 1, df, total, offs(), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 32, 44, 0, d, total, offs((5, -3)), stps(), None),
        lambda: lib.syldet_recordings_trigger_device_s16(rec._h, f, 32, 44, 0, d, total, offs(), stps((5, -1)), None),
        lambda: lib.syldet_recordings_trigger_device(rec._h, f, 32, 44, 0, df, total, offs((long_k, over)), stps(), None),
        lambda: lib.syldet_recordings_trigger_onsets_device(None, f, 32, 44, 0, idx.data_ptr(), 4, cnt.data_ptr(), None),
        lambda: lib.syldet_recordings_trigger_onsets_device(rec._h, None, 32, 44, 0, idx.data_ptr(), 4, cnt.data_ptr(), None),
        lambda: lib.syldet_recordings_trigger_onsets_device(rec._h, f, 32, 44, 0, None, 4, cnt.data_ptr(), None),
        lambda: lib.syldet_recordings_trigger_onsets_device(rec._h, f, 32, 44, 0, idx.data_ptr(), 4, None, None),
        lambda: lib.syldet_recordings_trigger_onsets_device(rec._h, f, 32, 44, 0, idx.data_ptr(), -1, cnt.data_ptr(), None),
        lambda: lib.syldet_recordings_trigger_onsets_device(rec._h, f, 16, 0, 0, idx.data_ptr(), 4, cnt.data_ptr(), None),
        lambda: lib.syldet_recordings_trigger_onsets_device(rec._h, f, 12, 44, 0, idx.data_ptr(), 4, cnt.data_ptr(), None),
        lambda: lib.syldet_recordings_trigger_onsets_device(rec._h, f, 32, 44, -2, idx.data_ptr(), 4, cnt.data_ptr(), None),
    ]
    for i, call in enumerate(refused):
        assert call() == _abi.ERR_INVALID_ARGUMENT, "refusal %d" % i
    lib.syldet_recordings_trace_device_s16(rec._h, o, 0, d, total, offs((long_k, over)), None, None)
    assert "recording %d " % long_k in _abi.last_error()    # the one that ends behind the destination is named
    torch.cuda.synchronize()
    for t in (dst, dstf, idx, cnt):
        assert bool((t == SENTINEL).all())
    # ... and the same arguments without the fault are taken (the longest ending exactly at the destination's end)
    assert lib.syldet_recordings_trace_device_s16(rec._h, o, 0, d, total, offs((long_k, over - 1)), None, None) == 0
    torch.cuda.synchronize()


def test_run_recordings_returns_the_tracks_next_to_the_events():
    cfg = util.sample_net()
    tmpl = util.template()
    mono = [synth.syllable_channel(n, tmpl, seed=30 + i, every=4000) for i, n in enumerate([30011, 900])]
    stereo = np.stack([synth.syllable_channel(22222, tmpl, seed=40, every=4000), synth.syllable_channel(22222, tmpl, seed=41, every=4000)], axis=1)
    arrays = [mono[0], stereo, mono[1], np.zeros((0, 2), np.float32)]
    each = [arrays[0], arrays[1][:, 0], arrays[1][:, 1], arrays[2], arrays[3][:, 0], arrays[3][:, 1]]
    with sd.SyllableDetector(cfg, channels=3) as det, sd.SyllableDetector(cfg, channels=1) as one:
        plain = det.runRecordings(arrays, 0.05)
        events, tracks = det.runRecordings(arrays, 0.05, tracks=("trace", "ttl"), bufferLength=8, width=100, latency=3)
        assert len(plain) == len(events) == len(each) and sorted(tracks) == ["trace", "ttl"]
        for (pi, pv), (ei, ev) in zip(plain, events):
            assert np.array_equal(pi, ei) and np.array_equal(pv, ev)
        high = 0
        for k, x in enumerate(each):
            t = torch.from_numpy(np.ascontiguousarray(x)[None, :]).cuda()
            if one.countEvaluations(x.size) > 0:
                out, fl = one.run(t)
            else:
                out, fl = torch.zeros((1, 0, 1), device="cuda"), torch.zeros((1, 0), dtype=torch.uint8, device="cuda")
            want_trace = one.trace(out, x.size, dtype=np.int16)[0].cpu().numpy()
            want_ttl = one.triggerTrack(fl, x.size, 8, 100, 3, dtype=np.int16)[0].cpu().numpy()
            assert tracks["trace"][k].dtype == np.int16 and np.array_equal(tracks["trace"][k], want_trace), k
            assert np.array_equal(tracks["ttl"][k], want_ttl), k
            high += int((want_ttl != 0).sum())
        assert high > 0
        only = det.runRecordings(arrays, 0.05, tracks=("ttl",), bufferLength=8, width=100, latency=3)[1]
        assert sorted(only) == ["ttl"] and all(np.array_equal(a, b) for a, b in zip(only["ttl"], tracks["ttl"]))
        with pytest.raises(ValueError):
            det.runRecordings(arrays, tracks=("levels",))
