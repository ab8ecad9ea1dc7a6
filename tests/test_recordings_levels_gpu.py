"""Packed recordings' level meters on the GPU (syldet_recordings_levels_device*, syldet_recordings_output_levels_device): every
recording's readings out of the packed rows and the packed results are, bit for bit, what the calls for one recording
(syldet_levels_device*, syldet_output_levels_device) give on that recording alone through a one-channel handle, and what the
numpy model (recordings_levels_ref.py) gives; nothing outside a recording is read as part of it (the rows hold NaN, or full
scale, everywhere else); the launch rule; the statuses.  No tolerance anywhere: the contract is bit identity (NaN at the same
places; a NaN's payload is not part of it)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import recordings_levels_ref as lref
import recordings_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth

pytestmark = pytest.mark.gpu

C = 3
TILE = 8192
LS = (8, 32, 4096)
PS = (1, 3, 16, 10 ** 9)       # a lane a reading, a wave a reading, one reading a recording
LONG = 30011                   # four tiles: with P L > 8192 a reading spans three workgroups and more
# none, 1, 7, 131; L - 1, L, L + 1 for every L; the long one and two that fill the other rows; 9000 behind 12001: it crosses a tile
# in the middle of a buffer and of a reading
LENGTHS = [0, 1, 7, 8, 9, 131, 31, 32, 33, 4095, 4096, 4097, LONG, 29000, 12001, 9000, 5000]
SENTINEL = -7.0


def _hop131(base):
    return nets.variant(base, windowOverlap=base.windowLength - 131)


def _audio(n, k):
    """noise at a level of the recording's own, so that a neighbour's samples would show in a reading"""
    return (np.random.default_rng(500 + k).standard_normal(n) * (0.02 + 0.05 * (k % 7))).astype(np.float32)


def _rows(slots, row_samples, recs, fill, dtype):
    """the packed rows with `fill` (NaN, full scale) everywhere outside the recordings: pads, tails, rows' ends"""
    rows = np.full((C, row_samples), fill, dtype)
    for (row, offset, _, _, n), x in zip(slots, recs):
        rows[row, offset:offset + n] = x
    return rows


def _make(cfg, make_bank, make_one, networks=None):
    det = make_bank()
    rec = det.recordings(LENGTHS, networks)
    f32 = [_audio(n, k) for k, n in enumerate(LENGTHS)]
    s16 = [np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16) for x in f32]
    ones = {net: make_one(net) for net in sorted(set(networks or [0]))}
    hop, need, T, D = ref.clock(cfg)
    return SimpleNamespace(cfg=cfg, det=det, rec=rec, ones=ones, networks=networks or [0] * len(LENGTHS), K=len(LENGTHS), hop=hop,
                           clock=(cfg.windowLength, cfg.windowOverlap, cfg.timeRange), f32=f32, s16=s16,
                           rows_f32=_rows(rec.slots, rec.rowSamples, f32, np.nan, np.float32),
                           rows_s16=_rows(rec.slots, rec.rowSamples, s16, 32767, np.int16))


def _close(b):
    b.rec.close()
    b.det.close()
    for d in b.ones.values():
        d.close()


_BANKS = {}


def _bank(hop):
    """the base case planned once per hop, shared by the tests of this module"""
    if hop not in _BANKS:
        cfg = util.sample_net() if hop == 132 else _hop131(util.sample_net())
        assert ref.clock(cfg)[0] == hop
        _BANKS[hop] = _make(cfg, lambda: sd.SyllableDetector(cfg, channels=C), lambda net: sd.SyllableDetector(cfg, channels=1))
    return _BANKS[hop]


@pytest.fixture(scope="module", autouse=True)
def _banks_closed_at_the_end():
    yield
    for b in _BANKS.values():
        _close(b)
    _BANKS.clear()


@pytest.fixture(params=[132, 131])
def bank(request):
    return _bank(request.param)


@pytest.fixture
def bank132():
    return _bank(132)


def _same(got, want, what):
    """NaN at the same places, the same bits everywhere else"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN at %s, wanted at %s" % (what, np.nonzero(gn)[0][:8], np.nonzero(wn)[0][:8])
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    bad = np.nonzero((got.view(bits) != want.view(bits)) & ~gn)[0]
    assert bad.size == 0, "%s: %d of %d readings differ, the first at %d: got %r, want %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def _alone_in(b, rows, L, P):
    """every recording through the one-recording call, alone on a one-channel handle: the flat table"""
    parts = []
    for k, (row, offset, _, _, n) in enumerate(b.rec.slots):
        if n == 0:
            continue
        one = b.ones[b.networks[k]]
        x = torch.from_numpy(rows[row:row + 1, offset:offset + n].copy()).cuda()
        parts.append((one.levelsPCM16 if rows.dtype == np.int16 else one.levels)(x, L, P)[0])
    return torch.cat(parts).cpu().numpy()


def _alone_out(b, outputs, L, P, output=0):
    parts = []
    for k, (row, _, first, n_evals, n) in enumerate(b.rec.slots):
        if n == 0:
            continue
        own = torch.from_numpy(outputs[row:row + 1, first:first + n_evals].copy()).cuda()
        parts.append(b.ones[b.networks[k]].outputLevels(own, n, output, L, P)[0])
    return torch.cat(parts).cpu().numpy()


def _follower(slots, k):
    """the recording with samples that follows recording k in its row, or None"""
    after = [j for j, s in enumerate(slots) if s[0] == slots[k][0] and s[1] > slots[k][1] and s[4] > 0]
    return min(after, key=lambda j: slots[j][1]) if after else None


def test_the_base_case_is_what_it_says(bank132):
    b = bank132
    slots = b.rec.slots
    assert b.K == 17 and len({s[0] for s in slots}) == C and b.rec.rowSamples > 4 * TILE
    for L in LS:
        masked = crossing = 0
        for k, (row, offset, _, _, n) in enumerate(slots):
            nxt = _follower(slots, k)
            # a short last buffer with a (loud) recording beginning within L samples of the recording's end
            masked += n % L != 0 and nxt is not None and slots[nxt][1] - (offset + n) < L
            # a tile boundary inside the recording, in the middle of a buffer and of a reading of 3 buffers
            for edge in range(TILE, b.rec.rowSamples, TILE):
                crossing += offset < edge < offset + n and (edge - offset) % L != 0 and (edge - offset) % (3 * L) != 0
        assert masked >= 1 and crossing >= 1, (L, masked, crossing)
    # 16-bit rows at hop 132: recordings that begin on a 16-byte line and recordings that begin 8 bytes behind one; at hop 131: odd offsets
    assert {(s[1] * 2) % 16 for s in slots if s[4] > 0} == {0, 8}
    assert any(s[1] % 2 == 1 for s in _bank(131).rec.slots if s[4] > 0)
    # the layout the library states is the binding's arithmetic
    for L, P in ((8, 1), (32, 3), (4096, 10 ** 9)):
        first = np.full(b.K + 1, -1, np.int64)
        total = ctypes.c_int64(-1)
        assert _abi.lib.syldet_recordings_levels_layout(b.rec._h, L, P, first.ctypes.data_as(_abi.c_int64_p), ctypes.byref(total)) == 0
        assert np.array_equal(first, b.rec.levelsLayout(L, P)) and total.value == first[-1] == lref.layout(slots, L, P)[-1]
        total.value = -1
        assert _abi.lib.syldet_recordings_levels_layout(b.rec._h, L, P, None, ctypes.byref(total)) == 0 and total.value == first[-1]
    for L, P in ((12, 3), (4, 3), (8192, 3), (32, 0)):
        assert _abi.lib.syldet_recordings_levels_layout(b.rec._h, L, P, None, ctypes.byref(total)) == _abi.ERR_INVALID_ARGUMENT
    assert _abi.lib.syldet_recordings_levels_layout(b.rec._h, 32, 3, None, None) == _abi.ERR_INVALID_ARGUMENT


# ---- the input meter ----
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("s16", [False, True], ids=["f32", "s16"])
def test_the_input_meter_is_every_recording_alone(bank, s16, L):
    b = bank
    rows = b.rows_s16 if s16 else b.rows_f32
    d_rows = torch.from_numpy(rows).cuda()
    for P in PS:
        got = b.rec.levels(d_rows, L, P).cpu().numpy()
        assert got.dtype == np.float64 and got.size == b.rec.levelsLayout(L, P)[-1] and not np.isnan(got).any()
        _same(got, _alone_in(b, rows, L, P), "hop %d, L %d, P %d against the recordings alone" % (b.hop, L, P))
        _same(got, lref.input_each(b.rec.slots, rows, L, P), "hop %d, L %d, P %d against the model" % (b.hop, L, P))


def test_the_rows_the_load_wrote_give_the_same_readings(bank):
    b = bank
    for recs, rows in ((b.f32, b.rows_f32), (b.s16, b.rows_s16)):
        offsets = np.cumsum([0] + [x.size + 3 for x in recs])[:-1]
        src = np.zeros(int(offsets[-1]) + recs[-1].size + 8, rows.dtype)
        for o, x in zip(offsets, recs):
            src[o:o + x.size] = x
        loaded = b.rec.load(torch.from_numpy(src).cuda(), offsets)
        for L, P in ((32, 3), (8, 10 ** 9)):
            _same(b.rec.levels(loaded, L, P).cpu().numpy(), b.rec.levels(torch.from_numpy(rows).cuda(), L, P).cpu().numpy(), "loaded rows")
        # a view of wider rows: channel_stride > row_samples
        wide = torch.full((C, b.rec.rowSamples + 24), 1.0, dtype=loaded.dtype, device="cuda")
        wide[:, :b.rec.rowSamples] = loaded
        _same(b.rec.levels(wide, 32, 3).cpu().numpy(), b.rec.levels(loaded, 32, 3).cpu().numpy(), "wider rows")


@pytest.mark.parametrize("L,P", [(32, 3), (32, 10 ** 9), (4096, 3), (4096, 10 ** 9), (8, 16)])
def test_planted_values(bank132, L, P):
    b = bank132
    slots = b.rec.slots
    long_k = LENGTHS.index(LONG)
    first = b.rec.levelsLayout(L, P)
    Pk = min(P, -(-LONG // L))

    def run(plants):
        rows = b.rows_f32.copy()
        for k, i, v in plants:
            rows[slots[k][0], slots[k][1] + i] = v
        got = b.rec.levels(torch.from_numpy(rows).cuda(), L, P).cpu().numpy()
        _same(got, _alone_in(b, rows, L, P), "planted, against the recordings alone")
        _same(got, lref.input_each(slots, rows, L, P), "planted, against the model")
        return got

    def reading(k, i):
        return int(first[k] + (i // L) // min(P, -(-LENGTHS[k] // L)))

    # NaN in a later buffer of a reading is ignored, +inf is the greatest; a NaN in the first sample of the next recording (and in
    # the pad in front of it, as everywhere in these rows) stays out of the recording before
    later = 20000 if (20000 // L) % Pk != 0 else 20000 + L
    assert (later // L) % Pk != 0
    pred = next(k for k in range(b.K) if LENGTHS[k] % L != 0 and _follower(slots, k) is not None and slots[_follower(slots, k)][1] - (slots[k][1] + LENGTHS[k]) < L)
    nxt = _follower(slots, pred)
    got = run([(long_k, later, np.nan), (long_k, 10000, np.inf), (nxt, 0, np.nan)])
    assert np.isinf(got[reading(long_k, 10000)]) and not np.isnan(got[reading(long_k, later)])
    assert np.isnan(got[first[nxt]]) and not np.isnan(got[first[pred]:first[pred + 1]]).any()
    assert np.isnan(got).sum() == 1
    # NaN as the first buffer of a reading sticks -- across workgroups too -- whatever follows it in the reading
    m = 1 if first[long_k + 1] - first[long_k] > 1 else 0
    behind = m * Pk * L + Pk * L // 2 + L
    assert behind < min((m + 1) * Pk * L, LONG)
    got = run([(long_k, m * Pk * L + 3, np.nan), (long_k, behind, np.inf)])
    assert np.isnan(got[first[long_k] + m]) and np.isnan(got).sum() == 1


# ---- the output meter ----
def _packed_run(b):
    """the recordings loaded and run: outputs [C, rowEvaluations, n_out] on the device and on the host"""
    if not hasattr(b, "out"):
        offsets = np.cumsum([0] + [x.size + 3 for x in b.f32])[:-1]
        src = np.zeros(int(offsets[-1]) + b.f32[-1].size + 8, np.float32)
        for o, x in zip(offsets, b.f32):
            src[o:o + x.size] = x
        b.out = b.det.run(b.rec.load(torch.from_numpy(src).cuda(), offsets))[0]
        torch.cuda.synchronize()
        b.outh = b.out.cpu().numpy()
    return b.out, b.outh


@pytest.mark.parametrize("L", LS)
def test_the_output_meter_on_a_real_run_is_every_recording_alone(bank, L):
    b = bank
    out, outh = _packed_run(b)
    assert sum(s[3] > 0 for s in b.rec.slots) >= 8 and sum(s[3] == 0 and s[4] > 0 for s in b.rec.slots) >= 5   # some shorter than one evaluation
    for P in PS:
        got = b.rec.outputLevels(out, 0, L, P).cpu().numpy()
        assert got.dtype == np.float32 and got.size == b.rec.levelsLayout(L, P)[-1]
        _same(got, _alone_out(b, outh, L, P), "hop %d, L %d, P %d against the recordings alone" % (b.hop, L, P))
        _same(got, lref.output_each(b.rec.slots, outh, 0, L, P, b.clock), "hop %d, L %d, P %d against the model" % (b.hop, L, P))


@pytest.mark.parametrize("L,P", [(8, 1), (32, 3), (32, 16), (4096, 3), (32, 10 ** 9)])
def test_the_output_meter_on_planted_outputs(bank132, L, P):
    b = bank132
    slots, E = b.rec.slots, b.rec.rowEvaluations
    rng = np.random.default_rng(11)
    # few values: NaN first and NaN later, -0 in front of +0 and behind it, equal maxima -- at scale; 77 in every row evaluation
    # outside the recordings, which must never appear
    values = np.array([-0.0, 0.0, 0.25, 0.5, np.nan, -1.0], np.float32)
    inside = np.zeros((C, E), bool)
    for row, _, f, n_evals, _ in slots:
        inside[row, f:f + n_evals] = True
    assert (~inside).sum() > 0
    outputs = values[rng.integers(0, len(values), (C, E, 1))]
    outputs[~inside] = 77.0
    # one reading of the long recording that is -0, +0, -0, ...: StatMax keeps the first of equal values
    long_k = LENGTHS.index(LONG)
    one = b.ones[0]
    first = b.rec.levelsLayout(L, P)
    m = int(first[long_k + 1] - first[long_k]) // 2
    f, count = one.levelsEvalRange(LONG, slots[long_k][3], m, L, P)
    assert (count >= 2) == (P * L >= 2 * b.hop)                               # (shorter readings hold one evaluation at the most)
    row, _, fe, _, _ = slots[long_k]
    if count >= 2:
        outputs[row, fe + f:fe + f + count, 0] = np.where(np.arange(count) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    got = b.rec.outputLevels(torch.from_numpy(outputs).cuda(), 0, L, P).cpu().numpy()
    _same(got, _alone_out(b, outputs, L, P), "planted outputs against the recordings alone")
    model = lref.output_each(slots, outputs, 0, L, P, b.clock)
    _same(got, model, "planted outputs against the model")
    if count >= 2:
        assert got[first[long_k] + m].view(np.uint32) == 0x80000000
    assert not (got == 77.0).any() and np.isnan(got).any() and (got == 0.5).any()
    # readings without an evaluation are 0: every reading of a recording shorter than one evaluation, and the readings in front of the first one
    for k, s in enumerate(slots):
        if s[3] == 0:
            assert (got[first[k]:first[k + 1]].view(np.uint32) == 0).all()
    before_first = one.levelsEvalRange(LONG, slots[long_k][3], 0, L, P)[1] == 0
    assert before_first or (L, P) != (8, 1)
    if before_first:
        assert got[first[long_k]].view(np.uint32) == 0


@pytest.mark.parametrize("kind", ["multi", "mixed"])
def test_both_meters_on_banks_of_several_networks(kind):
    base = util.sample_net()
    if kind == "multi":
        cfgs = [base, nets.perturbed(base, 1)]
        make = lambda: sd.SyllableDetector.multi(cfgs, [0, 1, 0])
    else:
        f0, f1 = sd.frequencyIndexRange(512, base.samplingRate, 1000.0, 9000.0)
        net = nets.random_net(np.random.default_rng(2), (f1 - f0) * base.timeRange, (8,), 1, in_fns=("normalize", "mapminmax"))
        cfgs = [base, nets.variant(base, fourierLength=512, freqRange=(1000.0, 9000.0), net=net, thresholds=[0.1], spectrogramScaling="log")]
        make = lambda: sd.SyllableDetector.mixed(cfgs, [0, 1, 0])
    networks = [k % 2 for k in range(len(LENGTHS))]
    b = _make(cfgs[0], make, lambda n: sd.SyllableDetector(cfgs[n], channels=1), networks)
    try:
        assert {b.rec.slots[k][0] for k in range(b.K) if networks[k] == 1} == {1}
        out, outh = _packed_run(b)
        for L, P in ((32, 3), (8, 10 ** 9)):
            _same(b.rec.outputLevels(out, 0, L, P).cpu().numpy(), _alone_out(b, outh, L, P), "%s bank, output meter" % kind)
            _same(b.rec.levels(torch.from_numpy(b.rows_f32).cuda(), L, P).cpu().numpy(), _alone_in(b, b.rows_f32, L, P), "%s bank, input meter" % kind)
    finally:
        _close(b)


# ---- the launch rule ----
def test_the_same_pair_again_is_launches_only(bank132):
    b = bank132
    det, rec = b.det, b.rec
    out, _ = _packed_run(b)
    rows = torch.from_numpy(b.rows_f32).cuda()
    rows16 = torch.from_numpy(b.rows_s16).cuda()
    det.profile(True)
    try:
        for _ in range(2):
            rec.levels(rows, 32, 3)
        torch.cuda.synchronize()
        names = det.lastTimings()
        assert [n for n, _ in names] == ["recordings_levels_zero_kernel", "recordings_levels_in_kernel"] and all(ms > 0 for _, ms in names)
        rec.levels(rows16, 32, 3)
        torch.cuda.synchronize()
        assert util.launched(det) == ["recordings_levels_zero_kernel", "recordings_levels_in_kernel"]
        for _ in range(2):
            rec.outputLevels(out, 0, 32, 3)
        torch.cuda.synchronize()
        assert util.launched(det) == ["recordings_levels_out_kernel"]
        # rows of one tile: no reading can cross workgroups, nothing is zeroed first
        with det.recordings([100, 50, 0, 7]) as small:
            small.levels(torch.zeros((C, small.rowSamples), device="cuda"), 8, 3)
            torch.cuda.synchronize()
            assert util.launched(det) == ["recordings_levels_in_kernel"]
    finally:
        det.profile(False)


def test_a_changed_pair_gives_the_new_pairs_results(bank132):
    b = bank132
    out, outh = _packed_run(b)
    rows = torch.from_numpy(b.rows_f32).cuda()
    pairs = [(32, 3), (8, 16), (32, 16), (4096, 1)]
    want_in = {p: lref.input_each(b.rec.slots, b.rows_f32, *p) for p in pairs}
    want_out = {p: lref.output_each(b.rec.slots, outh, 0, p[0], p[1], b.clock) for p in pairs}
    for _ in range(2):
        for p in pairs:                                                      # the two meters share the kept pair and take turns
            got_in = b.rec.levels(rows, *p)
            got_out = b.rec.outputLevels(out, 0, *p)
            _same(got_in.cpu().numpy(), want_in[p], "input meter, pair %r" % (p,))
            _same(got_out.cpu().numpy(), want_out[p], "output meter, pair %r" % (p,))
    # `out`: a table of the caller's, longer than the readings -- nothing behind them is written
    total = int(b.rec.levelsLayout(32, 3)[-1])
    dst = torch.full((total + 5,), SENTINEL, dtype=torch.float64, device="cuda")
    assert b.rec.levels(rows, 32, 3, out=dst) is dst
    dst = dst.cpu().numpy()
    _same(dst[:total], want_in[(32, 3)], "a table of the caller's")
    assert (dst[total:] == SENTINEL).all()
    for k in range(b.K):
        assert b.rec.levelsView(dst, k, 32, 3).size == -(-(-(-LENGTHS[k] // 32)) // 3)


# ---- the statuses ----
def test_every_refusal_leaves_the_destination_alone(bank132):
    b = bank132
    rec, lib = b.rec, _abi.lib
    out, _ = _packed_run(b)
    rows = torch.from_numpy(b.rows_f32).cuda()
    rows16 = torch.from_numpy(b.rows_s16).cuda()
    total = int(rec.levelsLayout(32, 3)[-1])
    ms = torch.full((total,), SENTINEL, dtype=torch.float64, device="cuda")
    lv = torch.full((total,), SENTINEL, dtype=torch.float32, device="cuda")
    x, q, o, m, l, S = rows.data_ptr(), rows16.data_ptr(), out.data_ptr(), ms.data_ptr(), lv.data_ptr(), rec.rowSamples
    refused = [
        lambda: lib.syldet_recordings_levels_device(None, x, S, 32, 3, m, total, None),
        lambda: lib.syldet_recordings_levels_device(rec._h, None, S, 32, 3, m, total, None),
        lambda: lib.syldet_recordings_levels_device(rec._h, x, S, 32, 3, None, total, None),
        lambda: lib.syldet_recordings_levels_device(rec._h, x, S - 1, 32, 3, m, total, None),
        lambda: lib.syldet_recordings_levels_device_s16(rec._h, q, S - 8, 32, 3, m, total, None),
        lambda: lib.syldet_recordings_levels_device(rec._h, x, S, 12, 3, m, total, None),
        lambda: lib.syldet_recordings_levels_device(rec._h, x, S, 4, 3, m, total, None),
        lambda: lib.syldet_recordings_levels_device_s16(rec._h, q, S, 8192, 3, m, total, None),
        lambda: lib.syldet_recordings_levels_device(rec._h, x, S, 32, 0, m, total, None),
        lambda: lib.syldet_recordings_levels_device_s16(rec._h, q, S, 32, -5, m, total, None),
        lambda: lib.syldet_recordings_levels_device(rec._h, x, S, 32, 3, m, total - 1, None),
        lambda: lib.syldet_recordings_levels_device_s16(rec._h, q, S, 32, 3, m, 0, None),
        lambda: lib.syldet_recordings_levels_device(rec._h, x, S, 32, 1, m, total, None),       # P = 1 needs more than the table holds
        lambda: lib.syldet_recordings_output_levels_device(None, o, 0, 32, 3, l, total, None),
        lambda: lib.syldet_recordings_output_levels_device(rec._h, None, 0, 32, 3, l, total, None),
        lambda: lib.syldet_recordings_output_levels_device(rec._h, o, 0, 32, 3, None, total, None),
        lambda: lib.syldet_recordings_output_levels_device(rec._h, o, -1, 32, 3, l, total, None),
        lambda: lib.syldet_recordings_output_levels_device(rec._h, o, 1, 32, 3, l, total, None),
        lambda: lib.syldet_recordings_output_levels_device(rec._h, o, 0, 48, 3, l, total, None),
        lambda: lib.syldet_recordings_output_levels_device(rec._h, o, 0, 32, 0, l, total, None),
        lambda: lib.syldet_recordings_output_levels_device(rec._h, o, 0, 32, 3, l, total - 1, None),
    ]
    for i, call in enumerate(refused):
        assert call() == _abi.ERR_INVALID_ARGUMENT, "refusal %d" % i
    lib.syldet_recordings_levels_device(rec._h, x, S, 32, 3, m, total - 1, None)
    assert str(total) in _abi.last_error()                                   # how many are needed
    torch.cuda.synchronize()
    assert bool((ms == SENTINEL).all()) and bool((lv == SENTINEL).all())
    with pytest.raises(Exception):
        rec.levels(rows, 32, 3, out=ms[:total - 1])
    with pytest.raises(ValueError):
        rec.levels(rows.double(), 32, 3)
    with pytest.raises(ValueError):
        rec.levels(rows, 33, 3)
    # ... and the same arguments without the fault are taken
    assert lib.syldet_recordings_levels_device(rec._h, x, S, 32, 3, m, total, None) == 0
    assert lib.syldet_recordings_output_levels_device(rec._h, o, 0, 32, 3, l, total, None) == 0
    torch.cuda.synchronize()
    assert not bool((ms == SENTINEL).any()) and not bool((lv == SENTINEL).any())


def test_run_recordings_returns_the_tables_next_to_the_events():
    cfg = util.sample_net()
    tmpl = util.template()
    mono = [synth.syllable_channel(n, tmpl, seed=30 + i, every=4000) for i, n in enumerate([30011, 900])]
    stereo = np.stack([synth.syllable_channel(22222, tmpl, seed=40, every=4000), synth.syllable_channel(22222, tmpl, seed=41, every=4000)], axis=1)
    arrays = [mono[0], stereo, mono[1], np.zeros((0, 2), np.float32)]
    each = [arrays[0], arrays[1][:, 0], arrays[1][:, 1], arrays[2], arrays[3][:, 0], arrays[3][:, 1]]
    with sd.SyllableDetector(cfg, channels=3) as det, sd.SyllableDetector(cfg, channels=1) as one:
        plain = det.runRecordings(arrays, 0.05)
        for L, P in ((32, None), (8, 7)):
            events, tables = det.runRecordings(arrays, 0.05, levels=(L, P))
            assert len(plain) == len(events) == len(each) and sorted(tables) == ["input", "output"]
            for (pi, pv), (ei, ev) in zip(plain, events):
                assert np.array_equal(pi, ei) and np.array_equal(pv, ev)
            for k, x in enumerate(each):
                if x.size == 0:                                              # a recording without samples has no reading
                    assert tables["input"][k].size == 0 and tables["output"][k].size == 0
                    continue
                t = torch.from_numpy(np.ascontiguousarray(x)[None, :]).cuda()
                out = one.run(t)[0] if one.countEvaluations(x.size) > 0 else torch.zeros((1, 0, 1), device="cuda")
                _same(tables["input"][k], one.levels(t, L, P)[0].cpu().numpy(), "runRecordings, input of recording %d" % k)
                _same(tables["output"][k], one.outputLevels(out, x.size, 0, L, P)[0].cpu().numpy(), "runRecordings, output of recording %d" % k)
            assert tables["input"][0].size == one.levelsCount(30011, L, P) > 1 and tables["input"][4].size == 0
        # beside the tracks: events, tracks, tables
        events, tracks, tables2 = det.runRecordings(arrays, 0.05, tracks=("ttl",), levels=(8, 7))
        assert sorted(tracks) == ["ttl"] and all(np.array_equal(a, c) for a, c in zip(tables2["output"], tables["output"]))
        # recordings that are all shorter than one evaluation still have an input level; 16-bit arrays
        short = [np.full(50, 16384, np.int16), np.full(9, -32768, np.int16)]
        events, tables = det.runRecordings(short, levels=(8, 2))
        assert all(i.size == 0 for i, _ in events)
        assert np.array_equal(tables["input"][0], np.full(4, 0.25)) and np.array_equal(tables["input"][1], np.full(1, 1.0))
        assert np.array_equal(tables["output"][0], np.zeros(4, np.float32))
