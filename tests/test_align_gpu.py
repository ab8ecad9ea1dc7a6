"""Event-aligned windows on the GPU (syldet_align_device, syldet_align_stats_device; include/syldet.h "event-aligned windows"):
the windows of every recording of a packed bank are, bit for bit, what the numpy model (align_ref.py) cuts out of the downloaded
source array and what a one-channel handle on that recording alone gives for the same events; on multi-network and mixed banks
too; the event table and the flat form give the same bytes; every element of the destination is written and nothing beyond it;
the stack statistics are the model's fixed tree; the launch rule; the statuses; and the packed rows' columns (Recordings.spectrogram,
columnsView).  No tolerance anywhere: the contract is bit identity, NaN at the same places.

The sources of the packed tests hold NaN in every unit outside the recordings: the sample rows in every pad and tail, the columns
and the outputs in every row frame and row evaluation that is not a recording's own (they are made from rows loaded with the pads'
+0, then every such unit is set to NaN -- those that straddle only the next recording of the row too, which NaN rows would leave
finite).  A window that reads one shows it.  One test runs the engines over the NaN rows themselves."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import align_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

pytestmark = pytest.mark.gpu

C = 3
LENGTHS = [0, 255, 256, 387, 388, 1443, 1444, 1575, 1576, 5000, 12001, 30011]
LIMIT = 2 ** 62 - 1
SENTINEL = 77.0
SOURCES = {"columns": ref.COLUMNS, "outputs": ref.OUTPUTS, "samples": ref.SAMPLES}
NAN = np.float32(np.nan)


def _hop131(base):
    return nets.variant(base, windowOverlap=base.windowLength - 131)


def _pairs(T, source):
    return [(0, 0), (T - 1, 0), (0, 5), (7, 9), (300, 300)] + ([(0, 3), (1, 2), (2, 1), (3, 0)] if source == ref.SAMPLES else [])


def _events(cfg, n, seed):
    """the events of a recording of n samples: the fixed ones, and 20 seeded random ones, unsorted and with repeats"""
    hop, need, T, first = ref.clock(cfg)
    last = first + max(ref.count_evals(cfg, n) - 1, 0) * hop
    rnd = np.random.default_rng(seed).integers(-1000, n + 1001, 20)
    rnd[15:] = rnd[:5]
    return [-5000, -1, 0, need - 1, need, first - 1, first, first + hop - 1, first + hop, last, n - 1, n, n + 10 ** 6, LIMIT, -LIMIT] + [int(v) for v in rnd]


def _audio(n, k):
    return (np.random.default_rng(900 + k).standard_normal(n) * (0.02 + 0.05 * (k % 7))).astype(np.float32)


def _make(cfg, make_bank, make_one, networks=None, columns=True):
    det = make_bank()
    rec = det.recordings(LENGTHS, networks)
    nets_of = networks or [0] * len(LENGTHS)
    ones = {net: make_one(net) for net in sorted(set(nets_of))}
    audio = [_audio(n, k) for k, n in enumerate(LENGTHS)]
    slots = rec.slots
    # the rows as a load writes them (+0 outside the recordings) for the engines, and with NaN outside the recordings as a source
    offsets = np.cumsum([0] + [x.size + 3 for x in audio])[:-1]
    flat = np.zeros(int(offsets[-1]) + audio[-1].size + 8, np.float32)
    for o, x in zip(offsets, audio):
        flat[o:o + x.size] = x
    loaded = rec.load(torch.from_numpy(flat).cuda(), offsets)
    rows = np.full((C, rec.rowSamples), NAN, np.float32)
    for (row, offset, _, _, n), x in zip(slots, audio):
        rows[row, offset:offset + n] = x
    host, dev = {ref.SAMPLES: rows}, {}
    out = det.run(loaded)[0]
    cols = rec.spectrogram(loaded) if columns else None
    torch.cuda.synchronize()
    for source, t in ((ref.OUTPUTS, out), (ref.COLUMNS, cols)):
        if t is None:
            continue
        a = t.cpu().numpy()
        own = np.zeros(a.shape[:2], bool)
        for row, _, first, _, n in slots:
            own[row, first:first + ref.units_of(cfg, source, n)] = True
        assert (~own).sum() > 0
        a[~own] = NAN
        host[source] = a
    for source, a in host.items():
        dev[source] = torch.from_numpy(a).cuda()
    # every recording alone, through a one-channel handle of its network
    alone = {source: [] for source in host}
    for k, x in enumerate(audio):
        one = ones[nets_of[k]]
        t = torch.from_numpy(x[None, :].copy()).cuda()
        alone[ref.SAMPLES].append(t)
        E, J = max(one.countEvaluations(x.size), 0), max(one.countFrames(x.size), 0)
        alone[ref.OUTPUTS].append(one.run(t)[0] if E > 0 else torch.zeros((1, 0, one.geometry.outputs), device="cuda"))
        if columns:
            alone[ref.COLUMNS].append(one.spectrogram(t) if J > 0 else torch.zeros((1, 0, one.geometry.bins), device="cuda"))
    torch.cuda.synchronize()
    return SimpleNamespace(cfg=cfg, det=det, rec=rec, ones=ones, networks=nets_of, K=len(LENGTHS), slots=slots, audio=audio, host=host, dev=dev,
                           alone=alone, cols=cols, events=[_events(cfg, n, 77 + k) for k, n in enumerate(LENGTHS)], hop=ref.clock(cfg)[0],
                           T=cfg.timeRange)


def _close(b):
    b.rec.close()
    b.det.close()
    for d in b.ones.values():
        d.close()


_BANKS = {}


def _bank(hop):
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


def _model(b, source, before, after):
    """(windows with NaN fill, present, event_begin) of every recording's events, from the downloaded packed array"""
    origin, step = ref.anchor(b.cfg, source)
    units = [ref.detector_units(b.host[source], source, slot, b.cfg) for slot in b.slots]
    return ref.windows_each(units, b.events, origin, step, before, after, NAN)


def _guarded(N, n, width, shift):
    """a destination inside a block of sentinels, `shift` floats behind a 16-byte line: (block, out view, first element)"""
    L = N * n * width
    block = torch.full((64 + L + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    first = 60 + shift
    return block, block[first:first + L].view(N, n, width), first


def _check_packed(b, sources, pairs_of, fills=(np.float32(-7.0), NAN)):
    """packed windows against the model and against every recording alone, for every (before, after) and fill"""
    for source in sources:
        models = {pair: _model(b, source, *pair) for pair in pairs_of(source)}
        # the model must itself produce windows in each of the five states, or an all-fill result could pass
        seen = dict.fromkeys(("whole", "left", "right", "both", "absent"), 0)
        for _, present, _ in models.values():
            for key, v in ref.states(present).items():
                seen[key] += v
        assert all(v > 0 for v in seen.values()), (source, seen)
        for i, (pair, (want_nan, present, begin)) in enumerate(models.items()):
            before, after = pair
            ones = {net: d.aligner(source, before, after) for net, d in b.ones.items()}
            with b.rec.aligner(source, before, after) as al:
                N, n, width = int(begin[-1]), al.shape[1], al.shape[2]
                assert al.shape[0] == b.K and n == before + after + 1 and want_nan.shape == (N, n, width)
                for fill in fills:
                    want = np.where(present, want_nan, fill).astype(np.float32)
                    block, out, first = _guarded(N, n, width, i % 4)
                    assert al.windows(b.dev[source], b.events, fill=float(fill), out=out) is out
                    assert np.array_equal(al.eventBegin, begin)
                    got = block.cpu().numpy()
                    what = "hop %d, source %d, (%d, %d), fill %r" % (b.hop, source, before, after, float(fill))
                    ref.same(got[first:first + want.size].reshape(want.shape), want, what + ", against the model")
                    # every element was written, nothing beyond them
                    assert (got[:first] == SENTINEL).all() and (got[first + want.size:] == SENTINEL).all(), what
                    assert not (got[first:first + want.size] == SENTINEL).any(), what
                    # every recording alone: its own array through a one-channel handle, r = NULL
                    packed = got[first:first + want.size].reshape(want.shape)
                    for k in range(b.K):
                        own = ones[b.networks[k]].windows(b.alone[source][k], [b.events[k]], fill=float(fill)).cpu().numpy()
                        ref.same(packed[begin[k]:begin[k + 1]], own, what + ", recording %d alone" % k)
            for one in ones.values():
                one.close()


@pytest.mark.parametrize("name", list(SOURCES))
def test_packed_windows_are_the_models_and_every_recordings_alone(bank, name):
    b = bank
    # rows that hold several recordings back to back, recordings without a frame, with frames but no evaluation, with exactly one
    assert max(sum(s[0] == row and s[4] > 0 for s in b.slots) for row in range(C)) >= 3
    frames = [ref.count_frames(b.cfg, s[4]) for s in b.slots]
    assert 0 in frames and 1 in frames and any(f > 0 and s[3] == 0 for f, s in zip(frames, b.slots)) and any(s[3] == 1 for s in b.slots)
    _check_packed(b, [SOURCES[name]], lambda source: _pairs(b.T, source))


def test_rows_that_hold_nan_outside_the_recordings_through_the_engines(bank):
    """The issue's own recipe, once: the sample rows hold NaN everywhere outside the recordings and go through
    syldet_spectrogram_device and syldet_run_device as they are, so the row frames and row evaluations that read a pad come out NaN by
    themselves, and the windows are the model's on the downloaded arrays, bit for bit.
    The engines' own values are NOT held to bit identity with the recording alone here, and cannot be: the fold kernel's precision
    guard sends what lies next to a non-finite sample through the exact recomputation (include/syldet.h says so where it states that
    a load writes +0 into the pads), and a recording's own evaluation then carries the exact path's bits, not the fast path's -- on
    the MI355X recording 6's one evaluation at hop 132 came out -0.00048953295 against -0.00048965216 alone.  They are held to the
    library's 1e-5 (tests/util.py); bit identity of the packed columns and outputs is held on rows with +0 pads, by every other test
    of this file."""
    b = bank
    rows = b.dev[ref.SAMPLES]
    cols, out = b.rec.spectrogram(rows), b.det.run(rows)[0]
    torch.cuda.synchronize()
    host = {ref.COLUMNS: cols.cpu().numpy(), ref.OUTPUTS: out.cpu().numpy()}
    differing = 0
    for k in range(b.K):
        own_cols, own_out = b.rec.columnsView(host[ref.COLUMNS], k), b.rec.view(host[ref.OUTPUTS], k)
        alone_cols, alone_out = b.alone[ref.COLUMNS][k][0].cpu().numpy(), b.alone[ref.OUTPUTS][k][0].cpu().numpy()
        assert not np.isnan(own_cols).any() and not np.isnan(own_out).any(), k
        differing += int((own_cols.view(np.uint32) != alone_cols.view(np.uint32)).sum()) + int((own_out.view(np.uint32) != alone_out.view(np.uint32)).sum())
        if own_cols.size:
            util.assert_columns_close(own_cols, alone_cols)
        if own_out.size:
            util.assert_outputs_close(own_out, alone_out)
    print("hop %d: %d own values differ in bits from the recordings alone under NaN pads" % (b.hop, differing))
    assert np.isnan(host[ref.COLUMNS]).any() and np.isnan(host[ref.OUTPUTS]).any()         # the junk between the recordings shows
    for source, array in ((ref.COLUMNS, cols), (ref.OUTPUTS, out)):
        origin, step = ref.anchor(b.cfg, source)
        units = [ref.detector_units(host[source], source, slot, b.cfg) for slot in b.slots]
        want, present, _ = ref.windows_each(units, b.events, origin, step, 7, 9, np.float32(-7.0))
        with b.rec.aligner(source, 7, 9) as al:
            got = al.windows(array, b.events, fill=-7.0).cpu().numpy()
        ref.same(got, want, "hop %d, source %d, from NaN rows" % (b.hop, source))
        assert not np.isnan(got).any() and present.any() and not present.all()


def test_the_geometry_of_the_sample_network_is_what_the_issue_says(bank132):
    hop, need, T, first = ref.clock(bank132.cfg)
    assert (hop, need, T, first) == (132, 256, 10, 1444) and ref.clock(_bank(131).cfg) == (131, 256, 10, 1435)
    g = bank132.det.geometry
    for source, (origin, step, width) in ((ref.COLUMNS, (need, hop, g.bins)), (ref.OUTPUTS, (first, hop, g.outputs)), (ref.SAMPLES, (0, 1, 1))):
        o, s, w = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        assert _abi.lib.syldet_align_anchor(bank132.det._h, source, ctypes.byref(o), ctypes.byref(s), ctypes.byref(w)) == 0
        assert (o.value, s.value, w.value) == (origin, step, width) and ref.anchor(bank132.cfg, source) == (origin, step)


@pytest.mark.parametrize("kind", ["multi", "mixed"])
def test_banks_of_several_networks(kind):
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
    b = _make(cfgs[0], make, lambda n: sd.SyllableDetector(cfgs[n], channels=1), networks, columns=kind == "multi")
    try:
        assert {b.slots[k][0] for k in range(b.K) if networks[k] == 1} == {1}                    # recordings on the rows of their networks
        sources = [ref.COLUMNS, ref.OUTPUTS, ref.SAMPLES] if kind == "multi" else [ref.OUTPUTS, ref.SAMPLES]
        _check_packed(b, sources, lambda source: [(b.T - 1, 0), (7, 9), (300, 300)] + ([(1, 2)] if source == ref.SAMPLES else []), fills=(NAN,))
        if kind == "mixed":
            for r in (None, b.rec._h):
                h = _abi.Handle()
                assert _abi.lib.syldet_aligner_create(b.det._h, r, ref.COLUMNS, 1, 1, ctypes.byref(h)) == _abi.ERR_UNSUPPORTED and not h
            assert _abi.lib.syldet_align_anchor(b.det._h, ref.COLUMNS, None, None, None) == _abi.ERR_UNSUPPORTED
            with pytest.raises(sd.SyllableDetectorError):
                b.rec.aligner("columns", 1, 1)
    finally:
        _close(b)


def test_the_event_table_and_the_flat_form_give_the_same_bytes(bank132):
    b = bank132
    cap = 41
    table = np.full((b.K, cap), 12345, np.int64)
    counts = np.array([len(e) for e in b.events], np.int64)
    for k, e in enumerate(b.events):
        table[k, :len(e)] = e
    d_table = torch.from_numpy(table).cuda()
    d_flat = torch.from_numpy(np.concatenate([np.asarray(e, np.int64) for e in b.events])).cuda()
    for name, pair in (("columns", (7, 9)), ("samples", (2, 1))):
        with b.rec.aligner(name, *pair) as al:
            src = b.dev[SOURCES[name]]
            listed = al.windows(src, b.events).cpu().numpy()
            ref.same(al.windows(src, d_table, counts=counts).cpu().numpy(), listed, "the [D][capacity] table")
            ref.same(al.windows(src, d_table, counts=torch.from_numpy(counts).cuda()).cpu().numpy(), listed, "counts on the device")
            ref.same(al.windows(src, d_flat, counts=counts).cpu().numpy(), listed, "the flat form")
            # a count beyond the capacity means the capacity, as the detection calls' counts do
            few = al.windows(src, d_table[:, :7].contiguous(), counts=counts).cpu().numpy()
            want = np.concatenate([listed[i:i + 7] for i in np.concatenate([[0], np.cumsum(counts)[:-1]])])
            ref.same(few, want, "counts beyond the capacity")


def test_a_banks_channels_and_the_detection_calls_tables(bank132):
    """r = NULL: a detector is a channel.  The (indices, counts) pair of detections() goes in as it is; with before = T - 1 and
    after = 0 a detection's COLUMNS window is the network's input in spectrogram values."""
    b = bank132
    det, T = b.det, b.T
    x = torch.from_numpy(np.stack([_audio(20000, 50 + c) for c in range(C)])).cuda()
    cols, (out, _) = det.spectrogram(x), det.run(x)
    # flags of our own: every 7th evaluation of channel 0, none of channel 1, all of channel 2 (more than the capacity)
    E = out.shape[1]
    flags = torch.zeros((C, E), dtype=torch.uint8, device="cuda")
    flags[0, ::7] = 1
    flags[2, :] = 1
    idx, cnt = det.detections(flags, capacity=40)
    colsh, idxh, cnth = cols.cpu().numpy(), idx.cpu().numpy(), np.minimum(cnt.cpu().numpy(), 40)
    assert cnth.tolist() == [min(40, -(-E // 7)), 0, 40]
    with det.aligner("columns", T - 1, 0) as al:
        assert al.shape == (C, T, det.geometry.bins)
        got = al.windows(cols, idx, counts=cnt).cpu().numpy()
        hop, _, _, first = ref.clock(b.cfg)
        at = 0
        for c in range(C):
            for j in range(cnth[c]):
                e = (idxh[c, j] - first) // hop
                ref.same(got[at], colsh[c, e:e + T], "channel %d, detection %d" % (c, j))
                at += 1
        assert at == got.shape[0] > 0
        count, total, _ = al.stats(torch.from_numpy(got).cuda(), groups=[0, 1, 0], groupCount=2)
        assert (count[0].cpu().numpy() == at).all() and (count[1].cpu().numpy() == 0).all() and (total[1].cpu().numpy() == 0).all()
    with det.aligner("outputs", 2, 2) as al, det.aligner("samples", 0, 3) as als:
        want, _, _ = ref.windows_each([out.cpu().numpy()[c] for c in range(C)], [idxh[c, :cnth[c]] for c in range(C)], first, hop, 2, 2, NAN)
        ref.same(al.windows(out, idx, counts=cnt).cpu().numpy(), want, "outputs of a bank's channels")
        want, _, _ = ref.windows_each([x.cpu().numpy()[c] for c in range(C)], [idxh[c, :cnth[c]] for c in range(C)], 0, 1, 0, 3, NAN)
        # rows of a wider tensor: row_stride > n_units
        wide = torch.zeros((C, 20000 + 24), device="cuda")
        wide[:, :20000] = x
        ref.same(als.windows(wide[:, :20000], idx, counts=cnt).cpu().numpy(), want, "samples of a bank's channels")


# ---- the stack statistics ----
def _spread(total, parts):
    return [total // parts + (i < total % parts) for i in range(parts)]


def _stack_events(b, counts):
    """counts[k] events of recording k, by repeating its own events"""
    return [[b.events[k][i % len(b.events[k])] for i in range(c)] for k, c in enumerate(counts)]


@pytest.mark.parametrize("name,pair", [("columns", (7, 9)), ("samples", (1, 2))])
def test_the_statistics_are_the_models_tree(bank132, name, pair):
    b = bank132
    source = SOURCES[name]
    origin, step = ref.anchor(b.cfg, source)
    small = [k for k in range(b.K) if 0 < LENGTHS[k] <= 5000]
    # a source with one NaN inside a recording
    host = b.host[source].copy()
    k_nan = LENGTHS.index(5000)
    row, offset, first_eval, _, _ = b.slots[k_nan]
    if source == ref.COLUMNS:
        host[row, first_eval + 12, 3] = NAN                                   # (the event first_index anchors at frame 9: frames 2 .. 18)
    else:
        host[row, offset + ref.clock(b.cfg)[3]] = NAN                         # (the sample of the event first_index)
    src = torch.from_numpy(host).cuda()
    units = [ref.detector_units(host, source, slot, b.cfg) for slot in b.slots]
    cases = [([n], 1) for n in (1, 255, 256, 257, 513)] + [([255, 256, 513], 3), ([1, 0, 257], 3)]
    seen_nan = False
    with b.rec.aligner(name, *pair) as al:
        for sizes, G in cases:
            # G = 1: the events spread over the small recordings; G = 3: interleaved group numbers, group g on the recordings k = g mod 3
            group = np.zeros(b.K, np.int32) if G == 1 else (np.arange(b.K) % 3).astype(np.int32)
            counts = [0] * b.K
            for g, size in enumerate(sizes):
                members = [k for k in small if group[k] == g]
                for k, c in zip(members, _spread(size, len(members))):
                    counts[k] = c
            if k_nan in small and G == 1 and sizes[0] >= 255:
                assert counts[k_nan] > 0
            events = _stack_events(b, counts)
            want_nan, present, begin = ref.windows_each(units, events, origin, step, pair[0], pair[1], NAN)
            model = None
            for fill in (NAN, np.float32(0.0)):
                w = al.windows(src, events, fill=float(fill))
                ref.same(w.cpu().numpy(), np.where(present, want_nan, fill).astype(np.float32), "%s, the windows of %r" % (name, sizes))
                got = [t.cpu().numpy() for t in al.stats(w, groups=group, groupCount=G)]
                want = ref.stats(np.where(present, want_nan, fill).astype(np.float32), present, begin, group, G)
                for a, m, what in zip(got, want, ("count", "sum", "sumsq")):
                    ref.same(a, m, "%s, %s of groups %r, fill %r" % (name, what, sizes, float(fill)))
                # the count goes by presence, not by value: the same under either fill, and the sums too (absent elements add nothing)
                if model is not None:
                    for a, m in zip(got, model):
                        ref.same(a, m, "the two fills")
                model = got
                assert np.array_equal(got[0].sum(axis=0), present.sum(axis=0).reshape(got[0].shape[1:]))
                for g, size in enumerate(sizes):
                    assert got[0][g].max() <= size
            # the NaN reaches the sums at exactly the positions of the windows that hold it
            holds = np.isnan(want_nan) & present
            seen_nan |= bool(holds.any())
            if holds.any():
                where = np.zeros(got[1].shape, bool)
                for d in range(b.K):
                    where[group[d]] |= holds[begin[d]:begin[d + 1]].any(axis=0)
                assert np.array_equal(np.isnan(got[1]), where) and np.array_equal(np.isnan(got[2]), where) and not where.all()
    assert seen_nan


# ---- the launch rule ----
def test_the_same_arrays_again_are_launches_only(bank132):
    b = bank132
    det = b.det
    out = torch.empty((sum(len(e) for e in b.events), 17, det.geometry.bins), device="cuda")
    d_flat = torch.from_numpy(np.concatenate([np.asarray(e, np.int64) for e in b.events])).cuda()
    counts = np.array([len(e) for e in b.events], np.int64)
    det.profile(True)
    try:
        with b.rec.aligner("columns", 7, 9) as al:
            for _ in range(2):
                al.windows(b.dev[ref.COLUMNS], d_flat, counts=counts, out=out)
            torch.cuda.synchronize()
            names = det.lastTimings()
            assert [n for n, _ in names] == ["align_windows_kernel"] and all(ms > 0 for _, ms in names)
            first = out.cpu().numpy()
            for _ in range(2):
                stats = al.stats(out, groups=np.arange(b.K) % 3)
            torch.cuda.synchronize()
            assert util.launched(det) == ["align_stats_kernel", "align_combine_kernel"]
            # other counts, then the first ones again: each gives its own results
            half = counts // 2
            al.windows(b.dev[ref.COLUMNS], d_flat, counts=half)
            again = al.windows(b.dev[ref.COLUMNS], d_flat, counts=counts)
            ref.same(again.cpu().numpy(), first, "the first arrays again")
            for a, m in zip(al.stats(again, groups=np.arange(b.K) % 3), stats):
                ref.same(a.cpu().numpy(), m.cpu().numpy(), "the statistics again")
        # long windows go to workgroups, short ones to waves: one kernel name either way
        with b.rec.aligner("columns", 300, 300) as al:
            al.windows(b.dev[ref.COLUMNS], d_flat, counts=counts)
            torch.cuda.synchronize()
            assert util.launched(det) == ["align_windows_kernel"]
    finally:
        det.profile(False)


# ---- the statuses ----
def test_every_refusal_leaves_the_destination_alone(bank132):
    b = bank132
    lib, rec, det = _abi.lib, b.rec, b.det
    cols, rows = b.dev[ref.COLUMNS], b.dev[ref.SAMPLES]
    J, S, bins = cols.shape[1], rec.rowSamples, det.geometry.bins
    counts = np.array([len(e) for e in b.events], np.int64)
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N = int(begin[-1])
    ev = torch.from_numpy(np.concatenate([np.asarray(e, np.int64) for e in b.events])).cuda()
    dst = torch.full((N * 3 * bins,), SENTINEL, dtype=torch.float32, device="cuda")
    p64 = lambda a: a.ctypes.data_as(_abi.c_int64_p)
    p32 = lambda a: a.ctypes.data_as(_abi.c_int32_p)
    h = _abi.Handle()
    for args in ((det._h, rec._h, 3, 1, 1), (det._h, rec._h, -1, 1, 1), (det._h, rec._h, 0, -1, 1), (det._h, rec._h, 0, 1, -1),
                 (det._h, rec._h, 0, 2 ** 20, 0), (det._h, rec._h, 2, 2 ** 19, 2 ** 19), (det._h, None, 0, 20000, 20000)):
        assert lib.syldet_aligner_create(*args, ctypes.byref(h)) == _abi.ERR_INVALID_ARGUMENT and not h, args
    assert lib.syldet_aligner_create(det._h, rec._h, 2, 2 ** 19, 2 ** 19 - 1, ctypes.byref(h)) == 0      # exactly 2^20 elements
    assert lib.syldet_aligner_destroy(h) == 0
    with rec.aligner("columns", 1, 1) as al, rec.aligner("samples", 1, 1) as als:
        a, c, e, d = al._h, cols.data_ptr(), ev.data_ptr(), dst.data_ptr()
        bad0, down = begin.copy(), begin.copy()
        bad0[0] = 1
        down[5] = down[4] - 1
        group = np.zeros(b.K, np.int32)
        out_of = group.copy()
        out_of[3] = 2
        neg = group.copy()
        neg[0] = -1
        cnt = torch.zeros((3, 3, bins), dtype=torch.int64, device="cuda")                      # (room for the three groups asked for below)
        s1, s2 = torch.zeros((3, 3, bins), dtype=torch.float64, device="cuda"), torch.zeros((3, 3, bins), dtype=torch.float64, device="cuda")
        refused = [
            lambda: lib.syldet_align_device(None, c, J, 0, e, 0, p64(begin), 0.0, d, None),
            lambda: lib.syldet_align_device(a, None, J, 0, e, 0, p64(begin), 0.0, d, None),
            lambda: lib.syldet_align_device(a, c, J, 0, None, 0, p64(begin), 0.0, d, None),
            lambda: lib.syldet_align_device(a, c, J, 0, e, 0, None, 0.0, d, None),
            lambda: lib.syldet_align_device(a, c, J, 0, e, 0, p64(begin), 0.0, None, None),
            lambda: lib.syldet_align_device(a, c, J - 1, 0, e, 0, p64(begin), 0.0, d, None),            # not the rows' frames
            lambda: lib.syldet_align_device(a, c, J + 1, 0, e, 0, p64(begin), 0.0, d, None),
            lambda: lib.syldet_align_device(a, c, -1, 0, e, 0, p64(begin), 0.0, d, None),
            lambda: lib.syldet_align_device(a, c, J, J * bins - 1, e, 0, p64(begin), 0.0, d, None),      # a row needs J x bins elements
            lambda: lib.syldet_align_device(als._h, rows.data_ptr(), S, S - 1, e, 0, p64(begin), 0.0, d, None),
            lambda: lib.syldet_align_device(als._h, rows.data_ptr(), S - 8, 0, e, 0, p64(begin), 0.0, d, None),
            lambda: lib.syldet_align_device(a, c, J, 0, e, 0, p64(bad0), 0.0, d, None),
            lambda: lib.syldet_align_device(a, c, J, 0, e, 0, p64(down), 0.0, d, None),
            lambda: lib.syldet_align_device(a, c, J, 0, e, int(counts.max()) - 1, p64(begin), 0.0, d, None),
            lambda: lib.syldet_align_device(a, c, J, 0, e, -1, p64(begin), 0.0, d, None),
            # the statistics describe the last windows call: there has been none
            lambda: lib.syldet_align_stats_device(a, d, p64(begin), p32(group), 1, cnt.data_ptr(), s1.data_ptr(), s2.data_ptr(), None),
        ]
        for i, call in enumerate(refused):
            assert call() == _abi.ERR_INVALID_ARGUMENT, "refusal %d" % i
        torch.cuda.synchronize()
        assert bool((dst == SENTINEL).all())
        # ... and the same arguments without the fault are taken
        assert lib.syldet_align_device(a, c, J, 0, e, 0, p64(begin), 0.0, d, None) == 0
        assert lib.syldet_align_device(a, c, J, J * bins, e, int(counts.max()), p64(begin), 0.0, d, None) == 0
        torch.cuda.synchronize()
        assert not bool((dst == SENTINEL).any())
        st = lambda *x: lib.syldet_align_stats_device(*x, cnt.data_ptr(), s1.data_ptr(), s2.data_ptr(), None)
        cnt.fill_(-5)
        for i, args in enumerate(((None, d, p64(begin), p32(group), 1), (a, None, p64(begin), p32(group), 1), (a, d, None, p32(group), 1),
                                  (a, d, p64(begin), None, 1), (a, d, p64(begin), p32(group), 0), (a, d, p64(begin), p32(out_of), 2),
                                  (a, d, p64(begin), p32(neg), 2), (a, d, p64(bad0), p32(group), 1), (a, d, p64(down), p32(group), 1),
                                  (a, d, p64((begin // 2 * 2).astype(np.int64)), p32(group), 1))):          # not the last call's event_begin
            assert st(*args) == _abi.ERR_INVALID_ARGUMENT, "statistics refusal %d" % i
        assert lib.syldet_align_stats_device(a, d, p64(begin), p32(group), 2, None, s1.data_ptr(), s2.data_ptr(), None) == _abi.ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert bool((cnt == -5).all())
        assert st(a, d, p64(begin), p32(out_of), 3) == 0 and st(a, d, p64(begin), p32(group), 2) == 0
        torch.cuda.synchronize()
        assert not bool((cnt == -5).any()) and bool((cnt[1] == 0).all())
        # the Python layer's own argument errors
        with pytest.raises(ValueError):
            al.windows(cols.double(), b.events)
        with pytest.raises(ValueError):
            al.windows(cols, b.events[:-1])
        with pytest.raises(ValueError):
            al.windows(cols, ev)                                                                  # a tensor of events needs counts
        with pytest.raises(ValueError):
            al.stats(torch.zeros((3, 3, bins), device="cuda"))
        with pytest.raises(sd.SyllableDetectorError):
            al.windows(cols[:, :-1].contiguous(), b.events)
    # no events at all: nothing is launched, nothing is needed
    with rec.aligner("outputs", 2, 2) as al:
        w = al.windows(b.dev[ref.OUTPUTS], [[] for _ in range(b.K)])
        assert tuple(w.shape) == (0, 5, 1)
        count, total, squares = al.stats(w)
        assert bool((count == 0).all()) and bool((total == 0).all()) and bool((squares == 0).all())


# ---- the packed rows' columns ----
def test_the_packed_rows_columns_are_every_recordings_own(bank):
    b = bank
    colsh = b.cols.cpu().numpy()
    assert b.cols.shape == (C, b.det.countFrames(b.rec.rowSamples), b.det.geometry.bins)
    frames = 0
    for k, n in enumerate(LENGTHS):
        view = b.rec.columnsView(b.cols, k)
        assert view.shape[0] == ref.count_frames(b.cfg, n)
        assert view.shape[0] == 0 or view.data_ptr() == b.cols[b.slots[k][0], b.slots[k][2]:].data_ptr()       # no copy
        ref.same(b.rec.columnsView(colsh, k), b.alone[ref.COLUMNS][k][0].cpu().numpy(), "hop %d, the columns of recording %d" % (b.hop, k))
        frames += view.shape[0]
    assert frames > 300 and sum(ref.count_frames(b.cfg, n) == 0 for n in LENGTHS) == 2 and sum(ref.count_frames(b.cfg, n) == 1 for n in LENGTHS) >= 1
