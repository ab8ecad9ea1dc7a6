"""Packed recordings on the GPU: the rows recordings_load_kernel lays out, element for element; each recording's outputs and
flags out of the packed run, bit for bit those of a run of that recording alone (the routes whose position independence
tests/test_ingest_gpu.py and tests/test_sharded_gpu.py hold: the fold kernel, the generic engine, the 1024-point kernel -- the
pass-scaled kernels and the wide engine keep their 1e-5 / 1e-2 contract instead, include/syldet.h); each recording's debounced
events and their values out of the packed flags; runRecordings."""
import numpy as np
import pytest
import torch

import pyoracle as po
import recordings_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth

pytestmark = pytest.mark.gpu

# K = 9 on C = 3: the longest about 20 000 samples, one without samples, one shorter than a window, one of exactly one
# evaluation of the sample network, a multiple of hop 132, odd lengths
LENGTHS = [20003, 0, 100, 1444, 5280, 7777, 1575, 12001, 333]
STEPS = [1, 2, 3, 1, 2, 3, 1, 2, 3]


def _hop131(base):
    return nets.variant(base, windowOverlap=base.windowLength - 131)


def _sources(lengths, steps, dtype, first):
    """-> (src, offsets): a 1-D source of distinct non-zero values, recording k at offsets[k] with step steps[k]; `first`
    makes the offsets odd or even in turn"""
    rng = np.random.default_rng(5)
    offsets, pos = [], first
    for k, (n, s) in enumerate(zip(lengths, steps)):
        offsets.append(pos)
        pos += n * s + (k % 2)                              # (the next one starts at the other parity every second time)
    if dtype == np.int16:
        src = rng.integers(1, 32767, size=pos + 8).astype(np.int16) * rng.choice([-1, 1], size=pos + 8).astype(np.int16)
    else:
        src = (rng.uniform(0.1, 1.0, size=pos + 8) * rng.choice([-1.0, 1.0], size=pos + 8)).astype(np.float32)
    return src, offsets


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("hop", [132, 131])
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_rows_equal_the_model_element_for_element(dtype, hop, aligned):
    cfg = util.sample_net() if hop == 132 else _hop131(util.sample_net())
    assert ref.clock(cfg)[0] == hop
    C = 3
    bits = np.uint32 if dtype == np.float32 else np.uint16
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(LENGTHS) as rec:
        want_plan = ref.plan(LENGTHS, *ref.clock(cfg)[:3], C)
        assert (rec.slots, rec.rowSamples, rec.rowEvaluations, rec.fill) == want_plan
        assert det.planRecordings(LENGTHS) == want_plan
        sentinel = dtype(77)
        tdtype = torch.float32 if dtype == np.float32 else torch.int16
        # aligned: rows of whole 16 bytes, base and stride (the wide stores); else a base one element off and an odd stride (the
        # plain kernel); `stride` elements of each row are handed over, of which the call may write the first rowSamples
        stride = rec.rowSamples + (16 if aligned else 9)
        for first in (0, 1):                                # even and odd source offsets (and a second load: new sources)
            src, offsets = _sources(LENGTHS, STEPS, dtype, first)
            assert {o % 2 for o in offsets} == {0, 1}
            if first == 0:                                  # contiguous recordings at whole 16 bytes (wide reads) and not
                assert {(o * src.itemsize) % 16 == 0 for o, s in zip(offsets, STEPS) if s == 1} == {True, False}
            big = torch.full((C, stride + (8 if aligned else 1)), sentinel.item(), dtype=tdtype, device="cuda")
            out = big[:, :stride] if aligned else big[:, 1:]
            assert (out.data_ptr() % 16 == 0 and (out.stride(0) * src.itemsize) % 16 == 0) == aligned
            for _ in range(2):                              # (the second time with the kept sources: a launch only)
                got = rec.load(torch.from_numpy(src).cuda(), offsets, STEPS, out=out)
            assert got is out
            torch.cuda.synchronize()
            want = ref.rows(rec.slots, rec.rowSamples, C, src, offsets, STEPS, sentinel, stride)
            assert np.array_equal(out.cpu().numpy().view(bits), want.view(bits))   # (+0 in the pads, the sentinels beyond row_samples)
            rest = big.cpu().numpy()
            assert (rest[:, stride:] == sentinel).all() if aligned else (rest[:, 0] == sentinel).all()
        # steps None: all 1, into rows of the call's own
        src, offsets = _sources(LENGTHS, [1] * 9, dtype, 0)
        got = rec.load(torch.from_numpy(src).cuda(), offsets)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().view(bits), ref.rows(rec.slots, rec.rowSamples, C, src, offsets, [1] * 9).view(bits))
        with pytest.raises(ValueError):
            rec.load(torch.from_numpy(src).cuda(), [o + src.size for o in offsets])       # outside the source
        st = _abi.lib.syldet_recordings_load_device(rec._h, 1, np.zeros(9, np.int64).ctypes.data_as(_abi.c_int64_p), None, 1, rec.rowSamples - 1, None)
        assert st == _abi.ERR_INVALID_ARGUMENT                                             # channel_stride below row_samples


def _quantise(x):
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def _alone(det1, x):
    """(outputs [E, n_out], flags [E]) of a 1-channel detector on recording x alone (fp32 or int16)"""
    t = torch.from_numpy(np.ascontiguousarray(x)[None, :]).cuda()
    out, fl = (det1.runPCM16 if x.dtype == np.int16 else det1.run)(t)
    return out[0], fl[0]


def _check_values(make_bank, make_one, lengths, networks, s16, fold=False):
    rng = np.random.default_rng(9)
    recs = [synth.channel(n, 40 + k) * np.float32(rng.uniform(0.2, 1.0)) for k, n in enumerate(lengths)]
    if s16:
        recs = [_quantise(x) for x in recs]
    offsets = np.cumsum([0] + [x.size + 3 for x in recs])[:-1]           # (sources at odd and even offsets)
    src = np.zeros(int(offsets[-1]) + recs[-1].size + 8, recs[0].dtype)
    for o, x in zip(offsets, recs):
        src[o:o + x.size] = x
    with make_bank() as det, det.recordings(lengths, networks) as rec:
        rows = rec.load(torch.from_numpy(src).cuda(), offsets)
        out, fl = (det.runPCM16 if s16 else det.run)(rows)
        torch.cuda.synchronize()
        if fold:
            assert det.lastFusedForm()[0] == 2                            # the symmetric-fold kernel ran
        assert out.shape[1] == rec.rowEvaluations
        ones = {}
        seen = 0
        for k, x in enumerate(recs):
            net = 0 if networks is None else networks[k]
            if net not in ones:
                ones[net] = make_one(net)
            n_evals = rec.slots[k][3]
            assert tuple(rec.view(fl, k).shape) == (n_evals,) and tuple(rec.view(out, k).shape) == (n_evals, out.shape[2])
            if n_evals == 0:
                continue
            o1, f1 = _alone(ones[net], x)
            torch.cuda.synchronize()
            assert o1.shape[0] == n_evals
            assert torch.equal(rec.view(out, k), o1), "recording %d: outputs differ from the run alone" % k
            assert torch.equal(rec.view(fl, k), f1), "recording %d: flags differ from the run alone" % k
            assert rec.view(out, k).data_ptr() == out[rec.slots[k][0], rec.slots[k][2]].data_ptr()      # no copy
            seen += 1
        for d in ones.values():
            d.close()
        assert seen >= 4


@pytest.mark.parametrize("s16", [False, True])
@pytest.mark.parametrize("route", ["fold", "generic", "config3", "multi"])
def test_each_recording_has_the_values_of_its_own_run(route, s16):
    base = util.sample_net()
    if route == "config3":
        cfg = nets.config3()
        lengths = [2 * n for n in LENGTHS]                                # 1024-point frames: lengths scaled to them
        _check_values(lambda: sd.SyllableDetector(cfg, channels=3), lambda net: sd.SyllableDetector(cfg, channels=1), lengths, None, s16)
    elif route == "multi":
        cfgs = [base, nets.perturbed(base, 1)]
        networks = [k % 2 for k in range(len(LENGTHS))]
        _check_values(lambda: sd.SyllableDetector.multi(cfgs, [0, 1, 0]), lambda net: sd.SyllableDetector(cfgs[net], channels=1), LENGTHS, networks, s16,
                      fold=True)
    else:
        engine = _abi.ENGINE_AUTO if route == "fold" else _abi.ENGINE_GENERIC
        _check_values(lambda: sd.SyllableDetector(base, channels=3, engine=engine), lambda net: sd.SyllableDetector(base, channels=1, engine=engine),
                      LENGTHS, None, s16, fold=route == "fold")


HOP = 132


@pytest.fixture(scope="module")
def boundary_case():
    """Four recordings on two rows such that recording A fires within its last 20 evaluations, B -- the next on A's row -- within
    its first 20, and an evaluation between them (A ends with the first five hops of a syllable, B starts with the rest: the
    rows hold it whole) would be flagged if it were read.  All three hold on the CPU oracle before the GPU is asked."""
    cfg = util.sample_net()
    o = util.oracle_for(cfg)
    tmpl = util.template()
    rng = np.random.default_rng(3)
    syl = synth.syllable(tmpl, HOP, 256, 12, 256, rng, amplitude=0.5).astype(np.float32)
    cut = 5 * HOP

    def noise(n, seed):
        return (0.01 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)

    A = noise(150 * HOP, 1)
    A[125 * HOP:125 * HOP + syl.size] += syl
    A[-cut:] += syl[:cut]
    B = noise(110 * HOP, 2)
    B[:syl.size - cut] += syl[cut:]
    B[8 * HOP:8 * HOP + syl.size] += syl
    B[60 * HOP:60 * HOP + syl.size] += syl                  # (a second one: B overflows a capacity of 1, and 1 s of debounce hides it)
    D = synth.syllable_channel(160 * HOP, tmpl, seed=21)
    F = synth.syllable_channel(100 * HOP + 57, tmpl, seed=22)
    recs = [A, B, D, F]
    flags = [o.run(x, po.F64, cfg.rule)[1].astype(np.uint8) for x in recs]
    assert flags[0][-20:].any() and flags[1][:20].any()
    row = o.run(np.concatenate([A, B]), po.F64, cfg.rule)[1]
    assert row[len(flags[0]):150].any()                     # evaluations [140, 150) of the row belong to nobody
    return cfg, recs, flags


def test_events_restart_at_every_recording(boundary_case):
    cfg, recs, oracle_flags = boundary_case
    lengths = [x.size for x in recs]
    src = np.concatenate(recs)
    offsets = np.cumsum([0] + lengths)[:-1]
    first_index = ref.clock(cfg)[3]
    with sd.SyllableDetector(cfg, channels=2) as det, sd.SyllableDetector(cfg, channels=1) as one, det.recordings(lengths) as rec:
        (rowA, offA, firstA, evalsA, _), (rowB, offB, firstB, _, _) = rec.slots[0], rec.slots[1]
        assert rowA == rowB and offB == offA + lengths[0] and firstA + evalsA < firstB
        out, fl = det.run(rec.load(torch.from_numpy(src).cuda(), offsets))
        torch.cuda.synchronize()
        assert det.lastFusedForm()[0] == 2
        flh, outh = fl.cpu().numpy(), out.cpu().numpy()
        own = [rec.view(fl, k).cpu().numpy() for k in range(4)]
        assert own[0][-20:].any() and own[1][:20].any()
        assert flh[rowA, firstA + evalsA:firstB].any(), "no junk evaluation between A and B is flagged: the test would be vacuous"
        for debounce in (0.0, 0.05, 1.0):
            idx, val, cnt = rec.events(out, fl, debounce)
            torch.cuda.synchronize()
            idx, val, cnt = idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()
            for k in range(4):
                hi, hc = one.detectionsHost(own[k], debounce)
                n = int(hc[0])
                assert n == cnt[k] and np.array_equal(idx[k, :n], hi[0, :n])
                mi, me = ref.events(own[k], first_index, HOP, int(debounce * cfg.samplingRate))
                assert np.array_equal(idx[k, :n], mi)
                row, _, first, _, _ = rec.slots[k]
                assert np.array_equal(val[k, :n].view(np.uint32), outh[row, first + me].view(np.uint32))
            assert cnt[0] >= 1 and cnt[1] >= 1
            # B's first detection is its own first flag, whatever A's last detection left of its debounce
            assert idx[1, 0] == first_index + int(np.nonzero(own[1])[0][0]) * HOP
            assert idx[1, 0] + offB < idx[0, cnt[0] - 1] + offA + int(debounce * cfg.samplingRate) or debounce < 1.0
            if debounce == 0.0:
                full = cnt.copy()
                assert full[1] >= 2
            if debounce == 1.0:
                assert cnt[1] == 1                          # ... B's second detection, 52 evaluations behind its first
        # a small capacity: the counts are what would have been written; indices only (no outputs, no values)
        idx1, val1, cnt1 = rec.events(None, fl, 0.0, capacity=1)
        torch.cuda.synchronize()
        assert val1 is None and np.array_equal(cnt1.cpu().numpy(), full) and tuple(idx1.shape) == (4, 1)
        idx0, _, _ = rec.events(out, fl, 0.0)
        assert np.array_equal(idx1.cpu().numpy()[:, 0][full > 0], idx0.cpu().numpy()[:, 0][full > 0])
        st = _abi.lib.syldet_recordings_events_device(rec._h, out.data_ptr(), fl.data_ptr(), 0.0, idx1.data_ptr(), None, 1, cnt1.data_ptr(), None)
        assert st == _abi.ERR_INVALID_ARGUMENT                                # outputs without values


@pytest.mark.parametrize("s16", [False, True])
def test_run_recordings_on_mono_and_stereo_arrays(s16):
    cfg = util.sample_net()
    tmpl = util.template()
    mono = [synth.syllable_channel(n, tmpl, seed=30 + i) for i, n in enumerate([30011, 900, 14000])]
    stereo = np.stack([synth.syllable_channel(22222, tmpl, seed=40), synth.syllable_channel(22222, tmpl, seed=41)], axis=1)
    arrays = [mono[0], stereo, mono[1], mono[2], np.zeros((0, 2), np.float32)]
    if s16:
        arrays = [_quantise(a) for a in arrays]
    tracks = [arrays[0], arrays[1][:, 0], arrays[1][:, 1], arrays[2], arrays[3], arrays[4][:, 0], arrays[4][:, 1]]
    for debounce in (0.0, 0.05):
        with sd.SyllableDetector(cfg, channels=3) as det, sd.SyllableDetector(cfg, channels=1) as one:
            got = det.runRecordings(arrays, debounce)
            assert len(got) == len(tracks)
            total = 0
            for (gi, gv), x in zip(got, tracks):
                if one.countEvaluations(x.size) <= 0:
                    assert gi.size == 0 and gv.shape == (0, 1)
                    continue
                o1, f1 = _alone(one, np.ascontiguousarray(x))
                torch.cuda.synchronize()
                mi, me = ref.events(f1.cpu().numpy(), ref.clock(cfg)[3], HOP, int(debounce * cfg.samplingRate))
                assert np.array_equal(gi, mi) and np.array_equal(gv.view(np.uint32), o1.cpu().numpy()[me].view(np.uint32))
                total += gi.size
            assert total >= 3
