"""Threshold calibration on the GPU: score_kernel's tables equal the numpy model (tests/score_ref.py) exactly -- on a plain bank,
on a three-output network scored on its last output (the others +inf: a wrong stride fires), on a multi-network bank, on packed
recordings whose rows hold +inf wherever no recording's evaluation lies; at the threshold's edges; tied to detections() on
smoke()'s two channels; refused arguments; the same bits twice; choose()."""
import functools

import numpy as np
import pytest
import torch

import score_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth

pytestmark = pytest.mark.gpu

C3 = 3
HOP = 132
KS = (1, 64, 65, 130)
# tests/test_recordings_gpu.py's: K = 9 on C = 3, one without samples, one shorter than a window, one of exactly one evaluation
LENGTHS = [20003, 0, 100, 1444, 5280, 7777, 1575, 12001, 333]


def _first_index():
    g = util.sample_net().geometry()
    assert int(g.hop) == HOP
    return int(g.first_index)


@functools.lru_cache(maxsize=None)
def _values(E):
    return ref.outputs(C3, E, 1, E)[:, :, 0]


@functools.lru_cache(maxsize=None)
def _model(E, K, deb):
    """(labels, tables [3, K, 6]) of the generator's three detectors: computed once, shared by the banks, never written to"""
    first = _first_index()
    lab = ref.labels(C3, E, first, HOP)
    y = _values(E)
    t = np.stack([ref.score(y[d], ref.thresholds(K), lab[d], 3 * HOP, first, HOP, deb) for d in range(C3)])
    t.setflags(write=False)
    return lab, t


@pytest.fixture(scope="module")
def banks():
    base = util.sample_net()
    three = nets.variant(base, net=nets.random_net(np.random.default_rng(5), base.net.inputs, (8,), 3), thresholds=[0.1, 0.2, 0.3])
    cfgs = [base, nets.perturbed(base, 1)]
    made = {"plain": sd.SyllableDetector(base, channels=C3), "three": sd.SyllableDetector(three, channels=C3),
            "multi": sd.SyllableDetector.multi(cfgs, [0, 1, 0])}
    for det in made.values():
        assert (det.geometry.hop, det.geometry.first_index) == (HOP, _first_index())
    assert made["three"].geometry.outputs == 3
    yield made
    for det in made.values():
        det.close()


def _outputs_for(det, y, output):
    """[C, E, n_out] on the device: y in column `output`, +inf in every other"""
    out = np.full((y.shape[0], y.shape[1], det.geometry.outputs), np.inf, np.float32)
    out[:, :, output] = y
    return torch.from_numpy(out).cuda()


@pytest.mark.parametrize("E", [1, 63, 64, 65, 256, 257, 1000, 4099])       # (64: a step; 256: the steps loaded together)
@pytest.mark.parametrize("bank", ["plain", "three"])
def test_tables_equal_the_model(banks, bank, E):
    det = banks[bank]
    output = det.geometry.outputs - 1
    outputs = _outputs_for(det, _values(E), output)
    for K in KS:
        for deb in ref.debounces(HOP):
            lab, want = _model(E, K, deb)
            with det.scorer(ref.thresholds(K), lab, 3 * HOP, deb / det.config.samplingRate + 1e-9) as s:
                assert (s.count, s.thresholdCount, s.labelCount) == (C3, K, sum(len(t) for t in lab))
                got = s.score(outputs, output=output)
                torch.cuda.synchronize()
            assert got.dtype == torch.int64 and tuple(got.shape) == (C3, K, 6)
            assert np.array_equal(got.cpu().numpy(), want), (bank, E, K, deb)
    if E == 1000:
        t = _model(E, 130, 0)[1]
        assert (t[:, :, 1] > 0).any() and (t[:, :, 2] > 0).any() and (t[:, :, 3] > 0).any()


def test_debounce_seconds_become_frames_as_the_reference_does(banks):
    det = banks["plain"]
    rate = det.config.samplingRate
    for deb in ref.debounces(HOP):
        assert int((deb / rate + 1e-9) * rate) == deb                      # Int(debounce_seconds * samplingRate), what the test above hands over


def test_a_multi_network_bank_scores_like_a_plain_one(banks):
    det = banks["multi"]
    E, K, deb = 1000, 65, 2 * HOP + 1
    lab, want = _model(E, K, deb)
    with det.scorer(ref.thresholds(K), lab, 3 * HOP, deb / det.config.samplingRate + 1e-9) as s:
        got = s.score(_outputs_for(det, _values(E), 0))
        torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_threshold_edges_nan_and_infinities(banks):
    first = _first_index()
    y, thr = ref.edge_values(), ref.edge_thresholds()
    rows = np.stack([y, y[::-1], np.roll(y, 77)])
    for bank in ("plain", "three"):
        det = banks[bank]
        output = det.geometry.outputs - 1
        outputs = _outputs_for(det, rows, output)
        for deb in (0, 2 * HOP + 1):
            want = np.stack([ref.score(np.ascontiguousarray(r), thr, [first + 50 * HOP], 0, first, HOP, deb) for r in rows])
            with det.scorer(thr, [[first + 50 * HOP]] * 3, 0, deb / det.config.samplingRate + 1e-9) as s:
                got = s.score(outputs, output=output)
                torch.cuda.synchronize()
            assert np.array_equal(got.cpu().numpy(), want), (bank, deb)
    n = ref.score(y, thr, [], 0, first, HOP, 0)[:, 0]
    assert n[1] == n[0] - 3 and n[3] == 1 and n[5] == 1 and n[4] == 198 and n[6] == 197


def test_packed_recordings_read_their_own_evaluations_only(banks):
    det = banks["plain"]
    first = _first_index()
    K = 65
    thr = ref.thresholds(K)
    with det.recordings(LENGTHS) as rec:
        evals = [s[3] for s in rec.slots]
        assert evals.count(0) >= 3 and 1 in evals and max(evals) > 64
        out = np.full((C3, rec.rowEvaluations, 1), np.inf, np.float32)    # +inf between and behind the recordings
        own, lab = [], []
        for k, (row, _, first_eval, n, _) in enumerate(rec.slots):
            y = ref.outputs(1, n, 1, 100 + k)[0, :, 0] if n else np.zeros(0, np.float32)
            out[row, first_eval:first_eval + n, 0] = y
            own.append(y)
            lab.append(ref.labels(k + 2, n, first, HOP)[k])
        assert np.isinf(out).sum() > 0
        outputs = torch.from_numpy(out).cuda()
        for deb in ref.debounces(HOP):
            with rec.scorer(thr, lab, 3 * HOP, deb / det.config.samplingRate + 1e-9) as s:
                assert (s.count, s.thresholdCount) == (len(LENGTHS), K)
                got = s.score(outputs)
                torch.cuda.synchronize()
                got = got.cpu().numpy()
                with pytest.raises(ValueError):
                    s.score(outputs[:, :-1].contiguous())                  # not the packed rows' evaluations
                assert _abi.lib.syldet_score_device(s._h, outputs.data_ptr(), rec.rowEvaluations - 1, 0, 1, None) == _abi.ERR_INVALID_ARGUMENT
            for k in range(len(LENGTHS)):
                view = rec.view(outputs, k)[:, 0].cpu().numpy()
                assert np.array_equal(view, own[k])
                want = ref.score(view, thr, lab[k], 3 * HOP, first, HOP, deb)
                assert np.array_equal(got[k], want), (k, deb)
                if evals[k] == 0:
                    assert not got[k].any()
        assert got[:, :, 1].sum() > 0


def test_detections_column_is_detections_and_its_own_indices_are_all_hits():
    """smoke()'s two channels through the fold kernel: K = 1, the configuration's threshold and the same debounce"""
    cfg = util.sample_net()
    assert cfg.rule == _abi.RULE_FIRST
    x = np.stack([synth.syllable_channel(44100, util.template(), seed=11), synth.channel(44100, 0)])
    with sd.SyllableDetector(cfg, channels=2) as det:
        out, fl = det.run(torch.from_numpy(x).cuda())
        for debounce in (0.0, 0.05):
            idx, cnt = det.detections(fl, debounce)
            torch.cuda.synchronize()
            idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
            assert cnt[0] > 0
            with det.scorer([cfg.thresholds[0]], [[], []], 0, debounce) as s:
                t = s.score(out).cpu().numpy()
            assert np.array_equal(t[:, 0, 0], cnt) and np.array_equal(t[:, 0, 2], cnt) and not t[:, 0, [1, 3, 4, 5]].any()
            with det.scorer([cfg.thresholds[0]], [idx[c, :cnt[c]] for c in range(2)], 0, debounce) as s:
                t = s.score(out).cpu().numpy()
            assert np.array_equal(t[:, 0, 0], cnt) and np.array_equal(t[:, 0, 1], cnt) and not t[:, 0, 2:].any()


def test_refused_arguments_the_same_bits_twice_and_choose(banks):
    det = banks["three"]
    E, K, deb = 1000, 130, 9 * HOP + 1
    lab, want = _model(E, K, deb)
    outputs = _outputs_for(det, _values(E), 1)
    bad = _abi.ERR_INVALID_ARGUMENT
    with det.scorer(ref.thresholds(K), lab, 3 * HOP, deb / det.config.samplingRate + 1e-9) as s:
        table = torch.full((C3, K, 6), -1, dtype=torch.int64, device="cuda")
        assert s.score(outputs, output=1, out=table) is table
        torch.cuda.synchronize()
        once = table.cpu().numpy().copy()
        assert np.array_equal(once, want)
        table.fill_(-1)
        s.score(outputs, output=1, out=table)
        torch.cuda.synchronize()
        assert np.array_equal(table.cpu().numpy(), once)
        score = _abi.lib.syldet_score_device
        assert score(s._h, None, E, 1, table.data_ptr(), None) == bad
        assert score(s._h, outputs.data_ptr(), E, 1, None, None) == bad
        assert score(None, outputs.data_ptr(), E, 1, table.data_ptr(), None) == bad
        assert score(s._h, outputs.data_ptr(), E, 3, table.data_ptr(), None) == bad and "output 3" in _abi.last_error()
        assert score(s._h, outputs.data_ptr(), E, -1, table.data_ptr(), None) == bad
        assert score(s._h, outputs.data_ptr(), -1, 1, table.data_ptr(), None) == bad
        assert score(s._h, outputs.data_ptr(), 0, 1, table.data_ptr(), None) == 0          # no evaluation: a table of zeros
        torch.cuda.synchronize()
        assert not table.cpu().numpy().any()
        for wrong in (outputs[:2], outputs.double(), outputs.cpu(), outputs[:, :, :2]):
            with pytest.raises(ValueError):
                s.score(wrong)
        with pytest.raises(ValueError):
            s.score(outputs, output=3)
        with pytest.raises(ValueError):
            s.score(outputs, out=table[:, :1])
        for cost in (0.0, 1.0, 2.5):
            k, theta, totals, costs = s.choose(torch.from_numpy(once).cuda(), cost)
            wk, wt, wc = sd.chooseThreshold(want, [len(t) for t in lab], cost)
            assert k == wk and theta == ref.thresholds(K)[k] and np.array_equal(totals, wt) and np.array_equal(costs, wc)
    with pytest.raises(ValueError):
        det.scorer([0.5], lab[:2], 0)                                                      # a detector without labels' array
    with pytest.raises(sd.SyllableDetectorError) as ei:
        det.scorer([0.5], [[0, 2 * HOP + 1], [5, 5 + 2 * HOP], []], HOP)
    assert ei.value.status == bad and "detector 1, label 1" in str(ei.value)
    with pytest.raises(sd.SyllableDetectorError):
        det.scorer([0.5, float("nan")], lab, 0)
    with pytest.raises(sd.SyllableDetectorError):
        det.scorer([], lab, 0)
