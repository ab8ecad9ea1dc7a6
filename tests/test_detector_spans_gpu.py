"""The one detector table (csrc/detector_spans.hpp) under every handle that reads it, on one packed plan: 6 recordings on a 2-row
bank of the sample network.  One row holds a normal recording and behind it one of fewer frames than the template (n = 12), one
with frames but fewer than timeRange and one shorter than a frame; the other row two normal ones.  (The planner places the longer
recording in front, so the short ones lie BEHIND the normal one of their row.  Only a recording without samples takes no room
and could share its first unit with another; the planner would place it behind everything, and this plan has none -- its shortest
has 100 samples.  A zero-unit recording in front of a non-empty one at the same unit is the host test's,
tests/cpp/detector_spans_test.cpp.)  Every normal recording k, bit for bit, against the same handle made on a
1-channel plain bank and fed recording k alone: the matcher's scores and peaks, a 2-template bank's class scores and `which`, the
trainer's and the multi trainer's targets, weights, loss and gradient, the aligner's windows in its three sources, the scorer's
table.  The short ones: no position, weight 0, counts 0."""
import numpy as np
import pytest
import torch

import align_ref
import train_cases
import util
import syllable_detector_swift_amd as sd

pytestmark = pytest.mark.gpu

N, BINS, HOP, W, T = 12, 29, 132, 256, 10
TILE = 320                                                                # the gradient kernel's tile on this network (asserted below)
_samples = lambda frames: W + HOP * (frames - 1)
# the caller's order: shorter than a frame | 5 frames, no evaluation | 11 frames (2 evaluations), no position of the template |
# the normal one of their row | the other row's two: the first ends where a tile of the gradient kernel ends, so that the second
# starts a tile as it does alone (a tile's sums are trees over the tile's threads)
LENGTHS = [100, _samples(5), _samples(11), TILE * HOP + 10 * HOP, TILE * HOP, _samples(49)]
SHORT, NORMAL = (0, 1, 2), (3, 4, 5)
_bytes = lambda a: np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a).tobytes()


@pytest.fixture(scope="module")
def plan():
    cfg = util.sample_net()
    slots, row_samples, row_evals, _ = sd.planRecordings(cfg, 2, LENGTHS)     # chosen on the CPU
    rows = [s[0] for s in slots]
    assert rows[0] == rows[1] == rows[2] == rows[3] != rows[4] == rows[5]
    assert [s[2] for s in slots][3] == 0 and sorted(s[2] for s in slots[:3]) == [s[2] for s in slots[2::-1]]   # normal, then 11, 5, 0 frames
    assert slots[5][2] == TILE and slots[4][2] == 0
    assert [s[3] for s in slots] == [0, 0, 2, TILE, TILE - 10, 40]
    assert len({(s[0], s[2]) for s in slots}) == 6                       # no two share a first unit: the planner cannot make them
    with sd.SyllableDetector(cfg, channels=2) as det, sd.SyllableDetector(cfg, channels=1) as one, det.recordings(LENGTHS) as rec:
        assert [tuple(s) for s in rec.slots] == [tuple(s) for s in slots] and rec.rowSamples == row_samples
        rng = np.random.default_rng(77)
        J, E, n_out = det.countFrames(row_samples), row_evals, det.geometry.outputs
        frames = [det.countFrames(n) for n in LENGTHS]
        assert frames == [0, 5, 11, TILE + 9, TILE - 1, 49]
        cols = np.full((2, J, BINS), np.float32(1e30), np.float32)       # (huge values wherever no recording is)
        outs = rng.uniform(0, 1, (2, E, n_out)).astype(np.float32)
        audio = rng.standard_normal((2, row_samples)).astype(np.float32)
        own = []
        for k, (row, off, first, n_ev, ns) in enumerate(slots):
            cols[row, first:first + frames[k]] = train_cases.columns(rng, frames[k], BINS)
            own.append(dict(cols=cols[row, first:first + frames[k]].copy(), outs=outs[row, first:first + n_ev].copy(), audio=audio[row, off:off + ns].copy()))
        yield dict(cfg=cfg, det=det, one=one, rec=rec, slots=slots, frames=frames, J=J, E=E, own=own, rng=rng,
                   cols=torch.from_numpy(cols).cuda(), outs=torch.from_numpy(outs).cuda(), audio=torch.from_numpy(audio).cuda())


def _alone(p, k, what):
    return torch.from_numpy(p["own"][k][what][None]).cuda()


def test_the_matchers_scores_and_peaks(plan):
    p = plan
    t = p["rng"].standard_normal((N, BINS)).astype(np.float32)
    with p["rec"].matcher(t) as m, p["one"].matcher(t) as m1:
        s = m.scores(p["cols"])
        thr = float(np.nanquantile(s.cpu().numpy(), 0.6))
        ev, cnt, es = m.peaks(s, thr, N, capacity=256)
        host, mine = s.cpu().numpy(), np.zeros((2, p["J"]), bool)
        for k in NORMAL:
            row, _, first, _, _ = p["slots"][k]
            f = p["frames"][k]
            mine[row, first:first + f - N + 1] = True
            s1 = m1.scores(_alone(p, k, "cols"))
            assert _bytes(host[row, first:first + f]) == _bytes(s1[0]), k
            e1, c1, x1 = m1.peaks(s1, thr, N, capacity=256)
            c = int(c1[0])
            assert 0 < c <= 256 and int(cnt[k]) == c and _bytes(ev[k, :c]) == _bytes(e1[0, :c]) and _bytes(es[k, :c]) == _bytes(x1[0, :c]), k
        assert (np.isnan(host) == ~mine).all()                           # the short ones: no position
        assert cnt.cpu().numpy()[list(SHORT)].tolist() == [0, 0, 0]


def test_a_matcher_banks_class_scores_and_which(plan):
    p = plan
    t = p["rng"].standard_normal((2, N, BINS)).astype(np.float32)
    with p["rec"].matcherBank(t, [0, 1]) as b, p["one"].matcherBank(t, [0, 1]) as b1:
        s, w = b.scores(p["cols"], which=True)
        host, which = s.cpu().numpy(), w.cpu().numpy()
        mine = np.zeros((2, p["J"]), bool)
        for k in NORMAL:
            row, _, first, _, _ = p["slots"][k]
            f = p["frames"][k]
            mine[row, first:first + f - N + 1] = True
            s1, w1 = b1.scores(_alone(p, k, "cols"), which=True)
            assert _bytes(host[:, row, first:first + f]) == _bytes(s1[:, 0]) and _bytes(which[:, row, first:first + f]) == _bytes(w1[:, 0]), k
        assert (np.isnan(host) == ~mine[None]).all() and ((which == -1) == ~mine[None]).all()


@pytest.mark.parametrize("multi", [False, True], ids=["trainer", "multi trainer at N = 1"])
def test_the_trainers_targets_weights_loss_and_gradient(plan, multi):
    p = plan
    make = (lambda x: x.multiTrainer()) if multi else (lambda x: x.trainer())
    rng = np.random.default_rng(5)
    labels = [np.sort(np.append(rng.integers(-300, n + 300, 1 + n // 3000), n // 2)) for n in LENGTHS]
    theta = torch.from_numpy(train_cases.theta_of(p["cfg"])).cuda()
    theta = theta[None].contiguous() if multi else theta
    with make(p["rec"]) as tr, make(p["one"]) as tr1:
        assert tr.tile == TILE == tr1.tile
        t, w = tr.targets(labels, 2 * HOP, 0.5, 0.25)
        ht, hw = t.cpu().numpy(), w.cpu().numpy()
        mine = np.zeros((2, p["E"]), bool)
        for k in NORMAL + (2,):                                          # (the 11-frame recording has two evaluations of its own)
            row, _, first, n_ev, _ = p["slots"][k]
            mine[row, first:first + n_ev] = True
            t1, w1 = tr1.targets([labels[k]], 2 * HOP, 0.5, 0.25, n_evals=n_ev)
            assert _bytes(ht[row, first:first + n_ev]) == _bytes(t1[0]) and _bytes(hw[row, first:first + n_ev]) == _bytes(w1[0]), k
            assert (hw[row, first:first + n_ev] > 0).all()
            if k == 2:
                continue
            assert (ht[row, first:first + n_ev] == 1).any() and (ht[row, first:first + n_ev] == 0).any()
            only = np.zeros_like(hw)
            only[row, first:first + n_ev] = hw[row, first:first + n_ev]
            got = tr.gradient(p["cols"], theta, t, torch.from_numpy(only).cuda())
            want = tr1.gradient(_alone(p, k, "cols"), theta, t1, w1)
            assert float(want[1].reshape(-1)[0]) > 0
            for g, x in zip(got, want):
                assert _bytes(g) == _bytes(x), k
        assert ((hw == 0) == ~mine).all() and (ht[~mine] == 0).all()     # the short ones and whatever lies between: weight 0


@pytest.mark.parametrize("source", ["columns", "outputs", "samples"])
def test_the_aligners_windows(plan, source):
    p = plan
    what = {"columns": "cols", "outputs": "outs", "samples": "audio"}[source]
    code = {"columns": align_ref.COLUMNS, "outputs": align_ref.OUTPUTS, "samples": align_ref.SAMPLES}[source]
    origin, step = align_ref.anchor(p["cfg"], code)
    units = [p["own"][k][what].shape[0] for k in range(6)]
    # an event at the first unit, at the last one, and one unit past the end -- of every recording, the short ones too
    events = [np.array([origin, origin + (u - 1) * step, origin + u * step], np.int64) for u in units]
    with p["rec"].aligner(source, 3, 4) as a, p["one"].aligner(source, 3, 4) as a1:
        got = a.windows(p[what], events).cpu().numpy()
        assert got.shape[0] == 18
        for k in NORMAL:
            want = a1.windows(_alone(p, k, what), [events[k]])
            assert _bytes(got[3 * k:3 * k + 3]) == _bytes(want), (source, k)
            assert not np.isnan(got[3 * k, 3:]).any() and np.isnan(got[3 * k, :3]).all() and np.isnan(got[3 * k + 2, 3:]).all()
        for k in SHORT:
            if units[k] == 0:
                assert np.isnan(got[3 * k:3 * k + 3]).all(), (source, k)  # nothing of a neighbour


def test_the_scorers_table(plan):
    p = plan
    thr = np.linspace(0.05, 0.95, 70)
    first = p["det"].geometry.first_index
    labels = [first + HOP * np.arange(3, max(s[3], 3), 7, dtype=np.int64) for s in p["slots"]]
    with p["rec"].scorer(thr, labels, 2 * HOP, 3 * HOP / 44100.0 + 1e-9) as s:
        table = s.score(p["outs"]).cpu().numpy()
        assert table.shape == (6, 70, 6)
    for k in NORMAL:
        with p["one"].scorer(thr, [labels[k]], 2 * HOP, 3 * HOP / 44100.0 + 1e-9) as s1:
            want = s1.score(_alone(p, k, "outs")).cpu().numpy()
            assert _bytes(table[k]) == _bytes(want[0]) and want[0, 0, 0] > 0 and want[0, :, 1].max() > 0, k
    assert (table[[0, 1]] == 0).all()                                     # no evaluation: counts 0
