"""Training end to end on the GPU: a network made here, from nothing but a labelled channel, detects held-out syllables.

One 6 s channel at 44.1 kHz -- 0.01 noise plus the template syllable about every 11 000 +- 3000 samples at amplitudes 0.05 .. 0.6,
planted by the test, which keeps the positions -- labels at position + first_index, halfWidth = hop, class weights 0.5 / N_pos and
0.5 / N_neg.  fitInputMap over all evaluations, seeded 1 / sqrt(fan-in) weights with hidden biases 0.2 N(0, 1), Adam at lr 0.01 for
200 full-batch steps (lr 0.03 saturates the tanh units and stalls at 0.25).  The same loop in torch float64 autograd on the CPU, on
the oracle's float32 columns, took the loss from 0.2562 to 0.00150 (0.0059 of the start) and then hit every label of two held-out
channels without a false positive at every threshold from 0.5 to 0.9.  Here: the device loop ends at or below 0.05 of its first
loss; a new bank made from configWith(params) runs two held-out channels, and the scorer at threshold 0.7, tolerance 2 hop,
debounce 50 ms finds every label hit and no false positive; toText() of the trained configuration loads again through
syldet_config_load_text and runs to the same flags."""
import numpy as np
import pytest
import torch

import train_cases as cases
import util
import syllable_detector_swift_amd as sd

pytestmark = pytest.mark.gpu


def test_a_network_trained_here_detects_held_out_syllables(tmp_path):
    base = util.sample_net()
    x, pos = cases.planted_channel(1)
    with sd.SyllableDetector(base, channels=1) as det:
        hop, first = det.geometry.hop, det.geometry.first_index
        cols = det.spectrogram(torch.from_numpy(x[None, :]).cuda())
        E = det.countEvaluations(x.size)
        with det.trainer() as tr:
            fitted = tr.fitInputMap(cols, [first + hop * np.arange(E, dtype=np.int64)])
    m = fitted.net.inputProcessing[1]
    assert m.function == "mapminmax" and m.y == -1.0 and np.isfinite(m.gains).all() and (m.gains > 0).all()
    with sd.SyllableDetector(fitted, channels=1) as det, det.trainer() as tr:
        labels = [pos + first]
        t, _ = tr.targets(labels, hop, 1.0, 1.0, n_evals=E)
        n_pos = int((t > 0).sum())
        n_neg = E - n_pos
        assert n_pos >= len(pos) and n_neg > 0
        t, w = tr.targets(labels, hop, 0.5 / n_pos, 0.5 / n_neg, n_evals=E)
        start = torch.from_numpy(cases.seeded_theta(np.random.default_rng(0), 290, 4, 1)).cuda()
        params, history = tr.fit(cols, t, w, start, steps=200, lr=0.01)
        final = float(tr.gradient(cols, params, t, w)[0]) / float(tr.gradient(cols, params, t, w)[1])
        print("mean loss: %.4g at the start, %.4g after 200 steps (%.4g of the start)" % (history[0], final, final / history[0]))
        assert len(history) == 200 and final <= 0.05 * history[0]
        trained = tr.configWith(params)
    trained.thresholds = [0.7]
    held = [cases.planted_channel(seed) for seed in (2, 3)]
    samples = torch.from_numpy(np.stack([h[0] for h in held])).cuda()
    held_labels = [h[1] + first for h in held]
    with sd.SyllableDetector(trained, channels=2) as det:
        out, flags = det.run(samples)
        with det.scorer([0.7], held_labels, 2 * hop, debounce=0.05) as sc:
            table = sc.score(out).cpu().numpy()
        flags = flags.cpu().numpy()
    for c in range(2):
        detections, hits, false_positives = (int(v) for v in table[c, 0, :3])
        print("held-out channel %d: %d labels, %d detections, %d hits, %d false positives" % (c, len(held_labels[c]), detections, hits, false_positives))
        assert hits == len(held_labels[c]) and false_positives == 0
    path = tmp_path / "trained.txt"
    path.write_text(trained.toText())
    again = sd.SyllableDetectorConfig.fromTextFile(str(path))
    with sd.SyllableDetector(again, channels=2) as det:
        assert np.array_equal(det.run(samples)[1].cpu().numpy(), flags) and flags.sum() > 0
