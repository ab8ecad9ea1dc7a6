#!/usr/bin/env python3
"""Measurement: what threshold calibration (syldet_scorer_*, kernels_score.hip) costs, against what it replaces.

    (a) the outputs of 64 channels x 2^24 samples of the example detector (nets.from_npz(), hop 132) on the benchmark's signal, one
        label a second on every channel, tolerance 20 ms, debounce 50 ms, K = 64 and K = 1024 thresholds from 0.05 to 0.95
    (b) the 2048 packed recordings of tools/recordings_timing.py (log-uniform 1 s to 60 s, 64 rows), one label a second, K = 64
      score     Scorer.score: one launch (score_kernel), against
      read      a plain device read of the same outputs (torch's sum): the practical floor of anything that looks at them all
      loop      the loop a user writes without the scorer: per threshold a torch comparison into flags, detections ((b): events,
                indices only) and the download of the counts and then of as many indices a row as the fullest has -- K round
                trips; matching against the labels on the host would come on top and is not timed
    (a) is measured a second time on planted outputs: 3 % of the evaluations between 0.05 and 1, the rest below every threshold
      run       (b) the packed run of the same rows (SyllableDetector.run): what the scoring is added to

Everything runs in one process; score, read and run alternate launch by launch, every launch between two HIP events of its own;
after a warm-up, the median of `launches` launches with the 10th and 90th percentile.  The loop is timed whole, `loops` times after
one warm-up loop, between two HIP events and a final synchronisation (its downloads wait for the device anyway).
Writes profiles/score_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/score_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--loops N] [--samples S]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    import numpy as np
    import torch
    import syllable_detector_swift_amd as sd
    from syllable_detector_swift_amd import nets, synth

    launches, out_path, R, C, loops, S = 20, os.path.join(ROOT, "profiles", "score_timing.json"), 2048, 64, 3, 1 << 24
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--recordings":
            R, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--rows":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--loops":
            loops, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--samples":
            S, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert launches >= 20, "at least 20 launches a candidate"
    assert torch.cuda.is_available(), "score_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM = 3
    cfg = nets.from_npz()
    fs = cfg.samplingRate
    tolerance, debounce, cap = int(0.02 * fs), 0.05, 4096

    def timed(fns, n=launches, warm=WARM):
        """the candidates alternate; -> {name: sorted milliseconds}"""
        ev = {k: [] for k in fns}
        for r in range(warm + n):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                if r >= warm:
                    ev[k].append((a, b))
        torch.cuda.synchronize()
        return {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}

    def stats(ms):
        return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
                "min_ms": float(ms[0]), "max_ms": float(ms[-1])}

    def case(scorer, outputs, thresholds, loop_body, extra):
        """score against read (and extra candidates), alternating; the user's loop whole"""
        table = torch.empty((scorer.count, len(thresholds), 6), dtype=torch.int64, device=dev)
        fns = {"score": lambda: scorer.score(outputs, out=table), "read": lambda: outputs.sum()}
        fns.update(extra)
        t = timed(fns)

        def loop():
            for theta in thresholds:
                loop_body((outputs[:, :, 0] >= float(theta)).to(torch.uint8))

        t.update(timed({"loop": loop}, n=loops, warm=1))
        med = {k: float(np.median(v)) for k, v in t.items()}
        totals = table.sum(dim=0).cpu().numpy()
        doc = {k: stats(v) for k, v in t.items()}
        doc.update({"thresholds": len(thresholds), "detectors": scorer.count, "labels": int(scorer.labelCount), "waves": scorer.count * ((len(thresholds) + 63) // 64),
                    "outputs_bytes": int(outputs.numel()) * 4, "loop_loops": loops,
                    "share_of_evaluations_at_or_above_the_least_threshold": float((outputs[:, :, 0] >= float(min(thresholds))).float().mean()),
                    "detections_at_the_least_and_greatest_threshold": [int(totals[0, 0]), int(totals[-1, 0])],
                    "hits_at_the_least_and_greatest_threshold": [int(totals[0, 1]), int(totals[-1, 1])],
                    "score_over_read": med["score"] / med["read"], "loop_over_score": med["loop"] / med["score"]})
        for k in extra:
            doc["score_over_" + k] = med["score"] / med[k]
        return doc

    results = {}
    # (a) a plain bank
    with sd.SyllableDetector(cfg, channels=C) as det:
        x = synth.channels_on_device(C, S, dev, fs=fs)
        out, _ = det.run(x)
        torch.cuda.synchronize()
        del x
        torch.cuda.empty_cache()
        labels = [np.arange(1, int(S // fs) + 1, dtype=np.int64) * int(fs) + 7 * c for c in range(C)]

        def download_detections(flags):
            idx, cnt = det.detections(flags, debounce, capacity=cap)
            idx[:, :max(int(cnt.cpu().max()), 1)].cpu()                    # the counts, then the indices there are

        for K in (64, 1024):
            thr = np.linspace(0.05, 0.95, K)
            with det.scorer(thr, labels, tolerance, debounce) as s:
                results["plain_K%d" % K] = case(s, out, thr, download_detections, {})
        # ... and a busy run: the same shape with 3 % of the evaluations planted between 0.05 and 1 (the scan visits them all)
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        busy = torch.rand(out.shape, generator=gen, device=dev) * 0.04
        planted = torch.rand(out.shape, generator=gen, device=dev) < 0.03
        busy[planted] = 0.05 + 0.95 * torch.rand(int(planted.sum()), generator=gen, device=dev)
        del planted
        thr = np.linspace(0.05, 0.95, 64)
        with det.scorer(thr, labels, tolerance, debounce) as s:
            results["plain_planted_K64"] = case(s, busy, thr, download_detections, {})
        del busy
        results["plain_evaluations_per_channel"] = int(out.shape[1])
        del out
        torch.cuda.empty_cache()

    # (b) packed recordings
    rng = np.random.default_rng(2048)
    lengths = np.exp(rng.uniform(np.log(1.0 * fs), np.log(60.0 * fs), size=R)).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum((lengths + 7) // 8 * 8)[:-1]])
    total = int(offsets[-1] + lengths[-1])
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    src = torch.empty(total + 8, dtype=torch.float32, device=dev)
    step = 1 << 27
    for a in range(0, src.numel(), step):                                # (0.05 N(0, 1), the benchmark's noise level, made in pieces)
        n = min(step, src.numel() - a)
        src[a:a + n] = torch.randn(n, generator=gen, dtype=torch.float32, device=dev) * 0.05
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(lengths) as rec:
        rows = rec.load(src, offsets)
        del src
        torch.cuda.empty_cache()
        out, fl = det.run(rows)
        torch.cuda.synchronize()
        labels = [np.arange(1, int(n // fs) + 1, dtype=np.int64) * int(fs) for n in lengths]
        thr = np.linspace(0.05, 0.95, 64)

        def download_events(flags):
            idx, _, cnt = rec.events(None, flags, debounce, capacity=cap)
            idx[:, :max(int(cnt.cpu().max()), 1)].cpu()

        with rec.scorer(thr, labels, tolerance, debounce) as s:
            results["packed_K64"] = case(s, out, thr, download_events, {"run": lambda: det.run(rows, out, fl)})
        results["packed_plan"] = {"recordings": R, "rows": C, "row_evals": int(rec.rowEvaluations), "fill": float(rec.fill)}
    doc = {"workload": "(a) %d channels x %d samples of the benchmark's signal, (b) %d packed recordings, log-uniform 1 s to 60 s at %g Hz, on %d rows; "
                       "the example detector; one label a second, tolerance %d samples, debounce %g s" % (C, S, R, fs, C, tolerance, debounce),
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every launch, candidates alternating, median of `launches` after 3 warm-up rounds; the loop: HIP events "
                     "around a whole loop of K comparisons, scans and downloads (Python's launch overhead included), median of `loop_loops` after one",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
