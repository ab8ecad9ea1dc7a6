#!/usr/bin/env python3
"""Measurement: what packed recordings (syldet_recordings_*, kernels_recordings.hip) cost and gain.

    2048 seeded mono recordings, lengths log-uniform between 1 s and 60 s at 44.1 kHz, already on the device (one 1-D source, every
    recording from a whole 16 bytes), through the example detector (nets.from_npz(), hop 132) on a bank of 64 rows.
      load      Recordings.load, fp32 and int16 (recordings_load_kernel), against
      copy      a device-to-device copy of the same number of bytes (torch's copy_): the practical ceiling, not code under test
      events    Recordings.events on the packed run's flags, with and without values (recordings_events_kernel), against
      detections  SyllableDetector.detections on the same [64, row_evals] flags (detections_kernel): the same bytes scanned
      packed    load + run + events on the 64 rows, against
      one_by_one  the same recordings one after another through a 1-channel handle, run + detections each (what the tool does
                without --batch, less its handle creation, copies and host debounce), and against
      plain     run alone on 64 plain rows of row_samples samples: the same kernel call without the packing around it

Everything runs in one process; the candidates of a group alternate launch by launch, every launch between two HIP events of its
own; after a warm-up, the median of `launches` launches with the 10th and 90th percentile (one_by_one: `loops` whole loops).
Writes profiles/recordings_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/recordings_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--loops N]
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
    from syllable_detector_swift_amd import nets

    launches, out_path, K, C, loops = 20, os.path.join(ROOT, "profiles", "recordings_timing.json"), 2048, 64, 5
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--recordings":
            K, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--rows":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--loops":
            loops, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert launches >= 20, "at least 20 launches a candidate"
    assert torch.cuda.is_available(), "recordings_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM = 3
    cfg = nets.from_npz()
    fs = cfg.samplingRate

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

    rng = np.random.default_rng(2048)
    lengths = np.exp(rng.uniform(np.log(1.0 * fs), np.log(60.0 * fs), size=K)).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum((lengths + 7) // 8 * 8)[:-1]])
    total = int(offsets[-1] + lengths[-1])
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    src = torch.empty(total + 8, dtype=torch.float32, device=dev)
    step = 1 << 27
    for a in range(0, src.numel(), step):                                # (0.05 N(0, 1), the benchmark's noise level, made in pieces)
        n = min(step, src.numel() - a)
        src[a:a + n] = torch.randn(n, generator=gen, dtype=torch.float32, device=dev) * 0.05
    src16 = (src * 32767.0).round_().to(torch.int16)
    results = {}
    with sd.SyllableDetector(cfg, channels=C) as det, sd.SyllableDetector(cfg, channels=1) as one, det.recordings(lengths) as rec:
        S, E = rec.rowSamples, rec.rowEvaluations
        plan = {"recordings": K, "rows": C, "samples": int(lengths.sum()), "row_samples": int(S), "row_evals": int(E), "fill": float(rec.fill),
                "shortest": int(lengths.min()), "longest": int(lengths.max())}
        rows = torch.empty((C, S), dtype=torch.float32, device=dev)
        rows16 = torch.empty((C, S), dtype=torch.int16, device=dev)
        flat, flat16 = rows.view(-1), rows16.view(-1)
        n_copy = min(total, flat.numel())                                  # (the recordings' own samples: what a load reads)

        # 1. the rows
        t = timed({"load": lambda: rec.load(src, offsets, out=rows), "copy": lambda: flat[:n_copy].copy_(src[:n_copy])})
        results["load_fp32"] = {"bytes_read": int(lengths.sum()) * 4, "bytes_written": C * S * 4, "bytes_copied": n_copy * 4, "load": stats(t["load"]),
                                "copy": stats(t["copy"]), "load_over_copy": float(np.median(t["load"]) / np.median(t["copy"]))}
        t = timed({"load": lambda: rec.load(src16, offsets, out=rows16), "copy": lambda: flat16[:n_copy].copy_(src16[:n_copy])})
        results["load_s16"] = {"bytes_read": int(lengths.sum()) * 2, "bytes_written": C * S * 2, "bytes_copied": n_copy * 2, "load": stats(t["load"]),
                               "copy": stats(t["copy"]), "load_over_copy": float(np.median(t["load"]) / np.median(t["copy"]))}
        del rows16, flat16, src16
        torch.cuda.empty_cache()

        # 2. the events
        rec.load(src, offsets, out=rows)
        out, fl = det.run(rows)
        torch.cuda.synchronize()
        cap = 4096
        t = timed({"events": lambda: rec.events(out, fl, 0.05, capacity=cap), "indices_only": lambda: rec.events(None, fl, 0.05, capacity=cap),
                   "detections": lambda: det.detections(fl, 0.05, capacity=cap)})
        results["events"] = {"flags_bytes": int(fl.numel()), "flags_set": int(fl.sum()), "events": stats(t["events"]),
                             "indices_only": stats(t["indices_only"]), "detections": stats(t["detections"]),
                             "events_over_detections": float(np.median(t["events"]) / np.median(t["detections"]))}
        fl_p = (torch.rand((C, E), device=dev) < 0.03).to(torch.uint8)     # planted: 3 % of the evaluations
        t = timed({"events": lambda: rec.events(out, fl_p, 0.0, capacity=cap), "detections": lambda: det.detections(fl_p, 0.0, capacity=cap)})
        results["events_planted"] = {"flags_set": int(fl_p.sum()), "events": stats(t["events"]), "detections": stats(t["detections"]),
                                     "events_over_detections": float(np.median(t["events"]) / np.median(t["detections"]))}
        del fl_p

        # 3. the figure the feature exists for
        o, f = torch.empty_like(out), torch.empty_like(fl)
        plain_rows = torch.randn((C, S), generator=gen, dtype=torch.float32, device=dev) * 0.05

        def packed():
            rec.load(src, offsets, out=rows)
            det.run(rows, o, f)
            rec.events(o, f, 0.05, capacity=cap)

        views = [src[int(a):int(a) + int(n)][None, :] for a, n in zip(offsets, lengths)]

        def one_by_one():
            for x in views:
                _, f1 = one.run(x)
                one.detections(f1, 0.05, capacity=cap)

        t = timed({"packed": packed, "run_packed_rows": lambda: det.run(rows, o, f), "plain": lambda: det.run(plain_rows, o, f)})
        t1 = timed({"one_by_one": one_by_one}, n=loops, warm=1)
        evals = int(sum(max(0, one.countEvaluations(int(n))) for n in lengths))
        frames = lambda ms, e: float(e / (ms * 1e-3))
        results["packed_against_one_by_one"] = {
            "packed": stats(t["packed"]), "run_packed_rows": stats(t["run_packed_rows"]), "plain": stats(t["plain"]), "one_by_one": stats(t1["one_by_one"]),
            "one_by_one_loops": loops, "evaluations_of_the_recordings": evals, "evaluations_of_the_rows": C * int(E),
            "packed_evaluations_per_s": frames(np.median(t["packed"]), evals), "one_by_one_evaluations_per_s": frames(np.median(t1["one_by_one"]), evals),
            "plain_row_evaluations_per_s": frames(np.median(t["plain"]), C * int(E)),
            "run_packed_rows_row_evaluations_per_s": frames(np.median(t["run_packed_rows"]), C * int(E)),
            "one_by_one_over_packed": float(np.median(t1["one_by_one"]) / np.median(t["packed"])),
            "run_packed_rows_over_plain": float(np.median(t["run_packed_rows"]) / np.median(t["plain"]))}
    doc = {"workload": "%d mono recordings, log-uniform 1 s to 60 s at %g Hz, on %d rows; the example detector" % (K, fs, C), "plan": plan,
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every launch (one_by_one: around a whole loop of K run + detections pairs, Python's launch overhead "
                     "included), candidates alternating, median of `launches` after 3 warm-up rounds",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
