#!/usr/bin/env python3
"""Measurement: what a bank of templates costs against the loop it replaces (syldet_match_bank_scores_device,
syldet_match_bank_peaks_device; kernels_match.hip).

    The workload of tools/match_timing.py: 2048 mono recordings of 1 to 60 s (seeded) on 64 rows of the example detector (hop 132,
    29 bins), the columns filled on the device.  K = 8 templates in C = 2 classes of four, at n = 12 and n = 91 frames, in the same
    process on the same arrays, the candidates alternating launch by launch:
      bank      MatcherBank.scores (scores and which): one launch                       match_bank_scores_mfma_kernel
      loop      what it replaces: 8 Matcher.scores calls, then a class's plane by three torch.maximum calls and its `which` by an
                argmax over the four planes
      single    one Matcher.scores call                                                 match_scores_mfma_kernel
      bank_peaks    MatcherBank.peaks on the two planes (S = 12): one launch            match_bank_peaks_kernel
      loop_peaks    2 Matcher.peaks calls on the same planes
    and from them: loop / bank, bank / single (8 would be no saving at all), the loop's own run-to-run spread (p90 - p10 of its
    launches, as a fraction of its median), whether the bank is slower than the loop by more than that spread, and the fraction of
    the fp32 matrix peak (157.3 TFLOPS) the useful 2 n bins K flop a position reach.  The bank's planes are compared with the
    loop's bit for bit on every position that holds a score.

    --single PATH   only the single matcher (for a comparison of two builds of the library, SYLDET_LIB naming the build): the
                    scores kernel's times at n = 12 and n = 91 as one JSON line, and its outputs' bytes written to PATH.n12 / PATH.n91

Everything runs in one process; every launch lies between two HIP events of its own; after a warm-up, the median of `launches`
launches.  Writes profiles/match_bank_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/match_bank_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--single PATH]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32_MATRIX = 157.3e12
TEMPLATES, CLASSES = 8, (0, 0, 0, 0, 1, 1, 1, 1)


def main(argv):
    import numpy as np
    import torch
    import syllable_detector_swift_amd as sd
    from syllable_detector_swift_amd import nets

    launches, out_path, K, C, single_path = 20, os.path.join(ROOT, "profiles", "match_bank_timing.json"), 2048, 64, None
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--recordings":
            K, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--rows":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--single":
            single_path, i = argv[i + 1], i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert torch.cuda.is_available(), "match_bank_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM = 3
    cfg = nets.from_npz()
    fs = cfg.samplingRate
    lengths = [int(v) for v in np.random.default_rng(2048).integers(int(fs), int(60 * fs), size=K)]

    def timed(fns):
        ev = {k: [] for k in fns}
        for r in range(WARM + launches):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                if r >= WARM:
                    ev[k].append((a, b))
        torch.cuda.synchronize()
        return {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}

    def stats(ms):
        return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
                "min_ms": float(ms[0]), "max_ms": float(ms[-1])}

    results = {}

    def save():
        doc = {"workload": "%d recordings of 1 to 60 s on %d rows; the columns made on the device; %d templates in %d classes" % (K, C, TEMPLATES, 2),
               "device": torch.cuda.get_device_name(0), "launches": launches,
               "timing": "HIP events around every launch, candidates alternating, median of `launches`", "results": results}
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump(doc, open(out_path, "w"), indent=1)
        return doc

    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(lengths) as rec:
        J, bins = det.countFrames(rec.rowSamples), det.geometry.bins
        frames = [max(det.countFrames(n), 0) for n in lengths]
        torch.manual_seed(1)
        cols = torch.rand((C, J, bins), device=dev) + 0.01
        print("columns: %d x %d x %d" % (C, J, bins), flush=True)
        if single_path:
            line = {"library": os.environ.get("SYLDET_LIB", "lib")}
            for n in (12, 91):
                t = np.random.default_rng(n).random((n, bins)).astype(np.float32)
                with rec.matcher(t) as m:
                    out = torch.empty((C, J), device=dev)
                    line["n=%d" % n] = stats(timed({"single": lambda: m.scores(cols, out=out)})["single"])
                    out.cpu().numpy().tofile("%s.n%d" % (single_path, n))
            print(json.dumps(line), flush=True)
            return 0
        results["shape"] = {"recordings": K, "rows": C, "row_frames": J, "bins": bins, "templates": TEMPLATES, "classes": 2}
        for n in (12, 91):
            t = np.random.default_rng(n).random((TEMPLATES, n, bins)).astype(np.float32)
            positions = int(sum(max(f - n + 1, 0) for f in frames))
            own = torch.zeros((C, J), dtype=torch.bool, device=dev)
            for (row, _, first, _, _), f in zip(rec.slots, frames):
                own[row, first:first + max(f - n + 1, 0)] = True
            singles = [rec.matcher(t[k]) for k in range(TEMPLATES)]
            try:
                with rec.matcherBank(t, CLASSES) as bank:
                    assert bank.form == "matrix" and singles[0].form == "matrix"
                    s_bank = torch.empty((2, C, J), device=dev)
                    w_bank = torch.empty((2, C, J), dtype=torch.int32, device=dev)
                    per = torch.empty((TEMPLATES, C, J), device=dev)
                    s_loop = torch.empty((2, C, J), device=dev)
                    w_loop = [None, None]

                    def loop():
                        for k in range(TEMPLATES):
                            singles[k].scores(cols, out=per[k])
                        for c in range(2):
                            p = per[4 * c:4 * c + 4]
                            torch.maximum(p[0], p[1], out=s_loop[c])
                            torch.maximum(s_loop[c], p[2], out=s_loop[c])
                            torch.maximum(s_loop[c], p[3], out=s_loop[c])
                            w_loop[c] = torch.argmax(p, dim=0)

                    ts = timed({"bank": lambda: bank.scores(cols, which=True, out=(s_bank, w_bank)), "loop": loop,
                                "single": lambda: singles[0].scores(cols, out=per[0])})
                    loop()
                    torch.cuda.synchronize()
                    same = bool(torch.equal(s_bank.view(torch.int32)[:, own], s_loop.view(torch.int32)[:, own]))
                    tp = timed({"bank_peaks": lambda: bank.peaks(s_bank, [0.77, 0.8], 12, capacity=4096, which=w_bank),
                                "loop_peaks": lambda: [singles[0].peaks(s_bank[c], thr, 12, capacity=4096) for c, thr in enumerate((0.77, 0.8))]})
                    r = {"positions": positions, "flop": 2 * positions * n * bins * TEMPLATES}
                    for k in ("bank", "loop", "single"):
                        r[k] = stats(ts[k])
                    for k in ("bank_peaks", "loop_peaks"):
                        r[k] = stats(tp[k])
                    bank_ms, loop_ms = r["bank"]["median_ms"], r["loop"]["median_ms"]
                    r["loop_over_bank"] = loop_ms / bank_ms
                    r["bank_over_single"] = bank_ms / r["single"]["median_ms"]
                    r["loop_spread"] = (r["loop"]["p90_ms"] - r["loop"]["p10_ms"]) / loop_ms
                    r["bank_slower_than_loop_by_more_than_its_spread"] = bool(bank_ms > loop_ms + (r["loop"]["p90_ms"] - r["loop"]["p10_ms"]))
                    r["loop_peaks_over_bank_peaks"] = r["loop_peaks"]["median_ms"] / r["bank_peaks"]["median_ms"]
                    r["fraction_of_fp32_matrix_peak"] = r["flop"] / (bank_ms * 1e-3) / PEAK_FP32_MATRIX
                    r["single_fraction_of_fp32_matrix_peak"] = r["flop"] / TEMPLATES / (r["single"]["median_ms"] * 1e-3) / PEAK_FP32_MATRIX
                    r["bank_and_loop_bits_equal"] = same
                    results["n=%d" % n] = r
                    save()
                    print(json.dumps(r), flush=True)
                    assert same, "the bank's planes differ from the loop's"
                    del s_bank, w_bank, per, s_loop, w_loop
            finally:
                for m in singles:
                    m.close()
            torch.cuda.empty_cache()

    print(json.dumps(save()))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
