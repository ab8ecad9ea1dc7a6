#!/usr/bin/env python3
"""Measurement: what template matching costs (syldet_match_scores_device, syldet_match_peaks_device; kernels_match.hip).

    The workload of "Packed recordings": 2048 mono recordings of 1 to 60 s (seeded) on 64 rows of the example detector
    (nets.from_npz(), hop 132, 29 bins).  The kernels' time does not depend on the values, so the columns [C, frames, bins] are
    filled on the device.  For templates of n = 12 and n = 91 frames, in the same process on the same arrays:
      scores    Matcher.scores on the packed columns: one launch                       match_scores_mfma_kernel
      plain     the same through a matcher made under SYLDET_MATCH_PLAIN=1             match_scores_plain_kernel
      copy      a device copy of the columns' bytes: the floor of the reads (torch's copy_; not code under test)
      torch     what a user writes today: conv1d of the columns with the template and a second one of their squares with ones,
                a division; then, for the peaks, max_pool1d over 2 S + 1 positions and a comparison, with the recordings' masks
      peaks     Matcher.peaks on the scores (threshold 0.77, S = 12): one launch       match_peaks_kernel
    and from them the fraction of the fp32 matrix peak (157.3 TFLOPS) the useful 2 n bins flop a position reach, the copy's time
    over the kernel's, and which of the two bounds is the nearer.

Everything runs in one process; the candidates alternate launch by launch, every launch between two HIP events of its own; after a
warm-up, the median of `launches` launches (torch: of 3).  Writes profiles/match_timing.json (or --out PATH) and prints it as one
JSON line.

    python tools/match_timing.py [launches] [--out PATH] [--recordings K] [--rows C]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_FP32_MATRIX = 157.3e12


def main(argv):
    import numpy as np
    import torch
    import syllable_detector_swift_amd as sd
    from syllable_detector_swift_amd import nets

    launches, out_path, K, C = 20, os.path.join(ROOT, "profiles", "match_timing.json"), 2048, 64
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--recordings":
            K, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--rows":
            C, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert torch.cuda.is_available(), "match_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM = 3
    cfg = nets.from_npz()
    fs = cfg.samplingRate
    lengths = [int(v) for v in np.random.default_rng(2048).integers(int(fs), int(60 * fs), size=K)]

    def timed(fns, n=None):
        ev = {k: [] for k in fns}
        for r in range(WARM + (n or launches)):
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
        doc = {"workload": "%d recordings of 1 to 60 s on %d rows; the columns made on the device" % (K, C), "device": torch.cuda.get_device_name(0),
               "launches": launches, "timing": "HIP events around every launch, candidates alternating, median of `launches` (torch: of 3)",
               "results": results}
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump(doc, open(out_path, "w"), indent=1)
        return doc

    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(lengths) as rec:
        J, bins = det.countFrames(rec.rowSamples), det.geometry.bins
        frames = [max(det.countFrames(n), 0) for n in lengths]
        cols = torch.rand((C, J, bins), device=dev) + 0.01
        other = torch.empty_like(cols)
        results["shape"] = {"recordings": K, "rows": C, "row_frames": J, "bins": bins, "columns_bytes": int(cols.numel() * 4)}
        print("columns: %d x %d x %d" % (C, J, bins), flush=True)
        tc = timed({"copy": lambda: other.copy_(cols)})
        results["copy"] = stats(tc["copy"])
        del other
        torch.cuda.empty_cache()
        copy_ms = results["copy"]["median_ms"]
        for n in (12, 91):
            t = np.random.default_rng(n).random((n, bins)).astype(np.float32)
            positions = int(sum(max(f - n + 1, 0) for f in frames))
            own = torch.zeros((C, J), dtype=torch.bool, device=dev)
            for (row, _, first, _, _), f in zip(rec.slots, frames):
                own[row, first:first + max(f - n + 1, 0)] = True
            os.environ["SYLDET_MATCH_PLAIN"] = "1"
            plain = rec.matcher(t)
            del os.environ["SYLDET_MATCH_PLAIN"]
            with rec.matcher(t) as m, plain:
                assert m.form == "matrix" and plain.form == "plain"
                out, out_p = torch.empty((C, J), device=dev), torch.empty((C, J), device=dev)
                ts = timed({"scores": lambda: m.scores(cols, out=out), "plain": lambda: plain.scores(cols, out=out_p)})
                same = bool(torch.equal(out.view(torch.int32)[own], out_p.view(torch.int32)[own]))
                print("n = %d: scores %.3f ms, plain %.3f ms" % (n, np.median(ts["scores"]), np.median(ts["plain"])), flush=True)
                tp = timed({"peaks": lambda: m.peaks(out, 0.77, 12, capacity=4096)})
                r = {"positions": positions, "flop": 2 * positions * n * bins, "scores": stats(ts["scores"]), "plain": stats(ts["plain"]),
                     "peaks": stats(tp["peaks"]), "matrix_and_plain_bits_equal": same}
                med = r["scores"]["median_ms"]
                r["fraction_of_fp32_matrix_peak"] = r["flop"] / (med * 1e-3) / PEAK_FP32_MATRIX
                r["copy_over_scores"] = copy_ms / med
                r["flop_bound_ms"] = r["flop"] / PEAK_FP32_MATRIX * 1e3
                r["nearer_bound"] = "matrix peak" if r["flop_bound_ms"] > copy_ms else "reads (copy)"
                results["n=%d" % n] = r
                save()                                                                           # (kept if the PyTorch form below takes too long)
                # the PyTorch form
                try:
                    w = torch.from_numpy(m.template.T.copy()[None]).to(dev)                      # [1, bins, n]
                    ones = torch.ones_like(w)

                    def torch_scores():
                        x = cols.permute(0, 2, 1).contiguous()                                   # [C, bins, J]
                        dot = torch.nn.functional.conv1d(x, w)[:, 0]
                        e = torch.nn.functional.conv1d(x * x, ones)[:, 0]
                        s = torch.full((C, J), float("nan"), device=dev)
                        s[:, :J - n + 1] = torch.where(e > 0, dot / torch.sqrt(e), torch.zeros_like(e))
                        return torch.where(own, s, torch.full_like(s, float("nan")))

                    def torch_peaks(s):
                        z = torch.nan_to_num(s, nan=-1e30)
                        # (a recording's neighbours would have to be masked row by row: this is the cheaper, wrong-at-the-seams form)
                        mx = torch.nn.functional.max_pool1d(z[:, None], 25, 1, 12)[:, 0]
                        return torch.nonzero((z >= mx) & (z >= 0.77) & own)

                    print("torch form: first call", flush=True)
                    s_t = torch_scores()
                    torch.cuda.synchronize()
                    err = float((s_t[own] - out[own]).abs().max())
                    tt = timed({"torch_scores": torch_scores}, n=3)
                    tk = timed({"torch_peaks": lambda: torch_peaks(s_t)}, n=3)
                    r["torch_scores"], r["torch_peaks"] = stats(tt["torch_scores"]), stats(tk["torch_peaks"])
                    r["torch_scores_over_scores"] = r["torch_scores"]["median_ms"] / med
                    r["torch_peaks_over_peaks"] = r["torch_peaks"]["median_ms"] / r["peaks"]["median_ms"]
                    r["max_abs_difference_from_torch"] = err
                    del s_t
                except Exception as e:                                                           # (the operator library's refusal is a result too)
                    r["torch_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
                results["n=%d" % n] = r
                print(json.dumps(r), flush=True)
                del out, out_p
                torch.cuda.empty_cache()

    print(json.dumps(save()))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
