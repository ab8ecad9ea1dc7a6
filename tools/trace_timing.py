#!/usr/bin/env python3
"""Measurement: what the Simulator's output track (syldet_trace*, kernels_trace.hip) costs.

    64 channels x 2^24 samples, the example detector (nets.from_npz(), hop 132) and hop 128; the outputs of one run() expanded as
      s16      trace(dtype=int16)                      trace_kernel              2 GiB written
      s16i     trace(dtype=int16, interleaved=True)    trace_interleaved_s16_kernel
      f32      trace(dtype=float32)                    trace_kernel              4 GiB written
    each against
      fill     torch's fill_(0) of a buffer of the trace's size and dtype: the practical store-bandwidth ceiling (not code under test)
      torch    (s16 only) the same track made with PyTorch: the clamped quotient, repeat_interleave, cat with the leading zeros,
               round, to(int16)
    and, at hop 132, simulate() against run() alone: what the track adds to a step.

Everything runs in one process; the candidates of a shape alternate launch by launch, every launch between two HIP events of its
own; after a warm-up, the median of `launches` launches, with the 10th and 90th percentile.  Writes profiles/trace_timing.json
(or --out PATH) and prints it as one JSON line.

    python tools/trace_timing.py [launches] [--out PATH] [--channels C] [--log2-samples L]
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

    launches, out_path, C, L = 30, os.path.join(ROOT, "profiles", "trace_timing.json"), 64, 24
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--channels":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--log2-samples":
            L, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert launches >= 20, "at least 20 launches a candidate"
    assert torch.cuda.is_available(), "trace_timing needs a GPU"
    dev = torch.device("cuda", 0)
    S, WARM = 1 << L, 5
    base = nets.from_npz()

    def timed(fns):
        """the candidates alternate; -> {name: sorted milliseconds}"""
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

    results = []
    for hop in (132, 128):
        cfg = base if hop == 132 else nets.variant(base, windowOverlap=base.windowLength - hop)
        x = synth.channels_on_device(C, S, dev, fs=cfg.samplingRate)
        with sd.SyllableDetector(cfg, channels=C) as det:
            assert det.geometry.hop == hop
            # (a [C, 1] tensor of thresholds: what a bank needs, and a true division -- PyTorch multiplies by the reciprocal of a scalar)
            D, thr = det.geometry.first_index, torch.full((C, 1), float(np.float32(cfg.thresholds[0])), dtype=torch.float32, device=dev)
            out, fl = det.run(x)
            torch.cuda.synchronize()
            E = out.shape[1]
            for form in ("s16", "s16i", "f32"):
                tdt = torch.float32 if form == "f32" else torch.int16
                buf = torch.empty((S, C) if form == "s16i" else (C, S), dtype=tdt, device=dev)
                kw = dict(dtype=np.float32 if form == "f32" else np.int16, interleaved=form == "s16i", out=buf)
                fns = {"trace": lambda: det.trace(out, S, **kw), "fill": lambda: buf.fill_(0)}
                if form == "s16":
                    def with_torch():
                        v = (out[:, :, 0] / thr).clamp_(0.0, 1.0)
                        body = v.repeat_interleave(hop, dim=1)[:, :S - D]
                        return torch.cat([torch.zeros((C, D), dtype=torch.float32, device=dev), body], dim=1).mul_(32767.0).round_().to(torch.int16)
                    fns["torch"] = with_torch
                    # (ordinary values: no NaN.  A difference is flagged below; the tests hold the kernel to numpy bit for bit)
                    differing = int((det.trace(out, S, **kw) != with_torch()).sum())
                t = timed(fns)
                rec = {"case": "hop%d_%s" % (hop, form), "channels": C, "samples": S, "evaluations": int(E), "bytes_written": int(buf.numel() * buf.element_size()),
                       "launches": launches, "trace": stats(t["trace"]), "fill": stats(t["fill"]),
                       "trace_over_fill": float(np.median(t["trace"]) / np.median(t["fill"])),
                       "trace_GBps": float(buf.numel() * buf.element_size() / np.median(t["trace"]) / 1e6)}
                if "torch" in t:
                    rec["torch"] = stats(t["torch"])
                    rec["torch_over_trace"] = float(np.median(t["torch"]) / np.median(t["trace"]))
                    rec["samples_differing_from_torch"] = differing
                results.append(rec)
                del buf
            if hop == 132:
                o = torch.empty_like(out)
                f = torch.empty_like(fl)
                tr = torch.empty((C, S), dtype=torch.int16, device=dev)

                def sim():
                    det.run(x, o, f)
                    det.trace(o, S, dtype=np.int16, out=tr)
                t = timed({"run": lambda: det.run(x, o, f), "simulate": sim})
                results.append({"case": "hop132_simulate_against_run", "channels": C, "samples": S, "launches": launches, "run": stats(t["run"]),
                                "simulate": stats(t["simulate"]), "simulate_over_run": float(np.median(t["simulate"]) / np.median(t["run"]))})
        del x, out, fl
        torch.cuda.empty_cache()
    doc = {"workload": "%d channels x 2^%d samples; outputs of run() expanded into the Simulator's track" % (C, L),
           "device": torch.cuda.get_device_name(0), "timing": "HIP events around every launch, candidates alternating, median of `launches`",
           "results": results}
    # what the numbers are held against: the aligned planar int16 trace within 1.25x of the fill of the same bytes (beyond that
    # the stores are not the 16-byte ones or evaluations are recomputed per lane: a defect, not a figure), the kernel no slower
    # than the PyTorch way to the same track, and the same track
    broken = []
    for r in results:
        if r["case"].endswith("_s16"):
            if r["trace_over_fill"] > 1.25:
                broken.append("%s: trace / fill = %.3f > 1.25" % (r["case"], r["trace_over_fill"]))
            if r["torch_over_trace"] < 1.0:
                broken.append("%s: the kernel is slower than PyTorch (%.3f ms against %.3f)" % (r["case"], r["trace"]["median_ms"], r["torch"]["median_ms"]))
            if r["samples_differing_from_torch"] != 0:
                broken.append("%s: %d samples differ from PyTorch's track" % (r["case"], r["samples_differing_from_torch"]))
    doc["flagged"] = broken
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    for b in broken:
        print("FLAGGED:", b, file=sys.stderr)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
