#!/usr/bin/env python3
"""Measurement: what the per-sample tracks of packed recordings cost (syldet_recordings_trace_device*,
syldet_recordings_trigger*_device*; kernels_recordings_tracks.hip).

    The workload of "Packed recordings": 2048 mono recordings of 1 to 60 s (seeded) on 64 rows of the example detector
    (nets.from_npz(), hop 132), int16 tracks, L = 32, N = 44, no latency.  The tracks read only the run's results, so the
    outputs and flags [C, rowEvaluations] are made on the device (uniform outputs around the threshold, 3 % of the flags
    set); no audio is loaded.
      trace     Recordings.trace               recordings_trace_kernel
      trigger   Recordings.triggerTrack        recordings_trigger_scan_kernel + recordings_trigger_kernel
      onsets    Recordings.triggerOnsets       recordings_trigger_scan_kernel + recordings_trigger_onsets_kernel
    against
      fill      torch's fill_(0) of the destination's bytes: the practical store-bandwidth ceiling (not code under test)
      loop      what a user writes today: K calls of syldet_trace_device_s16 / syldet_trigger_device_s16 through a one-channel
                handle on pointers into the packed outputs / flags, straight through the C ABI
    and a stereo archive -- the same recordings as 1024 files of two tracks, step 2 -- against
    syldet_trace_interleaved_device_s16 of a two-channel handle on the same number of bytes (whole frames from LDS).
    --cli N: also the tool end to end on N files of 5 s: --batch --simulate-dir against one --simulate run a file.

Everything runs in one process; the candidates alternate launch by launch, every launch between two HIP events of its own; after a
warm-up, the median of `launches` launches.  Writes profiles/recordings_tracks_timing.json (or --out PATH) and prints it as one
JSON line.

    python tools/recordings_tracks_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--cli N]
"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    import numpy as np
    import torch
    import syllable_detector_swift_amd as sd
    from syllable_detector_swift_amd import _abi, nets

    launches, out_path, K, C, n_cli = 20, os.path.join(ROOT, "profiles", "recordings_tracks_timing.json"), 2048, 64, 0
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--recordings":
            K, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--rows":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--cli":
            n_cli, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert launches >= 20, "at least 20 launches a candidate"
    assert torch.cuda.is_available(), "recordings_tracks_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM, L, N, LAT = 3, 32, 44, 0
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

    def ratio(t, a, b):
        return float(np.median(t[a]) / np.median(t[b]))

    def kernels(det, fn, repeats=7):
        got = {}
        for _ in range(repeats):
            fn()
            torch.cuda.synchronize()
            for name, ms in det.lastTimings():
                got.setdefault(name, []).append(ms)
        return {k: float(np.median(v)) for k, v in got.items()}

    results = {}
    thr = float(cfg.thresholds[0])
    with sd.SyllableDetector(cfg, channels=C) as det, sd.SyllableDetector(cfg, channels=1) as one, det.recordings(lengths) as rec:
        E = rec.rowEvaluations
        out = torch.rand((C, E, 1), device=dev) * (1.5 * thr)
        fl = (torch.rand((C, E), device=dev) < 0.03).to(torch.uint8)
        offsets, total = rec.trackLayout()
        dst = torch.zeros(total, dtype=torch.int16, device=dev)
        dst2 = torch.zeros(total, dtype=torch.int16, device=dev)
        stream = det._stream_ptr(None)
        lib = _abi.lib

        def loop_trace():
            for (row, _, first, n_evals, n), o in zip(rec.slots, offsets):
                lib.syldet_trace_device_s16(one._h, out.data_ptr() + 4 * (row * E + first), n_evals, 0, dst2.data_ptr() + 2 * int(o), n, n, stream)

        def loop_trigger():
            for (row, _, first, n_evals, n), o in zip(rec.slots, offsets):
                lib.syldet_trigger_device_s16(one._h, fl.data_ptr() + row * E + first, n_evals, L, N, LAT, dst2.data_ptr() + 2 * int(o), n, n, stream)

        # the two paths give the same bytes before either is timed
        rec.trace(out, out=dst)
        loop_trace()
        trace_differing = int((dst != dst2).sum())
        rec.triggerTrack(fl, L, N, LAT, out=dst)
        loop_trigger()
        trigger_differing = int((dst != dst2).sum())

        t = timed({"trace": lambda: rec.trace(out, out=dst), "trigger": lambda: rec.triggerTrack(fl, L, N, LAT, out=dst),
                   "onsets": lambda: rec.triggerOnsets(fl, L, N, LAT, capacity=4096), "fill": lambda: dst.fill_(0)})
        tl = timed({"loop_trace": loop_trace, "loop_trigger": loop_trigger}, n=5)
        det.profile(True)
        k_ms = {}
        for fn in (lambda: rec.trace(out, out=dst), lambda: rec.triggerTrack(fl, L, N, LAT, out=dst), lambda: rec.triggerOnsets(fl, L, N, LAT, capacity=4096)):
            k_ms.update(kernels(det, fn))
        det.profile(False)
        results["mono"] = {"recordings": K, "rows": C, "row_samples": rec.rowSamples, "row_evaluations": E, "fill_share": rec.fill,
                           "bytes_written": int(dst.numel() * 2), "flags_set": int(fl.sum()),
                           "trace": stats(t["trace"]), "trigger": stats(t["trigger"]), "onsets": stats(t["onsets"]), "fill": stats(t["fill"]),
                           "loop_trace": stats(tl["loop_trace"]), "loop_trigger": stats(tl["loop_trigger"]), "kernels_ms": k_ms,
                           "trace_over_fill": ratio(t, "trace", "fill"), "trigger_over_fill": ratio(t, "trigger", "fill"),
                           "loop_trace_over_trace": float(np.median(tl["loop_trace"]) / np.median(t["trace"])),
                           "loop_trigger_over_trigger": float(np.median(tl["loop_trigger"]) / np.median(t["trigger"])),
                           "trace_elements_differing_from_loop": trace_differing, "trigger_elements_differing_from_loop": trigger_differing}
        del dst2
        torch.cuda.empty_cache()

    # the stereo archive: pairs of equal length, frames [n][2], against the frame-tile kernel on the same number of bytes
    pairs = [n for n in lengths[:K // 2] for _ in range(2)]
    with sd.SyllableDetector(cfg, channels=C) as det, sd.SyllableDetector(cfg, channels=2) as two, det.recordings(pairs) as rec:
        E = rec.rowEvaluations
        out = torch.rand((C, E, 1), device=dev) * (1.5 * thr)
        offsets, steps, pos = [], [], 0
        for n in pairs[::2]:
            offsets += [pos, pos + 1]
            steps += [2, 2]
            pos += (2 * n + 7) // 8 * 8
        dst = torch.zeros(pos, dtype=torch.int16, device=dev)
        frames = pos // 2
        out2 = torch.rand((2, two.countEvaluations(frames), 1), device=dev) * (1.5 * thr)
        whole = dst[:2 * frames].view(frames, 2)
        t = timed({"step2": lambda: rec.trace(out, offsets=offsets, steps=steps, out=dst),
                   "interleaved": lambda: two.trace(out2, frames, dtype=np.int16, interleaved=True, out=whole), "fill": lambda: dst.fill_(0)})
        results["stereo"] = {"files": len(pairs) // 2, "bytes_written": int(dst.numel() * 2), "step2": stats(t["step2"]),
                             "interleaved": stats(t["interleaved"]), "fill": stats(t["fill"]),
                             "step2_over_interleaved": ratio(t, "step2", "interleaved"), "step2_over_fill": ratio(t, "step2", "fill")}
        del dst, whole
        torch.cuda.empty_cache()

    if n_cli > 0:
        import wave
        cli = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
        with tempfile.TemporaryDirectory() as d:
            net = os.path.join(d, "net.txt")
            open(net, "w").write(cfg.toText())
            rng = np.random.default_rng(7)
            paths = []
            for k in range(n_cli):
                p = os.path.join(d, "f%03d.wav" % k)
                with wave.open(p, "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(int(fs))
                    w.writeframes((rng.standard_normal(int(5 * fs)) * 300).astype("<i2").tobytes())
                paths.append(p)
            audio = [a for p in paths for a in ("-a", p)]
            runs = {"batch": [], "per_file": []}
            for _ in range(3):
                t0 = time.perf_counter()
                subprocess.run([cli, "-n", net, *audio, "--batch", "--simulate-dir", os.path.join(d, "A")], check=True, capture_output=True)
                runs["batch"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                for p in paths:
                    subprocess.run([cli, "-n", net, "-a", p, "--simulate", os.path.join(d, "one.wav")], check=True, capture_output=True)
                runs["per_file"].append(time.perf_counter() - t0)
            results["cli"] = {"files": n_cli, "seconds_each": 5, "batch_s": float(np.median(runs["batch"])), "per_file_s": float(np.median(runs["per_file"])),
                              "per_file_over_batch": float(np.median(runs["per_file"]) / np.median(runs["batch"]))}

    doc = {"workload": "%d recordings of 1 to 60 s on %d rows, int16 tracks, L %d, N %d, latency %d; outputs and flags made on the device" % (K, C, L, N, LAT),
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every launch, candidates alternating, median of `launches` (the loops: of 5); kernels_ms: the handle's profile",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
