#!/usr/bin/env python3
"""Measurement: what event-aligned windows cost (syldet_align_device, syldet_align_stats_device; kernels_align.hip).

    The workload of "Packed recordings": 2048 mono recordings of 1 to 60 s (seeded) on 64 rows of the example detector
    (nets.from_npz(), hop 132), one event a second in every recording.  The kernels' time does not depend on the values, so the
    sources are filled on the device (the columns [C, frames, bins], the outputs [C, evaluations, 1], the sample rows).
      columns   (before, after) = (60, 30): windows of 91 frames
      outputs, samples   windows of as many bytes as a columns window (91 x bins units, split evenly)
    For every source, in the same process on the same arrays:
      packed    Aligner.windows on the packed arrays: one launch                        align_windows_kernel
      copy      a device copy of as many bytes as the windows hold: the floor (torch's copy_; not code under test)
      loop      (columns only) what a user writes today: per recording a slice of the spectrogram and a torch gather with a mask
    and the statistics of the columns windows as one stack:
      stats     Aligner.stats                                                              align_stats_kernel + align_combine_kernel
      torch     count, sum and sum of squares with torch in fp64 over the same table (not bit-stable: the reason for the tree)

Everything runs in one process; the candidates alternate launch by launch, every launch between two HIP events of its own; after a
warm-up, the median of `launches` launches (the loop: of 3).  Writes profiles/align_timing.json (or --out PATH) and prints it as one
JSON line.

    --cli N: only the tool end to end on N files of 5 s with planted syllables, --align-dir with and without --batch (median of 3),
    merged into the JSON at PATH under "cli".

    python tools/align_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--cli N]
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

    launches, out_path, K, C, n_cli = 20, os.path.join(ROOT, "profiles", "align_timing.json"), 2048, 64, 0
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
    assert torch.cuda.is_available(), "align_timing needs a GPU"
    if n_cli > 0:
        return cli_only(n_cli, out_path)
    dev = torch.device("cuda", 0)
    WARM = 3
    cfg = nets.from_npz()
    fs = cfg.samplingRate
    lengths = [int(v) for v in np.random.default_rng(2048).integers(int(fs), int(60 * fs), size=K)]
    events = [np.arange(1, n // int(fs) + 1, dtype=np.int64) * int(fs) for n in lengths]
    counts = np.array([e.size for e in events], np.int64)
    begin = np.concatenate([[0], np.cumsum(counts)])

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

    def kernels(det, fn, repeats=7):
        got = {}
        for _ in range(repeats):
            fn()
            torch.cuda.synchronize()
            for name, ms in det.lastTimings():
                got.setdefault(name, []).append(ms)
        return {k: float(np.median(v)) for k, v in got.items()}

    results = {}
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(lengths) as rec:
        S, E, J, bins = rec.rowSamples, rec.rowEvaluations, det.countFrames(rec.rowSamples), det.geometry.bins
        hop, need = det.geometry.hop, det.geometry.gap + cfg.windowLength
        d_events = torch.from_numpy(np.concatenate(events)).to(dev)
        N = int(begin[-1])
        units = 91 * bins
        shapes = {"columns": (60, 30), "outputs": (units // 2, units - 1 - units // 2), "samples": (units // 2, units - 1 - units // 2)}
        results["shape"] = {"recordings": K, "rows": C, "row_samples": S, "row_frames": J, "row_evaluations": E, "bins": bins, "events": N,
                            "window_bytes": units * 4, "windows_bytes": N * units * 4}
        for name, (before, after) in shapes.items():
            if name == "columns":
                src = torch.rand((C, J, bins), device=dev)
            elif name == "outputs":
                src = torch.rand((C, E, 1), device=dev)
            else:
                src = torch.rand((C, S), device=dev)
            with rec.aligner(name, before, after) as al:
                n, width = al.shape[1], al.shape[2]
                out = torch.empty((N, n, width), device=dev)
                other = torch.rand((N, n, width), device=dev)
                fns = {"packed": lambda: al.windows(src, d_events, counts=counts, out=out), "copy": lambda: out.copy_(other)}
                t = timed(fns)
                det.profile(True)
                k_ms = kernels(det, fns["packed"])
                det.profile(False)
                med = {k: float(np.median(v)) for k, v in t.items()}
                results[name] = {"before": before, "after": after, "width": width, "bytes_written": int(out.numel() * 4),
                                 "destination_starts_mod_16_bytes": sorted({int(w * n * width * 4 % 16) for w in range(min(N, 64))}),
                                 "packed": stats(t["packed"]), "copy": stats(t["copy"]), "kernels_ms": k_ms,
                                 "packed_over_copy": med["packed"] / med["copy"], "packed_GBps_written": out.numel() * 4 / med["packed"] / 1e6}
                if name == "columns":
                    span = torch.arange(-before, after + 1, device=dev)
                    d_ev = [torch.from_numpy(e).to(dev) for e in events]

                    def loop():
                        parts = []
                        for k in range(K):
                            view = rec.columnsView(src, k)
                            u = torch.div(d_ev[k] - need, hop, rounding_mode="floor")[:, None] + span[None, :]
                            ok = (u >= 0) & (u < view.shape[0])
                            w = view[u.clamp(0, max(view.shape[0] - 1, 0))]
                            parts.append(torch.where(ok[:, :, None], w, torch.full_like(w, float("nan"))))
                        return torch.cat(parts)

                    al.windows(src, d_events, counts=counts, out=out)
                    got = loop()
                    differing = int(((out.view(torch.int32) != got.view(torch.int32)) & ~(torch.isnan(out) & torch.isnan(got))).sum())
                    tl = timed({"loop": loop}, n=3)
                    results[name]["loop"] = stats(tl["loop"])
                    results[name]["loop_over_packed"] = float(np.median(tl["loop"])) / med["packed"]
                    results[name]["elements_differing_from_loop"] = differing
                    del got
                    # the statistics of the one stack
                    present = ~torch.isnan(out)

                    def plain():
                        x = torch.where(present, out, torch.zeros_like(out)).to(torch.float64)
                        return present.sum(0), x.sum(0), (x * x).sum(0)

                    ts = timed({"stats": lambda: al.stats(out), "torch": plain})
                    det.profile(True)
                    k_ms = kernels(det, lambda: al.stats(out))
                    det.profile(False)
                    a, b = al.stats(out), al.stats(out)
                    p = plain()
                    results["stats"] = {"events": N, "window_elements": n * width, "bytes_read": int(out.numel() * 4), "stats": stats(ts["stats"]),
                                        "torch": stats(ts["torch"]), "kernels_ms": k_ms,
                                        "stats_over_torch": float(np.median(ts["stats"]) / np.median(ts["torch"])),
                                        "stats_GBps_read": out.numel() * 4 / float(np.median(ts["stats"])) / 1e6,
                                        "run_to_run_identical": bool(all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))),
                                        "counts_equal_torch": bool(torch.equal(a[0][0], p[0])),
                                        "sums_differing_from_torch_bits": int((a[1][0].view(torch.int64) != p[1].view(torch.int64)).sum())}
                    del present
                del out, other, src
                torch.cuda.empty_cache()

    doc = {"workload": "%d recordings of 1 to 60 s on %d rows, one event a second; the sources made on the device" % (K, C),
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every launch, candidates alternating, median of `launches` (the loop: of 3); kernels_ms: the handle's profile",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


def cli_only(n_files, out_path):
    import subprocess
    import tempfile
    import time
    import wave
    import numpy as np
    from syllable_detector_swift_amd import nets, synth
    cfg = nets.from_npz()
    fs = int(cfg.samplingRate)
    cli = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
    tmpl = np.load(os.path.join(ROOT, "tests", "golden", "syllable_template.npy"))
    with tempfile.TemporaryDirectory() as d:
        net = os.path.join(d, "net.txt")
        open(net, "w").write(cfg.toText())
        audio = []
        for k in range(n_files):
            p = os.path.join(d, "f%03d.wav" % k)
            x = synth.syllable_channel(5 * fs, tmpl, seed=k, every=6000)
            with wave.open(p, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(fs)
                w.writeframes(np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2").tobytes())
            audio += ["-a", p]
        runs = {"batch": [], "per_file": [], "batch_without_align": [], "per_file_without_align": []}
        for _ in range(3):
            for key, extra in (("batch", ["--batch", "--align-dir", os.path.join(d, "A")]), ("per_file", ["--align-dir", os.path.join(d, "B")]),
                               ("batch_without_align", ["--batch"]), ("per_file_without_align", [])):
                t0 = time.perf_counter()
                subprocess.run([cli, "-n", net, *audio, "-d", "0.05", *extra], check=True, capture_output=True)
                runs[key].append(time.perf_counter() - t0)
        names = sorted(os.listdir(os.path.join(d, "A")))
        same = names == sorted(os.listdir(os.path.join(d, "B"))) and all(
            open(os.path.join(d, "A", n), "rb").read() == open(os.path.join(d, "B", n), "rb").read() for n in names)
        events = int(np.load(os.path.join(d, "A", "count.npy")).max())
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {"results": {}}
    doc["results"]["cli"] = {"files": n_files, "seconds_each": 5, "source": "columns", "events": events,
                             **{k + "_s": float(np.median(v)) for k, v in runs.items()}, "files_identical_both_ways": bool(same)}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc["results"]["cli"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
