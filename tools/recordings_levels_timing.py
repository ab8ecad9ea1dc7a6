#!/usr/bin/env python3
"""Measurement: what the level meters of packed recordings cost (syldet_recordings_levels_device*,
syldet_recordings_output_levels_device; kernels_recordings_levels.hip).

    The workload of "Packed recordings": 2048 mono recordings of 1 to 60 s (seeded) on 64 rows of the example detector
    (nets.from_npz(), hop 132), L = 32, a reading every 0.1 s (137 buffers).  The meters' time does not depend on the samples'
    values, so the rows [C, rowSamples] are filled on the device (noise; the pads too: the packed meter never reads them).
      packed_f32 / packed_s16   Recordings.levels on fp32 / int16 rows     recordings_levels_zero_kernel + recordings_levels_in_kernel
    against, in the same process on the same rows,
      plain_f32 / plain_s16     SyllableDetector.levels / levelsPCM16 on the 64 rows as 64 recordings of rowSamples: the same
                                bytes, and the yardstick                    levels_in_kernel + levels_fold_kernel
      read_f32 / read_s16       a plain device read of the same bytes (torch's sum over the rows as 32-bit words; not code under test)
      loop_f32 / loop_s16       what a user writes today: K calls of syldet_levels_device* through a one-channel handle on pointers
                                into the packed rows, straight through the C ABI
    and the output meter, Recordings.outputLevels, against SyllableDetector.outputLevels on the plain rows' outputs (made on the
    device: uniform values).
    --cli N: also the tool end to end on N files of 5 s: --batch --levels-dir against one --levels run a file.

Everything runs in one process; the candidates alternate launch by launch, every launch between two HIP events of its own; after a
warm-up, the median of `launches` launches (the loops: of 5).  Writes profiles/recordings_levels_timing.json (or --out PATH) and
prints it as one JSON line.

    python tools/recordings_levels_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--cli N]
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

    launches, out_path, K, C, n_cli = 20, os.path.join(ROOT, "profiles", "recordings_levels_timing.json"), 2048, 64, 0
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
    assert torch.cuda.is_available(), "recordings_levels_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM, L = 3, 32
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

    def kernels(det, fn, repeats=7):
        got = {}
        for _ in range(repeats):
            fn()
            torch.cuda.synchronize()
            for name, ms in det.lastTimings():
                got.setdefault(name, []).append(ms)
        return {k: float(np.median(v)) for k, v in got.items()}

    results = {}
    with sd.SyllableDetector(cfg, channels=C) as det, sd.SyllableDetector(cfg, channels=1) as one, det.recordings(lengths) as rec:
        P = det.defaultBuffersPerReading(L)
        S, E = rec.rowSamples, rec.rowEvaluations
        first = rec.levelsLayout(L, P)
        total = int(first[-1])
        stream = det._stream_ptr(None)
        lib = _abi.lib
        starts = sorted({(s[1] * 4) % 16 for s in rec.slots}), sorted({(s[1] * 2) % 16 for s in rec.slots})
        results["shape"] = {"recordings": K, "rows": C, "row_samples": S, "row_evaluations": E, "fill_share": rec.fill, "L": L, "P": P,
                            "readings": total, "plain_readings": C * det.levelsCount(S, L, P),
                            "recording_starts_mod_16_bytes": {"f32": starts[0], "s16": starts[1]}}
        for name, dtype, size in (("f32", torch.float32, 4), ("s16", torch.int16, 2)):
            if dtype == torch.float32:
                rows = torch.randn((C, S), device=dev) * 0.1
            else:
                rows = torch.randint(-3000, 3000, (C, S), device=dev, dtype=torch.int16)
            words = rows.view(torch.int32)
            dst = torch.zeros(total, dtype=torch.float64, device=dev)
            dst2 = torch.zeros(total, dtype=torch.float64, device=dev)
            plain = det.levelsPCM16 if dtype == torch.int16 else det.levels
            fn1 = lib.syldet_levels_device_s16 if dtype == torch.int16 else lib.syldet_levels_device

            def loop():
                for (row, offset, _, _, n), f in zip(rec.slots, first):
                    fn1(one._h, rows.data_ptr() + size * (row * S + offset), n, n, L, P, dst2.data_ptr() + 8 * int(f), stream)

            # the two paths give the same bits before either is timed
            rec.levels(rows, L, P, out=dst)
            loop()
            differing = int((dst.view(torch.int64) != dst2.view(torch.int64)).sum())
            t = timed({"packed": lambda: rec.levels(rows, L, P, out=dst), "plain": lambda: plain(rows, L, P), "read": lambda: words.sum()})
            tl = timed({"loop": loop}, n=5)
            det.profile(True)
            k_ms = kernels(det, lambda: rec.levels(rows, L, P, out=dst))
            k_ms.update(kernels(det, lambda: plain(rows, L, P)))
            det.profile(False)
            med = {k: float(np.median(v)) for k, v in t.items()}
            results[name] = {"bytes_read": int(rows.numel() * size), "packed": stats(t["packed"]), "plain": stats(t["plain"]), "read": stats(t["read"]),
                             "loop": stats(tl["loop"]), "kernels_ms": k_ms, "packed_over_plain": med["packed"] / med["plain"],
                             "packed_over_read": med["packed"] / med["read"], "loop_over_packed": float(np.median(tl["loop"])) / med["packed"],
                             "packed_GBps": rows.numel() * size / med["packed"] / 1e6, "readings_differing_from_loop": differing}
            del rows, words, dst, dst2
            torch.cuda.empty_cache()
        # int16 rows once more with every length rounded up to a multiple of 2 hop: every recording then begins on a 16-byte line, and
        # what is left of the distance to the plain meter is not the 8-byte loads of the recordings that begin between two lines
        hop2 = 2 * int(det.geometry.hop)
        with det.recordings([-(-n // hop2) * hop2 for n in lengths]) as rec2:
            rows = torch.randint(-3000, 3000, (C, rec2.rowSamples), device=dev, dtype=torch.int16)
            dst = torch.zeros(int(rec2.levelsLayout(L, P)[-1]), dtype=torch.float64, device=dev)
            t = timed({"packed": lambda: rec2.levels(rows, L, P, out=dst), "plain": lambda: det.levelsPCM16(rows, L, P)})
            results["s16_every_start_on_a_16_byte_line"] = {
                "row_samples": rec2.rowSamples, "recording_starts_mod_16_bytes": sorted({(s[1] * 2) % 16 for s in rec2.slots}),
                "packed": stats(t["packed"]), "plain": stats(t["plain"]), "packed_over_plain": float(np.median(t["packed"]) / np.median(t["plain"]))}
            del rows, dst
            torch.cuda.empty_cache()
        # the output meter
        out = torch.rand((C, E, 1), device=dev)
        lv = torch.zeros(total, dtype=torch.float32, device=dev)
        t = timed({"packed": lambda: rec.outputLevels(out, 0, L, P, out=lv), "plain": lambda: det.outputLevels(out, S, 0, L, P)})
        det.profile(True)
        k_ms = kernels(det, lambda: rec.outputLevels(out, 0, L, P, out=lv))
        k_ms.update(kernels(det, lambda: det.outputLevels(out, S, 0, L, P)))
        det.profile(False)
        results["output"] = {"bytes_read": int(out.numel() * 4), "packed": stats(t["packed"]), "plain": stats(t["plain"]), "kernels_ms": k_ms,
                             "packed_over_plain": float(np.median(t["packed"]) / np.median(t["plain"]))}

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
                subprocess.run([cli, "-n", net, *audio, "--batch", "--levels-dir", os.path.join(d, "A")], check=True, capture_output=True)
                runs["batch"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                for p in paths:
                    subprocess.run([cli, "-n", net, "-a", p, "--levels", os.path.join(d, "one.tsv")], check=True, capture_output=True)
                runs["per_file"].append(time.perf_counter() - t0)
            same = all(open(os.path.join(d, "A", os.path.basename(p) + ".tsv"), "rb").read() != b"" for p in paths)
            results["cli"] = {"files": n_cli, "seconds_each": 5, "batch_s": float(np.median(runs["batch"])), "per_file_s": float(np.median(runs["per_file"])),
                              "per_file_over_batch": float(np.median(runs["per_file"]) / np.median(runs["batch"])), "tables_written": bool(same)}

    doc = {"workload": "%d recordings of 1 to 60 s on %d rows, L %d, a reading every 0.1 s; rows and outputs made on the device" % (K, C, L),
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every launch, candidates alternating, median of `launches` (the loops: of 5); kernels_ms: the handle's profile",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
