#!/usr/bin/env python3
"""Measurement: what the 16-bit PCM entry points cost against their fp32 twins.

    device  64 channels x 2^24 samples of synth.channels_on_device quantised to int16, the example detector (nets.from_npz(),
            hop 132, the fold kernel), the same audio as fp32 (x * 2^-15):
              dev_f32     run()         fused_s_kernel
              dev_s16     runPCM16()    fused_s_kernel's 16-bit PCM form (2 bytes a sample)
              dev_s16w    runPCM16()    on rows that start 2 bytes off a word: widen_s16_kernel + fused_s_kernel (route b)
            and at hop 128 (the fold kernel's CS8 ring): hop128_f32 / hop128_s16
    host    16 channels x 2^23 samples in page-locked memory (bank.PinnedArray), results into page-locked arrays:
              host_f32    runHost()          (4 bytes a sample across the bus)
              host_s16    runPCM16Host()     (2 bytes a sample)

Each configuration runs in its own child process, the configurations alternate within the run (rounds); kernel times come
from syldet_timings after a warm-up, host calls are timed by the wall clock around the blocking call.  Writes
profiles/pcm16_timing.json and prints it as one JSON line.

    python tools/pcm16_timing.py [rounds]
    python tools/pcm16_timing.py --child CASE      (one configuration, one JSON line: what a profiler run wraps)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys, time
sys.path.insert(0, %r)
import numpy as np
import torch
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import nets, synth
from syllable_detector_swift_amd.bank import PinnedArray
case = sys.argv[1]
base = nets.from_npz()
cfg = nets.variant(base, windowOverlap=128) if case.startswith("hop128") else base
res = {"case": case}
dev = torch.device("cuda", 0)
if case.startswith(("dev", "hop128")):
    C, S, WARM, N = 64, 1 << 24, 20, 60
    x16 = (synth.channels_on_device(C, S, dev, fs=cfg.samplingRate) * 32767.0).round_().to(torch.int16)
    if case.endswith("s16w"):                  # (the same samples, each row one element off a 4-byte word: the widened route)
        big = torch.zeros((C, S + 2), dtype=torch.int16, device=dev)
        big[:, 1:1 + S] = x16
        x16 = big[:, 1:1 + S]
    x = x16 if "s16" in case else x16.float().mul_(2.0 ** -15)
    det = sd.SyllableDetector(cfg, channels=C)
    E = det.countEvaluations(S)
    o = torch.empty((C, E, 1), dtype=torch.float32, device=dev)
    f = torch.empty((C, E), dtype=torch.uint8, device=dev)
    det.profile(True)
    go = det.runPCM16 if "s16" in case else det.run
    per, total = {}, []
    for i in range(WARM + N):
        go(x, o, f)
        if i >= WARM:
            t = [(name, ms) for name, ms in det.lastTimings() if name != "fixup_kernel"]
            for name, ms in t:
                per.setdefault(name, []).append(ms)
            total.append(sum(ms for _, ms in t))
    torch.cuda.synchronize()
    for v in per.values():
        v.sort()
    total.sort()
    med = {k: v[len(v) // 2] for k, v in per.items()}
    J = det.countFrames(S)
    res.update({"channels": C, "samples": S, "kernels": sorted(per), "kernel_ms": {k: round(v, 4) for k, v in med.items()},
                "total_ms_median": total[len(total) // 2], "total_ms_min": total[0],
                "frames_per_s": C * J / (total[len(total) // 2] * 1e-3)})
    # bytes the call moves in HBM at the least (what its kernels must read and write of samples), over 8 TB/s
    smp = C * S
    moved = smp * (2 + 4 + 4) if "widen_s16_kernel" in per else smp * (2 if "s16" in case else 4)
    res["sample_bytes"] = moved
    res["sample_bytes_over_8TBps"] = moved / 8e12 / (total[len(total) // 2] * 1e-3)
    det.close()
else:
    C, S, WARM, N = 16, 1 << 23, 3, 12
    x16 = (synth.channels_on_device(C, S, dev, fs=cfg.samplingRate) * 32767.0).round_().to(torch.int16).cpu().numpy()
    det = sd.SyllableDetector(cfg, channels=C)
    E = det.countEvaluations(S)
    s16 = case.endswith("s16")
    px = PinnedArray((C, S), np.int16 if s16 else np.float32)
    px.array[...] = x16 if s16 else x16.astype(np.float32) * np.float32(2.0 ** -15)
    po, pf = PinnedArray((C, E, 1), np.float32), PinnedArray((C, E), np.uint8)
    go = det.runPCM16Host if s16 else det.runHost
    wall = []
    for i in range(WARM + N):
        t0 = time.perf_counter()
        go(px.array, po.array, pf.array)
        if i >= WARM:
            wall.append(time.perf_counter() - t0)
    wall.sort()
    J = det.countFrames(S)
    res.update({"channels": C, "samples": S, "wall_ms_median": 1e3 * wall[len(wall) // 2], "wall_ms_min": 1e3 * wall[0],
                "frames_per_s": C * J / wall[len(wall) // 2], "input_bytes": C * S * (2 if s16 else 4),
                "input_GBps": C * S * (2 if s16 else 4) / wall[len(wall) // 2] / 1e9})
    px.free(); po.free(); pf.free()
    det.close()
print(json.dumps(res))
''' % ROOT

CASES = ["dev_f32", "dev_s16", "dev_s16w", "hop128_f32", "hop128_s16", "host_f32", "host_s16"]


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        r = subprocess.run([sys.executable, "-c", CHILD, sys.argv[2]], timeout=600)
        sys.exit(r.returncode)
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    got = {}
    for rnd in range(rounds):
        for case in CASES:
            r = subprocess.run([sys.executable, "-c", CHILD, case], capture_output=True, text=True, timeout=600)
            line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
            if r.returncode != 0 or not line.startswith("{"):
                print(json.dumps({"error": "child failed", "case": case, "rc": r.returncode, "stderr": r.stderr[-600:]}))
                sys.exit(1)
            got.setdefault(case, []).append(json.loads(line))
            print(line, flush=True)
    out = {"workload": "device: 64 channels x 2^24 samples, example detector (hop 132) and hop 128; host: 16 channels x 2^23 "
                       "samples, page-locked", "rounds": rounds, "results": []}
    by = {}
    for case, rs in got.items():
        key = "total_ms_median" if "total_ms_median" in rs[0] else "wall_ms_median"
        best = min(rs, key=lambda r: r[key])
        row = dict(best)
        row[key + "_rounds"] = [round(r[key], 4) for r in rs]
        out["results"].append(row)
        by[case] = row
    out["device_s16_over_f32_time"] = round(by["dev_s16"]["total_ms_median"] / by["dev_f32"]["total_ms_median"], 4)
    out["device_s16_over_widened_time"] = round(by["dev_s16"]["total_ms_median"] / by["dev_s16w"]["total_ms_median"], 4)
    out["hop128_widen_ms"] = by["hop128_s16"]["kernel_ms"].get("widen_s16_kernel")
    out["hop128_kernel_ms"] = {k: v for k, v in by["hop128_s16"]["kernel_ms"].items() if k != "widen_s16_kernel"}
    out["host_s16_over_f32_frames_per_s"] = round(by["host_s16"]["frames_per_s"] / by["host_f32"]["frames_per_s"], 4)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pcm16_timing.json"), "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
