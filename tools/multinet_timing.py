#!/usr/bin/env python3
"""Measurement: what a network per channel costs.  64 channels x 2^24 samples of synth.channels_on_device through K networks
of the example detector's structure (nets.from_npz(), nets.perturbed variants), K = 1, 2, 8, 64:

    a  one syldet_create handle (one network for every channel: the reference point)
    b  one syldet_create_multi handle, channel c on network (5 c) mod K
    c  K syldet_create handles of 64 / K channels each, one after another on one stream (the only way before multi handles)
    d  the streaming callback round trip -- callbacks of 32 audio frames for 64 channels (bench.py's live record), each
       appendInterleavedData + processAll + draining processNewValue -- for b (one handle) against c (K handles, each fed its
       channels of the stream)

Each configuration runs in its own child process, the configurations alternate within the run (rounds), kernel times come
from syldet_timings after the warm-up tools/ab_kernel.py uses (the first 100 launches: the clock governor's ramp).  Prints
one JSON line.

    python tools/multinet_timing.py [rounds]
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
case, K = sys.argv[1], int(sys.argv[2])
base = nets.from_npz()
cfgs = [base] + [nets.perturbed(base, 1000 + k) for k in range(1, K)]
C, S, WARM, N = 64, 1 << 24, 100, 200
net = [(5 * c) %% K for c in range(C)]
res = {"case": case, "K": K}
if case in ("a", "b", "c"):
    x = synth.channels_on_device(C, S, torch.device("cuda", 0), fs=base.samplingRate)
    if case == "a":
        dets = [(sd.SyllableDetector(base, channels=C), x)]
    elif case == "b":
        dets = [(sd.SyllableDetector.multi(cfgs, net), x)]
    else:                                        # K handles over contiguous blocks of 64 / K channels
        n = C // K
        dets = [(sd.SyllableDetector(cfgs[k], channels=n), x[k * n:(k + 1) * n]) for k in range(K)]
    outs = []
    for d, xs in dets:
        E = d.countEvaluations(S)
        outs.append((torch.empty((d.channels, E, 1), dtype=torch.float32, device="cuda"),
                     torch.empty((d.channels, E), dtype=torch.uint8, device="cuda")))
        d.profile(True)
    kern, wall = [], []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(WARM + N):
        ev0.record()
        t = 0.0
        for (d, xs), (o, f) in zip(dets, outs):
            d.run(xs, o, f)
        ev1.record()
        if i >= WARM:
            t = sum(tm for d, _ in dets for name, tm in d.lastTimings() if name != "fixup_kernel")
            torch.cuda.synchronize()
            kern.append(t)
            wall.append(ev0.elapsed_time(ev1))
    torch.cuda.synchronize()
    res["names"] = sorted(set(name for d, _ in dets for name, _ in d.lastTimings()))
    kern.sort(); wall.sort()
    res.update({"kernel_ms_median": kern[len(kern) // 2], "kernel_ms_min": kern[0], "step_ms_median": wall[len(wall) // 2]})
    for d, _ in dets:
        d.close()
else:                                            # d: streaming round trip, "d_b" one multi handle, "d_c" K handles
    n = 32
    rounds = 3000
    xh = np.stack([synth.channel(n * rounds, 3000 + c) for c in range(C)])
    if case == "d_b":
        dets = [(sd.SyllableDetector.multi(cfgs, net), None)]
    else:
        m = C // K
        dets = [(sd.SyllableDetector(cfgs[k], channels=m), np.arange(k * m, (k + 1) * m, dtype=np.int32)) for k in range(K)]
    rt, evals = [], 0
    for r in range(rounds):
        blk = np.ascontiguousarray(xh[:, r * n:(r + 1) * n].T)
        t0 = time.perf_counter()
        for d, src in dets:
            d.appendInterleavedData(blk, src)
            d.processAll()
            for c in range(d.channels):
                while d.processNewValue(c):
                    evals += 1
        rt.append(time.perf_counter() - t0)
    rt = np.array(rt[rounds // 10:])
    res.update({"samples_per_callback": n, "evaluations": evals, "round_trip_us_median": 1e6 * float(np.median(rt)),
                "round_trip_us_p99": 1e6 * float(np.percentile(rt, 99))})
    for d, _ in dets:
        d.close()
print(json.dumps(res))
''' % ROOT


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    configs = [(case, K) for K in (1, 2, 8, 64) for case in ("a", "b", "c")] + [(case, K) for K in (1, 2, 8, 64) for case in ("d_b", "d_c")]
    got = {}
    for rnd in range(rounds):
        for case, K in configs:
            if case == "a" and K != 1:
                continue                         # (a does not depend on K)
            r = subprocess.run([sys.executable, "-c", CHILD, case, str(K)], capture_output=True, text=True, timeout=600)
            line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
            if r.returncode != 0 or not line.startswith("{"):
                print(json.dumps({"error": "child failed", "case": case, "K": K, "rc": r.returncode, "stderr": r.stderr[-600:]}))
                sys.exit(1)
            got.setdefault((case, K), []).append(json.loads(line))
    out = {"workload": "64 channels x 2^24 samples, nets.from_npz() structure, K networks", "rounds": rounds, "results": []}
    for (case, K), rs in got.items():
        row = {"case": case, "K": K}
        for key in ("kernel_ms_median", "kernel_ms_min", "step_ms_median", "round_trip_us_median", "round_trip_us_p99"):
            if key in rs[0]:
                row[key] = round(min(r[key] for r in rs), 4)          # best round of the run
                row[key + "_rounds"] = [round(r[key], 4) for r in rs]
        if "names" in rs[0]:
            row["kernels"] = rs[0]["names"]
        out["results"].append(row)
    a = next(r for r in out["results"] if r["case"] == "a")
    for r in out["results"]:
        if r["case"] in ("b", "c"):
            r["kernel_vs_a"] = round(r["kernel_ms_median"] / a["kernel_ms_median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
