#!/usr/bin/env python3
"""Measurement: what a mixed bank costs (syldet_create_mixed: networks of different bands and shapes in one handle).

    batch  64 channels x 2^24 samples of synth.channels_on_device, three classes interleaved (channel c on network c mod 3):
           the example detector (nets.from_npz()), the same framing with a narrower band (other bins, another first layer),
           and 512-point frames with 8 hidden units and log columns behind normalize (AUTO keeps it on the generic engine).
             mixed    one mixed handle
             classes  the three classes' own handles, each on its own contiguous channels, one after another on one stream
    stream the streaming callback round trip -- callbacks of 32 audio frames for 64 channels (bench.py's live record), each
           appendInterleavedData + processAll + draining processNewValue -- for k = 1, 2, 4, 8 classes (k fold-kernel networks
           of different bands, channel c on network c mod k):
             s_mixed  one mixed handle
             s_sep    k handles, each fed its channels of the stream

Each configuration runs in its own child process, the configurations alternate within the run (rounds), kernel times come
from syldet_timings after a warm-up of 100 launches.  Writes profiles/mixed_timing.json and prints it as one JSON line.

    python tools/mixed_timing.py [rounds]
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

def with_band(lo, hi, N=None, hidden=4, seed=0, in_fns=("l2normalize", "mapminmax"), **changes):
    N = N or base.fourierLength
    f0, f1 = sd.frequencyIndexRange(N, base.samplingRate, lo, hi)
    net = nets.random_net(np.random.default_rng(seed), (f1 - f0) * base.timeRange, (hidden,), 1, in_fns=in_fns)
    return nets.variant(base, fourierLength=N, freqRange=(lo, hi), net=net, thresholds=[0.1], **changes)

C = 64
res = {"case": case, "K": K}
if case in ("mixed", "classes"):
    S, WARM, N = 1 << 24, 100, 200
    cfgs = [base, with_band(2000.0, 5000.0, seed=1),
            with_band(1000.0, 9000.0, N=512, hidden=8, seed=2, in_fns=("normalize", "mapminmax"), spectrogramScaling="log")]
    net = [c %% 3 for c in range(C)]
    x = synth.channels_on_device(C, S, torch.device("cuda", 0), fs=base.samplingRate)
    if case == "mixed":
        dets = [(sd.SyllableDetector.mixed(cfgs, net), x)]
    else:
        dets, c0 = [], 0
        for k in range(3):
            n = net.count(k)
            dets.append((sd.SyllableDetector(cfgs[k], channels=n), x[c0:c0 + n]))
            c0 += n
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
else:                                            # streaming round trip: one mixed handle against K handles
    cfgs = [with_band(2000.0 + 170.0 * k, 7000.0 - 170.0 * k, seed=k) for k in range(K)]
    net = [c %% K for c in range(C)]
    n, rounds = 32, 2000
    xh = np.stack([synth.channel(n * rounds, 3000 + c) for c in range(C)])
    if case == "s_mixed":
        dets = [(sd.SyllableDetector.mixed(cfgs, net), None)]
    else:
        dets = [(sd.SyllableDetector(cfgs[k], channels=net.count(k)), np.array([c for c in range(C) if net[c] == k], np.int32))
                for k in range(K)]
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
    configs = [("mixed", 3), ("classes", 3)] + [(case, K) for K in (1, 2, 4, 8) for case in ("s_mixed", "s_sep")]
    got = {}
    for rnd in range(rounds):
        for case, K in configs:
            r = subprocess.run([sys.executable, "-c", CHILD, case, str(K)], capture_output=True, text=True, timeout=600)
            line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
            if r.returncode != 0 or not line.startswith("{"):
                print(json.dumps({"error": "child failed", "case": case, "K": K, "rc": r.returncode, "stderr": r.stderr[-600:]}))
                sys.exit(1)
            got.setdefault((case, K), []).append(json.loads(line))
    out = {"workload": "batch: 64 channels x 2^24 samples, three interleaved classes; stream: 64 channels, 32-frame callbacks, "
                       "k fold-kernel classes", "rounds": rounds, "results": []}
    for (case, K), rs in got.items():
        row = {"case": case, "K": K}
        for key in ("kernel_ms_median", "kernel_ms_min", "step_ms_median", "round_trip_us_median", "round_trip_us_p99"):
            if key in rs[0]:
                row[key] = round(min(r[key] for r in rs), 4)          # best round of the run
                row[key + "_rounds"] = [round(r[key], 4) for r in rs]
        if "names" in rs[0]:
            row["kernels"] = rs[0]["names"]
        out["results"].append(row)
    by = {(r["case"], r["K"]): r for r in out["results"]}
    out["mixed_vs_classes_kernel"] = round(by[("mixed", 3)]["kernel_ms_median"] / by[("classes", 3)]["kernel_ms_median"], 4)
    one = by[("s_mixed", 1)]["round_trip_us_median"]
    out["stream_us_per_added_class"] = {str(K): round((by[("s_mixed", K)]["round_trip_us_median"] - one) / (K - 1), 2) for K in (2, 4, 8)}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mixed_timing.json"), "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
