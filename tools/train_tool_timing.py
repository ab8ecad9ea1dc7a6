#!/usr/bin/env python3
"""Measurement: training from the tool (syldet_train_input_range_device, syldet_train_adam_device, syldet_train_fit_device, --train).

    The workload of "Packed recordings": 2048 mono recordings of 1 to 60 s (seeded) on 64 rows of the example detector, one label a
    second in every recording, halfWidth = hop, class weights 0.5 / N_pos and 0.5 / N_neg.  The columns are filled on the device.
      fit_device_step   one step of Trainer.fitDevice (a call of 5 steps, divided by 5)      gradient + combine + adam kernels
      fit_torch_step    one step of Trainer.fit (torch.optim.Adam; a call of 5 steps, divided by 5) on the same arrays
      range             Trainer.inputRange over every recording's evaluations
      fit_input_map     Trainer.fitInputMap over the same evaluations (aligner windows and torch operators, in chunks); once
      read              a device read of the same columns (torch's sum; not code under test)
      adam              one Trainer.adamStep                                                  train_adam_kernel
      copy_3p           a device copy of 3 P floats (not code under test)
      tool              the tool's wall time on 8 files of 5 s, 16-bit, with --train (200 steps, seed 0, --train-fit-map) and without

Everything on the device runs in one process; the candidates of a group alternate call by call, every call between two HIP events
of its own; after a warm-up, the median of `launches` calls with the 10th and 90th percentiles.  Writes
profiles/train_tool_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/train_tool_timing.py [launches] [--out PATH] [--recordings K] [--rows C]
"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for extra in ("tests", "oracle"):                      # (the planted recordings of tests/train_cases.py, for the tool's run)
    sys.path.insert(0, os.path.join(ROOT, extra))


def main(argv):
    import numpy as np
    import torch
    import syllable_detector_swift_amd as sd
    from syllable_detector_swift_amd import nets

    launches, out_path, K, C = 20, os.path.join(ROOT, "profiles", "train_tool_timing.json"), 2048, 64
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
    assert torch.cuda.is_available(), "train_tool_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM = 3
    cfg = nets.from_npz()
    fs = cfg.samplingRate
    lengths = [int(v) for v in np.random.default_rng(2048).integers(int(fs), int(60 * fs), size=K)]
    labels = [np.arange(1, n // int(fs) + 1, dtype=np.int64) * int(fs) for n in lengths]

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

    def stats(ms, per=1.0):
        ms = [m / per for m in ms]
        return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)), "calls": len(ms)}

    results = {}
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(lengths) as rec, rec.trainer() as tr:
        E, J, bins, hop, first = rec.rowEvaluations, det.countFrames(rec.rowSamples), det.geometry.bins, det.geometry.hop, det.geometry.first_index
        cols = torch.rand((C, J, bins), device=dev) + 0.01
        theta = tr.params()
        t, w1 = tr.targets(labels, hop, 1.0, 1.0)
        n_pos = int((t > 0).sum())
        n_all = int((w1 > 0).sum())
        t, w = tr.targets(labels, hop, 0.5 / n_pos, 0.5 / (n_all - n_pos))
        P = tr.paramCount
        results["shape"] = {"recordings": K, "rows": C, "row_frames": J, "row_evaluations": E, "parameters": P, "tile": tr.tile, "evaluations": n_all,
                            "positives": n_pos, "columns_bytes": int(cols.numel() * 4), "input_matrix_bytes": n_all * bins * cfg.timeRange * 4}
        STEPS = 5
        tm = timed({"fit_device": lambda: tr.fitDevice(cols, t, w, theta, STEPS), "fit_torch": lambda: tr.fit(cols, t, w, theta, STEPS)})
        results["fit_device_step"] = stats(tm["fit_device"], STEPS)
        results["fit_torch_step"] = stats(tm["fit_torch"], STEPS)
        a, b = tr.fitDevice(cols, t, w, theta, STEPS), tr.fitDevice(cols, t, w, theta, STEPS)
        results["fit_run_to_run_identical"] = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]))
        tm = timed({"range": lambda: tr.inputRange(cols, w), "read": lambda: cols.sum()})
        results["range"] = stats(tm["range"])
        results["read"] = stats(tm["read"])
        results["range"]["over_read"] = results["range"]["median_ms"] / results["read"]["median_ms"]
        slots = rec.slots
        events = [first + hop * np.arange(s[3], dtype=np.int64) for s in slots]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fitted = tr.fitInputMap(cols, events)
        torch.cuda.synchronize()
        results["fit_input_map"] = {"seconds": time.perf_counter() - t0, "calls": 1}
        r, n = tr.inputRange(cols, w)
        xo, g = sd.trainInputMapHost(r.cpu().numpy())
        m = fitted.net.inputProcessing[1]
        results["range_equals_fit_input_map"] = {"count": int(n), "x_offsets_max_abs_difference": float(np.abs(xo - m.xOffsets).max()),
                                                 "gains_max_relative_difference": float((np.abs(g - m.gains) / np.abs(m.gains)).max())}
        out = (torch.empty(2, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.float32, device=dev))
        tr.gradient(cols, theta, t, w, out=out)
        p = theta.clone()
        src, dst = torch.empty(3 * P, device=dev), torch.empty(3 * P, device=dev)
        step = [0]

        def adam():
            step[0] += 1
            tr.adamStep(p, out[0], out[1], step[0])

        tm = timed({"adam": adam, "copy_3p": lambda: dst.copy_(src)}, n=max(launches, 50))
        results["adam"] = stats(tm["adam"])
        results["copy_3p"] = stats(tm["copy_3p"])

    # the tool: 8 files of 5 s
    import train_cases as cases
    import wavutil
    cli = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")
    with tempfile.TemporaryDirectory() as d:
        net = os.path.join(d, "net.txt")
        open(net, "w").write(cfg.toText())
        audio, lines = [], []
        for k in range(8):
            x, pos = cases.planted_channel(10 + k, n=5 * 44100)
            path = os.path.join(d, "f%d.wav" % k)
            wavutil.write_wav(path, np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)[:, None], 44100, "pcm16")
            audio += ["-a", path]
            lines += ["%s\t0\t%d" % (path, q + first) for q in pos]
        open(os.path.join(d, "labels.tsv"), "w").write("\n".join(lines) + "\n")
        train = ["--train", os.path.join(d, "labels.tsv"), "--train-out", os.path.join(d, "out.txt"), "--train-seed", "0", "--train-fit-map", "--train-log",
                 os.path.join(d, "log.tsv")]
        wall = {"with_train": [], "without": []}
        for rep in range(4):
            for name, extra in (("without", []), ("with_train", train)):
                t0 = time.perf_counter()
                r = subprocess.run([cli, "-n", net, *audio, "--batch", *extra], capture_output=True, timeout=600)
                assert r.returncode == 0, r.stderr
                if rep:
                    wall[name].append(time.perf_counter() - t0)
        log = [l.split("\t") for l in open(os.path.join(d, "log.tsv")).read().splitlines() if not l.startswith("#")]
        results["tool"] = {"files": 8, "seconds_each": 5, "steps": 200, "labels": len(lines),
                           "with_train_s": {"median": float(np.median(wall["with_train"])), "min": min(wall["with_train"]), "max": max(wall["with_train"])},
                           "without_s": {"median": float(np.median(wall["without"])), "min": min(wall["without"]), "max": max(wall["without"])},
                           "first_loss": float(log[0][1]), "last_loss": float(log[-1][1])}

    doc = {"workload": "%d recordings of 1 to 60 s on %d rows, one label a second, halfWidth = hop; the columns made on the device" % (K, C),
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every call, the candidates of a group alternating, median and 10th / 90th percentile of `launches` calls after 3 of "
                     "warm-up (fit: a call of 5 steps divided by 5; fit_input_map: one call, wall clock; the tool: wall clock of 3 runs after one)",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
