#!/usr/bin/env python3
"""Measurement: one fit of N networks (syldet_trainer_create_multi) against the loop of N plain fits, and the plain trainer's
gradient against another checkout of the project (the parent commit) on the same box.

    fit      N networks of the example detector's shape (nets.from_npz(), 290 -> 4 TanSig -> 1 PureLin, hop 132; the others are
             nets.perturbed copies), rows of 60 s each, one label a second, halfWidth = hop, `steps` Adam steps from seeded weights.
               multi   one MultiTrainer.fitDevice on the multi bank: 3 x steps launches
               loop    the reference for this number: N plain banks, N plain trainers, N Trainer.fitDevice calls one after another
                       on the same arrays gathered per network: N x 3 x steps launches
             for 64 networks x 1 row and for 8 networks x 8 rows.  Each candidate is timed whole -- a host clock around the call(s)
             and a device synchronise -- after a warm-up call of each, the candidates alternating, `repeats` times; the median.
             The two must agree to the bit (parameters and histories): checked on the timed sizes, reported.
    plain    (--plain-ab BASE) the plain trainer's gradient on the archive of MEASUREMENTS "Training" (2048 recordings of 1 to 60 s
             on 64 rows, every evaluation selected), this checkout against the checkout at BASE (its own package and library), each
             run in a child process of its own, alternating, `rounds` rounds; per run the median of 100 calls between HIP events after
             30 warm-up calls.  The spread of BASE's own medians from round to round is the yardstick.

Writes profiles/train_multi_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/train_multi_timing.py [--steps K] [--repeats R] [--plain-ab BASE] [--rounds N] [--out PATH] [--seconds S]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import nets
cfg = nets.from_npz()
fs = cfg.samplingRate
K, C, WARM, CALLS = 2048, 64, 30, 100
lengths = [int(v) for v in np.random.default_rng(2048).integers(int(fs), int(60 * fs), size=K)]
labels = [np.arange(1, n // int(fs) + 1, dtype=np.int64) * int(fs) for n in lengths]
with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(lengths) as rec, rec.trainer() as tr:
    J = det.countFrames(rec.rowSamples)
    torch.manual_seed(0)
    cols = torch.rand((C, J, det.geometry.bins), device="cuda") + 0.01
    theta = tr.params()
    t, w = tr.targets(labels, det.geometry.hop, 1.0, 1.0)
    out = (torch.empty(2, dtype=torch.float64, device="cuda"), torch.empty(tr.paramCount, dtype=torch.float32, device="cuda"))
    ev = []
    for r in range(WARM + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.gradient(cols, theta, t, w, out=out)
        b.record()
        if r >= WARM:
            ev.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    print(json.dumps({"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "p90_ms": ms[int(0.9 * len(ms))],
                      "gradient_bits": int(out[1].view(torch.int32).to(torch.int64).sum()), "loss": float(out[0][0])}))
'''


def fit_case(N, rows_per, steps, repeats, seconds):
    import numpy as np
    import torch
    import syllable_detector_swift_amd as sd
    from syllable_detector_swift_amd import nets

    base = nets.from_npz()
    fs = int(base.samplingRate)
    cfgs = [base] + [nets.perturbed(base, 100 + n) for n in range(1, N)]
    C = N * rows_per
    channel_net = [r % N for r in range(C)]            # interleaved: network n has the rows n, n + N, ..
    n_samples = seconds * fs
    labels = [np.arange(1, seconds + 1, dtype=np.int64) * fs for _ in range(C)]
    start = np.stack([sd.trainInitHost(n, 290, 4, 1) for n in range(N)])
    with sd.SyllableDetector.multi(cfgs, channel_net) as det, det.multiTrainer() as mt:
        E, J, hop = det.countEvaluations(n_samples), det.countFrames(n_samples), det.geometry.hop
        torch.manual_seed(N)
        cols = torch.rand((C, J, det.geometry.bins), device="cuda") + 0.01
        t, w = mt.targets(labels, hop, 1.0, 1.0, n_evals=E)
        r, _ = mt.inputRange(cols, w)
        maps = [sd.trainInputMapHost(r[n].cpu().numpy()) for n in range(N)]
        for n in range(N):
            mt.setInputMap(n, *maps[n])
        p0 = torch.from_numpy(start).cuda()
        plain = []
        for n in range(N):
            rows = [r_ for r_ in range(C) if channel_net[r_] == n]
            d = sd.SyllableDetector(cfgs[n], channels=len(rows))
            tr = d.trainer()
            tr.setInputMap(*maps[n])
            plain.append((d, tr, cols[rows].contiguous(), t[rows].contiguous(), w[rows].contiguous(), p0[n].contiguous()))

        def multi():
            return mt.fitDevice(cols, t, w, p0, steps=steps)

        def loop():
            return [tr.fitDevice(c_, t_, w_, p_, steps=steps) for _, tr, c_, t_, w_, p_ in plain]

        got_m, got_l = multi(), loop()                 # (the warm-up of both, and the comparison)
        torch.cuda.synchronize()
        same = all(torch.equal(got_m[0][n].view(torch.int32), got_l[n][0].view(torch.int32))
                   and torch.equal(got_m[1][:, n].contiguous().view(torch.int64), got_l[n][1].view(torch.int64)) for n in range(N))
        times = {"multi": [], "loop": []}
        for _ in range(repeats):
            for name, fn in (("multi", multi), ("loop", loop)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        groups = mt.groups(E).tolist()
        for d, tr, *_ in plain:
            tr.close()
            d.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"networks": N, "rows_per_network": rows_per, "row_seconds": seconds, "row_evaluations": int(E), "steps": steps, "tile": mt.tile,
            "groups_per_network": groups[0], "launches_multi": 3 * steps, "launches_loop": 3 * steps * N,
            "multi_ms": med["multi"], "loop_ms": med["loop"], "loop_over_multi": med["loop"] / med["multi"],
            "multi_all_ms": sorted(times["multi"]), "loop_all_ms": sorted(times["loop"]), "identical_to_the_bit": bool(same),
            "mean_loss_first_last": [float(got_m[1][0].mean()), float(got_m[1][-1].mean())]}


def plain_ab(base_root, rounds):
    runs = {"this": [], "base": []}
    for rnd in range(rounds):
        for name, root in (("base", base_root), ("this", ROOT)):
            env = {k: v for k, v in os.environ.items() if k != "SYLDET_LIB"}
            r = subprocess.run([sys.executable, "-c", CHILD, root], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError("%s: %s" % (name, r.stderr.strip()[-500:]))
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print("round %d  %-5s %s" % (rnd, name, runs[name][-1]), flush=True)
    med = {k: sorted(x["median_ms"] for x in v) for k, v in runs.items()}
    spread = med["base"][-1] - med["base"][0]
    mid = lambda v: v[len(v) // 2]
    return {"workload": "2048 recordings of 1 to 60 s on 64 rows, every evaluation selected: Trainer.gradient (gradient + combine kernels)",
            "rounds": rounds, "this_median_ms": med["this"], "base_median_ms": med["base"], "base_spread_ms": spread,
            "this_minus_base_ms": mid(med["this"]) - mid(med["base"]),
            "within_base_spread": bool(med["base"][0] - spread <= mid(med["this"]) <= med["base"][-1] + spread),
            "same_bits": len({x["gradient_bits"] for v in runs.values() for x in v}) == 1 and len({x["loss"] for v in runs.values() for x in v}) == 1}


def main(argv):
    steps, repeats, rounds, seconds, base_root, out_path = 200, 5, 4, 60, None, os.path.join(ROOT, "profiles", "train_multi_timing.json")
    i = 0
    while i < len(argv):
        if argv[i] == "--steps":
            steps = int(argv[i + 1])
        elif argv[i] == "--repeats":
            repeats = int(argv[i + 1])
        elif argv[i] == "--rounds":
            rounds = int(argv[i + 1])
        elif argv[i] == "--seconds":
            seconds = int(argv[i + 1])
        elif argv[i] == "--plain-ab":
            base_root = os.path.abspath(argv[i + 1])
        elif argv[i] == "--out":
            out_path = argv[i + 1]
        else:
            raise SystemExit(__doc__)
        i += 2
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "train_multi_timing needs a GPU"
    doc = {"device": torch.cuda.get_device_name(0),
           "timing": "fit: a host clock around the whole call(s) and a device synchronise, the candidates alternating, the median of "
                     "`repeats`; plain: HIP events around every call, the median of 100 after 30, a child process a run",
           "fit": [fit_case(64, 1, steps, repeats, seconds), fit_case(8, 8, steps, repeats, seconds)]}
    for case in doc["fit"]:
        print("fit %d x %d: multi %.1f ms, loop %.1f ms, loop / multi %.2f, identical %s" %
              (case["networks"], case["rows_per_network"], case["multi_ms"], case["loop_ms"], case["loop_over_multi"], case["identical_to_the_bit"]), flush=True)
    if base_root:
        doc["plain_gradient"] = plain_ab(base_root, rounds)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
