#!/usr/bin/env python3
"""Measurement: what a gradient of the network over an archive costs (syldet_train_gradient_device; kernels_train.hip).

    The workload of "Packed recordings": 2048 mono recordings of 1 to 60 s (seeded) on 64 rows of the example detector
    (nets.from_npz(), 290 -> 4 TanSig -> 1 PureLin, hop 132), one label a second in every recording, halfWidth = hop.  The columns
    are filled on the device (positive values of a spectrogram's size: the kernels' time does not depend on them).
      all         every evaluation of every recording selected                             train_gradient_kernel + train_combine_kernel
      subsampled  the positives and one negative in sixteen
    against, in the same process on the same arrays:
      read        a device read of the same columns (torch's sum; not code under test): the floor of a pass over them
      loop        what a user writes today: per row and chunk the selected evaluations unfolded into the [n, 290] matrix, the same
                  forward in torch, backward() -- on both selections

Everything runs in one process; the candidates alternate launch by launch, every launch between two HIP events of its own; after a
warm-up, the median of `launches` launches (the loop: of 3).  Writes profiles/train_timing.json (or --out PATH) and prints it as one
JSON line.

    python tools/train_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--chunk N]
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

    launches, out_path, K, C, chunk = 20, os.path.join(ROOT, "profiles", "train_timing.json"), 2048, 64, 1 << 19
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--recordings":
            K, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--rows":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--chunk":
            chunk, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert launches >= 20, "at least 20 launches a candidate"
    assert torch.cuda.is_available(), "train_timing needs a GPU"
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
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(lengths) as rec, rec.trainer() as tr:
        E, J, bins, T, hop = rec.rowEvaluations, det.countFrames(rec.rowSamples), det.geometry.bins, cfg.timeRange, det.geometry.hop
        I = bins * T
        cols = torch.rand((C, J, bins), device=dev) + 0.01
        theta = tr.params()
        t, w_all = tr.targets(labels, hop, 1.0, 1.0)
        keep = (torch.arange(E, device=dev) % 16 == 0)[None, :] | (t[:, :, 0] > 0)
        w_sub = torch.where(keep, w_all, torch.zeros_like(w_all))
        out = (torch.empty(2, dtype=torch.float64, device=dev), torch.empty(tr.paramCount, dtype=torch.float32, device=dev))
        n_all, n_sub = int((w_all > 0).sum()), int((w_sub > 0).sum())
        results["shape"] = {"recordings": K, "rows": C, "row_frames": J, "row_evaluations": E, "bins": bins, "inputs": I, "parameters": tr.paramCount,
                            "tile": tr.tile, "columns_bytes": int(cols.numel() * 4), "input_matrix_bytes": int(n_all) * I * 4,
                            "selected_all": n_all, "selected_subsampled": n_sub}
        fns = {"all": lambda: tr.gradient(cols, theta, t, w_all, out=out), "subsampled": lambda: tr.gradient(cols, theta, t, w_sub, out=out),
               "read": lambda: cols.sum()}
        tm = timed(fns)
        det.profile(True)
        k_all, k_sub = kernels(det, fns["all"]), kernels(det, fns["subsampled"])
        det.profile(False)
        med = {k: float(np.median(v)) for k, v in tm.items()}
        H = cfg.net.layers[0].outputs
        flops = lambda n: 4.0 * n * I * H                  # two multiply-adds an input and hidden unit: forward and dW1
        for name, n, k_ms in (("all", n_all, k_all), ("subsampled", n_sub, k_sub)):
            results[name] = {"selected": n, "call": stats(tm[name]), "kernels_ms": k_ms, "over_read": med[name] / med["read"],
                             "first_layer_GFLOPs_per_s": flops(n) / med[name] / 1e6, "columns_GBps": cols.numel() * 4 / med[name] / 1e6}
        results["read"] = {"call": stats(tm["read"]), "GBps": cols.numel() * 4 / med["read"] / 1e6}

        # the loop a user writes today
        fn_l2, fn_map = cfg.net.inputProcessing
        xo, gain = torch.from_numpy(fn_map.xOffsets).to(dev), torch.from_numpy(fn_map.gains).to(dev)
        om = cfg.net.outputProcessing[0]
        oxo, og, oy = float(om.xOffsets[0]), float(om.gains[0]), float(om.y)

        def loop(w):
            p = theta.clone().requires_grad_(True)
            W1, b1, W2, b2 = p[:H * I].view(H, I), p[H * I:H * I + H], p[H * I + H:H * I + 2 * H].view(1, H), p[H * I + 2 * H:]
            total = torch.zeros((), dtype=torch.float64, device=dev)
            for c in range(C):
                for e0 in range(0, E, chunk):
                    n = min(chunk, E - e0)
                    sel = torch.nonzero(w[c, e0:e0 + n] > 0)[:, 0]          # only the selected evaluations are unfolded and run
                    x = cols[c, e0:e0 + n + T - 1].unfold(0, T, 1)[sel].permute(0, 2, 1).reshape(sel.numel(), I)
                    x = x / torch.sqrt((x * x).sum(dim=1, keepdim=True))
                    x = (x - xo) * gain + fn_map.y
                    y = torch.tanh(x @ W1.T + b1) @ W2.T + b2
                    y = (y - oy) / og + oxo
                    loss = (w[c, e0:e0 + n][sel] * ((y - t[c, e0:e0 + n][sel]) ** 2).sum(dim=1)).sum()
                    loss.backward()
                    total += loss.detach().double()
            return total, p.grad

        results["loop"] = {"chunk_evaluations": chunk}
        for name, w in (("all", w_all), ("subsampled", w_sub)):
            loss_k, _, grad_k = tr.gradient(cols, theta, t, w)
            loss_l, grad_l = loop(w)
            torch.cuda.synchronize()
            tl = timed({"loop": lambda: loop(w)}, n=3)
            results["loop"][name] = {"call": stats(tl["loop"]), "loop_over_kernel": float(np.median(tl["loop"])) / med[name],
                                     "loss_relative_difference": abs(float(loss_l) - float(loss_k)) / abs(float(loss_k)),
                                     "gradient_relative_difference": float((grad_l - grad_k).norm() / grad_k.norm())}
        a, b = tr.gradient(cols, theta, t, w_all), tr.gradient(cols, theta, t, w_all)
        results["run_to_run_identical"] = bool(torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and float(a[0]) == float(b[0]))

    doc = {"workload": "%d recordings of 1 to 60 s on %d rows, one label a second, halfWidth = hop; the columns made on the device" % (K, C),
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every call, candidates alternating, median of `launches` (the loop: of 3); kernels_ms: the handle's profile",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
