#!/usr/bin/env python3
"""Measurement: what the TTL trigger track (syldet_trigger*, kernels_trigger.hip) costs.

    64 channels x 2^24 samples, the example detector (nets.from_npz(), hop 132), L = 32, N = 44, no latency; the flags of one run()
    on the benchmark's input expanded as
      s16      triggerTrackPCM16                 trigger_scan_kernel + trigger_kernel                   2 GiB written
      mux      triggerMuxPCM16                   trigger_scan_kernel + trigger_interleaved_s16_kernel   2 GiB read, 4 GiB written
      onsets   triggerOnsets                     trigger_scan_kernel + trigger_onsets_kernel
    against
      fill     torch's fill_(0) of the int16 track's 2 GiB: the practical store-bandwidth ceiling (not code under test)
      trace    trace(dtype=int16) of the same handle: the same bytes written, the yardstick
      copy     (mux) a device copy of the 2 GiB of audio into one half of the 4 GiB buffer and a fill of the other: the bytes the mux moves
      torch    the same track and onsets made with PyTorch operators on the device
    the time of each of the four kernels (the handle's profile), and rehearse() against run() alone.

Everything runs in one process; the candidates alternate launch by launch, every launch between two HIP events of its own; after a
warm-up, the median of `launches` launches, with the 10th and 90th percentile.  Writes profiles/trigger_timing.json (or --out PATH)
and prints it as one JSON line.

    python tools/trigger_timing.py [launches] [--out PATH] [--channels C] [--log2-samples L]
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

    launches, out_path, C, lg = 20, os.path.join(ROOT, "profiles", "trigger_timing.json"), 64, 24
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--channels":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--log2-samples":
            lg, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert launches >= 20, "at least 20 launches a candidate"
    assert torch.cuda.is_available(), "trigger_timing needs a GPU"
    dev = torch.device("cuda", 0)
    S, WARM, L, N, LAT = 1 << lg, 3, 32, 44, 0
    cfg = nets.from_npz()

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

    def kernels(det, fn, repeats=7):
        """{kernel: median ms} of fn's launches under the handle's profile"""
        got = {}
        for _ in range(repeats):
            fn()
            torch.cuda.synchronize()
            for name, ms in det.lastTimings():
                got.setdefault(name, []).append(ms)
        return {k: float(np.median(v)) for k, v in got.items()}

    x = synth.channels_on_device(C, S, dev, fs=cfg.samplingRate)
    results = {}
    with sd.SyllableDetector(cfg, channels=C) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        out, fl = det.run(x)
        torch.cuda.synchronize()
        E = int(fl.shape[1])
        track = torch.empty((C, S), dtype=torch.int16, device=dev)
        tr = torch.empty((C, S), dtype=torch.int16, device=dev)

        Bp = (S + 2 * L - 2) // L
        e_buf = (D + torch.arange(E, device=dev, dtype=torch.int64) * hop - 1) // L
        b_idx = torch.arange(Bp, device=dev, dtype=torch.int32)

        def torch_table(fl=fl):
            seen = torch.zeros((C, Bp), dtype=torch.bool, device=dev)
            c_i, e_i = fl.nonzero(as_tuple=True)
            seen[c_i, e_buf[e_i]] = True
            last = torch.where(seen, b_idx[None, :], torch.tensor(-1, dtype=torch.int32, device=dev)).cummax(dim=1).values
            return seen, last

        def torch_track(fl=fl):
            _, last = torch_table(fl)
            s = torch.arange(S, device=dev, dtype=torch.int64)
            q = ((s - LAT) // L - 1).clamp_(0, Bp - 1)
            b = last[:, q].to(torch.int64)
            high = (s[None, :] - LAT >= L) & (b >= 0) & (s[None, :] < (b + 1) * L + LAT + N)
            return high.to(torch.int16) * 32767

        def torch_onsets():
            seen, last = torch_table()
            prev = torch.cat([torch.full((C, 1), -1, dtype=torch.int32, device=dev), last[:, :-1]], dim=1)
            t = (b_idx.to(torch.int64) + 1) * L + LAT
            on = seen & (t[None, :] < S) & ((prev < 0) | (prev < b_idx[None, :] - N // L))
            return on.nonzero()

        differing = int((det.triggerTrackPCM16(fl, S, L, N, LAT) != torch_track()).sum())
        idx, cnt = det.triggerOnsets(fl, S, L, N, LAT)
        onsets_differing = int(int(cnt.sum()) != int(torch_onsets().shape[0]))
        torch.cuda.empty_cache()

        t = timed({"trigger": lambda: det.triggerTrackPCM16(fl, S, L, N, LAT, out=track), "trace": lambda: det.trace(out, S, dtype=np.int16, out=tr),
                   "fill": lambda: track.fill_(0), "torch": torch_track})
        bytes_written = int(track.numel() * 2)
        results["s16"] = {"bytes_written": bytes_written, "flags_set": int(fl.sum()), "evaluations": E,
                          "trigger": stats(t["trigger"]), "trace": stats(t["trace"]), "fill": stats(t["fill"]), "torch": stats(t["torch"]),
                          "trigger_over_fill": float(np.median(t["trigger"]) / np.median(t["fill"])),
                          "trace_over_fill": float(np.median(t["trace"]) / np.median(t["fill"])),
                          "trigger_over_trace": float(np.median(t["trigger"]) / np.median(t["trace"])),
                          "torch_over_trigger": float(np.median(t["torch"]) / np.median(t["trigger"])),
                          "samples_differing_from_torch": differing}
        # the same with planted flags (3 % of the evaluations of every channel): the scan's marking path and the pulses' stores
        fl_p = (torch.rand((C, E), device=dev) < 0.03).to(torch.uint8)
        differing_p = int((det.triggerTrackPCM16(fl_p, S, L, N, LAT) != torch_track(fl_p)).sum())
        t = timed({"trigger": lambda: det.triggerTrackPCM16(fl_p, S, L, N, LAT, out=track), "trace": lambda: det.trace(out, S, dtype=np.int16, out=tr),
                   "fill": lambda: track.fill_(0)})
        det.profile(True)
        k_p = kernels(det, lambda: det.triggerTrackPCM16(fl_p, S, L, N, LAT, out=track))
        k_o = kernels(det, lambda: det.triggerOnsets(fl_p, S, L, N, LAT))
        det.profile(False)
        results["s16_planted"] = {"flags_set": int(fl_p.sum()), "trigger": stats(t["trigger"]), "trace": stats(t["trace"]), "fill": stats(t["fill"]),
                                  "trigger_over_fill": float(np.median(t["trigger"]) / np.median(t["fill"])),
                                  "trigger_over_trace": float(np.median(t["trigger"]) / np.median(t["trace"])),
                                  "kernels_ms": {**k_p, **k_o}, "onsets": int(det.triggerOnsets(fl_p, S, L, N, LAT)[1].sum()),
                                  "samples_differing_from_torch": differing_p}
        t = timed({"onsets": lambda: det.triggerOnsets(fl, S, L, N, LAT), "torch": torch_onsets})
        results["onsets"] = {"onsets": stats(t["onsets"]), "torch": stats(t["torch"]), "count": int(cnt.sum()),
                             "torch_over_onsets": float(np.median(t["torch"]) / np.median(t["onsets"])), "count_differs_from_torch": onsets_differing}
        del tr
        torch.cuda.empty_cache()

        x16 = (x * 32767.0).round_().to(torch.int16)
        frames = torch.empty((S, 2 * C), dtype=torch.int16, device=dev)
        halves = frames.view(2, C, S)

        def copy():                                                     # 2 GiB read, 4 GiB written
            halves[0].copy_(x16)
            halves[1].fill_(0)
        t = timed({"mux": lambda: det.triggerMuxPCM16(fl, x16, L, N, LAT, out=frames), "copy": copy})
        results["mux"] = {"bytes_read": int(x16.numel() * 2), "bytes_written": int(frames.numel() * 2), "mux": stats(t["mux"]), "copy": stats(t["copy"]),
                          "mux_over_copy": float(np.median(t["mux"]) / np.median(t["copy"]))}

        det.profile(True)
        results["kernels_ms"] = {}
        for fn in (lambda: det.triggerTrackPCM16(fl, S, L, N, LAT, out=track), lambda: det.triggerMuxPCM16(fl, x16, L, N, LAT, out=frames),
                   lambda: det.triggerOnsets(fl, S, L, N, LAT)):
            results["kernels_ms"].update(kernels(det, fn))
        det.profile(False)
        del frames, halves, x16
        torch.cuda.empty_cache()

        o, f = torch.empty_like(out), torch.empty_like(fl)

        def rehearse():                                                 # (one scan for the track and the onsets)
            det.run(x, o, f)
            det.triggerRehearse(f, S, L, N, LAT, dtype=np.int16, out=track)
        t = timed({"run": lambda: det.run(x, o, f), "rehearse": rehearse})
        results["rehearse_against_run"] = {"run": stats(t["run"]), "rehearse": stats(t["rehearse"]),
                                           "rehearse_over_run": float(np.median(t["rehearse"]) / np.median(t["run"]))}
    doc = {"workload": "%d channels x 2^%d samples, L %d, N %d, latency %d; flags of run() on the benchmark's input" % (C, lg, L, N, LAT),
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every launch, candidates alternating, median of `launches`; kernels_ms: the handle's profile",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
