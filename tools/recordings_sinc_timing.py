#!/usr/bin/env python3
"""Measurement: what converting packed recordings as the rows load (syldet_recordings_load_sinc_device*,
kernels_recordings_sinc.hip) costs and gains.

    2048 seeded mono recordings, lengths log-uniform between 1 s and 60 s, already on the device (one 1-D source, every recording
    from a whole 16 bytes), into the rows of a bank of 64 of the example detector (nets.from_npz(), 44.1 kHz, hop 132), the
    converter at its default quality.
    1. every source at 48 kHz
      load_sinc   Recordings.loadSinc, fp32 and int16 sources (recordings_load_sinc_kernel: one launch), against
      loop        what a user writes without it: convertRate(method="sinc") of every recording into scratch rows, one call each,
                  then one Recordings.load of the scratch (Python's launch overhead included), and against
      whole       one convertRate(method="sinc") call on 64 rows whose outputs number as many as the plan's recordings hold: the
                  same tap loop without a plan around it -- the floor, with its own run-to-run spread (two identical candidates,
                  `whole` and `whole_again`, alternate with the load)
    2. a quarter each at 44.1 (copied), 48, 96 and 22.05 kHz
      packed      loadSinc + run + events on the 64 rows, against
      one_by_one  every recording through a 1-channel handle: convertRate sinc (not at 44.1 kHz), run, detections -- what the tool
                  does file by file, less its handle creation, copies and host debounce

Everything runs in one process; the candidates of a group alternate launch by launch, every launch between two HIP events of its
own; after a warm-up, the median of `launches` launches with the 10th and 90th percentile (loop, one_by_one: `loops` whole loops).
Before anything is timed, every recording of both archives is compared with the shipped converter on it alone: the same bits.
Writes profiles/recordings_sinc_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/recordings_sinc_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--loops N]
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

    launches, out_path, K, C, loops = 20, os.path.join(ROOT, "profiles", "recordings_sinc_timing.json"), 2048, 64, 3
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--recordings":
            K, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--rows":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--loops":
            loops, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert launches >= 20, "at least 20 launches a candidate"
    assert torch.cuda.is_available(), "recordings_sinc_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM = 3
    cfg = nets.from_npz()
    fs = cfg.samplingRate
    Z, beta, rho = sd.sincDefaults()

    def timed(fns, n=launches, warm=WARM):
        """the candidates alternate; -> {name: sorted milliseconds}"""
        ev = {k: [] for k in fns}
        for r in range(warm + n):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                if r >= warm:
                    ev[k].append((a, b))
        torch.cuda.synchronize()
        return {k: sorted(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}

    def stats(ms):
        return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
                "min_ms": float(ms[0]), "max_ms": float(ms[-1])}

    def archive(rates, seed):
        """-> (n_in, offsets, src): recordings of log-uniform 1 .. 60 s at their own rates"""
        rng = np.random.default_rng(seed)
        seconds = np.exp(rng.uniform(np.log(1.0), np.log(60.0), size=K))
        n_in = (seconds * np.asarray(rates)).astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum((n_in + 7) // 8 * 8)[:-1]])
        total = int(offsets[-1] + n_in[-1])
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        src = torch.empty(total + 8, dtype=torch.float32, device=dev)
        step = 1 << 27
        for a in range(0, src.numel(), step):                            # (0.05 N(0, 1), the benchmark's noise level, made in pieces)
            n = min(step, src.numel() - a)
            src[a:a + n] = torch.randn(n, generator=gen, dtype=torch.float32, device=dev) * 0.05
        return n_in, offsets, src

    def same_bits(rec, rows, src, offsets, n_in, rates, every=1):
        """every recording's part of the rows against the shipped converter on it alone -> recordings compared"""
        seen = 0
        for k in range(0, K, every):
            row, off, _, _, n = rec.slots[k]
            x = src[int(offsets[k]):int(offsets[k]) + int(n_in[k])]
            want = x.to(torch.float32) * (2.0 ** -15 if x.dtype == torch.int16 else 1.0) if rates[k] == fs else \
                sd.convertRate(x[None, :], rates[k], fs, "sinc")[0]
            assert torch.equal(rows[row, off:off + n].view(torch.int32), want.view(torch.int32)), "recording %d differs from the converter alone" % k
            seen += 1
        return seen

    results = {}
    # ---- 1. every source at 48 kHz ----
    rates = [48000.0] * K
    n_in, offsets, src = archive(rates, 2048)
    lengths = sd.recordingLengths(n_in, rates, fs)
    src16 = (src * 32767.0).round_().to(torch.int16)
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(lengths) as rec:
        S, E = rec.rowSamples, rec.rowEvaluations
        n_total = int(np.sum(lengths))
        plan = {"recordings": K, "rows": C, "source_samples": int(n_in.sum()), "samples": n_total, "row_samples": int(S), "row_evals": int(E),
                "fill": float(rec.fill), "shortest": int(min(lengths)), "longest": int(max(lengths))}
        rows = torch.empty((C, S), dtype=torch.float32, device=dev)
        rec.loadSinc(src, offsets, n_in, rates, out=rows)
        checked = same_bits(rec, rows, src, offsets, n_in, rates, every=8)
        rec.loadSinc(src16, offsets, n_in, rates, out=rows)
        checked16 = same_bits(rec, rows, src16, offsets, n_in, rates, every=8)
        torch.cuda.synchronize()
        # (b) one call on C rows with as many outputs in all: rows of ceil(n_total / C) outputs
        per_row = -(-n_total // C)
        row_in = int((per_row - 1) * 48000.0 / fs) + 1
        while sd.recordingLengths([row_in], [48000.0], fs)[0] < per_row:
            row_in += 1
        assert C * row_in <= src.numel()
        whole_in = src[:C * row_in].view(C, row_in)
        whole_in16 = src16[:C * row_in].view(C, row_in)
        scratch = torch.empty(n_total + 8 * K, dtype=torch.float32, device=dev)
        s_off = np.concatenate([[0], np.cumsum((np.asarray(lengths) + 7) // 8 * 8)[:-1]])
        views = [src[int(a):int(a) + int(n)][None, :] for a, n in zip(offsets, n_in)]

        def loop():
            for k, x in enumerate(views):
                y = sd.convertRate(x, 48000.0, fs, "sinc")
                scratch[int(s_off[k]):int(s_off[k]) + lengths[k]] = y[0]
            rec.load(scratch, s_off, out=rows)

        def loop_into_scratch():
            """the same with every recording converted straight into its scratch row (the C ABI's d_out): no copy of the result"""
            import ctypes
            from syllable_detector_swift_amd import _abi
            got = ctypes.c_int64(0)
            stream = torch.cuda.current_stream(dev).cuda_stream
            base = scratch.data_ptr()
            for k in range(K):
                _abi.lib.syldet_convert_rate_sinc_device(src.data_ptr() + 4 * int(offsets[k]), int(n_in[k]), int(n_in[k]), 1, 48000.0, fs, Z, beta, rho,
                                                         base + 4 * int(s_off[k]), lengths[k], ctypes.byref(got), stream)
            rec.load(scratch, s_off, out=rows)

        for name, s, w in (("fp32", src, whole_in), ("s16", src16, whole_in16)):
            t = timed({"load_sinc": lambda: rec.loadSinc(s, offsets, n_in, rates, out=rows),
                       "whole": lambda: sd.convertRate(w, 48000.0, fs, "sinc"),
                       "whole_again": lambda: sd.convertRate(w, 48000.0, fs, "sinc")})
            m = {k: float(np.median(v)) for k, v in t.items()}
            results["load_sinc_" + name] = {
                "load_sinc": stats(t["load_sinc"]), "whole": stats(t["whole"]), "whole_again": stats(t["whole_again"]),
                "whole_outputs": C * int(sd.recordingLengths([row_in], [48000.0], fs)[0]), "load_sinc_outputs": n_total,
                "row_positions": C * int(S), "load_sinc_over_whole": m["load_sinc"] / m["whole"],
                "whole_again_over_whole": m["whole_again"] / m["whole"],
                "whole_spread": (float(np.percentile(t["whole"], 90)) - float(np.percentile(t["whole"], 10))) / m["whole"]}
        t = timed({"loop": loop, "loop_into_scratch": loop_into_scratch}, n=loops, warm=1)
        load_ms = results["load_sinc_fp32"]["load_sinc"]["median_ms"]
        results["loop_fp32"] = {"loop": stats(t["loop"]), "loop_into_scratch": stats(t["loop_into_scratch"]), "loops": loops,
                                "loop_over_load_sinc": float(np.median(t["loop"])) / load_ms,
                                "loop_into_scratch_over_load_sinc": float(np.median(t["loop_into_scratch"])) / load_ms}
        results["bits"] = {"recordings_compared_fp32": checked, "recordings_compared_s16": checked16}
        del scratch, views, whole_in, whole_in16, src16
    del src, rows
    torch.cuda.empty_cache()

    # ---- 2. a mixed archive, end to end ----
    mixed = [(44100.0, 48000.0, 96000.0, 22050.0)[k % 4] for k in range(K)]
    n_in, offsets, src = archive(mixed, 4096)
    lengths = sd.recordingLengths(n_in, mixed, fs)
    cap = 4096
    with sd.SyllableDetector(cfg, channels=C) as det, sd.SyllableDetector(cfg, channels=1) as one, det.recordings(lengths) as rec:
        S, E = rec.rowSamples, rec.rowEvaluations
        rows = torch.empty((C, S), dtype=torch.float32, device=dev)
        rec.loadSinc(src, offsets, n_in, mixed, out=rows)
        checked = same_bits(rec, rows, src, offsets, n_in, mixed, every=8)
        o, f = det.run(rows)
        torch.cuda.synchronize()

        def packed():
            rec.loadSinc(src, offsets, n_in, mixed, out=rows)
            det.run(rows, o, f)
            rec.events(o, f, 0.05, capacity=cap)

        views = [src[int(a):int(a) + int(n)][None, :] for a, n in zip(offsets, n_in)]

        def one_by_one():
            for x, r in zip(views, mixed):
                y = x if r == fs else sd.convertRate(x, r, fs, "sinc")
                _, f1 = one.run(y)
                one.detections(f1, 0.05, capacity=cap)

        t = timed({"packed": packed, "load_sinc": lambda: rec.loadSinc(src, offsets, n_in, mixed, out=rows), "run_packed_rows": lambda: det.run(rows, o, f)})
        t1 = timed({"one_by_one": one_by_one}, n=loops, warm=1)
        evals = int(sum(max(0, one.countEvaluations(int(n))) for n in lengths))
        results["mixed_rates"] = {
            "rates": "a quarter each at 44100 (copied), 48000, 96000 and 22050 Hz", "source_samples": int(n_in.sum()), "samples": int(np.sum(lengths)),
            "row_samples": int(S), "row_evals": int(E), "fill": float(rec.fill), "recordings_compared": checked,
            "packed": stats(t["packed"]), "load_sinc": stats(t["load_sinc"]), "run_packed_rows": stats(t["run_packed_rows"]),
            "one_by_one": stats(t1["one_by_one"]), "one_by_one_loops": loops, "evaluations_of_the_recordings": evals,
            "packed_evaluations_per_s": float(evals / (np.median(t["packed"]) * 1e-3)),
            "one_by_one_evaluations_per_s": float(evals / (np.median(t1["one_by_one"]) * 1e-3)),
            "one_by_one_over_packed": float(np.median(t1["one_by_one"]) / np.median(t["packed"]))}
    doc = {"workload": "%d mono recordings, log-uniform 1 s to 60 s, on %d rows of the example detector at %g Hz; the converter at (%d, %g, %g)" % (K, C, fs, Z, beta, rho),
           "plan_48k": plan, "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every launch (loop, one_by_one: around a whole loop over the K recordings, Python's launch overhead "
                     "included), candidates alternating, median of `launches` after 3 warm-up rounds",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
