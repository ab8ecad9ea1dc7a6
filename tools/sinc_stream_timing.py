#!/usr/bin/env python3
"""Measurement: what the streaming band-limited resampler (syldet_sinc_resampler_*, ResamplerSinc) costs beside the code that was
there, on the same box in the same run.

  1  throughput.  64 channels x 2^24 samples, 48000 -> 44100 Hz, the default quality:
       whole      one syldet_convert_rate_sinc_device call on the rows          convert_rate_sinc_kernel<float>
       stream_20  pushes of 2^20 samples and a flush through one handle         16 x (convert_rate_sinc_stream_kernel + sinc_carry_kernel) + 1
       stream_18, stream_22, stream_24   the same in pushes of 2^18, 2^22 and in ONE push: what the number of launches costs, and
                  (one push) what the kernel's own addressing costs with the launches taken out
     The candidates alternate, each between two HIP events of its own, into output rows made beforehand; after a warm-up the median
     of `launches` rounds.  Once, the streamed outputs are compared with the whole call's, bit for bit.

  2  live latency.  One push of 64 channels x 32 frames INCLUDING the wait for its result (a host clock around the call and the
     stream's synchronise), Z = 32 and Z = 8, beside the same push through syldet_resample_device (ResamplerLinear); the
     candidates alternate push by push; median and 99th percentile of `pushes` pushes after a warm-up.

Writes profiles/sinc_stream_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/sinc_stream_timing.py [launches] [--pushes N] [--out PATH] [--channels C] [--log2-samples L]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv):
    import numpy as np
    import torch
    import sinc_ref
    import syllable_detector_swift_amd as sd
    from syllable_detector_swift_amd import _abi

    launches, pushes, out_path, CH, LG = 10, 2000, os.path.join(ROOT, "profiles", "sinc_stream_timing.json"), 64, 24
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--channels":
            CH, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--log2-samples":
            LG, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--pushes":
            pushes, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert torch.cuda.is_available(), "sinc_stream_timing needs a GPU"
    lib = _abi.lib
    dev = torch.device("cuda", 0)
    S, WARM, RI, RO = 1 << LG, 2, 48000.0, 44100.0
    Z, beta, rho = sd.sincDefaults()
    stream = torch.cuda.current_stream(dev)
    sp = int(stream.cuda_stream)

    def create(z):
        h = _abi.Handle()
        st = lib.syldet_sinc_resampler_create(RI, RO, CH, 0, z, beta, rho, C.byref(h))
        assert st == 0, _abi.last_error()
        return h

    def stats(ms, tail=90):
        ms = sorted(ms)
        return {"median": float(np.median(ms)), "p10": float(np.percentile(ms, 10)), "p%d" % tail: float(np.percentile(ms, tail)),
                "min": float(ms[0]), "max": float(ms[-1])}

    # ---- 1: throughput ----
    g = torch.Generator(device=dev).manual_seed(48)
    x = torch.rand((CH, S), generator=g, device=dev, dtype=torch.float32).mul_(2.0).sub_(1.0)
    n_out = sinc_ref.count(S, RI, RO)
    out_whole = torch.empty((CH, n_out), dtype=torch.float32, device=dev)
    out_stream = torch.empty((CH, n_out), dtype=torch.float32, device=dev)
    got = C.c_int64(0)
    h = create(Z)

    def whole():
        st = lib.syldet_convert_rate_sinc_device(x.data_ptr(), S, S, CH, RI, RO, Z, beta, rho, out_whole.data_ptr(), n_out, C.byref(got), sp)
        assert st == 0 and got.value == n_out

    def streamed(lg):
        size = min(1 << lg, S)

        def run():
            assert lib.syldet_sinc_resampler_reset(h) == 0
            m = 0
            for pos in range(0, S, size):
                n = min(size, S - pos)
                st = lib.syldet_sinc_resample_device(h, x.data_ptr() + 4 * pos, n, S, out_stream.data_ptr() + 4 * m, n_out, C.byref(got), sp)
                assert st == 0
                m += got.value
            st = lib.syldet_sinc_resampler_flush_device(h, out_stream.data_ptr() + 4 * m, n_out, C.byref(got), sp)
            assert st == 0 and m + got.value == n_out
        return run

    fns = {"whole": whole}
    for lg in (20, 18, 22, 24):
        if lg <= LG:
            fns["stream_%d" % lg] = streamed(lg)
    fns["stream_20"]()
    whole()
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(out_stream.view(torch.int32), out_whole.view(torch.int32)))
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
    t1 = {k: [a.elapsed_time(b) for a, b in v] for k, v in ev.items()}
    med1 = {k: float(np.median(v)) for k, v in t1.items()}
    lib.syldet_sinc_resampler_destroy(h)
    del x, out_whole, out_stream
    torch.cuda.empty_cache()

    # ---- 2: live latency ----
    FR, ROUNDS = 32, 64
    live = torch.rand((CH, FR * ROUNDS), generator=g, device=dev, dtype=torch.float32).mul_(2.0).sub_(1.0)
    out_live = torch.empty((CH, 64), dtype=torch.float32, device=dev)
    hs = {"sinc_z32": create(32), "sinc_z8": create(8)}
    lin = _abi.Handle()
    assert lib.syldet_resampler_create(RI, RO, CH, 0, C.byref(lin)) == 0

    def one(name, j):
        p = live.data_ptr() + 4 * FR * (j % ROUNDS)
        t0 = time.perf_counter_ns()
        if name == "linear":
            st = lib.syldet_resample_device(lin, p, FR, FR * ROUNDS, out_live.data_ptr(), 64, C.byref(got), sp)
        else:
            st = lib.syldet_sinc_resample_device(hs[name], p, FR, FR * ROUNDS, out_live.data_ptr(), 64, C.byref(got), sp)
        stream.synchronize()
        t1_ = time.perf_counter_ns()
        assert st == 0
        return (t1_ - t0) / 1e3

    names = ["linear", "sinc_z32", "sinc_z8"]
    t2 = {k: [] for k in names}
    for j in range(100 + pushes):
        for k in names:
            us = one(k, j)
            if j >= 100:
                t2[k].append(us)
    for hh in hs.values():
        lib.syldet_sinc_resampler_destroy(hh)
    lib.syldet_resampler_destroy(lin)
    med2 = {k: float(np.median(v)) for k, v in t2.items()}

    doc = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__,
           "throughput": {
               "workload": "%d channels x 2^%d samples, %g -> %g Hz, Z = %d, beta = %g, rolloff = %g" % (CH, LG, RI, RO, Z, beta, rho),
               "timing": "HIP events around each candidate's whole sequence of calls, candidates alternating, median of `launches` rounds",
               "launches": launches, "outputs_per_channel": n_out,
               "results_ms": {k: stats(v) for k, v in t1.items()},
               "over_whole": {k: med1[k] / med1["whole"] for k in med1 if k != "whole"},
               "streamed_outputs_equal_the_whole_calls_bits": same_bits},
           "live_latency": {
               "workload": "one push of %d channels x %d frames and the wait for its result, %g -> %g Hz" % (CH, FR, RI, RO),
               "timing": "host clock around the call and the stream's synchronise, candidates alternating push by push",
               "pushes": pushes,
               "results_us": {k: stats(v, 99) for k, v in t2.items()},
               "over_linear": {k: med2[k] / med2["linear"] for k in med2 if k != "linear"}}}
    doc["flagged"] = [] if same_bits else ["the streamed outputs differ from the whole-recording call's"]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    for b in doc["flagged"]:
        print("FLAGGED:", b, file=sys.stderr)
    return 1 if doc["flagged"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
