#!/usr/bin/env python3
"""Measurement: what the band-limited rate converter (syldet_convert_rate_sinc_device*, kernels_sinc.hip) costs.

    64 channels x 2^24 samples, 48000 -> 44100 Hz, the default quality (32 zero crossings, beta 12, rolloff 0.9), as
      sinc_f32   convertRate(fp32 rows, method="sinc")     convert_rate_sinc_kernel<float>     4 GiB read, 3.7 GiB written
      sinc_s16   convertRate(int16 rows, method="sinc")    convert_rate_sinc_kernel<int16>     2 GiB read, 3.7 GiB written
    beside
      linear     convertRate(fp32 rows)                    convert_rate_kernel, the converter the tool had
      copy       a device-to-device copy that moves as many bytes as sinc_f32 reads and writes together (not code under test:
                 the practical ceiling of a read-plus-write)
      h2d_f32 / h2d_s16   the copy of the input from pinned host memory, which every file pays before its conversion

Everything runs in one process; the device candidates alternate launch by launch, every launch between two HIP events of its own;
after a warm-up, the median of `launches` launches with the 10th and 90th percentile.  The figure a user meets is sinc over h2d.
Once, 4096 outputs of one channel are compared with the fp64 model of tests/sinc_ref.py against the bar of tests/test_sinc_gpu.py.
Writes profiles/sinc_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/sinc_timing.py [launches] [--out PATH] [--channels C] [--log2-samples L]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv):
    import numpy as np
    import torch
    import sinc_ref
    import syllable_detector_swift_amd as sd

    launches, out_path, C, LG = 20, os.path.join(ROOT, "profiles", "sinc_timing.json"), 64, 24
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--channels":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--log2-samples":
            LG, i = int(argv[i + 1]), i + 2
        else:
            launches, i = int(argv[i]), i + 1
    assert launches >= 10, "at least 10 launches a candidate"
    assert torch.cuda.is_available(), "sinc_timing needs a GPU"
    dev = torch.device("cuda", 0)
    S, WARM, RI, RO = 1 << LG, 3, 48000.0, 44100.0
    Z, beta, rho = sd.sincDefaults()

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

    g = torch.Generator(device=dev).manual_seed(48)
    x = torch.rand((C, S), generator=g, device=dev, dtype=torch.float32).mul_(2.0).sub_(1.0)
    q = (x * 32768.0).round_().clamp_(-32768, 32767).to(torch.int16)
    n_out = sinc_ref.count(S, RI, RO)
    bytes_f32, bytes_s16, bytes_out = C * S * 4, C * S * 2, C * n_out * 4
    half = (bytes_f32 + bytes_out) // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)

    # once: the converter's outputs at this size against the model (the first 2048 and the last 2048 outputs of channel 0)
    got = sd.convertRate(x, RI, RO, method="sinc")
    got16 = sd.convertRate(q, RI, RO, method="sinc")
    torch.cuda.synchronize()
    head = 4096
    x0 = x[0, :head + 200].cpu().numpy()
    want, A, X, T = sinc_ref.convert(x0, RI, RO, Z, beta, rho, start=0, stop=2048)
    worst = float((np.abs(got[0, :2048].cpu().numpy().astype(np.float64) - want) / sinc_ref.bound(A, X, T)).max())
    xl = x[0].cpu().numpy()
    want, A, X, T = sinc_ref.convert(xl, RI, RO, Z, beta, rho, start=n_out - 2048, stop=n_out)
    worst = max(worst, float((np.abs(got[0, n_out - 2048:].cpu().numpy().astype(np.float64) - want) / sinc_ref.bound(A, X, T)).max()))
    s16_equal = bool(torch.equal(got16[:2], sd.convertRate(q[:2].to(torch.float32) / 32768.0, RI, RO, method="sinc")))
    del got, got16, xl

    t = timed({"sinc_f32": lambda: sd.convertRate(x, RI, RO, method="sinc"),
               "sinc_s16": lambda: sd.convertRate(q, RI, RO, method="sinc"),
               "linear": lambda: sd.convertRate(x, RI, RO),
               "copy": lambda: dst.copy_(src)})
    del src, dst
    torch.cuda.empty_cache()
    h2d = {}
    for name, dtype, target in (("h2d_f32", torch.float32, x), ("h2d_s16", torch.int16, q)):
        host = torch.empty((C, S), dtype=dtype, pin_memory=True)
        host.copy_(target)
        torch.cuda.synchronize()
        h2d.update(timed({name: lambda: target.copy_(host, non_blocking=True)}))
        del host
    t.update(h2d)

    taps = C * n_out * (2 * Z / (min(1.0, RO / RI) * rho))
    med = {k: float(np.median(v)) for k, v in t.items()}
    doc = {"workload": "%d channels x 2^%d samples, %g -> %g Hz, Z = %d, beta = %g, rolloff = %g" % (C, LG, RI, RO, Z, beta, rho),
           "device": torch.cuda.get_device_name(0),
           "timing": "HIP events around every launch, device candidates alternating, median of `launches`; the host copies from pinned memory",
           "launches": launches, "outputs_per_channel": n_out,
           "bytes": {"in_f32": bytes_f32, "in_s16": bytes_s16, "out": bytes_out, "copy_moves": 2 * half},
           "results": {k: stats(v) for k, v in t.items()},
           "sinc_f32_over_h2d_f32": med["sinc_f32"] / med["h2d_f32"], "sinc_s16_over_h2d_s16": med["sinc_s16"] / med["h2d_s16"],
           "sinc_f32_over_copy": med["sinc_f32"] / med["copy"], "sinc_f32_over_linear": med["sinc_f32"] / med["linear"],
           "taps": taps, "sinc_f32_Gtaps_per_s": taps / med["sinc_f32"] / 1e6, "sinc_s16_Gtaps_per_s": taps / med["sinc_s16"] / 1e6,
           "sinc_f32_GBps": (bytes_f32 + bytes_out) / med["sinc_f32"] / 1e6, "copy_GBps": 2 * half / med["copy"] / 1e6,
           "h2d_f32_GBps": bytes_f32 / med["h2d_f32"] / 1e6, "h2d_s16_GBps": bytes_s16 / med["h2d_s16"] / 1e6,
           "largest_error_over_bar": worst, "s16_gives_the_f32_bits": s16_equal}
    doc["flagged"] = [m for ok, m in ((worst <= 1.0, "an output misses the bar of tests/test_sinc_gpu.py"),
                                      (s16_equal, "the int16 form's bits differ from the fp32 form's")) if not ok]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    for b in doc["flagged"]:
        print("FLAGGED:", b, file=sys.stderr)
    return 1 if doc["flagged"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
