#!/usr/bin/env python3
"""Measurement: what the input level meter (syldet_levels_device*, kernels_levels.hip) costs.

    64 channels x 2^24 samples, buffers of 32 samples, the 0.1 s timer's buffers per reading (137 at 44.1 kHz), as
      f32      levels()         levels_in_kernel<float> + levels_fold_kernel      4 GiB read
      s16      levelsPCM16()    levels_in_kernel<int16> + levels_fold_kernel      2 GiB read
    each against
      read     a plain read of the same bytes, the loop of tools/ubench/read_bw.hip (tools/ubench/plain_read.hip: grid-stride,
               8 non-temporal 16-byte loads in flight a lane): the practical read-bandwidth ceiling (not code under test)
      torch    the same readings made with PyTorch operators: square, sum over the buffer, to float64, / L, max over the reading
               (its sums are in PyTorch's order: the same readings to rounding, not to the bit)
    and the output meter (outputLevels() on the outputs of one run()) on its own.

Everything runs in one process; the candidates of a shape alternate launch by launch, every launch between two HIP events of its
own; after a warm-up, the median of `launches` launches, with the 10th and 90th percentile.  Once, the device readings of one
channel of that size are compared with the PyTorch-free reference of tests/levels_ref.py for equality.  Writes
profiles/levels_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/levels_timing.py [launches] [--out PATH] [--channels C] [--log2-samples L]
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def plain_read_library():
    """tools/ubench/libplain_read.so, built on first use"""
    src = os.path.join(ROOT, "tools", "ubench", "plain_read.hip")
    lib = os.path.join(ROOT, "tools", "ubench", "libplain_read.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-o", lib, src], check=True)
    so = ctypes.CDLL(lib)
    so.plain_read.restype = ctypes.c_int
    so.plain_read.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    return so


def main(argv):
    import numpy as np
    import torch
    import levels_ref
    import syllable_detector_swift_amd as sd
    from syllable_detector_swift_amd import nets, synth

    launches, out_path, C, LG = 30, os.path.join(ROOT, "profiles", "levels_timing.json"), 64, 24
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
    assert launches >= 20, "at least 20 launches a candidate"
    assert torch.cuda.is_available(), "levels_timing needs a GPU"
    so = plain_read_library()
    dev = torch.device("cuda", 0)
    S, WARM, L = 1 << LG, 5, 32
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

    results = []
    sink = torch.zeros(1, dtype=torch.float32, device=dev)
    x = synth.channels_on_device(C, S, dev, fs=cfg.samplingRate)
    with sd.SyllableDetector(cfg, channels=C) as det:
        P = det.defaultBuffersPerReading(L)
        B = S // L
        M = det.levelsCount(S, L)
        stream = lambda: int(torch.cuda.current_stream().cuda_stream)
        for form in ("f32", "s16"):
            src = x if form == "f32" else (x * 32768.0).round_().clamp_(-32768, 32767).to(torch.int16)
            meter = (lambda: det.levels(src, L)) if form == "f32" else (lambda: det.levelsPCM16(src, L))
            nbytes = src.numel() * src.element_size()

            def with_torch():
                f = src if form == "f32" else src.to(torch.float32).mul_(2.0 ** -15)
                ms = (f * f).view(C, B, L).sum(-1).to(torch.float64).div_(L)
                pad = torch.full((C, M * P), -1.0, dtype=torch.float64, device=dev)
                pad[:, :B] = ms
                return pad.view(C, M, P).amax(-1)

            def plain():
                assert so.plain_read(src.data_ptr(), nbytes, sink.data_ptr(), stream()) == 0

            got = meter()
            rel = float(((got - with_torch()).abs() / got.abs().clamp_min(1e-300)).max())
            # one channel against the PyTorch-free reference: equality
            want = levels_ref.input_readings((src[0].cpu().numpy().astype(np.float32) * np.float32(2.0 ** -15)) if form == "s16" else src[0].cpu().numpy(), L, P)
            equal = bool(np.array_equal(got[0].cpu().numpy().view(np.uint64), want.view(np.uint64)))
            det.profile(True)
            meter()
            torch.cuda.synchronize()
            kernels = det.lastTimings()
            det.profile(False)
            t = timed({"meter": meter, "read": plain, "torch": with_torch})
            results.append({"case": "input_%s" % form, "channels": C, "samples": S, "buffer_length": L, "buffers_per_reading": P, "readings": M,
                            "bytes_read": int(nbytes), "launches": launches, "meter": stats(t["meter"]), "read": stats(t["read"]),
                            "torch": stats(t["torch"]), "meter_over_read": float(np.median(t["meter"]) / np.median(t["read"])),
                            "torch_over_meter": float(np.median(t["torch"]) / np.median(t["meter"])),
                            "meter_GBps": float(nbytes / np.median(t["meter"]) / 1e6), "read_GBps": float(nbytes / np.median(t["read"]) / 1e6),
                            "kernels_ms": {n: ms for n, ms in kernels},
                            "one_channel_equals_levels_ref": equal, "max_relative_difference_from_torch": rel})
            del src
            torch.cuda.empty_cache()
        out, _ = det.run(x)
        torch.cuda.synchronize()
        t = timed({"output_meter": lambda: det.outputLevels(out, S, 0, L)})
        results.append({"case": "output", "channels": C, "samples": S, "evaluations": int(out.shape[1]), "readings": M, "launches": launches,
                        "output_meter": stats(t["output_meter"])})
    doc = {"workload": "%d channels x 2^%d samples, buffers of %d samples, %d buffers a reading" % (C, LG, L, P),
           "device": torch.cuda.get_device_name(0), "timing": "HIP events around every launch, candidates alternating, median of `launches`",
           "results": results}
    broken = ["%s: the device readings of channel 0 differ from tests/levels_ref.py" % r["case"] for r in results
              if not r.get("one_channel_equals_levels_ref", True)]
    doc["flagged"] = broken
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    for b in broken:
        print("FLAGGED:", b, file=sys.stderr)
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
