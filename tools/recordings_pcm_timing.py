#!/usr/bin/env python3
"""Measurement: what loading packed recordings from the files' own bytes (syldet_recordings_load_pcm_device,
syldet_recordings_load_sinc_pcm_device; kernels_recordings_pcm.hip, kernels_recordings_sinc.hip) costs and gains.

    2048 seeded mono recordings, lengths log-uniform between 1 s and 60 s, into the rows of a bank of 64 of the example detector
    (nets.from_npz(), 44.1 kHz, hop 132): the README's case.  Every recording starts at a whole 16 bytes of its source.
    1. load_pcm   Recordings.loadPCM (recordings_load_pcm_kernel: one launch) from sources already on the device -- all S24, all S16,
                  all F32 and a mix (S16, S24, F32, S24 in turn), each contiguous and as one track of a two-track file -- against
       load       Recordings.load (the parent's call) on fp32 copies of the same recordings in the same layout, in the same run:
                  the two alternate launch by launch
    2. load_sinc_pcm   Recordings.loadSincPCM, every source at 48 kHz, all S24 and the mix, against Recordings.loadSinc on the fp32
                  copies
    3. ingest     the whole way of the mix from host memory: the files' bytes, one upload, loadPCM -- against what the tool did
                  before: every recording converted on the host by the WAV reader's loop (syldet_pcm_decode: the same statements,
                  one thread), the fp32 upload, Recordings.load.  Host clocks around work that ends in a device synchronise;
                  pageable host memory on both sides.

Before anything is timed the rows of every candidate are compared with the rows of its reference: the same bits.  Device times are
HIP events around every launch, candidates alternating, the median of `launches` launches after a warm-up with the 10th and 90th
percentile.  Writes profiles/recordings_pcm_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/recordings_pcm_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--loops N]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv):
    import numpy as np
    import torch
    import syllable_detector_swift_amd as sd
    import ctypes as C_
    from syllable_detector_swift_amd import _abi, nets

    launches, out_path, K, C, loops = 20, os.path.join(ROOT, "profiles", "recordings_pcm_timing.json"), 2048, 64, 3
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
    assert torch.cuda.is_available(), "recordings_pcm_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM = 3
    cfg = nets.from_npz()
    fs = cfg.samplingRate
    SIZE = {sd.PCM_S16: 2, sd.PCM_S24: 3, sd.PCM_F32: 4}

    def say(text):
        print("[recordings_pcm_timing] " + text, file=sys.stderr, flush=True)

    def timed(fns, n=launches, warm=WARM):
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
        ms = sorted(ms)
        return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
                "min_ms": float(ms[0]), "max_ms": float(ms[-1])}

    def lengths_at(rate, seed):
        rng = np.random.default_rng(seed)
        return (np.exp(rng.uniform(np.log(1.0), np.log(60.0), size=K)) * rate).astype(np.int64)

    def noise(total, seed):
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        src = torch.empty(total, dtype=torch.float32, device=dev)
        step = 1 << 27
        for a in range(0, total, step):                                  # (0.05 N(0, 1), the benchmark's noise level, made in pieces)
            n = min(step, total - a)
            src[a:a + n] = torch.randn(n, generator=gen, dtype=torch.float32, device=dev) * 0.05
        return src

    def as_format(x, fmt):
        """float32 [n] on the device -> (its bytes in the format, uint8 [n * size]; the float32 those bytes mean)"""
        if fmt == sd.PCM_F32:
            return x.view(torch.uint8), x
        if fmt == sd.PCM_S16:
            v = (x * 32767.0).round_().to(torch.int16)
            return v.view(torch.uint8), v.to(torch.float32) * 2.0 ** -15
        v = (x * 8388607.0).round_().to(torch.int32)
        return v.view(torch.uint8).view(-1, 4)[:, :3].contiguous().view(-1), v.to(torch.float32) * 2.0 ** -23

    def sources(n, formats, tracks, seed):
        """-> (bytes uint8, byte offsets, byte steps, fp32 copy, element offsets, element steps): recording k, n[k] samples of
        formats[k], one track of a file of `tracks` tracks (the others hold the same samples); every file from a whole 16 bytes of
        either source"""
        at_el = np.concatenate([[0], np.cumsum((n * tracks + 7) // 8 * 8)[:-1]]).astype(np.int64)
        x = noise(int(at_el[-1] + n[-1] * tracks), seed)
        if len(set(formats)) == 1:
            # one format: the whole source at once (an element offset that is a multiple of 8 is a byte offset that is one of 16 / 8)
            raw, f32 = as_format(x, formats[0])
            size = SIZE[formats[0]]
            return raw, at_el * size, np.full(K, tracks * size, np.int32), f32, at_el, np.full(K, tracks, np.int32)
        pieces, at_b, pos, f32 = [], [], 0, torch.empty_like(x)
        for k in range(K):
            a, m = int(at_el[k]), int(n[k]) * tracks
            raw, f = as_format(x[a:a + m], formats[k])
            f32[a:a + m] = f
            pad = -raw.numel() % 16
            pieces += [raw, torch.zeros(pad, dtype=torch.uint8, device=dev)]
            at_b.append(pos)
            pos += raw.numel() + pad
        steps = np.array([tracks * SIZE[f] for f in formats], np.int32)
        return torch.cat(pieces), np.asarray(at_b, np.int64), steps, f32, at_el, np.full(K, tracks, np.int32)

    MIX = [(sd.PCM_S16, sd.PCM_S24, sd.PCM_F32, sd.PCM_S24)[k % 4] for k in range(K)]
    kinds = [("s24", [sd.PCM_S24] * K), ("s16", [sd.PCM_S16] * K), ("f32", [sd.PCM_F32] * K), ("mix", MIX)]
    results = {}

    # ---- 1. the plain form ----
    n = lengths_at(fs, 2048)
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(n) as rec, det.recordings(n) as ref:
        S = rec.rowSamples
        plan = {"recordings": K, "rows": C, "samples": int(n.sum()), "row_samples": int(S), "row_evals": int(rec.rowEvaluations), "fill": float(rec.fill),
                "shortest": int(n.min()), "longest": int(n.max())}
        rows, want = torch.empty((C, S), dtype=torch.float32, device=dev), torch.empty((C, S), dtype=torch.float32, device=dev)
        for tracks in (1, 2):
            for name, formats in kinds:
                tag = "load_pcm_%s_%s" % (name, "contiguous" if tracks == 1 else "stereo")
                say(tag)
                raw, at_b, st_b, f32, at_el, st_el = sources(n, formats, tracks, 2048)
                fmt = np.asarray(formats, np.int32)
                rec.loadPCM(raw, at_b, st_b, fmt, out=rows)
                ref.load(f32, at_el, st_el, out=want)
                torch.cuda.synchronize()
                assert torch.equal(rows.view(torch.int32), want.view(torch.int32)), tag + ": rows differ from the plain load of the fp32 copy"
                t = timed({"load_pcm": lambda: rec.loadPCM(raw, at_b, st_b, fmt, out=rows), "load_fp32": lambda: ref.load(f32, at_el, st_el, out=want)})
                m = {k: float(np.median(v)) for k, v in t.items()}
                source_bytes = int(sum(int(a) * SIZE[f] for a, f in zip(n, formats)))
                results[tag] = {"load_pcm": stats(t["load_pcm"]), "load_fp32": stats(t["load_fp32"]), "load_pcm_over_load_fp32": m["load_pcm"] / m["load_fp32"],
                                "sample_bytes_read": source_bytes, "fp32_sample_bytes_read": 4 * int(n.sum()), "row_bytes_written": 4 * C * int(S),
                                "load_pcm_gb_per_s": (source_bytes + 4 * C * int(S)) / (m["load_pcm"] * 1e6),
                                "load_fp32_gb_per_s": (4 * int(n.sum()) + 4 * C * int(S)) / (m["load_fp32"] * 1e6), "same_bits": True}
                del raw, f32
                torch.cuda.empty_cache()

        # ---- 3. the whole ingest of the mix, from host memory ----
        say("ingest")
        raw, at_b, st_b, f32, at_el, st_el = sources(n, MIX, 1, 2048)
        fmt = np.asarray(MIX, np.int32)
        host_raw = raw.cpu().numpy()
        del raw, f32
        torch.cuda.empty_cache()
        host_f32 = np.empty(int(at_el[-1] + n[-1]), np.float32)
        new_s, old_s, convert_s = [], [], []
        for r in range(loops + 1):
            t0 = time.perf_counter()
            d_raw = torch.from_numpy(host_raw).to(dev)
            rec.loadPCM(d_raw, at_b, st_b, fmt, out=rows)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for k in range(K):                                           # the WAV reader's loop, a recording at a time
                a, b = int(at_b[k]), int(at_el[k])
                st = _abi.lib.syldet_pcm_decode(MIX[k], host_raw.ctypes.data + a, int(n[k]), SIZE[MIX[k]], C_.cast(host_f32.ctypes.data + 4 * b, _abi.c_float_p))
                assert st == 0
            t2 = time.perf_counter()
            d_f32 = torch.from_numpy(host_f32).to(dev)
            ref.load(d_f32, at_el, st_el, out=want)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            assert torch.equal(rows.view(torch.int32), want.view(torch.int32)), "ingest: rows differ"
            if r > 0:                                                    # (the first round warms both)
                new_s.append(t1 - t0)
                old_s.append(t3 - t1)
                convert_s.append(t2 - t1)
            del d_raw, d_f32
            say("ingest round %d: bytes %.3f s, host conversion + fp32 %.3f s" % (r, t1 - t0, t3 - t1))
        results["ingest_mix"] = {"bytes_upload_load_pcm_s": sorted(new_s), "host_decode_fp32_upload_load_s": sorted(old_s), "host_decode_s": sorted(convert_s),
                                 "loops": loops, "upload_bytes": int(host_raw.nbytes), "fp32_upload_bytes": int(host_f32.nbytes),
                                 "median_bytes_upload_load_pcm_s": float(np.median(new_s)), "median_host_decode_fp32_upload_load_s": float(np.median(old_s)),
                                 "median_host_decode_s": float(np.median(convert_s)),
                                 "old_over_new": float(np.median(old_s) / np.median(new_s)), "host_memory": "pageable", "same_bits": True}
        del host_raw, host_f32, rows, want
    torch.cuda.empty_cache()

    # ---- 2. the converting form: every source at 48 kHz ----
    rates = [48000.0] * K
    n_in = lengths_at(48000.0, 2048)
    planned = sd.recordingLengths(n_in, rates, fs)
    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(planned) as rec, det.recordings(planned) as ref:
        S = rec.rowSamples
        rows, want = torch.empty((C, S), dtype=torch.float32, device=dev), torch.empty((C, S), dtype=torch.float32, device=dev)
        for name, formats in (("s24", [sd.PCM_S24] * K), ("mix", MIX)):
            tag = "load_sinc_pcm_%s_48k" % name
            say(tag)
            raw, at_b, st_b, f32, at_el, st_el = sources(n_in, formats, 1, 4096)
            fmt = np.asarray(formats, np.int32)
            rec.loadSincPCM(raw, at_b, st_b, fmt, n_in, rates, out=rows)
            ref.loadSinc(f32, at_el, n_in, rates, st_el, out=want)
            torch.cuda.synchronize()
            assert torch.equal(rows.view(torch.int32), want.view(torch.int32)), tag + ": rows differ from the converting load of the fp32 copy"
            t = timed({"load_sinc_pcm": lambda: rec.loadSincPCM(raw, at_b, st_b, fmt, n_in, rates, out=rows),
                       "load_sinc_fp32": lambda: ref.loadSinc(f32, at_el, n_in, rates, st_el, out=want)})
            m = {k: float(np.median(v)) for k, v in t.items()}
            results[tag] = {"load_sinc_pcm": stats(t["load_sinc_pcm"]), "load_sinc_fp32": stats(t["load_sinc_fp32"]),
                            "load_sinc_pcm_over_load_sinc_fp32": m["load_sinc_pcm"] / m["load_sinc_fp32"], "source_samples": int(n_in.sum()),
                            "row_samples": int(S), "same_bits": True}
            del raw, f32
            torch.cuda.empty_cache()

    doc = {"workload": "%d mono recordings, log-uniform 1 s to 60 s, on %d rows of the example detector at %g Hz" % (K, C, fs), "plan": plan,
           "device": torch.cuda.get_device_name(0), "launches": launches,
           "timing": "HIP events around every launch, a candidate and its reference alternating, median of `launches` after 3 warm-up rounds; ingest: host "
                     "clocks around work that ends in a device synchronise, `loops` rounds after one warm-up round",
           "results": results}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
