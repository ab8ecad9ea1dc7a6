#!/usr/bin/env python3
"""Measurement: what a ragged bank costs (syldet_matcher_bank_create_ragged, match_ragged_scores_mfma_kernel; kernels_match.hip).

    The workload of tools/match_bank_timing.py: 2048 mono recordings of 1 to 60 s (seeded) on 64 rows of the example detector (hop 132,
    29 bins), the columns filled on the device.  In one process on the same arrays, the candidates alternating launch by launch:
    (a) a ragged bank against today's method.  8 templates in 2 classes, class 0 of 11, 12, 12 and 13 frames, class 1 of 89, 91, 91
        and 93, every anchor the template's last frame:
          ragged    MatcherBank.scores of the ragged bank (scores only): one launch         match_ragged_scores_mfma_kernel
          banks     what it replaces: one uniform bank a distinct length (six of them), then the torch shift-and-fmax that lines
                    their planes up at the anchors and joins a class's (scores only; `which` would cost the method more)
        with the ragged planes compared with the joined ones bit for bit.
    (b) an equal-length ragged bank against the uniform bank on the same 8 templates, at n = 12 and n = 91 (scores and which): their
        ratio, the uniform call's own run-to-run spread (p90 - p10 over its median), and whether the ragged call is slower by more.
    and the fraction of the fp32 matrix peak (157.3 TFLOPS) the useful 2 n_k bins flop a window reach.

    --uniform PATH  only the uniform bank and the single matcher at n = 12 and n = 91, one JSON line, their outputs' bytes written to
                    PATH.bank.n12 .. PATH.single.n91: for a comparison of two checkouts (--package DIR: import the package from that
                    tree, whose own library it loads)

Every launch lies between two HIP events of its own; after a warm-up, the median of `launches` launches.  Writes
profiles/match_ragged_timing.json (or --out PATH) and prints it as one JSON line.

    python tools/match_ragged_timing.py [launches] [--out PATH] [--recordings K] [--rows C] [--uniform PATH] [--package DIR]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_FP32_MATRIX = 157.3e12
LENGTHS, CLASSES = (11, 12, 12, 13, 89, 91, 91, 93), (0, 0, 0, 0, 1, 1, 1, 1)


def main(argv):
    launches, out_path, K, C, uniform_path, package = 20, os.path.join(ROOT, "profiles", "match_ragged_timing.json"), 2048, 64, None, ROOT
    i = 0
    while i < len(argv):
        if argv[i] == "--out":
            out_path, i = argv[i + 1], i + 2
        elif argv[i] == "--recordings":
            K, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--rows":
            C, i = int(argv[i + 1]), i + 2
        elif argv[i] == "--uniform":
            uniform_path, i = argv[i + 1], i + 2
        elif argv[i] == "--package":
            package, i = argv[i + 1], i + 2
        else:
            launches, i = int(argv[i]), i + 1
    sys.path.insert(0, package)
    import numpy as np
    import torch
    import syllable_detector_swift_amd as sd
    from syllable_detector_swift_amd import nets

    assert torch.cuda.is_available(), "match_ragged_timing needs a GPU"
    dev = torch.device("cuda", 0)
    WARM = 3
    cfg = nets.from_npz()
    fs = cfg.samplingRate
    lengths = [int(v) for v in np.random.default_rng(2048).integers(int(fs), int(60 * fs), size=K)]

    def timed(fns):
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

    def spread(s):
        return (s["p90_ms"] - s["p10_ms"]) / s["median_ms"]

    results = {}

    def save():
        doc = {"workload": "%d recordings of 1 to 60 s on %d rows; the columns made on the device; 8 templates in 2 classes" % (K, C),
               "device": torch.cuda.get_device_name(0), "launches": launches,
               "timing": "HIP events around every launch, candidates alternating, median of `launches`", "results": results}
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump(doc, open(out_path, "w"), indent=1)
        return doc

    with sd.SyllableDetector(cfg, channels=C) as det, det.recordings(lengths) as rec:
        J, bins = det.countFrames(rec.rowSamples), det.geometry.bins
        frames = [max(det.countFrames(n), 0) for n in lengths]
        torch.manual_seed(1)
        cols = torch.rand((C, J, bins), device=dev) + 0.01
        print("columns: %d x %d x %d" % (C, J, bins), flush=True)
        if uniform_path:
            line = {"package": package}
            for n in (12, 91):
                t = np.random.default_rng(n).random((8, n, bins)).astype(np.float32)
                with rec.matcherBank(t, CLASSES) as bank, rec.matcher(t[0]) as m:
                    s_bank, w_bank = torch.empty((2, C, J), device=dev), torch.empty((2, C, J), dtype=torch.int32, device=dev)
                    one = torch.empty((C, J), device=dev)
                    ts = timed({"bank": lambda: bank.scores(cols, which=True, out=(s_bank, w_bank)), "single": lambda: m.scores(cols, out=one)})
                    line["n=%d" % n] = {k: stats(v) for k, v in ts.items()}
                    s_bank.cpu().numpy().tofile("%s.bank.n%d" % (uniform_path, n))
                    one.cpu().numpy().tofile("%s.single.n%d" % (uniform_path, n))
            print(json.dumps(line), flush=True)
            return 0
        results["shape"] = {"recordings": K, "rows": C, "row_frames": J, "bins": bins, "templates": 8, "classes": 2}

        # ---- (a) a ragged bank against one uniform bank a length and the join ----
        t = [np.random.default_rng(100 + k).random((n, bins)).astype(np.float32) for k, n in enumerate(LENGTHS)]
        distinct = sorted(set(LENGTHS))
        uniform = {n: rec.matcherBank(np.stack([t[k] for k in range(8) if LENGTHS[k] == n])) for n in distinct}
        planes = {n: torch.empty((uniform[n].nClasses, C, J), device=dev) for n in distinct}
        try:
            with rec.matcherBank(t, CLASSES) as bank:
                assert bank.ragged and bank.form == "matrix" and all(u.form == "matrix" for u in uniform.values())
                s_rag = torch.empty((2, C, J), device=dev)
                s_join = torch.empty((2, C, J), device=dev)

                def banks():
                    for n in distinct:
                        uniform[n].scores(cols, out=planes[n])
                    s_join.fill_(float("nan"))
                    for n in distinct:                                    # element u of the joined plane: the window that ends at u
                        c = 0 if n < 50 else 1
                        for p in planes[n]:
                            torch.fmax(s_join[c, :, n - 1:], p[:, :J - n + 1], out=s_join[c, :, n - 1:])

                ts = timed({"ragged": lambda: bank.scores(cols, out=s_rag), "banks": banks})
                banks()
                torch.cuda.synchronize()
                a, b = s_rag.view(torch.int32), s_join.view(torch.int32)
                same = bool(torch.equal(torch.isnan(s_rag), torch.isnan(s_join)) and torch.equal(a[~torch.isnan(s_rag)], b[~torch.isnan(s_join)]))
                windows = {n: int(sum(max(f - n + 1, 0) for f in frames)) for n in distinct}
                r = {"lengths": list(LENGTHS), "windows": sum(windows[n] for n in LENGTHS), "flop": sum(2 * windows[n] * n * bins for n in LENGTHS)}
                for k in ("ragged", "banks"):
                    r[k] = stats(ts[k])
                r["banks_over_ragged"] = r["banks"]["median_ms"] / r["ragged"]["median_ms"]
                r["banks_spread"] = spread(r["banks"])
                r["fraction_of_fp32_matrix_peak"] = r["flop"] / (r["ragged"]["median_ms"] * 1e-3) / PEAK_FP32_MATRIX
                r["ragged_and_joined_bits_equal"] = same
                results["ragged_8_templates_2_classes"] = r
                save()
                print(json.dumps(r), flush=True)
                assert same, "the ragged bank's planes differ from the joined ones"
                del s_rag, s_join
        finally:
            for u in uniform.values():
                u.close()
        del planes
        torch.cuda.empty_cache()

        # ---- (b) an equal-length ragged bank against the uniform bank ----
        for n in (12, 91):
            t = np.random.default_rng(n).random((8, n, bins)).astype(np.float32)
            with rec.matcherBank(t, CLASSES) as uni, rec.matcherBank(list(t), CLASSES, ragged=True) as rag:
                assert rag.ragged and not uni.ragged and rag.form == uni.form == "matrix"
                su, wu = torch.empty((2, C, J), device=dev), torch.empty((2, C, J), dtype=torch.int32, device=dev)
                sr, wr = torch.empty((2, C, J), device=dev), torch.empty((2, C, J), dtype=torch.int32, device=dev)
                ts = timed({"uniform": lambda: uni.scores(cols, which=True, out=(su, wu)), "ragged": lambda: rag.scores(cols, which=True, out=(sr, wr))})
                torch.cuda.synchronize()
                same = bool(torch.equal(sr[:, :, n - 1:].view(torch.int32)[~torch.isnan(sr[:, :, n - 1:])],
                                        su[:, :, :J - n + 1].view(torch.int32)[~torch.isnan(su[:, :, :J - n + 1])]))
                windows = int(sum(max(f - n + 1, 0) for f in frames))
                r = {"windows": windows, "flop": 2 * windows * n * bins * 8, "uniform": stats(ts["uniform"]), "ragged": stats(ts["ragged"])}
                r["ragged_over_uniform"] = r["ragged"]["median_ms"] / r["uniform"]["median_ms"]
                r["uniform_spread"] = spread(r["uniform"])
                r["ragged_slower_than_uniform_by_more_than_its_spread"] = bool(
                    r["ragged"]["median_ms"] > r["uniform"]["median_ms"] + (r["uniform"]["p90_ms"] - r["uniform"]["p10_ms"]))
                r["ragged_fraction_of_fp32_matrix_peak"] = r["flop"] / (r["ragged"]["median_ms"] * 1e-3) / PEAK_FP32_MATRIX
                r["uniform_fraction_of_fp32_matrix_peak"] = r["flop"] / (r["uniform"]["median_ms"] * 1e-3) / PEAK_FP32_MATRIX
                r["shifted_bits_equal"] = same
                results["equal_lengths_n=%d" % n] = r
                save()
                print(json.dumps(r), flush=True)
                assert same, "the equal-length ragged bank's planes are not the uniform bank's shifted"
                del su, wu, sr, wr
            torch.cuda.empty_cache()

    print(json.dumps(save()))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
