#!/usr/bin/env python3
"""Debug / experiment: log columns behind a normaliser, where tests/wide_ref.py cannot follow the wide engine's preparation
kernel to the last place (the hardware logarithm against the correctly rounded one, handed on by (x - mean) / sd).  Runs that
configuration on the wide engine, and for every evaluation beyond the bar searches greedily for the operands whose OTHER bf16
rounding reproduces the engine's output: how many flips it takes, how far each flipped operand's fp32 value lies from its
rounding boundary (in fp32 ulps), and what is left afterwards.  If the misses are rounding flips of single operands and not a
fault of the GEMM, every one is reproduced to the bar by a few flips of operands a few ulps outside the model's window.

    python tools/debug/wide_log_normaliser.py [--out profiles/wide_log_normaliser.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np                                                                 # noqa: E402
import torch                                                                       # noqa: E402
import syllable_detector_swift_amd as sd                                           # noqa: E402
from syllable_detector_swift_amd import _abi                                       # noqa: E402
import wide_cases                                                                  # noqa: E402
import wide_ref                                                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_log_normaliser.json"))
ap.add_argument("--max-flips", type=int, default=6)
a = ap.parse_args()

case = wide_cases.log_behind_normaliser()
cfg, S = case.cfg, case.sizes()[0]
x = torch.from_numpy(case.samples(S)).cuda()
with sd.SyllableDetector(cfg, channels=case.C, engine=_abi.ENGINE_WIDE_BF16) as det:
    det.profile(True)
    out = det.run(x)[0]
    torch.cuda.synchronize()
    kernels = [k for k, _ in det.lastTimings()]
    cols = det.spectrogram(x)
    torch.cuda.synchronize()
out, cols = out.cpu().numpy(), cols.cpu().numpy()

rel = lambda g, m: float((np.abs(g - m) / np.maximum(1.0, np.abs(m))).max())
misses, total, alt_needed = [], 0, 0
for c in range(case.C):
    res = wide_ref.evaluate(cfg, cols[c])
    bar = wide_ref.bar_of(wide_ref.own_of(res))
    r = wide_ref.compare(res, out[c], bar)
    total += r["judged"]
    alt_needed += r["alt_needed"]
    other = wide_ref.bf16_other(res.values).astype(np.float64)
    lo = (res.values.view(np.uint32) & 0xffff).astype(np.int64)
    for e in r["bad"]:
        row, flipped, err0 = res.operands[e].copy(), [], rel(out[c][e], res.out[e])
        err = err0
        while err > bar[e] and len(flipped) < a.max_flips:
            rows = np.repeat(row[None, :], len(row), axis=0)
            idx = np.arange(len(row))
            rows[idx, idx] = np.where(rows[idx, idx] == res.operands[e], other[e], res.operands[e])
            errs = np.array([rel(out[c][e], y) for y in wide_ref._forward(res.plan, rows)])
            i = int(np.argmin(errs))
            if errs[i] >= err:
                break
            row, err = rows[i], float(errs[i])
            flipped.append({"input": i, "value": float(res.values[e, i]), "ulps_from_boundary": int(abs(lo[e, i] - 0x8000))})
        misses.append({"channel": c, "evaluation": int(e), "error": err0, "bar": float(bar[e]), "near_ties_named": int(res.near[e]),
                       "flips": flipped, "error_after_flips": err, "reproduced": bool(err <= bar[e])})
rec = {"what": "log columns + normalizestd, mapstd on the wide engine: evaluations beyond the bar against tests/wide_ref.py, and the operand "
               "roundings that reproduce them", "kernels": kernels, "evaluations": total, "beyond_bar": len(misses), "alt_needed": alt_needed,
       "reproduced_by_flips": sum(m["reproduced"] for m in misses), "worst": max([m["error"] for m in misses], default=0.0),
       "worst_after_flips": max([m["error_after_flips"] for m in misses], default=0.0),
       "flips_per_miss": sorted(len(m["flips"]) for m in misses),
       "ulps_from_boundary_of_flipped": sorted(f["ulps_from_boundary"] for m in misses for f in m["flips"]), "misses": misses}
json.dump(rec, open(a.out, "w"), indent=1)
print(json.dumps({k: v for k, v in rec.items() if k != "misses"}, indent=1))
