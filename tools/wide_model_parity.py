#!/usr/bin/env python3
"""The wide bf16 engine against its bf16-exact model (tests/wide_ref.py), written down: runs the cases of
tests/test_wide_model_gpu.py and writes, per case and form, the worst |engine - model| relative to max(1, |model|), the model's
own fp32 spread, the bar, the evaluations that needed the other rounding of a near tie and those left out.

    python tools/wide_model_parity.py [--out profiles/wide_model_parity.json] [--only NAME ...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_wide_model_gpu as t                                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_model_parity.json"))
ap.add_argument("--only", nargs="*")
a = ap.parse_args()

records = []
for case in t.CASES:
    if a.only and case.name not in a.only:
        continue
    for rec in t.engine_against_model(case, os.environ.__setitem__, lambda k: os.environ.pop(k, None)):
        rec["route"] = case.route
        rec["failures"] = len(rec["failures"])
        records.append(rec)
for k in t.wide_cases.SWITCHES:
    os.environ.pop(k, None)
summary = {"cases": len(records), "evaluations": sum(r["evaluations"] for r in records), "worst": max(r["worst"] for r in records),
           "worst_case": max(records, key=lambda r: r["worst"])["case"], "own_max": max(r["own"] for r in records),
           "alt_needed": sum(r["alt_needed"] for r in records), "left_out": sum(r["left_out"] for r in records),
           "failing": [r["case"] + " [" + r["form"] + "]" for r in records if r["failures"]]}
json.dump({"what": "wide bf16 engine against tests/wide_ref.py, worst |engine - model| / max(1, |model|) per case and form",
           "summary": summary, "records": records}, open(a.out, "w"), indent=1)
print(json.dumps(summary, indent=1))
