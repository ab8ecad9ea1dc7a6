"""The wide bf16 engine (csrc/kernels_wide.hip, upload_wide) against a bf16-exact model of its own arithmetic (tests/wide_ref.py)
at the suite's 1e-5 -- not against the fp64 anchor at 1e-2, which measures what bf16 costs and lets a lost product, a missing
input or a truncating conversion pass (tests/test_wide_model_host.py shows it).  The model is fed the very columns the run
consumed (spectrogram() on the same handle and samples: syldet_spectrogram_device and the run both go through stft_on_stream,
and the test asserts that both launched the same transform kernel), so what is compared is the GEMM, its preparation and its
tables.  Per evaluation: |engine - model| <= max(1e-5, 4 own) max(1, |model|), own the model's fp32-sum form against itself at that evaluation;
where the model names operands within a few ulps of a bf16 rounding boundary, one of their rounding combinations must match
(on the front route, whose fp32 arithmetic is restated operation for operation, none may be needed); NaN / inf where the model
has them; flags equal to the model's decision outside a guard band of twice the bar, and to the engine's own outputs everywhere.

Measured on an MI355X (profiles/wide_model_parity.json): see MEASUREMENTS.md, "The wide engine against its bf16 model"."""
import numpy as np
import pytest

import pyoracle as po
import util
import wide_cases
import wide_ref
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

pytestmark = pytest.mark.gpu

CASES = wide_cases.all_cases()


def engine_against_model(case, setenv, delenv):
    """Runs every form of `case` and holds it to the model.  -> one record per form (tools/wide_model_parity.py writes them down);
    raises AssertionError with the figures where a form misses."""
    import torch
    cfg = case.cfg
    records, models = [], {}
    for form in case.forms:
        for k in wide_cases.SWITCHES:
            delenv(k)
        for k, v in form.env.items():
            setenv(k, v)
        rec = {"case": case.name, "form": form.label, "worst": 0.0, "own": 0.0, "bar": 0.0, "evaluations": 0, "near_evaluations": 0,
               "alt_needed": 0, "left_out": 0, "nan_evaluations": 0, "flags_bound": 0}
        failures = []
        with sd.SyllableDetector(cfg, channels=case.C, engine=_abi.ENGINE_WIDE_BF16) as det:
            assert det.geometry.engine == _abi.ENGINE_WIDE_BF16
            det.profile(True)
            for S in case.sizes():
                x = case.samples(S)
                xd = torch.from_numpy(x).cuda()
                out, fl = det.run(xd)
                torch.cuda.synchronize()
                ran = util.launched(det)
                cols = det.spectrogram(xd)
                torch.cuda.synchronize()
                transform = util.launched(det)
                out, fl, cols = out.cpu().numpy(), fl.cpu().numpy(), cols.cpu().numpy()
                # the kernels this form means to exercise, and the same transform under the run and under the columns
                assert [k for k in ran if k.startswith("wide_gemm")] == [form.gemm], (form.label, ran)
                assert [k for k in ran if k.startswith("wide_prep")] == ([form.prep] if form.prep else []), (form.label, ran)
                assert len(transform) == 1 and [k for k in ran if not k.startswith("wide_")] == transform, (ran, transform)
                assert out.shape[1] == case.E[case.sizes().index(S)]
                util.assert_flags_follow_outputs(fl, out, cfg.thresholds, cfg.rule)
                for c in range(case.C):
                    key = (tuple(sorted(form.model.items())), S, c, cols[c].tobytes())
                    if key not in models:
                        res = wide_ref.evaluate(cfg, cols[c], **form.model)
                        models[key] = (res, wide_ref.own_of(res))
                    res, own = models[key]
                    assert res.route == case.route
                    bar = wide_ref.bar_of(own)
                    r = wide_ref.compare(res, out[c], bar)
                    want, safe = wide_ref.decisions(res, cfg.thresholds, cfg.rule, bar)
                    wrong = np.nonzero((fl[c] != want) & safe)[0]
                    nan = ~np.isfinite(res.out).all(axis=1)
                    assert not fl[c][nan & ~res.left_out].any()
                    rec["worst"], rec["own"], rec["bar"] = max(rec["worst"], r["worst"]), max(rec["own"], float(own.max())), max(rec["bar"], float(bar.max()))
                    for k in ("near_evaluations", "alt_needed", "left_out"):
                        rec[k] += r[k]
                    rec["evaluations"] += len(res.out)
                    rec["nan_evaluations"] += int(nan.sum())
                    rec["flags_bound"] += int(safe.sum())
                    if r["bad"]:
                        e = r["bad"][0]
                        failures.append("S %d channel %d: %d of %d evaluations beyond the bar %.3g, first %d: engine %s model %s (near ties %d)"
                                        % (S, c, len(r["bad"]), r["judged"], bar[e], e, out[c][e], res.out[e], res.near[e]))
                    if len(wrong):
                        failures.append("S %d channel %d: flags differ from the model's decision at %s" % (S, c, wrong[:8]))
        print("%s [%s] %s: worst %.3g (bar %.3g, own %.3g), %d evaluations, %d near ties, %d needed another rounding, %d left out, %d NaN"
              % (case.name, form.label, "+".join([form.gemm] + ([form.prep] if form.prep else [])), rec["worst"], rec["bar"], rec["own"],
                 rec["evaluations"], rec["near_evaluations"], rec["alt_needed"], rec["left_out"], rec["nan_evaluations"]))
        rec["failures"] = failures
        records.append(rec)
    return records


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_wide_engine_against_its_bf16_model(case, monkeypatch):
    records = engine_against_model(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    for rec in records:
        assert not rec["failures"], "%s [%s]: %s" % (case.name, rec["form"], "; ".join(rec["failures"]))
        # the conditions under which the rule says anything: few near ties, hardly any evaluation left out
        assert rec["near_evaluations"] <= wide_ref.NEAR_LIMIT[case.route] * rec["evaluations"], rec
        assert rec["left_out"] <= wide_ref.LEFT_OUT_LIMIT * rec["evaluations"], rec
        assert rec["flags_bound"] >= 0.9 * (rec["evaluations"] - rec["nan_evaluations"]), rec
        if case.route == "front":
            assert rec["alt_needed"] == 0, "the front's fp32 arithmetic is restated operation for operation: %s" % rec
    if case.special == "silence_nan":
        assert all(rec["nan_evaluations"] >= 2 * case.cfg.timeRange for rec in records), records


def test_log_columns_behind_a_normaliser_at_bf16s_own_bar(oracle_lib):
    """wide_prep_kernel's scaling branch (log columns in front of normalizestd, mapstd), which the model cannot follow to 1e-5:
    the device's logf is within an ulp of the correctly rounded logarithm the model takes, and (x - mean) / sd hands that ulp on
    as more ulps of an operand than the w = 8 window holds (measured: 12 of 900 evaluations beyond 1e-5, each brought under it
    by the other rounding of ONE operand, eleven of them 10 - 79 ulps from its boundary -- tools/debug/wide_log_normaliser.py,
    MEASUREMENTS).  Held to the fp64 anchor at the
    engine's own 1e-2, as tests/test_ingest_gpu.py holds the other shapes, and the kernel that ran is asserted."""
    import torch
    case = wide_cases.log_behind_normaliser()
    cfg, S = case.cfg, case.sizes()[0]
    x = case.samples(S)
    o = po.Oracle(po.from_config(cfg))
    with sd.SyllableDetector(cfg, channels=case.C, engine=_abi.ENGINE_WIDE_BF16) as det:
        det.profile(True)
        out, fl = det.run(torch.from_numpy(x).cuda())
        torch.cuda.synchronize()
        assert [k for k in util.launched(det) if k.startswith("wide_")] == ["wide_prep_kernel", "wide_gemm16_kernel"]
        out, fl = out.cpu().numpy(), fl.cpu().numpy()
    util.assert_flags_follow_outputs(fl, out, cfg.thresholds, cfg.rule)
    for c in range(case.C):
        w64 = o.run(x[c], po.F64, cfg.rule)[2]
        util.assert_outputs_close(out[c], w64, 1e-2)
        util.assert_flags_exact(fl[c], w64, cfg.thresholds, cfg.rule, 1e-2)
