"""The wide engine's bf16 model (tests/wide_ref.py) and the rule the GPU tests apply with it, on the host (no GPU; the oracle
library only): the bf16 conversion against torch's; the folding of upload_wide, restated, against the plain numpy network; the
model against the fp64 anchor at the engine's own bar; the rule against a table of known faults -- every one rejected where the
1e-2 anchor comparison accepts several; the near-tie conditions of every case of tests/test_wide_model_gpu.py."""
import numpy as np
import pytest

import pyoracle as po
import wide_cases
import wide_ref
from test_oracle import _numpy_net

WIDE_TOL = 1e-2                       # tests/test_ingest_gpu.py: what bf16 itself costs against the anchor
CASES = wide_cases.all_cases()
_cache = {}


def _inputs(case, S):
    """per channel: (fp32 columns of the fp32 oracle, fp64 anchor outputs), computed once a case and size"""
    key = (case.name, S)
    if key not in _cache:
        o = po.Oracle(po.from_config(case.cfg))
        x = case.samples(S)
        _cache[key] = [(o.spectrogram(x[c], po.F32).astype(np.float32), o.run(x[c], po.F64, case.cfg.rule)[2]) for c in range(case.C)]
    return _cache[key]


def _model(case, S, c, **kw):
    key = (case.name, S, c, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = wide_ref.evaluate(case.cfg, _inputs(case, S)[c][0], **kw)
    return _cache[key]


def _models(case):
    """the distinct models of a case's forms: [(model switches, S, channel)]"""
    kws = []
    for f in case.forms:
        if f.model not in kws:
            kws.append(f.model)
    return [(kw, S, c) for kw in kws for S in case.sizes() for c in range(case.C)]


def test_bf16_is_torchs_conversion():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 20000).astype(np.float32),
                        rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),      # any bit pattern
                        # exact ties: to the even neighbour below, and to the one above
                        np.array([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001, 0x7f7f8000, 0x7f7fffff], np.uint32).view(np.float32),
                        # denormals (ties among them), zeros, the infinities, NaNs
                        np.array([0x00000001, 0x00008000, 0x00018000, 0x00017fff, 0x807fffff, 0x0, 0x80000000, 0x7f800000, 0xff800000,
                                  0x7fc00000, 0x7f800001, 0xffc12345, 0x7fffffff], np.uint32).view(np.float32)])
    want = torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()
    got = wide_ref.bf16(v)
    nan = np.isnan(v)
    assert (np.isnan(got) == nan).all() and (np.isnan(want) == nan).all()
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    assert (got.view(np.uint32) & 0xffff == 0).all()
    # the neighbour not chosen is one bf16 step away, on the other side of the value
    fin = np.isfinite(v) & np.isfinite(got)
    other = wide_ref.bf16_other(v)
    assert (np.abs(other.view(np.uint32)[fin].astype(np.int64) - got.view(np.uint32)[fin].astype(np.int64)) == 0x10000).all()
    assert ((other[fin].astype(np.float64) - v[fin]) * (got[fin].astype(np.float64) - v[fin]) <= 0).all()
    assert np.array_equal(wide_ref.bf16(v[fin], truncate=True).view(np.uint32), v[fin].view(np.uint32) & 0xffff0000)
    # the window: 0x8000 is the tie
    edge = np.array([0x3f808000, 0x3f807ffe, 0x3f808002, 0x3f807ffd, 0x3f808003, 0x7f808000], np.uint32).view(np.float32)
    assert wide_ref.near_boundary(edge, 2).tolist() == [True, True, True, False, False, False]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_folding_is_the_plain_network(oracle_lib, case):
    """With every rounding switched off the model -- upload_wide's folding of the affine maps into the first layer and of TanSig /
    LogSig into the tables, the polynomial form's own folding aside -- is the numpy network of tests/test_oracle.py to 1e-12."""
    net = po.from_config(case.cfg)
    cfg = case.cfg
    T = cfg.timeRange
    for kw, S, c in _models(case):
        if kw.get("tanh_poly"):
            continue                                   # (the polynomial is not tanh: 1.36e-3 from it, by design)
        cols = _inputs(case, S)[c][0]
        ex = wide_ref.evaluate(cfg, cols, exact=True, **kw)
        E = len(ex.out)
        for e in sorted({0, min(1, E - 1), E // 3, E // 2, E - 1}):
            v = cols[e:e + T].reshape(-1).astype(np.float64)
            with np.errstate(all="ignore"):
                v = np.log(v) if cfg.spectrogramScaling == "log" else 20 * np.log10(v) if cfg.spectrogramScaling == "db" else v
                want = _numpy_net(net, v)
            if not np.isfinite(want).all():
                assert (np.isnan(want) == np.isnan(ex.out[e])).all()
                continue
            assert np.abs(ex.out[e] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (kw, S, c, e, ex.out[e], want)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_model_is_within_the_engines_bar_of_the_anchor_and_within_its_conditions(oracle_lib, case):
    """With the roundings on, the model is within WIDE_TOL of the fp64 anchor (4 WIDE_TOL for the narrow-range maps, whose network
    inputs reach |u| ~ 25: tests/test_ingest_gpu.py) -- 1.3e-3 for configs[4] -- and the near ties it names stay within the
    conditions of the rule: at most 5 % (front) / 15 % (prepared) of a case's evaluations, at most 1 % left out."""
    tol = 4 * WIDE_TOL if case.name == "H64_narrow_range_maps" else WIDE_TOL
    worst, near, left, total = 0.0, 0, 0, 0
    seen = set()
    for kw, S, c in _models(case):
        res = _model(case, S, c, **kw)
        assert res.route == case.route
        w64 = _inputs(case, S)[c][1]
        ok = np.isfinite(w64).all(axis=1)
        assert (np.isfinite(res.out).all(axis=1) == ok).all()
        if ok.any():
            worst = max(worst, float((np.abs(res.out[ok] - w64[ok]) / np.maximum(1.0, np.abs(w64[ok]))).max()))
        if (S, c, res.route) not in seen:              # (the operands depend on the route and the input, not on the form)
            seen.add((S, c, res.route))
            near, left, total = near + int((res.near >= 1).sum()), left + int(res.left_out.sum()), total + len(res.near)
    print("%s: model against anchor %.3g; near-tie evaluations %d of %d, left out %d" % (case.name, worst, near, total, left))
    assert 1e-7 < worst <= tol
    assert near <= wide_ref.NEAR_LIMIT[case.route] * total and left <= wide_ref.LEFT_OUT_LIMIT * total, (near, left, total)


def _poly_net(net, v):
    """the plain network with the hidden TanSig / LogSig through the kernel's clamped polynomial: tanh(x) ~ poly(x),
    logsig(x) = 1/2 + tanh(x / 2) / 2 ~ 1/2 + poly(x / 2) / 2"""
    v = np.asarray(v, np.float64)
    for f in net["inputs"]:
        v = v / np.sqrt((v * v).sum()) if f["function"] == "l2normalize" else \
            (v - f["xOffsets"].astype(np.float64)) * f["gains"].astype(np.float64) + float(f["y"])
    L0, L1 = net["layers"]
    a = L0["weights"].astype(np.float64).reshape(L0["outputs"], L0["inputs"]) @ v + L0["biases"].astype(np.float64)
    h = wide_ref._poly(a) if L0["transferFunction"] == "TanSig" else 0.5 + 0.5 * wide_ref._poly(0.5 * a)
    y = L1["weights"].astype(np.float64).reshape(L1["outputs"], L1["inputs"]) @ h + L1["biases"].astype(np.float64)
    assert L1["transferFunction"] == "PureLin"
    for f in net["outputs"]:
        y = (y - float(f["y"])) / f["gains"].astype(np.float64) + f["xOffsets"].astype(np.float64)
    return y


@pytest.mark.parametrize("name", ["config5_front_forms", "H96_front_forms", "H96_logsig_tanh_poly"])
def test_polynomial_forms_folding(oracle_lib, name):
    """SYLDET_WIDE_TANH_POLY's own folding (sc = 1 and w1' = w1 for TanSig; sc = 1/2, w1' = w1 / 2 and b1' = b1 + sum w1 / 2 for
    LogSig), every rounding off, against the plain network with the polynomial in the transfer function's place, to 1e-12; and
    the polynomial itself within 1.5e-3 of tanh on its clamped range."""
    case = [c for c in CASES if c.name == name][0]
    assert any(f.model.get("tanh_poly") for f in case.forms)
    net, cfg, T = po.from_config(case.cfg), case.cfg, case.cfg.timeRange
    S = case.sizes()[0]
    for c in range(case.C):
        cols = _inputs(case, S)[c][0]
        ex = wide_ref.evaluate(cfg, cols, exact=True, tanh_poly=True)
        assert ex.plan.poly
        E = len(ex.out)
        for e in sorted({0, 1, E // 3, E // 2, E - 1}):
            want = _poly_net(net, cols[e:e + T].reshape(-1))
            assert np.abs(ex.out[e] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (c, e, ex.out[e], want)
    x = np.linspace(-6.0, 6.0, 24001)
    assert np.abs(wide_ref._poly(x) - np.tanh(x)).max() <= 1.5e-3


PASSES_TODAY = ("unit_term_lost", "product_lost_3pct", "truncation")


@pytest.mark.parametrize("name", ["config5_front_forms", "H32", "H96_front_forms"])
def test_the_rule_rejects_known_faults(oracle_lib, name):
    """Each fault is applied to the model (never to a kernel) and the faulted outputs are handed to compare() as an engine's: every
    one must fail the rule.  On configs[4] three of them pass the anchor comparison at 1e-2 -- the gap this file closes."""
    case = [c for c in CASES if c.name == name][0]
    S, c = case.sizes()[0], 0
    res = _model(case, S, c)
    w64 = _inputs(case, S)[c][1]
    own = wide_ref.own_of(res)
    bar = wide_ref.bar_of(own)
    assert bar.shape == own.shape and bar.max() < 4e-5, bar.max()     # (per evaluation; it stays three orders under the 1e-2 one)
    clean = wide_ref.compare(res, res.out, bar)
    assert not clean["bad"] and clean["alt_needed"] == 0
    # a legitimate other rounding of a near tie is accepted, and counted
    e = next(iter(res.alts))
    flipped = res.out.copy()
    flipped[e] = res.alts[e][0]
    r = wide_ref.compare(res, flipped, bar)
    assert not r["bad"] and r["alt_needed"] == (1 if np.abs(flipped[e] - res.out[e]).max() > bar[e] * max(1.0, np.abs(res.out[e]).max()) else 0)
    for fault in wide_ref.FAULTS:
        bad = wide_ref.evaluate(case.cfg, _inputs(case, S)[c][0], fault=fault)
        r = wide_ref.compare(res, bad.out, bar)
        anchor = float((np.abs(bad.out - w64) / np.maximum(1.0, np.abs(w64))).max())
        print("%s %s: %d of %d evaluations fail, worst %.3g against the model (bar %.3g); %.3g against the anchor"
              % (name, fault, len(r["bad"]), r["judged"], r["worst"], bar.max(), anchor))
        assert r["bad"] and r["worst"] > 2 * bar.max(), fault
        if name == "config5_front_forms" and fault in PASSES_TODAY:
            assert anchor <= WIDE_TOL, (fault, anchor)


def test_decisions_bind_only_away_from_the_threshold(oracle_lib):
    case = [c for c in CASES if c.name == "H64_4out_any"][0]
    res = _model(case, case.sizes()[0], 0)
    thr = np.median(res.out, axis=0)
    thr[1:] = res.out[:, 1:].max(axis=0) - 1e-3        # output 0 hits half the time, the others rarely
    for rule in (0, 1):
        want, safe = wide_ref.decisions(res, thr, rule, 1e-5)
        hit = res.out >= thr[None, :]
        assert np.array_equal(want, (hit[:, 0] if rule == 0 else hit.any(axis=1)).astype(np.uint8))
        assert safe.sum() > 0.9 * len(safe) and 0 < want.sum() < len(want)
    assert want.sum() > hit[:, 0].sum()
    e = int(np.argmax(res.out[:, 1]))
    moved = thr.copy()
    moved[1] = res.out[e, 1] * (1 + 1e-5)               # an output inside the guard band binds nothing under the any-output rule
    assert wide_ref.decisions(res, moved, 0, 1e-5)[1][e] and not wide_ref.decisions(res, moved, 1, 1e-5)[1][e]
