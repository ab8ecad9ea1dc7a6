"""The cases of tests/test_wide_model_gpu.py as data: a configuration, an input, the forms (environment switches) it runs under and
the kernels each form means to exercise.  tests/test_wide_model_host.py walks the same list on the CPU (the folding, the model
against the anchor, the near-tie conditions), tools/wide_model_parity.py records it."""
from types import SimpleNamespace

import numpy as np

RULE_ANY = 1                          # syldet.h: any output over its threshold


def _nets():
    """(the product package loads its library on import: taken when a case is built, so that listing the cases needs none)"""
    from syllable_detector_swift_amd import nets
    return nets

LEVELS = (1.0, 2e-3, 40.0)           # channel c's samples are scaled by LEVELS[c]
SWITCHES = ("SYLDET_WIDE_NO_FRONT", "SYLDET_WIDE_SHAPE32", "SYLDET_WIDE_M32", "SYLDET_WIDE_NOSTAGGER", "SYLDET_WIDE_WG16",
            "SYLDET_WIDE_T4", "SYLDET_WIDE_TANH_POLY", "SYLDET_WIDE_DMA_BUILTIN")
G16, G32S, G32 = "wide_gemm16_kernel", "wide_gemm32s_kernel", "wide_gemm_kernel"
CHAIN, PREP = "wide_prep_chain_kernel", "wide_prep_kernel"


def form(label="default", env=(), gemm=G16, prep=None, **model):
    """model: the switches the model must know (no_front, shape32, tanh_poly)"""
    return SimpleNamespace(label=label, env={k: "1" for k in env}, gemm=gemm, prep=prep, model=model)


DEFAULT = form()
PREPARED = form("no_front", ["SYLDET_WIDE_NO_FRONT"], prep=CHAIN, no_front=True)


def eval_samples(cfg, E):
    """S = window + (T - 1 + E - 1) hop, plus a few samples"""
    return cfg.windowLength + (cfg.timeRange - 1 + E - 1) * (cfg.windowLength - cfg.windowOverlap) + 3


def band(base, F, lo=2000.0):
    """a freqRange from `lo` that holds F bins: bins ceil(N lo / fs) .. floor(N hi / fs), both included (frequencyIndexRange,
    CircularShortTimeFourierTransform.swift:166-191)"""
    step = base.samplingRate / base.fourierLength
    start = int(np.ceil(lo / step))
    assert start + F <= base.fourierLength // 2
    return (lo, (start + F - 0.5) * step)


class Case:
    def __init__(self, name, make, forms=(DEFAULT,), C=2, E=300, first=60, route="front", special=None):
        self.name, self._make, self.forms, self.C, self.first, self.route, self.special = name, make, list(forms), C, first, route, special
        self.E = [E] if isinstance(E, int) else list(E)
        self._cfg = None

    @property
    def cfg(self):
        if self._cfg is None:
            self._cfg = self._make()
        return self._cfg

    def sizes(self):
        return [eval_samples(self.cfg, e) for e in self.E]

    def samples(self, S):
        from syllable_detector_swift_amd import synth
        x = synth.channels(self.C, S, first=self.first, fs=self.cfg.samplingRate)
        x = (x * np.array(LEVELS[:self.C], np.float32)[:, None]).astype(np.float32)
        if self.special == "silence_nan":              # a stretch of zeros longer than a window of frames; one NaN sample
            x[0, S // 3:S // 3 + 6000] = 0.0
            x[1, S // 2] = np.nan
        return x

    def __repr__(self):
        return self.name


def _net(seed, I=290, H=(64,), n_out=1, **kw):
    return _nets().random_net(np.random.default_rng(seed), I, H, n_out, **kw)


def _banded(seed, F, T, H=64, **kw):
    base = _nets().from_npz()
    return _nets().variant(base, freqRange=band(base, F), timeRange=T, net=_net(seed, F * T, (H,), 1, **kw))


def _narrow():
    net = _net(31, in_fns=("l2normalize", "mapminmax"))
    f = net.inputProcessing[1]
    f.xOffsets, f.gains = np.full(290, 0.05, np.float32), np.full(290, 100.0, np.float32)
    return _nets().variant(_nets().from_npz(), net=net)


def _scaled(seed, scaling, in_fns, F=40, T=7):
    """log / dB columns on a band of more than 32 bins (the run and spectrogram() then share the generic transform)"""
    cfg = _banded(seed, F, T, in_fns=in_fns)
    cfg.spectrogramScaling = scaling
    if in_fns == ("mapminmax",):                       # dB values of about -110 .. 40 onto about -1 .. 1
        f = cfg.net.inputProcessing[0]
        f.xOffsets, f.gains, f.y = np.full(F * T, -110.0, np.float32), np.full(F * T, 2.0 / 150.0, np.float32), -1.0
    if in_fns == ("mapstd",):                          # natural logarithms of about -13 .. 3 onto about -1 .. 1
        f = cfg.net.inputProcessing[0]
        f.xOffsets, f.gains, f.y = np.full(F * T, -5.0, np.float32), np.full(F * T, 0.125, np.float32), 0.0
    return cfg


def _forms_front():
    return [DEFAULT, form("m32", ["SYLDET_WIDE_M32"], gemm=G32S), form("nostagger", ["SYLDET_WIDE_NOSTAGGER"]),
            form("wg16", ["SYLDET_WIDE_WG16"]), form("t4", ["SYLDET_WIDE_T4"]),
            form("tanh_poly", ["SYLDET_WIDE_TANH_POLY"], tanh_poly=True)]


def _forms_prepared():
    return [PREPARED, form("shape32", ["SYLDET_WIDE_SHAPE32"], gemm=G32, prep=CHAIN, shape32=True)]


def log_behind_normaliser():
    """log columns in front of normalizestd, mapstd: wide_prep_kernel's scaling branch.  Not among all_cases(): the model cannot
    follow the hardware logarithm's last place through a normaliser (see H64_log_columns below, and tools/debug/wide_log_normaliser.py)"""
    return Case("H64_log_normalizestd_mapstd", lambda: _scaled(17, "log", ("normalizestd", "mapstd")), [form(prep=PREP)], C=3, first=150,
                route="prepared")


def all_cases():
    """(the configurations are built when a case is first used: listing the cases needs no built library)"""
    base = lambda: _nets().from_npz()
    v = lambda *a, **kw: _nets().variant(*a, **kw)
    wide_mlp = lambda b: _nets().wide_mlp(b)
    H96 = lambda: v(base(), net=_net(5, H=(96,)))
    cs = [
        # routes and forms: the shipped form and every A/B switch, on BASELINE configs[4] (H = 4096) and on H = 96
        Case("config5_front_forms", lambda: wide_mlp(base()), _forms_front(), C=2, E=521, first=60),
        Case("config5_prepared_forms", lambda: wide_mlp(base()), _forms_prepared(), C=2, E=521, first=60, route="prepared"),
        Case("H96_front_forms", H96, _forms_front(), C=3, E=521, first=70),
        Case("H96_prepared_forms", H96, _forms_prepared(), C=3, E=521, first=70, route="prepared"),
        # chains and transfer functions
        # the polynomial form's LogSig folding (acc halved, w1 halved, b1 + sum w1 / 2), beside the exp2 form of the same network
        Case("H96_logsig_tanh_poly", lambda: v(base(), net=_net(21, H=(96,), transfer=("LogSig", "PureLin")), thresholds=[0.1]),
             [DEFAULT, form("tanh_poly", ["SYLDET_WIDE_TANH_POLY"], tanh_poly=True)], C=3, first=75),
        Case("H96_3out_logsig", lambda: v(base(), net=_net(11, H=(96,), n_out=3, transfer=("LogSig", "TanSig")), thresholds=[0.1, 0.2, 0.3],
                                          rule=RULE_ANY), C=3, first=80),
        Case("H40_normalize", lambda: v(base(), net=_net(12, H=(40,), transfer=("SatLin", "PureLin"), in_fns=("normalize",), out_fns=())),
             [form(prep=PREP)], C=3, first=90, route="prepared"),
        Case("H72_2out_satlin", lambda: v(base(), net=_net(13, H=(72,), n_out=2, transfer=("SatLin", "TanSig")), thresholds=[0.1, 0.2]),
             C=3, first=100),
        # (no normaliser: the level goes straight into the operands, and at 40 bf16 itself costs more than its 1e-2 -- two channels)
        Case("H64_affine_only", lambda: v(base(), net=_net(14, in_fns=("mapstd",))), C=2, first=110),
        Case("H48_two_maps", lambda: v(base(), net=_net(15, H=(48,), in_fns=("l2normalize", "mapminmax", "mapstd"))), C=3, first=120),
        Case("H48_two_maps_prepared", lambda: v(base(), net=_net(15, H=(48,), in_fns=("l2normalize", "mapminmax", "mapstd"))),
             [form("no_front", ["SYLDET_WIDE_NO_FRONT"], prep=PREP, no_front=True)], C=3, first=120, route="prepared"),
        Case("H64_narrow_range_maps", _narrow, [form(prep=CHAIN)], C=3, first=130, route="prepared"),
        Case("H64_normalizestd_mapstd", lambda: v(base(), net=_net(16, in_fns=("normalizestd", "mapstd"))), [form(prep=PREP)], C=3, first=140,
             route="prepared"),
        # log / dB columns behind an affine map.  (Behind a NORMALISER the model cannot follow the engine: the hardware logarithm is within
        # an ulp of the correctly rounded one the model takes, 4.8e-7 at |log| ~ 5, and (x - mean) / sd hands that on as 8 and more
        # ulps of an operand near 1 -- outside the w = 8 window.  Measured with ("normalizestd", "mapstd") here: 12 of 900
        # evaluations beyond 1e-5, the worst 3.3e-4, none flagged as a near tie, every one brought under the bar by ONE operand's other
        # rounding: tools/debug/wide_log_normaliser.py.  That shape is log_behind_normaliser() above, held at 1e-2.)
        Case("H64_log_columns", lambda: _scaled(17, "log", ("mapstd",)), [form(prep=CHAIN)], C=3, first=150, route="prepared"),
        Case("H64_db_columns", lambda: _scaled(18, "db", ("mapminmax",)), [form(prep=CHAIN)], C=3, first=160, route="prepared"),
        Case("H64_4out_any", lambda: v(base(), net=_net(19, n_out=4), thresholds=[0.3, 0.1, 0.2, 0.4], rule=RULE_ANY), C=3, first=170),
    ]
    # hidden widths at chunk edges: one to five chunks, last chunks of 1 and 31 real units
    for k, H in enumerate((32, 33, 63, 64, 65, 96, 97, 128, 160)):
        cs.append(Case("H%d" % H, (lambda H=H: v(base(), net=_net(40 + H, H=(H,)))), first=200 + 10 * k))
    # network inputs I = F T: the K tail, the 19 / 20 k-step instantiations of the 32x32x16 kernel (I <= 304 / > 304), the LDS fits
    m32 = form("m32", ["SYLDET_WIDE_M32"], gemm=G32S)
    for k, (F, T, forms, route) in enumerate([
            (29, 1, [DEFAULT, m32], "front"), (32, 9, [DEFAULT], "front"), (16, 19, [DEFAULT, m32], "front"), (5, 61, [DEFAULT, m32], "front"),
            (29, 11, [DEFAULT, m32], "front"), (32, 10, [DEFAULT, m32], "front"),
            # either side of the two-workgroup forms' fit (columns under 256 evaluations in half a CU's LDS): past it one workgroup
            # of 16 waves, and the 32x32x16 switch keeps the 16x16x32 kernel
            (33, 9, [DEFAULT, m32], "front"), (34, 9, [DEFAULT, form("m32", ["SYLDET_WIDE_M32"], gemm=G16)], "front"),
            # either side of wide_front_fits (columns under 512 evaluations): past it the preparation route
            (52, 6, [DEFAULT], "front"), (53, 6, [form(prep=CHAIN)], "prepared")]):
        cs.append(Case("I%d_F%d_T%d" % (F * T, F, T), (lambda F=F, T=T: _banded(300 + F, F, T)), forms, first=300 + 10 * k, route=route))
    # evaluation counts at the tiles' edges (16 a wave's tile, 256 / 512 a workgroup), two channels: the front numbers evaluations
    # within a channel, the prepared route through all channels
    counts = (1, 15, 16, 17, 255, 256, 257, 511, 512, 513)
    for H in (32, 96):
        cs.append(Case("H%d_counts_front" % H, (lambda H=H: v(base(), net=_net(60 + H, H=(H,)))), E=counts, first=400 + H))
        cs.append(Case("H%d_counts_prepared" % H, (lambda H=H: v(base(), net=_net(60 + H, H=(H,)))), [PREPARED], E=counts, first=400 + H,
                       route="prepared"))
    # silence (0 / 0 = NaN behind l2normalize) and a NaN sample
    cs.append(Case("H96_silence_nan_front", H96, E=330, first=500, special="silence_nan"))
    cs.append(Case("H96_silence_nan_prepared", H96, [PREPARED], E=330, first=500, special="silence_nan", route="prepared"))
    return cs
