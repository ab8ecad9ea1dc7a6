"""The table of tests/fused_forms.py against the launchers' own source and their own routing, on the host (no GPU): every
instantiation the three fused kernel files compile is reached by exactly the case that names it, or is listed as unreachable with the
reason; syldet_fused_form_of_config runs the real launchers dry, so nothing here restates which shape goes where."""
import ctypes as C
import os

import pytest

import fused_forms as ff
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets

CHANNELS = 3


def predicted(case, monkeypatch, frames=None, **kw):
    ff.apply_env(monkeypatch, case.env)
    fa, fb = ff.sizes(case.cfg, case.leaf)
    return sd.fusedFormOfConfig(case.cfg, CHANNELS, ff.samples_for(case.cfg, frames or fb), s16=case.s16, spectrogram=case.spect, **kw)


def test_the_scanner_finds_the_leaves_of_every_file():
    """A broken scanner cannot pass by finding nothing; every tuple has the seam's shape."""
    per_file = {k: ff.scan(os.path.join(ff.CSRC, name)) for k, name in ff.FILES.items()}
    assert len(set(per_file[2])) >= 40 and len(set(per_file[0])) >= 60 and len(set(per_file[1])) >= 14, {k: len(set(v)) for k, v in per_file.items()}
    for v in per_file.values():
        assert all(len(p) == 10 and all(isinstance(a, int) for a in p) for p in v)
    # the diagnostic builds' instantiations stay out: one wave a SIMD, the stamped forms, the knock-outs, the multi-network recursion
    assert (2, (4, 0, 1, 4, 0, 1, 1, 0, 0, 0)) not in ff.leaves()
    assert not [p for p in per_file[0] if p[6] or p[7]] and not [p for p in per_file[1] if p[4]]
    assert not [p for p in per_file[2] if p[ff.S_MN]]


def test_every_leaf_has_exactly_the_case_that_reaches_it(monkeypatch):
    """{form_of_config(case) for case in CASES} and UNREACHABLE are disjoint and together are leaves(): a new or changed leaf
    fails here, by name, until a case reaches it; so does a case whose shape the routing moved elsewhere."""
    leaves = ff.leaves()
    reached = {}
    for case in ff.CASES:
        for frames in ff.sizes(case.cfg, case.leaf):              # both batch lengths of the GPU test take the same leaf
            got = predicted(case, monkeypatch, frames)
            assert got == case.leaf, "%s (%d frames): the launcher picks %s, the table says %s" % (case.name, frames, got, case.leaf)
        assert case.leaf not in reached, "%s and %s name the same leaf %s" % (reached[case.leaf], case.name, case.leaf)
        reached[case.leaf] = case.name
    assert not set(reached) & set(ff.UNREACHABLE), sorted(set(reached) & set(ff.UNREACHABLE))
    uncovered = leaves - set(reached) - set(ff.UNREACHABLE)
    assert not uncovered, "compiled instantiations no case reaches: %s" % sorted(uncovered)
    stale = (set(reached) | set(ff.UNREACHABLE)) - leaves
    assert not stale, "the table names instantiations the source no longer compiles: %s" % sorted(stale)
    assert all(isinstance(r, str) and len(r) > 20 for r in ff.UNREACHABLE.values())


def test_a_switch_only_where_no_public_configuration_reaches_the_leaf(monkeypatch):
    """The cases that set a switch need it: without it the same configuration runs another leaf."""
    for case in ff.CASES:
        if case.env:
            assert predicted(case._replace(env={}), monkeypatch) != case.leaf, case.name


NETWORK_FOLD_CASES = [c for c in ff.CASES if c.leaf[0] == 2 and not c.spect]


def test_every_network_leaf_of_the_fold_kernel_has_its_multi_network_twin(monkeypatch):
    """The same case as a bank of two networks of its class, channels alternating: the same tuple with MN = 1."""
    assert len(NETWORK_FOLD_CASES) == len([l for l in ff.leaves() if l[0] == 2 and not l[1][ff.S_SPECT]])
    for case in NETWORK_FOLD_CASES:
        ff.apply_env(monkeypatch, case.env)
        bank = [case.cfg, ff.sibling(case, 99)]
        assert sd.configsCompatible(*bank) == (True, None)
        fa, fb = ff.sizes(case.cfg, case.leaf)
        got = sd.fusedFormOfConfig(bank, CHANNELS, ff.samples_for(case.cfg, fb), channelNetworks=[0, 1, 0], s16=case.s16)
        p = list(case.leaf[1])
        p[ff.S_MN] = 1
        assert got == (2, tuple(p)), case.name


def test_the_16_bit_leaves_are_the_twins_of_their_fp32_cases(monkeypatch):
    s16 = [c for c in ff.CASES if c.s16]
    assert len(s16) == 2 == len([l for l in ff.leaves() if l[1][ff.S_S16] and l[0] == 2])
    for case in s16:
        p = list(case.leaf[1])
        p[ff.S_S16] = 0
        assert predicted(case._replace(s16=False), monkeypatch) == (2, tuple(p))
        assert predicted(case, monkeypatch) == case.leaf
    # a form without a 16-bit twin widens the samples first: the fp32 leaf
    cs8 = next(c for c in ff.CASES if c.name == "s_cs8_exact")
    assert predicted(cs8._replace(s16=True), monkeypatch) == cs8.leaf


def test_what_auto_keeps_elsewhere_is_not_on_the_fused_engine(monkeypatch):
    ff.apply_env(monkeypatch, {})
    base = ff.CASES[0].cfg
    for cfg, engine in ((nets.variant(base, spectrum=_abi.SPECTRUM_MAGNITUDE), _abi.ENGINE_AUTO), (base, _abi.ENGINE_GENERIC)):
        with pytest.raises(sd.SyllableDetectorError) as e:
            sd.fusedFormOfConfig(cfg, CHANNELS, 40000, engine=engine)
        assert e.value.status == _abi.ERR_UNSUPPORTED
    # no evaluation in the batch: nothing launches
    with pytest.raises(sd.SyllableDetectorError):
        sd.fusedFormOfConfig(base, CHANNELS, 10)


def test_band_cases_are_the_bands_intended(monkeypatch):
    ff.apply_env(monkeypatch, {})
    from syllable_detector_swift_amd.config import frequencyIndexRange
    seen = set()
    for b in ff.BAND_CASES:
        r = frequencyIndexRange(b.cfg.fourierLength, b.cfg.samplingRate, *b.cfg.freqRange)
        assert (r[0], r[1] - r[0]) == (b.f0, b.F), b.name
        fa, fb = ff.sizes(b.cfg, b.leaf)
        assert sd.fusedFormOfConfig(b.cfg, CHANNELS, ff.samples_for(b.cfg, fb)) == b.leaf, b.name
        seen.add((b.name.rsplit("_f0_", 1)[0], b.f0, b.F))
    for form in ("fold1_w128", "fold1_w256_n512", "fold2_w256"):
        N = 128 if form == "fold1_w128" else (512 if "n512" in form else 256)
        Fs = {F for f, f0, F in seen if f == form}
        assert {1, 2, 15, 16, 17, 31, 32} <= Fs, (form, Fs)
        assert {33, 64} <= Fs if form == "fold2_w256" else max(Fs) == 32
        f0s = {f0 for f, f0, F in seen if f == form}
        assert 0 in f0s and any(f % 2 for f in f0s) and any(f and f % 2 == 0 for f in f0s)
        assert any(f0 + F == N // 2 for f, f0, F in seen if f == form)


def _call(cfgs, channel_net, kernel, params, n_nets=1):
    return _abi.lib.syldet_fused_form_of_config(cfgs, n_nets, channel_net, CHANNELS, 40000, 0, 0, _abi.ENGINE_AUTO, kernel, params)


def test_the_seam_rejects_null_arguments_and_leaves_no_dry_run_behind(monkeypatch):
    ff.apply_env(monkeypatch, {})
    c, keep = ff.CASES[0].cfg.to_abi()
    ptrs = (_abi.Config_p * 1)(C.pointer(c))
    kernel, params = C.c_int32(), (C.c_int32 * 10)()
    assert _call(ptrs, None, C.byref(kernel), params) == _abi.OK
    assert _abi.lib.syldet_fused_dry_run_active() == 0
    assert _call(None, None, C.byref(kernel), params) == _abi.ERR_INVALID_ARGUMENT
    assert _call(ptrs, None, None, params) == _abi.ERR_INVALID_ARGUMENT
    assert _call(ptrs, None, C.byref(kernel), None) == _abi.ERR_INVALID_ARGUMENT
    assert _call((_abi.Config_p * 1)(), None, C.byref(kernel), params) == _abi.ERR_INVALID_ARGUMENT
    two = (_abi.Config_p * 2)(C.pointer(c), C.pointer(c))
    assert _call(two, None, C.byref(kernel), params, n_nets=2) == _abi.ERR_INVALID_ARGUMENT         # (two networks need a channel_net)
    assert _abi.lib.syldet_last_fused_form(None, C.byref(kernel), params) == _abi.ERR_INVALID_ARGUMENT
    assert _abi.lib.syldet_fused_dry_run_active() == 0
    # a plan that fails to build (a window longer than the transform: compute_geometry refuses it) ends the dry run too
    bad, keep_bad = nets.variant(ff.CASES[0].cfg, windowLength=1024).to_abi()
    assert _call((_abi.Config_p * 1)(C.pointer(bad)), None, C.byref(kernel), params) == _abi.ERR_FFT_SIZE
    assert _abi.lib.syldet_fused_dry_run_active() == 0
    # ... and one the fused engine refuses outright (more than 64 bins under ENGINE_FUSED)
    with pytest.raises(sd.SyllableDetectorError):
        sd.fusedFormOfConfig(nets.variant(ff.CASES[0].cfg, freqRange=(100.0, 20000.0)), CHANNELS, 40000, engine=_abi.ENGINE_FUSED)
    assert _abi.lib.syldet_fused_dry_run_active() == 0
    del keep, keep_bad
