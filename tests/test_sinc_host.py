"""The band-limited rate converter's host side (no device): syldet_sinc_coefficient against the fp64 model of tests/sinc_ref.py,
syldet_sinc_taps, every status the device entry points give before they touch a device, and the model held to what the design
promises -- tones in the band come through, tones between the new and the old Nyquist frequency do not."""
import ctypes as C
import math

import numpy as np
import pytest

import sinc_ref
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

LIB = _abi.lib
RATIOS = [(48000.0, 44100.0), (44100.0, 48000.0), (96000.0, 44100.0), (22050.0, 44100.0), (24414.0625, 44100.0)]
QUALITIES = [sinc_ref.DEFAULTS, (8, 6.0, 0.8), (64, 12.0, 0.9), (4, 0.0, 1.0), (64, 20.0, 0.05)]


def test_defaults():
    z, b, r = C.c_int32(0), C.c_double(0), C.c_double(0)
    LIB.syldet_sinc_defaults(C.byref(z), C.byref(b), C.byref(r))
    assert (z.value, b.value, r.value) == sinc_ref.DEFAULTS == sd.sincDefaults()
    LIB.syldet_sinc_defaults(None, None, None)                  # NULL: skipped


@pytest.mark.parametrize("rates", RATIOS + [(44100.0, 44100.0), (16.0, 1.0), (1.0, 16.0)])
@pytest.mark.parametrize("quality", QUALITIES)
def test_coefficient_matches_the_model(rates, quality):
    (ri, ro), (Z, beta, rho) = rates, quality
    s, H = sinc_ref.design(ri, ro, rho, Z)
    rng = np.random.default_rng(5)
    grid = np.linspace(-H, H, 4097)
    near = np.concatenate([np.arange(-8, 9) / s, np.arange(-8, 9) / s + 1e-9, [0.0, 1e-300, -1e-12]])   # zero crossings and the centre
    t = np.concatenate([grid, near, rng.uniform(-H, H, 4000), rng.uniform(-1.5, 1.5, 1000)])
    got = np.array([LIB.syldet_sinc_coefficient(float(v), ri, ro, Z, beta, rho) for v in t])
    want = sinc_ref.coefficient(t, ri, ro, Z, beta, rho)
    assert np.abs(got - want).max() <= 1e-12
    assert got[np.abs(t) < 0.5 / s].max() <= s + 1e-12 and LIB.syldet_sinc_coefficient(0.0, ri, ro, Z, beta, rho) == pytest.approx(s, abs=1e-15)
    for v in (H, -H, math.nextafter(H, math.inf), 2 * H, -1e30, math.inf, -math.inf):
        assert LIB.syldet_sinc_coefficient(v, ri, ro, Z, beta, rho) == 0.0
    assert sd.sincCoefficient(0.25, ri, ro, Z, beta, rho) == LIB.syldet_sinc_coefficient(0.25, ri, ro, Z, beta, rho)


@pytest.mark.parametrize("rates", RATIOS + [(44100.0, 44100.0), (16.0, 1.0), (1.0, 16.0)])
@pytest.mark.parametrize("quality", QUALITIES)
def test_taps(rates, quality):
    (ri, ro), (Z, _, rho) = rates, quality
    H = sinc_ref.design(ri, ro, rho, Z)[1]
    assert LIB.syldet_sinc_taps(ri, ro, Z, rho) == 2 * math.floor(H) + 1 == sinc_ref.taps(ri, ro, Z, rho) == sd.sincTaps(ri, ro, Z, rho)
    # it is the count of an output that falls on an input sample (the first one does); between two samples one more may fit
    p = np.arange(2000) * ri / ro
    T = np.floor(p + H) - np.ceil(p - H) + 1
    assert T[0] == 2 * math.floor(H) + 1 and T[0] <= T.max() <= min(T[0] + 1, math.floor(2 * H) + 1)


BAD_QUALITY = [(3, 12.0, 0.9), (65, 12.0, 0.9), (-1, 12.0, 0.9), (32, -0.5, 0.9), (32, 20.5, 0.9), (32, math.nan, 0.9),
               (32, 12.0, 0.0), (32, 12.0, -0.1), (32, 12.0, 1.0 + 1e-9), (32, 12.0, math.nan)]
BAD_RATES = [(0.0, 44100.0), (48000.0, 0.0), (-48000.0, 44100.0), (48000.0, -1.0), (math.nan, 44100.0), (48000.0, math.nan)]
OUTSIDE = [(16.0001, 1.0), (1.0, 16.0001), (1e6, 1.0)]


def test_host_functions_refuse_bad_parameters():
    for Z, beta, rho in BAD_QUALITY:
        assert math.isnan(LIB.syldet_sinc_coefficient(0.0, 48000.0, 44100.0, Z, beta, rho))
        assert math.isnan(sd.sincCoefficient(0.0, 48000.0, 44100.0, Z, beta, rho))
    for Z, _, rho in [q for q in BAD_QUALITY if q[1] == 12.0]:
        assert LIB.syldet_sinc_taps(48000.0, 44100.0, Z, rho) == -1
    for ri, ro in BAD_RATES + OUTSIDE:
        assert math.isnan(LIB.syldet_sinc_coefficient(0.0, ri, ro, 32, 12.0, 0.9))
        assert LIB.syldet_sinc_taps(ri, ro, 32, 0.9) == -1 == sd.sincTaps(ri, ro)
    assert LIB.syldet_sinc_taps(16.0, 1.0, 64, 0.9) == 2 * math.floor(64 * 16 / 0.9) + 1       # the edge of the ratio is inside


def device_call(fn, d_in=0x1000, n_in=100, in_stride=128, C_=3, ri=48000.0, ro=44100.0, Z=32, beta=12.0, rho=0.9, d_out=0x2000,
                out_stride=128, with_n_out=True):
    """A device entry point on pointers no call may follow: each of these returns before it touches a device."""
    n_out = C.c_int64(-7)
    st = fn(d_in, n_in, in_stride, C_, ri, ro, Z, beta, rho, d_out, out_stride, C.byref(n_out) if with_n_out else None, None)
    return st, n_out.value


@pytest.mark.parametrize("name", ["syldet_convert_rate_sinc_device", "syldet_convert_rate_sinc_device_s16"])
def test_statuses_come_back_without_a_device(name):
    fn = getattr(LIB, name)
    inv, uns = _abi.ERR_INVALID_ARGUMENT, _abi.ERR_UNSUPPORTED
    assert device_call(fn, d_in=None) == (inv, 0)
    assert device_call(fn, d_out=None) == (inv, 0)
    assert device_call(fn, n_in=-1) == (inv, 0)
    assert device_call(fn, C_=0) == (inv, 0)
    assert device_call(fn, C_=-2) == (inv, 0)
    for ri, ro in BAD_RATES:
        assert device_call(fn, ri=ri, ro=ro) == (inv, 0)
    assert device_call(fn, in_stride=99) == (inv, 0)                                 # below the row of 100
    n = sinc_ref.count(100, 48000.0, 44100.0)
    assert device_call(fn, out_stride=n - 1) == (inv, 0)
    for Z, beta, rho in BAD_QUALITY:
        assert device_call(fn, Z=Z, beta=beta, rho=rho) == (inv, 0)
        assert device_call(fn, Z=Z, beta=beta, rho=rho, ri=17.0, ro=1.0) == (inv, 0)       # a bad parameter at any ratio
    for ri, ro in OUTSIDE:
        assert device_call(fn, ri=ri, ro=ro, out_stride=10 ** 6) == (uns, 0)
    assert device_call(fn, Z=64, rho=1e-4) == (uns, 0)                               # H = 64 / (0.91875 * 1e-4) > 65536
    assert device_call(fn, d_in=None, with_n_out=False)[0] == inv                    # n_out may be NULL
    assert _abi.last_error()
    # an empty recording: nothing written, nothing launched, *n_out = 0
    assert device_call(fn, n_in=0, in_stride=0, out_stride=0) == (_abi.OK, 0)


def tone(f, rate, n, amplitude=0.5):
    return amplitude * np.sin(2 * np.pi * f * np.arange(n) / rate + 0.3)


@pytest.fixture(scope="module")
def inputs():
    return {48000.0: 6000, 96000.0: 12000}


@pytest.mark.parametrize("f", [1000.0, 7000.0, 15000.0])
def test_model_passes_the_band(f, inputs):
    """48 -> 44.1 kHz at the defaults: a tone in the band comes out as the same tone sampled at the new rate, to 1e-6 away from
    the ends (the Kaiser design's 117 dB of ripple at amplitude 0.5, with a factor of two; measured 3.2e-7)."""
    ri, ro, n = 48000.0, 44100.0, inputs[48000.0]
    out = sinc_ref.convert(tone(f, ri, n), ri, ro)[0]
    want = 0.5 * np.sin(2 * np.pi * f * np.arange(out.size) / ro + 0.3)
    edge = int(math.ceil(sinc_ref.design(ri, ro, 0.9, 32)[1] * ro / ri)) + 1
    err = np.abs(out - want)[edge:-edge].max()
    print("f = %g Hz: max |model - tone| = %.3g" % (f, err))
    assert err <= 1e-6


@pytest.mark.parametrize("ri,f", [(48000.0, 23000.0), (96000.0, 30000.0)])
def test_model_stops_what_would_alias(ri, f, inputs):
    """A tone between the new Nyquist frequency and the old one leaves an RMS below 1e-6 at amplitude 0.5 (measured 1.9e-7)."""
    ro, n = 44100.0, inputs[ri]
    out = sinc_ref.convert(tone(f, ri, n), ri, ro)[0]
    edge = int(math.ceil(sinc_ref.design(ri, ro, 0.9, 32)[1] * ro / ri)) + 1
    rms = float(np.sqrt(np.mean(out[edge:-edge] ** 2)))
    print("%g Hz at %g Hz: RMS residue = %.3g" % (f, ri, rms))
    assert rms <= 1e-6


def test_model_counts():
    x = np.ones(30)
    out, A, X, T = sinc_ref.convert(x, 48000.0, 44100.0)
    H = sinc_ref.design(48000.0, 44100.0, 0.9, 32)[1]
    assert out.size == sinc_ref.count(30, 48000.0, 44100.0) == LIB.syldet_convert_rate_count(30, 48000.0, 44100.0)
    assert (X == 30).all() and (T >= math.floor(2 * H)).all() and (T <= math.floor(2 * H) + 1).all()    # H > 30: every output reads the whole row
    assert (A >= np.abs(out) - 1e-15).all()
