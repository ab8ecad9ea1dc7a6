"""The band-limited rate converter on the GPU (syldet_convert_rate_sinc_device and its int16 form) against the fp64 model of
tests/sinc_ref.py.  The bar, for EVERY output of every case:

    |got - ref| <= T 2^-24 A + 2^-21 X

T the number of taps of the output, A = sum |h x|, X = sum |x|: the worst case of a T-term fp32 dot product, plus every fp32
coefficient allowed 2^-21 from the exact one (coefficients are at most 1 in size).  Each case prints the largest ratio of error
to bar it saw (MEASUREMENTS.md holds them).  The int16 form, other strides, other channel counts and a second run must give the
fp32 form's bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sinc_ref
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

pytestmark = pytest.mark.gpu

LIB = _abi.lib
RATIOS = [(48000.0, 44100.0), (44100.0, 48000.0), (96000.0, 44100.0), (22050.0, 44100.0), (24414.0625, 44100.0)]
DEFAULTS = sinc_ref.DEFAULTS
SENTINEL = 12345.0


def device_convert(rows, ri, ro, quality=DEFAULTS, out_stride=None, base=None, in_stride=None, n_in=None, channels=None):
    """rows: a 2-D CUDA tensor [C, n] (float32 or int16) whose rows are in_stride apart -> ([C, n_out] float32, status); the
    output rows are out_stride apart in a buffer of sentinels, and everything the call had no business writing is checked."""
    Cn = rows.shape[0] if channels is None else channels
    n = rows.shape[1] if n_in is None else n_in
    n_out = sinc_ref.count(n, ri, ro) if ri > 0 and ro > 0 else 0
    out_stride = n_out + 5 if out_stride is None else out_stride
    out = torch.full((Cn, max(out_stride, 1)), SENTINEL, dtype=torch.float32, device="cuda")
    got = C.c_int64(-1)
    fn = LIB.syldet_convert_rate_sinc_device_s16 if rows.dtype == torch.int16 else LIB.syldet_convert_rate_sinc_device
    Z, beta, rho = quality
    st = fn(rows.data_ptr() if base is None else base, n, rows.stride(0) if in_stride is None else in_stride, Cn, ri, ro, Z, beta, rho,
            out.data_ptr(), out_stride, C.byref(got), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if st == _abi.OK:
        assert got.value == n_out
        assert (out[:, n_out:] == SENTINEL).all(), "wrote behind the rows"
    else:
        assert got.value == 0 and (out == SENTINEL).all()
    return out[:, :n_out], st


def strided(x, stride, offset=0):
    """x [C, n] (numpy) on the device with its rows `stride` apart, `offset` elements into the buffer; the gaps hold sentinels."""
    Cn, n = x.shape
    fill = 77 if x.dtype == np.int16 else SENTINEL
    buf = torch.full((offset + Cn * stride,), fill, dtype=torch.int16 if x.dtype == np.int16 else torch.float32, device="cuda")
    view = buf[offset:].view(Cn, stride)[:, :n]
    view.copy_(torch.from_numpy(np.array(x)))                    # (a copy: the shared cases are read-only)
    return view


@functools.lru_cache(maxsize=None)
def case(ri, ro, n, quality, channels=3, seed=0):
    """The rows of a case (uniform in [-1, 1]) and the model's four arrays for each, made once."""
    x = np.random.default_rng([seed, n, int(ri), int(ro)]).uniform(-1.0, 1.0, (channels, n)).astype(np.float32)
    ref = [sinc_ref.convert(x[c], ri, ro, *quality) for c in range(channels)]
    for a in ref:
        for v in a:
            v.setflags(write=False)
    x.setflags(write=False)
    return x, ref


def check_against_model(got, ref, label):
    worst = 0.0
    for c, (want, A, X, T) in enumerate(ref):
        g = got[c].astype(np.float64)
        assert g.shape == want.shape
        err, bar = np.abs(g - want), sinc_ref.bound(A, X, T)
        assert np.isfinite(g).all()
        ratio = np.divide(err, bar, out=np.where(err > 0, np.inf, 0.0), where=bar > 0)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    print("%s: largest |got - ref| / bar = %.3f over %d outputs" % (label, worst, sum(r[0].size for r in ref)))
    for c, (want, A, X, T) in enumerate(ref):
        assert (np.abs(got[c].astype(np.float64) - want) <= sinc_ref.bound(A, X, T)).all(), label
    return worst


@pytest.mark.parametrize("n", [1, 2, 40, 3000])
@pytest.mark.parametrize("rates", RATIOS)
def test_defaults_against_the_model(rates, n):
    """n = 1, 2, 40: shorter than H, both ends under one filter; 3000: the seams of several workgroups."""
    ri, ro = rates
    x, ref = case(ri, ro, n, DEFAULTS)
    got, st = device_convert(strided(x, n + 7), ri, ro)
    assert st == _abi.OK
    check_against_model(got.cpu().numpy(), ref, "%g -> %g, n_in = %d, defaults" % (ri, ro, n))


@pytest.mark.parametrize("rates", RATIOS)
def test_another_quality_against_the_model(rates):
    ri, ro = rates
    q = (8, 6.0, 0.8)
    x, ref = case(ri, ro, 3000, q)
    got, st = device_convert(strided(x, 3011), ri, ro, q)
    assert st == _abi.OK
    check_against_model(got.cpu().numpy(), ref, "%g -> %g, n_in = 3000, Z = 8, beta = 6, rolloff = 0.8" % (ri, ro))


def test_largest_table():
    q = (64, 12.0, 0.9)
    x, ref = case(48000.0, 44100.0, 3000, q)
    got, st = device_convert(strided(x, 3001), 48000.0, 44100.0, q)
    assert st == _abi.OK
    check_against_model(got.cpu().numpy(), ref, "48000 -> 44100, n_in = 3000, Z = 64")


def test_edge_of_the_ratio_has_the_widest_halo():
    """16 : 1 with Z = 64: H = 1137.8 input samples either side, 16 inputs an output."""
    q = (64, 12.0, 0.9)
    x, ref = case(16.0, 1.0, 8192, q)
    got, st = device_convert(strided(x, 8200), 16.0, 1.0, q)
    assert st == _abi.OK
    check_against_model(got.cpu().numpy(), ref, "16 -> 1, n_in = 8192, Z = 64")
    x, ref = case(1.0, 16.0, 300, q)                            # ... and the other edge: 16 outputs an input
    got, st = device_convert(strided(x, 301), 1.0, 16.0, q)
    assert st == _abi.OK
    check_against_model(got.cpu().numpy(), ref, "1 -> 16, n_in = 300, Z = 64")


def test_late_positions_are_fp64():
    """n_in = 2^24 + 1000: behind 2^24 an fp32 position has no fraction left; the last 512 outputs against the model evaluated
    for that stretch alone."""
    ri, ro, n = 48000.0, 44100.0, 2 ** 24 + 1000
    x = np.random.default_rng(24).uniform(-1.0, 1.0, (1, n)).astype(np.float32)
    got, st = device_convert(torch.from_numpy(x).cuda(), ri, ro)
    assert st == _abi.OK
    n_out = sinc_ref.count(n, ri, ro)
    ref = sinc_ref.convert(x[0], ri, ro, start=n_out - 512, stop=n_out)
    check_against_model(got[:, n_out - 512:].cpu().numpy(), [ref], "48000 -> 44100, n_in = 2^24 + 1000, last 512 outputs")


@pytest.mark.parametrize("rates", RATIOS)
def test_int16_rows_give_the_fp32_bits(rates):
    """The rows syldet_deinterleave_device_s16 writes, one element into their buffer and an odd number of elements apart."""
    ri, ro = rates
    q16 = np.random.default_rng([16, int(ri)]).integers(-32768, 32768, (3, 3000)).astype(np.int16)
    q16[0, :4] = [-32768, 32767, 0, -1]
    as_float = (q16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    want, st = device_convert(strided(as_float, 3004), ri, ro)
    assert st == _abi.OK
    for stride, offset in ((3001, 1), (3003, 1), (3000, 0)):
        got, st = device_convert(strided(q16, stride, offset), ri, ro)
        assert st == _abi.OK
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (stride, offset)
    x, ref = as_float, [sinc_ref.convert(as_float[0], ri, ro)]
    check_against_model(want[:1].cpu().numpy(), ref, "%g -> %g, int16 rows" % (ri, ro))


@pytest.mark.parametrize("rates", RATIOS)
def test_an_output_depends_on_its_own_row_alone(rates):
    ri, ro = rates
    x, _ = case(ri, ro, 3000, DEFAULTS)
    alone, st = device_convert(torch.from_numpy(x[2:3].copy()).cuda(), ri, ro, out_stride=sinc_ref.count(3000, ri, ro))
    assert st == _abi.OK
    for stride, out_stride in ((3000, None), (3013, 6001), (4096, 8192)):
        among, st = device_convert(strided(x, stride), ri, ro, out_stride=out_stride)
        assert st == _abi.OK
        assert torch.equal(among[2].view(torch.int32), alone[0].view(torch.int32)), (stride, out_stride)
    again, _ = device_convert(torch.from_numpy(x[2:3].copy()).cuda(), ri, ro)
    assert torch.equal(again.view(torch.int32), alone.view(torch.int32))


def test_statuses_through_the_device_entry_points():
    inv, uns = _abi.ERR_INVALID_ARGUMENT, _abi.ERR_UNSUPPORTED
    for dtype in (np.float32, np.int16):
        rows = strided(np.zeros((3, 100), dtype), 128)
        ok = dict(ri=48000.0, ro=44100.0)
        assert device_convert(rows, **ok)[1] == _abi.OK
        assert device_convert(rows, base=0, **ok)[1] == inv                               # NULL input
        assert device_convert(rows, n_in=-1, **ok)[1] == inv
        assert device_convert(rows, channels=0, **ok)[1] == inv
        assert device_convert(rows, in_stride=99, **ok)[1] == inv
        assert device_convert(rows, out_stride=sinc_ref.count(100, 48000.0, 44100.0) - 1, **ok)[1] == inv
        for ri, ro in ((0.0, 44100.0), (48000.0, -1.0), (float("nan"), 44100.0)):
            assert device_convert(rows, ri, ro, out_stride=256)[1] == inv
        for q in ((3, 12.0, 0.9), (65, 12.0, 0.9), (32, -0.1, 0.9), (32, 20.1, 0.9), (32, 12.0, 0.0), (32, 12.0, 1.01)):
            assert device_convert(rows, quality=q, **ok)[1] == inv
        for ri, ro in ((16.001, 1.0), (1.0, 16.001)):
            assert device_convert(rows, ri, ro, out_stride=4096)[1] == uns
        assert device_convert(rows, quality=(64, 12.0, 1e-4), **ok)[1] == uns
        out, st = device_convert(rows, n_in=0, **ok)                                      # nothing written, *n_out = 0
        assert st == _abi.OK and out.shape[1] == 0
        n_out = C.c_int64(-1)
        fn = LIB.syldet_convert_rate_sinc_device_s16 if dtype == np.int16 else LIB.syldet_convert_rate_sinc_device
        assert fn(rows.data_ptr(), 100, 128, 3, 48000.0, 44100.0, 32, 12.0, 0.9, None, 128, C.byref(n_out), None) == inv and n_out.value == 0


def test_convertRate():
    """The Python surface: both methods, both sample types, one row or several."""
    ri, ro = 48000.0, 44100.0
    x, ref = case(ri, ro, 3000, DEFAULTS)
    rows = torch.from_numpy(x.copy()).cuda()
    want, _ = device_convert(rows, ri, ro)
    got = sd.convertRate(rows, ri, ro, method="sinc")
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(sd.convertRate(rows[1], ri, ro, method="sinc"), want[1])
    q = (8, 6.0, 0.8)
    assert torch.equal(sd.convertRate(rows, ri, ro, "sinc", *q), device_convert(rows, ri, ro, q)[0])
    q16 = torch.from_numpy(np.random.default_rng(3).integers(-32768, 32768, (2, 500)).astype(np.int16)).cuda()
    assert torch.equal(sd.convertRate(q16, ri, ro, "sinc"), sd.convertRate(q16.to(torch.float32) / 32768.0, ri, ro, "sinc"))
    # linear: syldet_convert_rate_device, as before
    lin = sd.convertRate(rows, ri, ro)
    pos = np.arange(lin.shape[1], dtype=np.float64) * (ri / ro)
    k = np.minimum(pos.astype(np.int64), 2999)
    model = (x[:, k].astype(np.float64) + (pos - k) * (x[:, np.minimum(k + 1, 2999)].astype(np.float64) - x[:, k])).astype(np.float32)
    assert np.array_equal(lin.cpu().numpy(), model)
    assert sd.convertRate(rows[:, :0], ri, ro, "sinc").shape == (3, 0)
    with pytest.raises(ValueError):
        sd.convertRate(rows, ri, ro, method="cubic")
    with pytest.raises(ValueError):
        sd.convertRate(q16, ri, ro)                              # the linear form takes float32
    with pytest.raises(ValueError):
        sd.convertRate(rows, ri, ro, rolloff=0.5)                # ... and no quality
    with pytest.raises(sd.SyllableDetectorError):
        sd.convertRate(rows, ri, ro, "sinc", zeroCrossings=2)
