"""ResamplerLinear (Common/Resampler.swift:20-76) for a bank of channels on the GPU.

Same surface as the reference class -- `ResamplerLinear(fromRate:toRate:)`, `resampleVector`, `resampleArray`
-- over libsyldet's `syldet_resample*`; state (fractional offset, last sample of every channel) carries over
between calls exactly as in the reference.

`convertRate` is the whole-recording converter of the file path (the step the reference's tool leaves to AVFoundation,
Common/SyllableDetector.swift:19-23): linear interpolation at fp64 positions, or the band-limited Kaiser-windowed sinc whose
convention include/syldet.h states; `sincCoefficient` and `sincTaps` are that convention's host functions.

`ResamplerSinc` is that band-limited converter as a second conformer of the reference's Resampler protocol: the same outputs block
by block (`resampleVector` push after push, then `flush`), bit for bit the whole-recording call's however the recording is cut;
`sincReady` is its emission rule in host arithmetic.
"""
import ctypes as C

import numpy as np

from . import _abi
from .config import check


def deinterleave(frames, first_channel: int = 0, channels=None, stream=None):
    """frames [n, total] float32 CUDA tensor -> [channels, n] channel-major (appendInterleavedData's strided copy,
    CircularShortTimeFourierTransform.swift:203-217, for all requested channels at once)."""
    import torch
    if not (frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 2 and frames.is_contiguous()):
        raise ValueError("frames must be a contiguous 2-D float32 CUDA tensor [n_frames, total_channels]")
    n, total = int(frames.shape[0]), int(frames.shape[1])
    channels = total - first_channel if channels is None else int(channels)
    out = torch.empty((channels, n), dtype=torch.float32, device=frames.device)
    s = stream if stream is not None else torch.cuda.current_stream(frames.device)
    check(_abi.lib.syldet_deinterleave_device(frames.data_ptr(), n, total, int(first_channel), channels, out.data_ptr(), n,
                                              int(s.cuda_stream)))
    return out


def sincDefaults():
    """(zeroCrossings, beta, rolloff) a call without them uses."""
    z, b, r = C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
    _abi.lib.syldet_sinc_defaults(C.byref(z), C.byref(b), C.byref(r))
    return int(z.value), float(b.value), float(r.value)


def _sinc_quality(zeroCrossings, beta, rolloff):
    z, b, r = sincDefaults()
    return (z if zeroCrossings is None else int(zeroCrossings), b if beta is None else float(beta),
            r if rolloff is None else float(rolloff))


def sincCoefficient(t: float, fromRate: float, toRate: float, zeroCrossings=None, beta=None, rolloff=None) -> float:
    """h(t) of the sinc convention in fp64 (t in input samples); NaN for parameters the converter refuses.  No device."""
    z, b, r = _sinc_quality(zeroCrossings, beta, rolloff)
    return float(_abi.lib.syldet_sinc_coefficient(float(t), float(fromRate), float(toRate), z, b, r))


def sincTaps(fromRate: float, toRate: float, zeroCrossings=None, rolloff=None) -> int:
    """2 floor(H) + 1, the input samples an output on an input sample reads (one more may fit between two); -1 for parameters
    the converter refuses.  No device."""
    z, _, r = _sinc_quality(zeroCrossings, None, rolloff)
    return int(_abi.lib.syldet_sinc_taps(float(fromRate), float(toRate), z, r))


def sincReady(nInTotal: int, fromRate: float, toRate: float, zeroCrossings=None, rolloff=None) -> int:
    """ready(N) of the streaming sinc convention: the outputs a ResamplerSinc has emitted once it has received nInTotal samples
    (before its flush); -1 for parameters the converter refuses.  No device."""
    z, _, r = _sinc_quality(zeroCrossings, None, rolloff)
    return int(_abi.lib.syldet_sinc_ready(int(nInTotal), float(fromRate), float(toRate), z, r))


def convertRate(rows, fromRate: float, toRate: float, method: str = "linear", zeroCrossings=None, beta=None, rolloff=None,
                stream=None):
    """rows [C, n] (or [n]) CUDA tensor at fromRate -> float32 rows [C, n_out] at toRate, asynchronous on `stream`.

    method "linear": syldet_convert_rate_device (float32 rows).  method "sinc": the band-limited converter, float32 rows or the
    int16 rows of 16-bit PCM (x meaning x / 32768; the float32 call's bits); zeroCrossings, beta and rolloff default to
    sincDefaults().  The first sinc call for a (zeroCrossings, beta) on a device copies the filter's table there and blocks."""
    import torch
    if method not in ("linear", "sinc"):
        raise ValueError("method must be 'linear' or 'sinc'")
    if method == "linear" and not (zeroCrossings is None and beta is None and rolloff is None):
        raise ValueError("zeroCrossings, beta and rolloff belong to method='sinc'")
    x = rows if rows.dim() == 2 else rows.reshape(1, -1)
    kinds = (torch.float32, torch.int16) if method == "sinc" else (torch.float32,)
    if not (x.is_cuda and x.dtype in kinds and x.dim() == 2 and x.shape[0] >= 1 and (x.shape[1] == 0 or x.stride(1) == 1)):
        raise ValueError("rows must be a %s CUDA tensor with one contiguous row per channel" % " or ".join(str(k) for k in kinds))
    channels, n_in = int(x.shape[0]), int(x.shape[1])
    n_out = int(_abi.lib.syldet_convert_rate_count(n_in, float(fromRate), float(toRate)))
    out = torch.empty((channels, n_out), dtype=torch.float32, device=x.device)
    if n_in == 0 and float(fromRate) > 0 and float(toRate) > 0:      # an empty recording: no buffer to hand over
        return out if rows.dim() == 2 else out.reshape(-1)
    got = C.c_int64(0)
    s = stream if stream is not None else torch.cuda.current_stream(x.device)
    with torch.cuda.device(x.device):
        if method == "linear":
            check(_abi.lib.syldet_convert_rate_device(x.data_ptr(), n_in, int(x.stride(0)), channels, float(fromRate), float(toRate),
                                                      out.data_ptr(), max(n_out, 1), C.byref(got), int(s.cuda_stream)))
        else:
            z, b, r = _sinc_quality(zeroCrossings, beta, rolloff)
            fn = _abi.lib.syldet_convert_rate_sinc_device_s16 if x.dtype == torch.int16 else _abi.lib.syldet_convert_rate_sinc_device
            check(fn(x.data_ptr(), n_in, int(x.stride(0)), channels, float(fromRate), float(toRate), z, b, r,
                     out.data_ptr(), max(n_out, 1), C.byref(got), int(s.cuda_stream)))
    assert got.value == n_out
    return out if rows.dim() == 2 else out.reshape(-1)


class ResamplerLinear:
    def __init__(self, fromRate: float, toRate: float, channels: int = 1, device: int = 0):
        self.samplingRateIn, self.samplingRateOut = float(fromRate), float(toRate)
        self.channels, self.device = int(channels), int(device)
        h = _abi.Handle()
        check(_abi.lib.syldet_resampler_create(self.samplingRateIn, self.samplingRateOut, self.channels, self.device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _abi.lib.syldet_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def countOutput(self, n_in: int) -> int:
        return int(_abi.lib.syldet_resampler_count(self._h, int(n_in)))

    def resampleVector(self, data, stream=None):
        """data [C, n] (or [n] for one channel) float32 CUDA tensor -> [C, n_out] resampled, asynchronous on `stream`."""
        import torch
        x = data if data.dim() == 2 else data.reshape(1, -1)
        if not (x.is_cuda and x.dtype == torch.float32 and x.shape[0] == self.channels and x.stride(1) == 1):
            raise ValueError("data must be a float32 CUDA tensor with one contiguous row per channel")
        n_in = int(x.shape[1])
        n_out = self.countOutput(n_in)
        out = torch.empty((self.channels, n_out), dtype=torch.float32, device=x.device)
        got = C.c_int64(0)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        check(_abi.lib.syldet_resample_device(self._h, x.data_ptr(), n_in, int(x.stride(0)), out.data_ptr(), max(n_out, 1),
                                              C.byref(got), int(s.cuda_stream)))
        assert got.value == n_out
        return out if data.dim() == 2 else out.reshape(-1)

    def resampleArray(self, arr) -> np.ndarray:
        """Host arrays ([n] or [C, n]); the reference's test helper (:71-75)."""
        a = np.ascontiguousarray(arr, dtype=np.float32)
        x = a.reshape(self.channels, -1)
        n_in = x.shape[1]
        n_out = self.countOutput(n_in)
        out = np.zeros((self.channels, n_out), np.float32)
        got = C.c_int64(0)
        check(_abi.lib.syldet_resample(self._h, x.ctypes.data_as(_abi.c_float_p), n_in, n_in,
                                       out.ctypes.data_as(_abi.c_float_p), max(n_out, 1), C.byref(got)))
        assert got.value == n_out
        return out if a.ndim == 2 else out.reshape(-1)


class ResamplerSinc:
    """The band-limited converter as a stream (syldet_sinc_resampler_*): push blocks of any sizes with `resampleVector` (device
    tensors, asynchronous) or `resampleArray` (host arrays, blocking), then `flush` / `flushArray` for the recording's last
    outputs.  The concatenation is `convertRate(rows, method="sinc")` of the whole rows, bit for bit.  Outputs trail inputs by
    H = zeroCrossings / (min(1, toRate / fromRate) * rolloff) input samples.  All device work of one object belongs on one
    stream (or is ordered by the caller)."""

    def __init__(self, fromRate: float, toRate: float, channels: int = 1, device: int = 0, zeroCrossings=None, beta=None, rolloff=None):
        self.samplingRateIn, self.samplingRateOut = float(fromRate), float(toRate)
        self.channels, self.device = int(channels), int(device)
        self.zeroCrossings, self.beta, self.rolloff = _sinc_quality(zeroCrossings, beta, rolloff)
        h = _abi.Handle()
        check(_abi.lib.syldet_sinc_resampler_create(self.samplingRateIn, self.samplingRateOut, self.channels, self.device,
                                                    self.zeroCrossings, self.beta, self.rolloff, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _abi.lib.syldet_sinc_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def reset(self):
        """Back to an empty stream (also after a flush)."""
        check(_abi.lib.syldet_sinc_resampler_reset(self._h))

    @property
    def position(self):
        """(samples received, outputs emitted, finished) per channel."""
        n, m, f = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        check(_abi.lib.syldet_sinc_resampler_position(self._h, C.byref(n), C.byref(m), C.byref(f)))
        return int(n.value), int(m.value), bool(f.value)

    def countOutput(self, n_in: int) -> int:
        return int(_abi.lib.syldet_sinc_resampler_count(self._h, int(n_in)))

    def countFlush(self) -> int:
        return int(_abi.lib.syldet_sinc_resampler_flush_count(self._h))

    def resampleVector(self, data, stream=None):
        """data [C, n] (or [n] for one channel) float32 or int16 CUDA tensor -> [C, n_out] float32, asynchronous on `stream`."""
        import torch
        x = data if data.dim() == 2 else data.reshape(1, -1)
        if not (x.is_cuda and x.dtype in (torch.float32, torch.int16) and x.shape[0] == self.channels and
                (x.shape[1] == 0 or x.stride(1) == 1)):
            raise ValueError("data must be a float32 or int16 CUDA tensor with one contiguous row per channel")
        n_in = int(x.shape[1])
        n_out = self.countOutput(n_in)
        out = torch.empty((self.channels, n_out), dtype=torch.float32, device=x.device)
        got = C.c_int64(0)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        fn = _abi.lib.syldet_sinc_resample_device_s16 if x.dtype == torch.int16 else _abi.lib.syldet_sinc_resample_device
        check(fn(self._h, x.data_ptr() if n_in else None, n_in, int(x.stride(0)), out.data_ptr() if n_out else None, max(n_out, 1),
                 C.byref(got), int(s.cuda_stream)))
        assert got.value == n_out
        return out if data.dim() == 2 else out.reshape(-1)

    def flush(self, stream=None):
        """Ends the recording: the outputs still owed, [C, n] float32 on the handle's device.  Then only reset() reopens it."""
        import torch
        n_out = self.countFlush()
        dev = torch.device("cuda", self.device)
        out = torch.empty((self.channels, n_out), dtype=torch.float32, device=dev)
        got = C.c_int64(0)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        check(_abi.lib.syldet_sinc_resampler_flush_device(self._h, out.data_ptr() if n_out else None, max(n_out, 1), C.byref(got),
                                                          int(s.cuda_stream)))
        assert got.value == n_out
        return out

    def resampleArray(self, arr) -> np.ndarray:
        """Host arrays ([n] or [C, n]), blocking; the reference's test helper (:71-75)."""
        a = np.ascontiguousarray(arr, dtype=np.float32)
        x = a.reshape(self.channels, -1)
        n_in = x.shape[1]
        n_out = self.countOutput(n_in)
        out = np.zeros((self.channels, n_out), np.float32)
        got = C.c_int64(0)
        check(_abi.lib.syldet_sinc_resample(self._h, x.ctypes.data_as(_abi.c_float_p), n_in, n_in,
                                            out.ctypes.data_as(_abi.c_float_p), max(n_out, 1), C.byref(got)))
        assert got.value == n_out
        return out if a.ndim == 2 else out.reshape(-1)

    def flushArray(self) -> np.ndarray:
        n_out = self.countFlush()
        out = np.zeros((self.channels, n_out), np.float32)
        got = C.c_int64(0)
        check(_abi.lib.syldet_sinc_resampler_flush(self._h, out.ctypes.data_as(_abi.c_float_p), max(n_out, 1), C.byref(got)))
        assert got.value == n_out
        return out
