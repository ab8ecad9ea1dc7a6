"""Host-side mirror of SyllableDetector over the C ABI.

Keeps the reference's surface (Common/SyllableDetector.swift): init(config:) :37,
appendAudioData :129, processNewValue :153, lastOutputs :26, lastDetected :27,
seenSyllable :220 -- per channel of a bank -- and adds the batch entry points the MI355X
engine is built around (whole recordings of many channels in one pass).  All arithmetic
happens in libsyldet's HIP kernels; torch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .config import SyllableDetectorConfig, SyllableDetectorError, check


def _torch():
    import torch
    return torch


class SyllableDetector:
    def __init__(self, config: SyllableDetectorConfig, channels: int = 1, device: int = 0,
                 engine: int = _abi.ENGINE_AUTO):
        self.config = config
        self.channels = int(channels)
        self.device = int(device)
        self._h = _abi.Handle()
        c, keep = config.to_abi()
        check(_abi.lib.syldet_create(C.byref(c), self.channels, self.device, int(engine), C.byref(self._h)))
        del keep                      # the library copied every array
        g = _abi.Geometry()
        check(_abi.lib.syldet_get_geometry(self._h, C.byref(g)))
        self.geometry = g

    @classmethod
    def multi(cls, configs: Sequence[SyllableDetectorConfig], channelNetworks, device: int = 0,
              engine: int = _abi.ENGINE_AUTO) -> "SyllableDetector":
        """One bank, a network per channel (syldet_create_multi; ProcessorBase.init, Processor.swift:50-86): channel c runs
        configs[channelNetworks[c]].  The configurations must be compatible (configsCompatible); `config` is configs[0] and
        `configs` the list."""
        return cls._banked(_abi.lib.syldet_create_multi, configs, channelNetworks, device, engine)

    @classmethod
    def mixed(cls, configs: Sequence[SyllableDetectorConfig], channelNetworks, device: int = 0,
              engine: int = _abi.ENGINE_AUTO) -> "SyllableDetector":
        """One bank of networks that differ in band, FFT size, chain or widths (syldet_create_mixed): channel c runs
        configs[channelNetworks[c]].  The configurations need only share the evaluation clock (configsShareClock); each class
        of compatible ones runs as a multi bank of its own would.  `geometry` holds -1 where the classes differ
        (channelGeometry(c) has each channel's own)."""
        return cls._banked(_abi.lib.syldet_create_mixed, configs, channelNetworks, device, engine)

    @classmethod
    def _banked(cls, create, configs, channelNetworks, device, engine) -> "SyllableDetector":
        configs = list(configs)
        nets = np.ascontiguousarray(channelNetworks, dtype=np.int32).reshape(-1)
        self = cls.__new__(cls)
        self.config = configs[0] if configs else None
        self.configs = configs
        self.channelNetworks = nets.copy()
        self.channels = int(nets.size)
        self.device = int(device)
        self._h = _abi.Handle()
        abi = [cfg.to_abi() for cfg in configs]
        ptrs = (_abi.Config_p * max(1, len(abi)))(*[C.pointer(c) for c, _ in abi])
        check(create(ptrs, len(abi), nets.ctypes.data_as(_abi.c_int32_p), self.channels, self.device, int(engine), C.byref(self._h)))
        del abi                       # the library copied every array
        g = _abi.Geometry()
        check(_abi.lib.syldet_get_geometry(self._h, C.byref(g)))
        self.geometry = g
        return self

    @classmethod
    def borrowed(cls, bank, shard: int) -> "SyllableDetector":
        """Shard `shard`'s own bank of a ShardedSyllableDetectorBank as a SyllableDetector (timings, fix-up statistics, spot
        checks); it belongs to the sharded bank and is not destroyed with this object."""
        self = cls.__new__(cls)
        self.config = bank.config
        self.channels = int(bank.shards[shard].channels)
        self.device = int(bank.shards[shard].device)
        self._h = _abi.Handle(_abi.lib.syldet_sharded_bank(bank._h, int(shard)))
        self._borrowed = True
        g = _abi.Geometry()
        check(_abi.lib.syldet_get_geometry(self._h, C.byref(g)))
        self.geometry = g
        return self

    def channelGeometry(self, channel: int):
        """syldet_channel_geometry: the geometry of channel `channel`'s own network (bins, inputs, engine of its class)."""
        g = _abi.Geometry()
        check(_abi.lib.syldet_channel_geometry(self._h, int(channel), C.byref(g)))
        return g

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                _abi.lib.syldet_destroy(self._h)
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

    # ---- geometry -----------------------------------------------------------------
    def countFrames(self, n_samples: int) -> int:
        return int(_abi.lib.syldet_count_frames(self._h, int(n_samples)))

    def countEvaluations(self, n_samples: int) -> int:
        return int(_abi.lib.syldet_count_evals(self._h, int(n_samples)))

    # ---- the reference's streaming API, one detector per channel -------------------
    def appendAudioData(self, data, channel: int = 0) -> None:
        a = np.ascontiguousarray(data, dtype=np.float32)
        check(_abi.lib.syldet_append(self._h, channel, a.ctypes.data_as(_abi.c_float_p), a.size))

    def appendInterleavedData(self, data, fromChannels=None) -> None:
        """appendInterleavedData(_:withSamples:fromChannel:ofTotalChannels:) (CircularShortTimeFourierTransform.swift:203-217):
        `data` [frames, total channels]; fromChannels (one stream channel per bank channel) picks a subset of a wider stream."""
        if fromChannels is None:
            a = np.ascontiguousarray(data, dtype=np.float32).reshape(-1, self.channels)
            check(_abi.lib.syldet_append_interleaved(self._h, a.ctypes.data_as(_abi.c_float_p), a.shape[0], self.channels))
            return
        a = np.ascontiguousarray(data, np.float32)
        src = np.ascontiguousarray(fromChannels, np.int32)
        if a.ndim != 2 or src.shape != (self.channels,):
            raise ValueError("data [frames, total channels] and one source channel per bank channel")
        check(_abi.lib.syldet_append_interleaved_channels(self._h, a.ctypes.data_as(_abi.c_float_p), a.shape[0], a.shape[1],
                                                          src.ctypes.data_as(_abi.C.POINTER(_abi.C.c_int32))))

    def appendAudioDataPCM16(self, data, channel: int = 0) -> None:
        """appendAudioData for 16-bit PCM (syldet_append_s16): an int16 array whose sample x means x / 32768, converted exactly on
        the way into the channel's fp32 ring."""
        a = np.ascontiguousarray(_pcm16(data))
        check(_abi.lib.syldet_append_s16(self._h, channel, a.ctypes.data_as(_abi.c_int16_p), a.size))

    def appendInterleavedDataPCM16(self, data) -> None:
        """appendInterleavedData for 16-bit PCM (syldet_append_interleaved_s16): int16 `data` [frames, channels]."""
        a = np.ascontiguousarray(_pcm16(data)).reshape(-1, self.channels)
        check(_abi.lib.syldet_append_interleaved_s16(self._h, a.ctypes.data_as(_abi.c_int16_p), a.shape[0], self.channels))

    def processNewValue(self, channel: int = 0) -> bool:
        return check(_abi.lib.syldet_process_new_value(self._h, channel)) == 1

    def processAll(self) -> int:
        """Evaluates what every channel has pending in one device round trip (the consumer loop of
        Processor.swift:128-141 over all detectors); returns the evaluations queued.  The following
        processNewValue calls hand them out without touching the device."""
        n = C.c_int64(0)
        check(_abi.lib.syldet_process_all(self._h, C.byref(n)))
        return n.value

    def pendingEvaluations(self, channel: int = 0) -> int:
        return check(_abi.lib.syldet_pending_evaluations(self._h, channel))

    def lastOutputsFor(self, channel: int) -> List[float]:
        out = np.zeros(self.geometry.outputs, np.float32)
        check(_abi.lib.syldet_last_outputs(self._h, channel, out.ctypes.data_as(_abi.c_float_p)))
        return out.tolist()

    @property
    def lastOutputs(self) -> List[float]:
        return self.lastOutputsFor(0)

    def lastDetectedFor(self, channel: int) -> bool:
        return check(_abi.lib.syldet_last_detected(self._h, channel)) == 1

    @property
    def lastDetected(self) -> bool:
        return self.lastDetectedFor(0)

    def seenSyllable(self, channel: int = 0) -> bool:
        return check(_abi.lib.syldet_seen_syllable(self._h, channel)) == 1

    # ---- batch, device tensors ----------------------------------------------------
    def _stream_ptr(self, stream) -> int:
        torch = _torch()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return int(s.cuda_stream)

    def _check_samples(self, samples):
        torch = _torch()
        if not (samples.is_cuda and samples.dtype == torch.float32 and samples.dim() == 2):
            raise ValueError("samples must be a 2-D float32 CUDA tensor [channels, n_samples]")
        if samples.shape[0] != self.channels or samples.stride(1) != 1:
            raise ValueError("samples must have one contiguous row per channel")
        if samples.device.index != self.device:
            raise ValueError("samples live on a different device than the detector")

    def _check_results(self, outputs, flags, E, device):
        """Caller-supplied result tensors go to the kernels as raw pointers: shape, dtype, layout and device must be right."""
        torch = _torch()
        if outputs is not None:
            want = (self.channels, E, self.geometry.outputs)
            if not (outputs.is_cuda and outputs.dtype == torch.float32 and tuple(outputs.shape) == want and outputs.is_contiguous()
                    and outputs.device == device):
                raise ValueError("outputs must be a contiguous float32 CUDA tensor of shape %s on the samples' device" % (want,))
        if flags is not None:
            want = (self.channels, E)
            if not (flags.is_cuda and flags.dtype == torch.uint8 and tuple(flags.shape) == want and flags.is_contiguous()
                    and flags.device == device):
                raise ValueError("flags must be a contiguous uint8 CUDA tensor of shape %s on the samples' device" % (want,))

    def run(self, samples, outputs=None, flags=None, stream=None):
        """samples [C, S] -> (outputs [C, E, n_out] f32, flags [C, E] u8), asynchronous on `stream`."""
        torch = _torch()
        self._check_samples(samples)
        S = int(samples.shape[1])
        E = self.countEvaluations(S)
        self._check_results(outputs, flags, E, samples.device)
        if outputs is None:
            outputs = torch.empty((self.channels, E, self.geometry.outputs), dtype=torch.float32, device=samples.device)
        if flags is None:
            flags = torch.empty((self.channels, E), dtype=torch.uint8, device=samples.device)
        check(_abi.lib.syldet_run_device(self._h, samples.data_ptr(), S, int(samples.stride(0)),
                                         outputs.data_ptr(), flags.data_ptr(), self._stream_ptr(stream)))
        return outputs, flags

    def runPCM16(self, samples, outputs=None, flags=None, stream=None):
        """16-bit PCM samples [C, S] (an int16 CUDA tensor, x meaning x / 32768) -> (outputs, flags) like run(), bit for bit what
        run() gives for samples.float() * 2**-15 (syldet_run_device_s16)."""
        torch = _torch()
        if not (samples.is_cuda and samples.dtype == torch.int16 and samples.dim() == 2):
            raise ValueError("samples must be a 2-D int16 CUDA tensor [channels, n_samples]")
        if samples.shape[0] != self.channels or samples.stride(1) != 1:
            raise ValueError("samples must have one contiguous row per channel")
        if samples.device.index != self.device:
            raise ValueError("samples live on a different device than the detector")
        S = int(samples.shape[1])
        E = self.countEvaluations(S)
        self._check_results(outputs, flags, E, samples.device)
        if outputs is None:
            outputs = torch.empty((self.channels, E, self.geometry.outputs), dtype=torch.float32, device=samples.device)
        if flags is None:
            flags = torch.empty((self.channels, E), dtype=torch.uint8, device=samples.device)
        check(_abi.lib.syldet_run_device_s16(self._h, samples.data_ptr(), S, int(samples.stride(0)),
                                             outputs.data_ptr(), flags.data_ptr(), self._stream_ptr(stream)))
        return outputs, flags

    def runInterleavedPCM16(self, frames, outputs=None, flags=None, stream=None):
        """16-bit PCM frames [n, C] (an int16 CUDA tensor) -> (outputs, flags) like runInterleaved() on frames.float() * 2**-15
        (syldet_run_interleaved_device_s16)."""
        torch = _torch()
        if not (frames.is_cuda and frames.dtype == torch.int16 and frames.dim() == 2 and frames.is_contiguous()):
            raise ValueError("frames must be a contiguous 2-D int16 CUDA tensor [n_frames, channels]")
        if frames.shape[1] != self.channels or frames.device.index != self.device:
            raise ValueError("frames must have one column per channel and live on the detector's device")
        n = int(frames.shape[0])
        E = max(self.countEvaluations(n), 0)
        self._check_results(outputs, flags, E, frames.device)
        if outputs is None:
            outputs = torch.empty((self.channels, E, self.geometry.outputs), dtype=torch.float32, device=frames.device)
        if flags is None:
            flags = torch.empty((self.channels, E), dtype=torch.uint8, device=frames.device)
        check(_abi.lib.syldet_run_interleaved_device_s16(self._h, frames.data_ptr(), n, self.channels, outputs.data_ptr(),
                                                         flags.data_ptr(), self._stream_ptr(stream)))
        return outputs, flags

    def runInterleaved(self, frames, outputs=None, flags=None, stream=None):
        """frames [n, C] (frame-major, as a decoder delivers audio) -> (outputs, flags) like run()."""
        torch = _torch()
        if not (frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 2 and frames.is_contiguous()):
            raise ValueError("frames must be a contiguous 2-D float32 CUDA tensor [n_frames, channels]")
        if frames.shape[1] != self.channels or frames.device.index != self.device:
            raise ValueError("frames must have one column per channel and live on the detector's device")
        n = int(frames.shape[0])
        E = max(self.countEvaluations(n), 0)
        self._check_results(outputs, flags, E, frames.device)
        if outputs is None:
            outputs = torch.empty((self.channels, E, self.geometry.outputs), dtype=torch.float32, device=frames.device)
        if flags is None:
            flags = torch.empty((self.channels, E), dtype=torch.uint8, device=frames.device)
        check(_abi.lib.syldet_run_interleaved_device(self._h, frames.data_ptr(), n, self.channels, outputs.data_ptr(),
                                                     flags.data_ptr(), self._stream_ptr(stream)))
        return outputs, flags

    def runInterleavedHost(self, frames: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        a = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, self.channels)
        n = a.shape[0]
        E = max(self.countEvaluations(n), 0)
        out = np.zeros((self.channels, E, self.geometry.outputs), np.float32)
        fl = np.zeros((self.channels, E), np.uint8)
        check(_abi.lib.syldet_run_interleaved(self._h, a.ctypes.data_as(_abi.c_float_p), n, self.channels,
                                              out.ctypes.data_as(_abi.c_float_p), fl.ctypes.data_as(_abi.c_uint8_p)))
        return out, fl

    def runInterleavedPCM16Host(self, frames: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """runInterleavedHost for 16-bit PCM: int16 frames [n, C] (syldet_run_interleaved_s16; half the bytes cross the bus)."""
        a = np.ascontiguousarray(_pcm16(frames)).reshape(-1, self.channels)
        n = a.shape[0]
        E = max(self.countEvaluations(n), 0)
        out = np.zeros((self.channels, E, self.geometry.outputs), np.float32)
        fl = np.zeros((self.channels, E), np.uint8)
        check(_abi.lib.syldet_run_interleaved_s16(self._h, a.ctypes.data_as(_abi.c_int16_p), n, self.channels,
                                                  out.ctypes.data_as(_abi.c_float_p), fl.ctypes.data_as(_abi.c_uint8_p)))
        return out, fl

    def spectrogram(self, samples, stream=None):
        """samples [C, S] -> columns [C, J, bins] f32 (what processFourierData appends)."""
        torch = _torch()
        self._check_samples(samples)
        S = int(samples.shape[1])
        J = self.countFrames(S)
        # (a mixed bank of several classes has no one bin count, -1: the library refuses the call)
        cols = torch.empty((self.channels, J, max(self.geometry.bins, 0)), dtype=torch.float32, device=samples.device)
        check(_abi.lib.syldet_spectrogram_device(self._h, samples.data_ptr(), S, int(samples.stride(0)),
                                                 cols.data_ptr(), self._stream_ptr(stream)))
        return cols

    def detections(self, flags, debounce: float = 0.0, capacity: Optional[int] = None, stream=None):
        """flags [C, E] u8 -> (indices [C, capacity] i64, counts [C] i64); TrackDetector.swift:65-100."""
        torch = _torch()
        if not (flags.is_cuda and flags.dtype == torch.uint8 and flags.dim() == 2 and flags.shape[0] == self.channels
                and flags.is_contiguous() and flags.device.index == self.device):
            raise ValueError("flags must be a contiguous uint8 CUDA tensor [channels, n_evals] on the detector's device")
        E = int(flags.shape[1])
        cap = E if capacity is None else int(capacity)
        idx = torch.empty((self.channels, max(cap, 1)), dtype=torch.int64, device=flags.device)
        cnt = torch.empty((self.channels,), dtype=torch.int64, device=flags.device)
        check(_abi.lib.syldet_detections_device(self._h, flags.data_ptr(), E, float(debounce), idx.data_ptr(), cap,
                                                cnt.data_ptr(), self._stream_ptr(stream)))
        return idx, cnt

    # ---- the Simulator's output track ---------------------------------------------------
    @staticmethod
    def _trace_dtype(dtype, interleaved):
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.float32), np.dtype(np.int16)):
            raise ValueError("dtype must be np.float32 or np.int16 (got %s)" % dt)
        if interleaved and dt != np.dtype(np.int16):
            raise ValueError("interleaved=True needs dtype=np.int16 (frames as a 16-bit WAV stores them)")
        return dt

    def trace(self, outputs, n_samples: int, output: int = 0, dtype=np.float32, interleaved: bool = False, out=None, stream=None):
        """The Simulator's output track (ViewControllerSimulator.swift:251-344; syldet_trace_device*): outputs [C, n_evals, n_out]
        (a float32 CUDA tensor, as run() returns it) -> trace [C, n_samples], output `output` as a fraction of its channel's
        threshold, clamped to [0, 1] and held from one evaluation to the next; 0 before the first evaluation's sample number and
        behind the last hold.  dtype np.float32: the reference's values; np.int16: rint(v * 32767), NaN -> 0.  interleaved=True
        (int16 only): frames [n_samples, C], what a 16-bit WAV of C tracks stores.  `out`: a tensor to write into (rows may be
        wider than n_samples: only the first n_samples of each are written).  Asynchronous on `stream`."""
        torch = _torch()
        dt = self._trace_dtype(dtype, interleaved)
        tdt = torch.float32 if dt == np.dtype(np.float32) else torch.int16
        n = int(n_samples)
        if n < 0:
            raise ValueError("n_samples must not be negative")
        if not (outputs.is_cuda and outputs.dtype == torch.float32 and outputs.dim() == 3 and outputs.is_contiguous()
                and outputs.shape[0] == self.channels and outputs.shape[2] == self.geometry.outputs
                and outputs.device.index == self.device):
            raise ValueError("outputs must be a contiguous float32 CUDA tensor [channels, n_evals, outputs] on the detector's device")
        E = int(outputs.shape[1])
        if out is None:
            out = torch.empty((n, self.channels) if interleaved else (self.channels, n), dtype=tdt, device=outputs.device)
        elif interleaved:
            if not (out.is_cuda and out.dtype == tdt and tuple(out.shape) == (n, self.channels) and out.is_contiguous()
                    and out.device == outputs.device):
                raise ValueError("out must be a contiguous int16 CUDA tensor [n_samples, channels] on the outputs' device")
        else:
            if not (out.is_cuda and out.dtype == tdt and out.dim() == 2 and out.shape[0] == self.channels and out.shape[1] >= n
                    and (out.shape[1] == 0 or out.stride(1) == 1) and (self.channels == 1 or out.stride(0) >= n)
                    and out.device == outputs.device):
                raise ValueError("out must be a CUDA tensor [channels, >= n_samples] of the trace's dtype with contiguous rows")
        if n == 0:
            return out
        # (an empty tensor has no address: a bank too short for one evaluation still gets its rows of zeros)
        src = outputs if E > 0 else torch.zeros(1, dtype=torch.float32, device=outputs.device)
        if interleaved:
            check(_abi.lib.syldet_trace_interleaved_device_s16(self._h, src.data_ptr(), E, int(output), out.data_ptr(), n,
                                                               self._stream_ptr(stream)))
        else:
            fn = _abi.lib.syldet_trace_device if dt == np.dtype(np.float32) else _abi.lib.syldet_trace_device_s16
            stride = int(out.stride(0)) if self.channels > 1 else max(int(out.shape[1]), n)
            check(fn(self._h, src.data_ptr(), E, int(output), out.data_ptr(), n, stride, self._stream_ptr(stream)))
        return out

    def traceHost(self, outputs: np.ndarray, n_samples: int, output: int = 0, dtype=np.float32) -> np.ndarray:
        """trace() on host arrays, blocking (syldet_trace / syldet_trace_s16): outputs [C, n_evals, n_out] -> [C, n_samples]."""
        dt = self._trace_dtype(dtype, False)
        n = int(n_samples)
        if n < 0:
            raise ValueError("n_samples must not be negative")
        a = np.ascontiguousarray(outputs, dtype=np.float32)
        if a.ndim != 3 or a.shape[0] != self.channels or a.shape[2] != self.geometry.outputs:
            raise ValueError("outputs must be [channels, n_evals, outputs]")
        E = a.shape[1]
        src = a if E > 0 else np.zeros(1, np.float32)
        tr = np.zeros((self.channels, n), dt)
        if n == 0:
            return tr
        if dt == np.dtype(np.float32):
            check(_abi.lib.syldet_trace(self._h, src.ctypes.data_as(_abi.c_float_p), E, int(output), tr.ctypes.data_as(_abi.c_float_p), n, n))
        else:
            check(_abi.lib.syldet_trace_s16(self._h, src.ctypes.data_as(_abi.c_float_p), E, int(output), tr.ctypes.data_as(_abi.c_int16_p), n, n))
        return tr

    def simulate(self, samples, output: int = 0, dtype=np.int16, stream=None):
        """The Simulator in one call (simulateNetwork, ViewControllerSimulator.swift:251-344): run() followed by trace() on device
        tensors; samples [C, S] float32 -> (trace [C, S], outputs [C, E, n_out], flags [C, E])."""
        self._trace_dtype(dtype, False)
        outputs, flags = self.run(samples, stream=stream)
        tr = self.trace(outputs, int(samples.shape[1]), output=output, dtype=dtype, stream=stream)
        return tr, outputs, flags

    # ---- the TTL trigger track (Processor.swift:128-148, AudioInterface.swift:13-40, :442-445) ---------
    def triggerWidth(self, seconds: float = 0.001) -> int:
        """Int(seconds * samplingRate), createHighOutput's width (AudioInterface.swift:444; syldet_trigger_width)."""
        n = int(_abi.lib.syldet_trigger_width(float(seconds), float(self.config.samplingRate)))
        if n < 1:
            raise ValueError("a pulse of %r s is shorter than one sample at this rate" % (seconds,))
        return n

    def _trigger_args(self, flags, n_samples, bufferLength, width, latency):
        torch = _torch()
        n = int(n_samples)
        if n < 0:
            raise ValueError("n_samples must not be negative")
        if not (flags.is_cuda and flags.dtype == torch.uint8 and flags.dim() == 2 and flags.shape[0] == self.channels
                and flags.is_contiguous() and flags.device.index == self.device):
            raise ValueError("flags must be a contiguous uint8 CUDA tensor [channels, n_evals] on the detector's device")
        L = int(bufferLength)
        N = self.triggerWidth() if width is None else int(width)
        lat = int(latency)
        if L < 8 or L > 4096 or L & (L - 1):
            raise ValueError("bufferLength must be a power of two in [8, 4096]")
        if not 1 <= N <= 1 << 24:
            raise ValueError("width must be in [1, 2**24] samples")
        if not 0 <= lat <= 1 << 24:
            raise ValueError("latency must be in [0, 2**24] samples")
        E = int(flags.shape[1])
        # (an empty tensor has no address: a bank too short for one evaluation still gets its zeros)
        src = flags if E > 0 else torch.zeros(1, dtype=torch.uint8, device=flags.device)
        return n, L, N, lat, E, src

    def triggerTrack(self, flags, n_samples: int, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0,
                     dtype=np.float32, interleaved: bool = False, out=None, stream=None):
        """The TTL track the rig would have emitted (syldet_trigger_device*): flags [C, n_evals] (a uint8 CUDA tensor, as run()
        returns it) -> track [C, n_samples], high for `width` samples (default triggerWidth(): 1 ms) from the render buffer behind
        every callback buffer of bufferLength samples that made a flagged evaluation available, `latency` samples later; a
        later detection inside a pulse extends it.  dtype np.float32: 1.0 / 0.0, the reference's floats; np.int16: 32767 / 0.
        interleaved=True (int16 only): frames [n_samples, C], what a 16-bit WAV of C tracks stores.  `out` as in trace().
        Asynchronous on `stream`."""
        torch = _torch()
        dt = self._trace_dtype(dtype, interleaved)
        tdt = torch.float32 if dt == np.dtype(np.float32) else torch.int16
        n, L, N, lat, E, src = self._trigger_args(flags, n_samples, bufferLength, width, latency)
        if out is None:
            out = torch.empty((n, self.channels) if interleaved else (self.channels, n), dtype=tdt, device=flags.device)
        elif interleaved:
            if not (out.is_cuda and out.dtype == tdt and tuple(out.shape) == (n, self.channels) and out.is_contiguous()
                    and out.device == flags.device):
                raise ValueError("out must be a contiguous int16 CUDA tensor [n_samples, channels] on the flags' device")
        else:
            if not (out.is_cuda and out.dtype == tdt and out.dim() == 2 and out.shape[0] == self.channels and out.shape[1] >= n
                    and (out.shape[1] == 0 or out.stride(1) == 1) and (self.channels == 1 or out.stride(0) >= n)
                    and out.device == flags.device):
                raise ValueError("out must be a CUDA tensor [channels, >= n_samples] of the track's dtype with contiguous rows")
        if n == 0:
            return out
        if interleaved:
            check(_abi.lib.syldet_trigger_interleaved_device_s16(self._h, src.data_ptr(), E, L, N, lat, out.data_ptr(), n,
                                                                 self._stream_ptr(stream)))
        else:
            fn = _abi.lib.syldet_trigger_device if dt == np.dtype(np.float32) else _abi.lib.syldet_trigger_device_s16
            stride = int(out.stride(0)) if self.channels > 1 else max(int(out.shape[1]), n)
            check(fn(self._h, src.data_ptr(), E, L, N, lat, out.data_ptr(), n, stride, self._stream_ptr(stream)))
        return out

    def triggerTrackPCM16(self, flags, n_samples: int, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0,
                          out=None, stream=None):
        """triggerTrack() as 16-bit PCM rows [C, n_samples]: 32767 / 0 (syldet_trigger_device_s16)."""
        return self.triggerTrack(flags, n_samples, bufferLength, width, latency, dtype=np.int16, out=out, stream=stream)

    def triggerTrackInterleavedPCM16(self, flags, n_samples: int, bufferLength: int = 32, width: Optional[int] = None,
                                     latency: int = 0, out=None, stream=None):
        """triggerTrack() as 16-bit PCM frames [n_samples, C] (syldet_trigger_interleaved_device_s16)."""
        return self.triggerTrack(flags, n_samples, bufferLength, width, latency, dtype=np.int16, interleaved=True, out=out, stream=stream)

    def triggerMuxPCM16(self, flags, samples, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0, out=None,
                        stream=None):
        """The file a DAQ would have recorded, for every channel at once (syldet_trigger_mux_device_s16): samples [C, S] (the int16
        CUDA tensor runPCM16() takes) and flags -> frames [S, 2 C] int16, frame f = (audio[0][f], ttl[0][f], audio[1][f], ...);
        the audio is copied bit for bit."""
        torch = _torch()
        if not (samples.is_cuda and samples.dtype == torch.int16 and samples.dim() == 2 and samples.shape[0] == self.channels
                and (samples.shape[1] == 0 or samples.stride(1) == 1) and samples.device.index == self.device):
            raise ValueError("samples must be a 2-D int16 CUDA tensor [channels, n_samples] with contiguous rows on the detector's device")
        n, L, N, lat, E, src = self._trigger_args(flags, int(samples.shape[1]), bufferLength, width, latency)
        if out is None:
            out = torch.empty((n, 2 * self.channels), dtype=torch.int16, device=flags.device)
        elif not (out.is_cuda and out.dtype == torch.int16 and tuple(out.shape) == (n, 2 * self.channels) and out.is_contiguous()
                  and out.device == flags.device):
            raise ValueError("out must be a contiguous int16 CUDA tensor [n_samples, 2 * channels] on the flags' device")
        if n == 0:
            return out
        stride = int(samples.stride(0)) if self.channels > 1 else n
        check(_abi.lib.syldet_trigger_mux_device_s16(self._h, src.data_ptr(), E, L, N, lat, samples.data_ptr(), stride, out.data_ptr(), n,
                                                     self._stream_ptr(stream)))
        return out

    def triggerOnsets(self, flags, n_samples: int, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0,
                      capacity: Optional[int] = None, stream=None):
        """The rising edges of triggerTrack() (syldet_trigger_onsets_device): flags [C, n_evals] -> (indices [C, capacity] i64,
        counts [C] i64), the sample numbers in order and how many there are (the first min(count, capacity) are written, like
        detections()).  capacity defaults to the most there can be."""
        torch = _torch()
        n, L, N, lat, E, src = self._trigger_args(flags, n_samples, bufferLength, width, latency)
        cap = min(E, n // L + 1) if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError("capacity must not be negative")
        idx = torch.empty((self.channels, max(cap, 1)), dtype=torch.int64, device=flags.device)
        cnt = torch.empty((self.channels,), dtype=torch.int64, device=flags.device)
        check(_abi.lib.syldet_trigger_onsets_device(self._h, src.data_ptr(), E, L, N, lat, n, idx.data_ptr(), cap, cnt.data_ptr(),
                                                    self._stream_ptr(stream)))
        return idx, cnt

    def _trigger_host_args(self, flags, n_samples, bufferLength, width):
        n = int(n_samples)
        if n < 0:
            raise ValueError("n_samples must not be negative")
        a = np.ascontiguousarray(flags, dtype=np.uint8)
        if a.ndim != 2 or a.shape[0] != self.channels:
            raise ValueError("flags must be [channels, n_evals]")
        E = a.shape[1]
        src = a if E > 0 else np.zeros(1, np.uint8)
        return n, int(bufferLength), self.triggerWidth() if width is None else int(width), E, src

    def triggerTrackHost(self, flags: np.ndarray, n_samples: int, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0,
                         dtype=np.float32) -> np.ndarray:
        """triggerTrack() on host arrays, blocking (syldet_trigger / syldet_trigger_s16): flags [C, n_evals] -> [C, n_samples]."""
        dt = self._trace_dtype(dtype, False)
        n, L, N, E, src = self._trigger_host_args(flags, n_samples, bufferLength, width)
        tr = np.zeros((self.channels, n), dt)
        if dt == np.dtype(np.float32):
            check(_abi.lib.syldet_trigger(self._h, src.ctypes.data_as(_abi.c_uint8_p), E, L, N, int(latency), tr.ctypes.data_as(_abi.c_float_p), n, n))
        else:
            check(_abi.lib.syldet_trigger_s16(self._h, src.ctypes.data_as(_abi.c_uint8_p), E, L, N, int(latency), tr.ctypes.data_as(_abi.c_int16_p), n, n))
        return tr

    def triggerOnsetsHost(self, flags: np.ndarray, n_samples: int, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0,
                          capacity: Optional[int] = None):
        """triggerOnsets() on host arrays, blocking (syldet_trigger_onsets): -> a list of one int64 array of samples per channel."""
        n, L, N, E, src = self._trigger_host_args(flags, n_samples, bufferLength, width)
        cap = min(E, n // max(L, 1) + 1) if capacity is None else int(capacity)
        idx = np.zeros((self.channels, max(cap, 1)), np.int64)
        cnt = np.zeros((self.channels,), np.int64)
        check(_abi.lib.syldet_trigger_onsets(self._h, src.ctypes.data_as(_abi.c_uint8_p), E, L, N, int(latency), n,
                                             idx.ctypes.data_as(_abi.c_int64_p), cap, cnt.ctypes.data_as(_abi.c_int64_p)))
        return [idx[c, :min(int(cnt[c]), cap)].copy() for c in range(self.channels)]

    def triggerRehearse(self, flags, n_samples: int, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0,
                        dtype=np.int16, capacity: Optional[int] = None, out=None, stream=None):
        """triggerTrack() (planar rows) and triggerOnsets() from one scan of the flags (syldet_trigger_rehearse_device*):
        -> (track [C, n_samples], indices [C, capacity], counts [C])."""
        torch = _torch()
        dt = self._trace_dtype(dtype, False)
        tdt = torch.float32 if dt == np.dtype(np.float32) else torch.int16
        n, L, N, lat, E, src = self._trigger_args(flags, n_samples, bufferLength, width, latency)
        if out is None:
            out = torch.empty((self.channels, n), dtype=tdt, device=flags.device)
        elif not (out.is_cuda and out.dtype == tdt and out.dim() == 2 and out.shape[0] == self.channels and out.shape[1] >= n
                  and (out.shape[1] == 0 or out.stride(1) == 1) and (self.channels == 1 or out.stride(0) >= n)
                  and out.device == flags.device):
            raise ValueError("out must be a CUDA tensor [channels, >= n_samples] of the track's dtype with contiguous rows")
        cap = min(E, n // L + 1) if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError("capacity must not be negative")
        idx = torch.empty((self.channels, max(cap, 1)), dtype=torch.int64, device=flags.device)
        cnt = torch.empty((self.channels,), dtype=torch.int64, device=flags.device)
        dst = out if out.numel() > 0 else torch.zeros(1, dtype=tdt, device=flags.device)
        fn = _abi.lib.syldet_trigger_rehearse_device if dt == np.dtype(np.float32) else _abi.lib.syldet_trigger_rehearse_device_s16
        stride = int(out.stride(0)) if self.channels > 1 else max(int(out.shape[1]), n)
        check(fn(self._h, src.data_ptr(), E, L, N, lat, dst.data_ptr(), n, stride, idx.data_ptr(), cap, cnt.data_ptr(), self._stream_ptr(stream)))
        return out, idx, cnt

    def rehearse(self, samples, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0, dtype=np.int16, stream=None):
        """A recording through the rig in one call: run() followed by triggerRehearse() on device tensors (one scan of the flags
        for the track and the onsets); samples [C, S] float32 -> (track [C, S], onsets [C, capacity], counts [C], outputs
        [C, E, n_out], flags [C, E])."""
        self._trace_dtype(dtype, False)
        outputs, flags = self.run(samples, stream=stream)
        track, onsets, counts = self.triggerRehearse(flags, int(samples.shape[1]), bufferLength, width, latency, dtype=dtype, stream=stream)
        return track, onsets, counts, outputs, flags

    def armTrigger(self, channel: int = 0, width: Optional[int] = None) -> None:
        """createHighOutput (AudioInterface.swift:442-445): the channel's TTL output stays high for `width` samples (default
        triggerWidth()) of the buffers rendered from now on -- set, not added to (syldet_trigger_arm)."""
        check(_abi.lib.syldet_trigger_arm(self._h, int(channel), self.triggerWidth() if width is None else int(width)))

    def renderTrigger(self, channel: int = 0, n_frames: int = 32) -> np.ndarray:
        """renderOutput (AudioInterface.swift:13-40) for one channel: the next n_frames samples of its TTL output, float32 1.0 while
        the armed pulse lasts and 0.0 behind it (syldet_trigger_render)."""
        out = np.zeros(int(n_frames), np.float32)
        check(_abi.lib.syldet_trigger_render(self._h, int(channel), out.ctypes.data_as(_abi.c_float_p), int(n_frames)))
        return out

    # ---- the level meters (Processor.swift:111-113, :138, :158-184) ---------------------------
    def defaultBuffersPerReading(self, bufferLength: int = 32) -> int:
        """Buffers between two firings of the reference's 0.1 s timer (ViewControllerProcessor.swift:57):
        max(1, floor(0.1 * samplingRate / bufferLength))."""
        return max(1, int(0.1 * float(self.config.samplingRate) / int(bufferLength)))

    def _levels_geometry(self, n_samples, bufferLength, buffersPerReading):
        L = int(bufferLength)
        P = self.defaultBuffersPerReading(L) if buffersPerReading is None else int(buffersPerReading)
        M = int(_abi.lib.syldet_levels_count(int(n_samples), L, P))
        if M < 0:
            raise ValueError("bufferLength must be a power of two in [8, 4096] and buffersPerReading >= 1")
        return L, P, M

    def levelsCount(self, n_samples: int, bufferLength: int = 32, buffersPerReading: Optional[int] = None) -> int:
        """syldet_levels_count: readings of n_samples samples."""
        return self._levels_geometry(n_samples, bufferLength, buffersPerReading)[2]

    def levelsEvalRange(self, n_samples: int, n_evals: int, reading: int, bufferLength: int = 32,
                        buffersPerReading: Optional[int] = None) -> Tuple[int, int]:
        """syldet_levels_eval_range: (first, count) of the evaluations of reading `reading` (count 0: an empty reading)."""
        L, P, _ = self._levels_geometry(n_samples, bufferLength, buffersPerReading)
        first, count = C.c_int64(), C.c_int64()
        check(_abi.lib.syldet_levels_eval_range(self._h, int(n_samples), int(n_evals), L, P, int(reading), C.byref(first), C.byref(count)))
        return int(first.value), int(count.value)

    def _levels_device(self, fn, tensor, n, stride_or_channels, bufferLength, buffersPerReading, stream):
        torch = _torch()
        L, P, M = self._levels_geometry(n, bufferLength, buffersPerReading)
        ms = torch.empty((self.channels, M), dtype=torch.float64, device=tensor.device)
        if n > 0:
            check(fn(self._h, tensor.data_ptr(), n, stride_or_channels, L, P, ms.data_ptr(), self._stream_ptr(stream)))
        return ms

    def levels(self, samples, bufferLength: int = 32, buffersPerReading: Optional[int] = None, stream=None):
        """The input meter of every channel over a recording (syldet_levels_device): samples [C, S] float32 -> the fp64 MEAN SQUARES
        [C, M] of the readings (the RMS is their sqrt), one reading per buffersPerReading buffers of bufferLength samples: the
        greatest mean square of its buffers, NaN if its first buffer's is.  buffersPerReading None: the 0.1 s timer
        (defaultBuffersPerReading).  Asynchronous on `stream`."""
        self._check_samples(samples)
        S = int(samples.shape[1])
        return self._levels_device(_abi.lib.syldet_levels_device, samples, S, max(int(samples.stride(0)), S), bufferLength,
                                   buffersPerReading, stream)

    def levelsPCM16(self, samples, bufferLength: int = 32, buffersPerReading: Optional[int] = None, stream=None):
        """levels() for 16-bit PCM [C, S] (an int16 CUDA tensor, x meaning x / 32768; syldet_levels_device_s16): levels()'s bits
        for samples.float() * 2**-15."""
        torch = _torch()
        if not (samples.is_cuda and samples.dtype == torch.int16 and samples.dim() == 2 and samples.shape[0] == self.channels
                and samples.stride(1) == 1 and samples.device.index == self.device):
            raise ValueError("samples must be a 2-D int16 CUDA tensor [channels, n_samples] with contiguous rows on the detector's device")
        S = int(samples.shape[1])
        return self._levels_device(_abi.lib.syldet_levels_device_s16, samples, S, max(int(samples.stride(0)), S), bufferLength,
                                   buffersPerReading, stream)

    def levelsInterleaved(self, frames, bufferLength: int = 32, buffersPerReading: Optional[int] = None, stream=None):
        """levels() on frames [n, C] float32 (syldet_levels_interleaved_device)."""
        torch = _torch()
        if not (frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 2 and frames.is_contiguous()
                and frames.shape[1] == self.channels and frames.device.index == self.device):
            raise ValueError("frames must be a contiguous 2-D float32 CUDA tensor [n_frames, channels] on the detector's device")
        return self._levels_device(_abi.lib.syldet_levels_interleaved_device, frames, int(frames.shape[0]), self.channels, bufferLength,
                                   buffersPerReading, stream)

    def levelsInterleavedPCM16(self, frames, bufferLength: int = 32, buffersPerReading: Optional[int] = None, stream=None):
        """levels() on 16-bit PCM frames [n, C] int16 (syldet_levels_interleaved_device_s16)."""
        torch = _torch()
        if not (frames.is_cuda and frames.dtype == torch.int16 and frames.dim() == 2 and frames.is_contiguous()
                and frames.shape[1] == self.channels and frames.device.index == self.device):
            raise ValueError("frames must be a contiguous 2-D int16 CUDA tensor [n_frames, channels] on the detector's device")
        return self._levels_device(_abi.lib.syldet_levels_interleaved_device_s16, frames, int(frames.shape[0]), self.channels,
                                   bufferLength, buffersPerReading, stream)

    def _levels_host(self, fn, a, ptr_type, bufferLength, buffersPerReading):
        S = a.shape[1]
        L, P, M = self._levels_geometry(S, bufferLength, buffersPerReading)
        rms = np.zeros((self.channels, M), np.float64)
        if S > 0:
            check(fn(self._h, a.ctypes.data_as(ptr_type), S, S, L, P, rms.ctypes.data_as(_abi.c_double_p)))
        return rms

    def levelsHost(self, samples: np.ndarray, bufferLength: int = 32, buffersPerReading: Optional[int] = None) -> np.ndarray:
        """syldet_levels: host samples [C, S] -> the RMS readings [C, M] (getInputForChannel's values), blocking."""
        a = np.ascontiguousarray(samples, dtype=np.float32)
        a = a.reshape(self.channels, a.size // self.channels)
        return self._levels_host(_abi.lib.syldet_levels, a, _abi.c_float_p, bufferLength, buffersPerReading)

    def levelsPCM16Host(self, samples: np.ndarray, bufferLength: int = 32, buffersPerReading: Optional[int] = None) -> np.ndarray:
        """syldet_levels_s16: levelsHost for an int16 array [C, S] (x meaning x / 32768)."""
        a = np.ascontiguousarray(_pcm16(samples))
        a = a.reshape(self.channels, a.size // self.channels)
        return self._levels_host(_abi.lib.syldet_levels_s16, a, _abi.c_int16_p, bufferLength, buffersPerReading)

    def outputLevels(self, outputs, n_samples: int, output: int = 0, bufferLength: int = 32, buffersPerReading: Optional[int] = None,
                     stream=None):
        """The output meter (syldet_output_levels_device): outputs [C, n_evals, n_out] (as run() returns them, for a recording of
        n_samples samples) -> float32 [C, M], the greatest value of output `output` among the evaluations each reading's buffers
        make available (NaN if the first of them is); 0 for a reading without an evaluation (levelsEvalRange tells which)."""
        torch = _torch()
        if not (outputs.is_cuda and outputs.dtype == torch.float32 and outputs.dim() == 3 and outputs.is_contiguous()
                and outputs.shape[0] == self.channels and outputs.shape[2] == self.geometry.outputs
                and outputs.device.index == self.device):
            raise ValueError("outputs must be a contiguous float32 CUDA tensor [channels, n_evals, outputs] on the detector's device")
        n, E = int(n_samples), int(outputs.shape[1])
        L, P, M = self._levels_geometry(n, bufferLength, buffersPerReading)
        lv = torch.empty((self.channels, M), dtype=torch.float32, device=outputs.device)
        if n > 0:
            # (an empty tensor has no address)
            src = outputs if E > 0 else torch.zeros(1, dtype=torch.float32, device=outputs.device)
            check(_abi.lib.syldet_output_levels_device(self._h, src.data_ptr(), E, int(output), n, L, P, lv.data_ptr(),
                                                       self._stream_ptr(stream)))
        return lv

    def outputLevelsHost(self, outputs: np.ndarray, n_samples: int, output: int = 0, bufferLength: int = 32,
                         buffersPerReading: Optional[int] = None) -> np.ndarray:
        """outputLevels() on host arrays, blocking (syldet_output_levels)."""
        a = np.ascontiguousarray(outputs, dtype=np.float32)
        if a.ndim != 3 or a.shape[0] != self.channels or a.shape[2] != self.geometry.outputs:
            raise ValueError("outputs must be [channels, n_evals, outputs]")
        n, E = int(n_samples), a.shape[1]
        L, P, M = self._levels_geometry(n, bufferLength, buffersPerReading)
        lv = np.zeros((self.channels, M), np.float32)
        if n > 0:
            src = a if E > 0 else np.zeros(1, np.float32)
            check(_abi.lib.syldet_output_levels(self._h, src.ctypes.data_as(_abi.c_float_p), E, int(output), n, L, P,
                                                lv.ctypes.data_as(_abi.c_float_p)))
        return lv

    def monitor(self, samples, bufferLength: int = 32, buffersPerReading: Optional[int] = None, stream=None):
        """run() and both meters on device tensors: samples [C, S] float32 -> (outputs, flags, mean squares [C, M] float64, output
        levels [C, M] float32) -- what a ProcessorBase row shows beside its detections."""
        outputs, flags = self.run(samples, stream=stream)
        ms = self.levels(samples, bufferLength, buffersPerReading, stream=stream)
        lv = self.outputLevels(outputs, int(samples.shape[1]), 0, bufferLength, buffersPerReading, stream=stream)
        return outputs, flags, ms, lv

    def enableMeters(self, enable: bool = True) -> None:
        """syldet_meters_enable: the streaming meters (off by default); enabling or disabling clears them."""
        check(_abi.lib.syldet_meters_enable(self._h, 1 if enable else 0))

    def inputLevel(self, channel: int = 0) -> Optional[float]:
        """getInputForChannel (Processor.swift:158-172): the RMS of the loudest buffer appended since the last call, read and
        reset; None if nothing was appended (or the meters are off)."""
        v, has = C.c_double(), C.c_int32()
        check(_abi.lib.syldet_input_level(self._h, int(channel), C.byref(v), C.byref(has)))
        return float(v.value) if has.value else None

    def outputLevel(self, channel: int = 0) -> Optional[float]:
        """getOutputForChannel (Processor.swift:174-184): the greatest output 0 evaluated since the last call, read and reset."""
        v, has = C.c_double(), C.c_int32()
        check(_abi.lib.syldet_output_level(self._h, int(channel), C.byref(v), C.byref(has)))
        return float(v.value) if has.value else None

    # ---- measurement ------------------------------------------------------------------
    def profile(self, enable: bool = True, history: int = 1) -> None:
        """Bracket every kernel of a batch call with HIP events; `history`: how many calls' events to keep (a timing loop
        that reads them at its end need not wait for every call before making the next)."""
        check(_abi.lib.syldet_profile_history(self._h, int(history)))
        check(_abi.lib.syldet_profile(self._h, 1 if enable else 0))

    def timingsOf(self, calls_back: int = 0):
        """[(kernel name, milliseconds)] of the batch call made `calls_back` calls before the last one."""
        ms = (C.c_double * 8)()
        names = (C.c_char_p * 8)()
        n = C.c_int32()
        check(_abi.lib.syldet_timings(self._h, int(calls_back), ms, names, 8, C.byref(n)))
        return [(names[i].decode(), float(ms[i])) for i in range(min(n.value, 8))]

    def lastTimings(self):
        """[(kernel name, milliseconds)] of the last batch call (HIP events on its stream)."""
        ms = (C.c_double * 8)()
        names = (C.c_char_p * 8)()
        n = C.c_int32()
        check(_abi.lib.syldet_last_timings(self._h, ms, names, 8, C.byref(n)))
        return [(names[i].decode(), float(ms[i])) for i in range(min(n.value, 8))]

    def fixupStats(self):
        """(work items of 16 evaluations the last batch call recomputed exactly, overflow flag): the fused kernels' precision
        guard at work (0 for ordinary audio).  Synchronise the call's stream first."""
        items, over = C.c_int64(), C.c_int32()
        check(_abi.lib.syldet_fixup_stats(self._h, C.byref(items), C.byref(over)))
        return int(items.value), int(over.value)

    def segmentEvaluations(self, n_samples: int) -> int:
        """Evaluations per workgroup segment of the fused kernels for a batch of this length (0: no seams)."""
        return int(_abi.lib.syldet_segment_evals(self._h, int(n_samples)))

    def lastFusedForm(self):
        """syldet_last_fused_form: (kernel, template arguments) of the fused kernel instantiation this thread's last batch or
        spectrogram call through the detector ran -- kernel 0 the 8-wave kernel, 1 the register-resident-basis kernel, 2 the
        symmetric-fold kernel; raises SyllableDetectorError (unsupported) if that call ran no fused kernel."""
        kernel, params = C.c_int32(), (C.c_int32 * 10)()
        check(_abi.lib.syldet_last_fused_form(self._h, C.byref(kernel), params))
        return int(kernel.value), tuple(int(v) for v in params)

    # ---- packed recordings: many recordings of different lengths through this bank ---------
    def planRecordings(self, lengths, networks=None):
        """syldet_recordings_plan, host only: (slots, rowSamples, rowEvaluations, fill) for recordings of these lengths (and, on a
        multi / mixed bank, these networks) -- slots as a list of (row, offset, first_eval, n_evals, n_samples)."""
        n, net = _recording_args(lengths, networks)
        slots = (_abi.Slot * max(1, n.size))()
        rs, re_, fill = C.c_int64(), C.c_int64(), C.c_double()
        check(_abi.lib.syldet_recordings_plan(self._h, n.ctypes.data_as(_abi.c_int64_p), None if net is None else net.ctypes.data_as(_abi.c_int32_p),
                                              n.size, slots, C.byref(rs), C.byref(re_), C.byref(fill)))
        return [_slot_tuple(slots[k]) for k in range(n.size)], rs.value, re_.value, fill.value

    def recordings(self, lengths, networks=None) -> "Recordings":
        """The plan with its tables on the device (syldet_recordings_create): lay recordings of these lengths end to end in the
        bank's rows with load(), run the rows through run() / runPCM16(), take each recording's results out with view() and
        events()."""
        return Recordings(self, lengths, networks)

    def runRecordings(self, arrays, debounce: float = 0.0, networks=None, rates=None, resample=None, zeroCrossings=None, beta=None,
                      rolloff=None, tracks=None, output: int = 0, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0,
                      levels=None):
        """Recordings of any lengths in one pass: one upload, load, run / runPCM16, events and one download.  `arrays`: 1-D
        (mono) or [frames, tracks] numpy arrays, all float32 or all int16 (16-bit PCM: int16 rows) -- or, each in its own sample
        format, any of uint8 (offset binary), int16, int32, float32, float64 and PCM24 (packed 24-bit): such a list is uploaded as
        its own bytes and decoded as the rows load (Recordings.loadPCM, with rates Recordings.loadSincPCM; fp32 rows), with the
        results of the same recordings given as float32; every track is a recording, in order
        (`networks`, on a multi / mixed bank: one entry a track).  Returns, per recording, (indices int64 [n], values float32
        [n, outputs]): its debounced detections and the outputs of their evaluations.
        `rates`: the sampling rate of every array (None: all at the network's, and nothing else changes).  With rates,
        resample="sinc" is required: the plan is made from recordingLengths of the arrays' lengths, the rows are loaded through
        Recordings.loadSinc (band-limited conversion as they load; an array at the network's rate is copied) and run as fp32 --
        per recording what convertRate(method="sinc"), run and detections give on it alone.  zeroCrossings, beta, rolloff: the
        converter's quality (None: sincDefaults()).
        `tracks`: None, or names out of ("trace", "ttl"): the per-sample tracks of the same run (Recordings.trace of `output`,
        Recordings.triggerTrack with bufferLength, width, latency), as 16-bit PCM at the network's rate.  The call then returns
        (events, tracks): events what it returns without, tracks a dict of a list per name, one int16 array a recording in the
        caller's order.
        `levels`: None, or (bufferLength, buffersPerReading) of the level meters (buffersPerReading None: the 0.1 s timer): the
        two tables of the same run, from the very rows that were run (Recordings.levels, Recordings.outputLevels of `output`).
        The call then returns one element more, behind the events (and the tracks, if any): a dict with "input", a list of one
        float64 array of MEAN SQUARES a recording, and "output", one float32 array a recording."""
        torch = _torch()
        names = () if tracks is None else tuple(tracks)
        if any(t not in ("trace", "ttl") for t in names):
            raise ValueError("tracks are 'trace' and 'ttl'")
        if rates is None and (resample is not None or zeroCrossings is not None or beta is not None or rolloff is not None):
            raise ValueError("resample, zeroCrossings, beta and rolloff belong to rates")
        if rates is not None and resample != "sinc":
            raise ValueError("recordings at rates of their own need resample='sinc' (there is no linear-interpolation load)")
        arrays = [a if isinstance(a, PCM24) else np.asarray(a) for a in arrays]
        dtypes = {None if isinstance(a, PCM24) else a.dtype for a in arrays}
        # one dtype, float32 or int16: arrays of elements, as ever; anything else: every array's own bytes, each in its format
        pcm = bool(arrays) and dtypes not in ({np.dtype(np.float32)}, {np.dtype(np.int16)})
        if pcm and not all(d is None or d in _PCM_OF_DTYPE for d in dtypes):
            raise ValueError("arrays are uint8, int16, int32, float32 or float64 numpy arrays, or PCM24")
        s16 = bool(arrays) and not pcm and arrays[0].dtype == np.int16
        if rates is not None and len(rates) != len(arrays):
            raise ValueError("one rate per array")
        lengths, offsets, steps, formats, track_rates, pos = [], [], [], [], [], 0
        # (in elements, or for arrays in their own formats in bytes: every file from a whole 16 bytes either way)
        unit = 16 if pcm else 8
        for i, a in enumerate(arrays):
            if isinstance(a, PCM24):
                n_frames, n_tracks, fmt, size, n_units = a.frames, a.tracks, _abi.PCM_S24, 3, a.bytes.size
            else:
                if a.ndim not in (1, 2):
                    raise ValueError("each array is 1-D (mono) or [frames, tracks]")
                n_frames, n_tracks = a.shape[0], 1 if a.ndim == 1 else a.shape[1]
                fmt = _PCM_OF_DTYPE[a.dtype] if pcm else 0
                size = a.dtype.itemsize if pcm else 1
                n_units = a.size * size
            for t in range(n_tracks):
                lengths.append(n_frames)
                offsets.append(pos + t * size)
                steps.append(n_tracks * size)
                formats.append(fmt)
                if rates is not None:
                    track_rates.append(float(rates[i]))
            pos += (n_units + unit - 1) // unit * unit
        flat = np.zeros(max(pos, unit), np.uint8 if pcm else np.int16 if s16 else np.float32)
        pos = 0
        for a in arrays:
            if pcm:
                raw = a.bytes.reshape(-1) if isinstance(a, PCM24) else np.ascontiguousarray(a).astype(a.dtype.newbyteorder("<"), copy=False).reshape(-1).view(np.uint8)
            else:
                raw = np.ascontiguousarray(a).reshape(-1)
            flat[pos:pos + raw.size] = raw
            pos += (raw.size + unit - 1) // unit * unit
        n_out = self.geometry.outputs
        planned = lengths if rates is None else recordingLengths(lengths, track_rates, self.config.samplingRate)
        with self.recordings(planned, networks) as rec:
            ran = rec.rowEvaluations > 0
            if not ran:
                events = [(np.zeros(0, np.int64), np.zeros((0, n_out), np.float32)) for _ in lengths]
                made = {t: [np.zeros(n, np.int16) for n in planned] for t in names}
            tables = None
            if ran or (levels is not None and rec.rowSamples > 0):
                if pcm and rates is None:
                    rows = rec.loadPCM(torch.from_numpy(flat).to("cuda:%d" % self.device), offsets, steps, formats)
                elif pcm:
                    rows = rec.loadSincPCM(torch.from_numpy(flat).to("cuda:%d" % self.device), offsets, steps, formats, lengths, track_rates,
                                           zeroCrossings, beta, rolloff)
                elif rates is None:
                    rows = rec.load(torch.from_numpy(flat).to("cuda:%d" % self.device), offsets, steps)
                else:
                    rows = rec.loadSinc(torch.from_numpy(flat).to("cuda:%d" % self.device), offsets, lengths, track_rates, steps, zeroCrossings,
                                        beta, rolloff)
                if ran:
                    out, fl = (self.runPCM16 if rows.dtype == torch.int16 else self.run)(rows)
                    idx, val, cnt = rec.events(out, fl, debounce)
                    made = {}
                    for t in names:
                        made[t] = rec.trace(out, output) if t == "trace" else rec.triggerTrack(fl, bufferLength, width, latency)
                else:
                    out = torch.zeros((self.channels, 0, n_out), dtype=torch.float32, device=rows.device)
                if levels is not None:
                    tables = (rec.levels(rows, levels[0], levels[1]), rec.outputLevels(out, output, levels[0], levels[1]))
                torch.cuda.current_stream(self.device).synchronize()
                if ran:
                    idx, val, cnt = idx.cpu().numpy(), val.cpu().numpy(), cnt.cpu().numpy()
                    made = {t: [rec.trackView(v, k).copy() for k in range(rec.count)] for t, v in ((t, v.cpu().numpy()) for t, v in made.items())}
                    events = [(idx[k, :cnt[k]].copy(), val[k, :cnt[k]].copy()) for k in range(len(lengths))]
            if levels is not None:
                if tables is None:                            # (no recording has a sample)
                    tables = (np.zeros(0, np.float64), np.zeros(0, np.float32))
                else:
                    tables = tuple(t.cpu().numpy() for t in tables)
                first = rec.levelsLayout(levels[0], levels[1])
                tables = {name: [t[first[k]:first[k + 1]].copy() for k in range(rec.count)] for name, t in zip(("input", "output"), tables)}
        result = (events,) + (() if tracks is None else (made,)) + (() if levels is None else (tables,))
        return result[0] if len(result) == 1 else result

    # ---- threshold calibration: score a run against labelled times -------------------------
    def scorer(self, thresholds, labels, tolerance: int, debounce: float = 0.0) -> "Scorer":
        """A Scorer over this bank's channels (syldet_scorer_create): labels[c] are channel c's labelled sample numbers, a
        detection within `tolerance` samples of one is a hit; score(outputs) then gives, for every channel and every candidate
        threshold, detections, hits, false positives, repeats and the hits' offset sums, in one launch."""
        return Scorer(self, thresholds, labels, tolerance, debounce)

    # ---- event-aligned windows: spectrogram, output and audio at each event -----------------
    def aligner(self, source="columns", before: Optional[int] = None, after: Optional[int] = None) -> "Aligner":
        """An Aligner over this bank's channels (syldet_aligner_create): windows(array, events) cuts, out of the columns
        spectrogram() made, the outputs run() made or the sample rows -- `source`: "columns", "outputs", "samples" or
        ALIGN_* -- the units `before` in front of to `after` behind every event's anchor unit, one window an event, in one
        launch.  before, after: in units of the source, default timeRange - 1 each."""
        return Aligner(self, source, before, after)

    # ---- training: loss and gradient of the network over labelled evaluations --------------
    def trainer(self) -> "Trainer":
        """A Trainer over this bank's channels (syldet_trainer_create): targets and class weights from labels, and loss and
        gradient of the two layers' parameters straight from the columns spectrogram() made.  A plain bank of a two-layer
        network, up to 16 hidden units and 4 outputs."""
        return Trainer(self)

    def multiTrainer(self) -> "MultiTrainer":
        """A MultiTrainer over this bank's channels (syldet_trainer_create_multi): one trainer for the N networks of a multi bank
        (or of a plain bank, N = 1), each trained on its own rows with the bits a plain Trainer would give."""
        return MultiTrainer(self)

    # ---- template matching: a syllable's occurrences in the columns ------------------------
    def matcher(self, template, anchor: Optional[int] = None) -> "Matcher":
        """A Matcher over this bank's channels (syldet_matcher_create): scores(cols) is the cosine between `template`
        [n, bins] and the window of n frames at every position of spectrogram()'s columns, peaks() the matches among them as
        the event tables detections() makes, find() both.  anchor: the template's frame a match's sample number names
        (default: its last, n - 1)."""
        return Matcher(self, template, anchor)

    def matcherBank(self, templates, classes=None, anchor=None, ragged: Optional[bool] = None) -> "MatcherBank":
        """A MatcherBank over this bank's channels (syldet_matcher_bank_create): `templates` [K, n, bins] in classes (`classes`
        [K], None: template k is class k) matched in one pass; a class's score is the greatest of its templates' scores.  A list
        of arrays [n_k, bins] of differing lengths makes a ragged bank (syldet_matcher_bank_create_ragged), whose planes are indexed
        by the anchor frame; anchor: None (each template's last frame), one frame for all, or one per template."""
        return MatcherBank(self, templates, classes, anchor, ragged=ragged)

    # ---- batch, host arrays -------------------------------------------------------
    def runHost(self, samples: np.ndarray, outputs: Optional[np.ndarray] = None, flags: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """syldet_run: the batch call on host arrays, pipelined along time inside the library.  `outputs` / `flags`: arrays to
        write into (e.g. bank.PinnedArray views, which the DMA engines write in place).  Any array is cast to float32 as it is:
        an np.int16 recording becomes integer-valued samples, not x / 32768 -- 16-bit PCM goes to runPCM16Host."""
        a = np.ascontiguousarray(samples, dtype=np.float32).reshape(self.channels, -1)
        return self._run_host(_abi.lib.syldet_run, a, _abi.c_float_p, outputs, flags)

    def runPCM16Host(self, samples: np.ndarray, outputs: Optional[np.ndarray] = None, flags: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """syldet_run_s16: runHost for 16-bit PCM, an int16 array [C, S] whose sample x means x / 32768 -- runHost's bits for
        samples * 2**-15, with half the bytes crossing the bus (a bank.PinnedArray of int16 is copied in place)."""
        a = np.ascontiguousarray(_pcm16(samples)).reshape(self.channels, -1)
        return self._run_host(_abi.lib.syldet_run_s16, a, _abi.c_int16_p, outputs, flags)

    def _run_host(self, fn, a, ptr_type, outputs, flags):
        S = a.shape[1]
        E = max(self.countEvaluations(S), 0)
        out = outputs if outputs is not None else np.zeros((self.channels, E, self.geometry.outputs), np.float32)
        fl = flags if flags is not None else np.zeros((self.channels, E), np.uint8)
        if out.shape != (self.channels, E, self.geometry.outputs) or out.dtype != np.float32 or not out.flags.c_contiguous:
            raise ValueError("outputs must be a C-contiguous float32 array [channels, E, outputs]")
        if fl.shape != (self.channels, E) or fl.dtype != np.uint8 or not fl.flags.c_contiguous:
            raise ValueError("flags must be a C-contiguous uint8 array [channels, E]")
        check(fn(self._h, a.ctypes.data_as(ptr_type), S, S, out.ctypes.data_as(_abi.c_float_p), fl.ctypes.data_as(_abi.c_uint8_p)))
        return out, fl

    def spectrogramHost(self, samples: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(samples, dtype=np.float32).reshape(self.channels, -1)
        S = a.shape[1]
        J = self.countFrames(S)
        cols = np.zeros((self.channels, J, max(self.geometry.bins, 0)), np.float32)
        check(_abi.lib.syldet_spectrogram(self._h, a.ctypes.data_as(_abi.c_float_p), S, S,
                                          cols.ctypes.data_as(_abi.c_float_p)))
        return cols

    def detectionsHost(self, flags: np.ndarray, debounce: float = 0.0, capacity: Optional[int] = None):
        f = np.ascontiguousarray(flags, dtype=np.uint8).reshape(self.channels, -1)
        E = f.shape[1]
        cap = E if capacity is None else int(capacity)
        idx = np.zeros((self.channels, max(cap, 1)), np.int64)
        cnt = np.zeros((self.channels,), np.int64)
        check(_abi.lib.syldet_detections(self._h, f.ctypes.data_as(_abi.c_uint8_p), E, float(debounce),
                                         idx.ctypes.data_as(_abi.c_int64_p), cap, cnt.ctypes.data_as(_abi.c_int64_p)))
        return idx, cnt


def _recording_args(lengths, networks):
    n = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
    net = None if networks is None else np.ascontiguousarray(networks, dtype=np.int32).reshape(-1)
    if net is not None and net.size != n.size:
        raise ValueError("one network per recording")
    return n, net


def recordingLengths(sourceSamples, sourceRates, rate: float):
    """syldet_convert_rate_count per entry, host only: the lengths at the network's `rate` of recordings of sourceSamples[k]
    samples at sourceRates[k] -- what a plan for Recordings.loadSinc is made from."""
    n = np.ascontiguousarray(sourceSamples, dtype=np.int64).reshape(-1)
    r = np.ascontiguousarray(sourceRates, dtype=np.float64).reshape(-1)
    if n.size != r.size:
        raise ValueError("one rate per recording")
    return [int(_abi.lib.syldet_convert_rate_count(int(a), float(b), float(rate))) for a, b in zip(n, r)]


# ---- the files' own sample formats (syldet_pcm_*: include/syldet.h, "packed recordings: the files' own sample formats") ----
_PCM_OF_DTYPE = {np.dtype(np.uint8): _abi.PCM_U8, np.dtype(np.int16): _abi.PCM_S16, np.dtype(np.int32): _abi.PCM_S32,
                 np.dtype(np.float32): _abi.PCM_F32, np.dtype(np.float64): _abi.PCM_F64}


class PCM24:
    """Packed 24-bit PCM as a WAV stores it, for runRecordings: a uint8 array [frames, tracks, 3] (or [frames, 3], mono), little
    endian, sample = the three bytes sign-extended, meaning v * 2**-23."""

    def __init__(self, array):
        a = np.ascontiguousarray(array)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.shape[-1] != 3:
            raise ValueError("PCM24 takes a uint8 array [frames, tracks, 3] or [frames, 3]")
        self.bytes = a
        self.frames = int(a.shape[0])
        self.tracks = 1 if a.ndim == 2 else int(a.shape[1])


def pcmSampleBytes(format: int) -> int:
    """syldet_pcm_sample_bytes: the bytes of one sample of a PCM_* format (0: no such format)."""
    return int(_abi.lib.syldet_pcm_sample_bytes(int(format)))


def pcmDecode(data, format: int, n: Optional[int] = None, byteStep: Optional[int] = None) -> np.ndarray:
    """syldet_pcm_decode, host only: the n float32 values of the `format` samples at data[i * byteStep] (data: bytes or a uint8
    array; byteStep None: contiguous samples; n None: as many as data holds) -- the values every load of the files' own bytes
    writes, and the tool's WAV reader gives."""
    raw = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data)
    if raw.dtype != np.uint8:
        raise ValueError("data must be bytes or a uint8 array")
    raw = raw.reshape(-1)
    size = pcmSampleBytes(format)
    step = size if byteStep is None else int(byteStep)
    if n is None:
        n = 0 if size == 0 or step < size or raw.size < size else (raw.size - size) // step + 1
    n = int(n)
    if size and step >= size and n > 0 and (n - 1) * step + size > raw.size:
        raise ValueError("the samples reach beyond data")
    out = np.empty(max(n, 0), np.float32)
    check(_abi.lib.syldet_pcm_decode(int(format), raw.ctypes.data, n, step, out.ctypes.data_as(_abi.c_float_p)))
    return out


def _slot_tuple(s):
    return (int(s.row), int(s.offset), int(s.first_eval), int(s.n_evals), int(s.n_samples))


def planRecordings(config: SyllableDetectorConfig, channels: int, lengths, channelNetworks=None, networks=None):
    """syldet_recordings_plan_of_config: the plan a bank of `channels` channels on config's evaluation clock makes for recordings
    of these lengths -- from the host alone, no device needed.  channelNetworks: the bank's network per channel (multi / mixed
    banks; None: a plain bank), networks: the network of each recording.  (slots, rowSamples, rowEvaluations, fill) as
    SyllableDetector.planRecordings."""
    n, net = _recording_args(lengths, networks)
    cn = None if channelNetworks is None else np.ascontiguousarray(channelNetworks, dtype=np.int32).reshape(-1)
    if cn is not None and cn.size != int(channels):
        raise ValueError("one network per channel")
    c, keep = config.to_abi()
    slots = (_abi.Slot * max(1, n.size))()
    rs, re_, fill = C.c_int64(), C.c_int64(), C.c_double()
    check(_abi.lib.syldet_recordings_plan_of_config(C.byref(c), int(channels), None if cn is None else cn.ctypes.data_as(_abi.c_int32_p),
                                                    n.ctypes.data_as(_abi.c_int64_p), None if net is None else net.ctypes.data_as(_abi.c_int32_p),
                                                    n.size, slots, C.byref(rs), C.byref(re_), C.byref(fill)))
    del keep
    return [_slot_tuple(slots[k]) for k in range(n.size)], rs.value, re_.value, fill.value


class Recordings:
    """Recordings of different lengths laid end to end in the rows of one bank (syldet_recordings_*; the reference's tool runs
    them one file after another, SyllableDetectorCLI/main.swift:63-130).  slots[k] = (row, offset, first_eval, n_evals,
    n_samples) of recording k; rows are rowSamples long and yield rowEvaluations evaluations; fill is the share of the rows'
    samples that are audio.  The detector must outlive it."""

    def __init__(self, detector: SyllableDetector, lengths, networks=None):
        self.detector = detector
        n, net = _recording_args(lengths, networks)
        self._h = _abi.Handle()
        check(_abi.lib.syldet_recordings_create(detector._h, n.ctypes.data_as(_abi.c_int64_p),
                                                None if net is None else net.ctypes.data_as(_abi.c_int32_p), n.size, C.byref(self._h)))
        self.count = int(n.size)
        slots = (_abi.Slot * max(1, self.count))()
        check(_abi.lib.syldet_recordings_slots(self._h, slots))
        self.slots = [_slot_tuple(slots[k]) for k in range(self.count)]
        rs, re_, fill = C.c_int64(), C.c_int64(), C.c_double()
        check(_abi.lib.syldet_recordings_shape(self._h, None, C.byref(rs), C.byref(re_), C.byref(fill)))
        self.rowSamples, self.rowEvaluations, self.fill = rs.value, re_.value, fill.value

    def close(self):
        if getattr(self, "_h", None):
            _abi.lib.syldet_recordings_destroy(self._h)
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

    def load(self, src, offsets, steps=None, out=None, stream=None):
        """The rows [C, rowSamples] from `src`, a 1-D float32 or int16 CUDA tensor: sample i of recording k is
        src[offsets[k] + i * steps[k]] (steps None: all 1; step n takes one track of an n-track file as its WAV stores it);
        everything else in the rows is +0.  `out`: rows to write into, [C, >= rowSamples] of src's dtype (what lies beyond
        rowSamples is left alone).  Asynchronous on `stream`; the same offsets and steps again make it one launch."""
        torch = _torch()
        det = self.detector
        if not (src.is_cuda and src.dim() == 1 and src.is_contiguous() and src.dtype in (torch.float32, torch.int16)
                and src.device.index == det.device):
            raise ValueError("src must be a contiguous 1-D float32 or int16 CUDA tensor on the detector's device")
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        stp = np.ones(self.count, np.int32) if steps is None else np.ascontiguousarray(steps, dtype=np.int32).reshape(-1)
        if off.size != self.count or stp.size != self.count:
            raise ValueError("one offset (and step) per recording")
        n = np.array([s[4] for s in self.slots], np.int64)
        if self.count and (off.min() < 0 or stp.min() < 1 or int((off + np.maximum(n - 1, 0) * stp)[n > 0].max(initial=-1)) >= src.numel()):
            raise ValueError("a recording reaches outside src")
        if out is None:
            out = torch.empty((det.channels, self.rowSamples), dtype=src.dtype, device=src.device)
        elif not (out.is_cuda and out.dtype == src.dtype and out.dim() == 2 and out.shape[0] == det.channels and out.shape[1] >= self.rowSamples
                  and out.stride(1) == 1 and out.device == src.device):
            raise ValueError("out must be [channels, >= rowSamples] of src's dtype on its device, rows contiguous")
        fn = _abi.lib.syldet_recordings_load_device_s16 if src.dtype == torch.int16 else _abi.lib.syldet_recordings_load_device
        stride = int(out.stride(0)) if det.channels > 1 else int(out.shape[1])
        check(fn(self._h, src.data_ptr(), off.ctypes.data_as(_abi.c_int64_p), stp.ctypes.data_as(_abi.c_int32_p), out.data_ptr(), stride,
                 det._stream_ptr(stream)))
        return out

    def loadSinc(self, src, offsets, sourceSamples, sourceRates, steps=None, zeroCrossings=None, beta=None, rolloff=None, out=None, stream=None):
        """load() for recordings that are each at a rate of their own (syldet_recordings_load_sinc_device*): recording k has
        sourceSamples[k] samples at sourceRates[k], sample j at src[offsets[k] + j * steps[k]], and this Recordings was planned
        from recordingLengths(sourceSamples, sourceRates, the network's rate).  Returns float32 rows [C, rowSamples] whatever
        src's dtype (int16: x / 32768): every recording at another rate converted band-limited in place, with the bits
        convertRate(method="sinc") gives on it alone; one at the network's rate copied; +0 everywhere else.  One launch.
        zeroCrossings, beta, rolloff: None for sincDefaults().  `out`: float32 rows [C, >= rowSamples] to write into."""
        torch = _torch()
        from .resampler import _sinc_quality
        det = self.detector
        if not (src.is_cuda and src.dim() == 1 and src.is_contiguous() and src.dtype in (torch.float32, torch.int16)
                and src.device.index == det.device):
            raise ValueError("src must be a contiguous 1-D float32 or int16 CUDA tensor on the detector's device")
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        stp = np.ones(self.count, np.int32) if steps is None else np.ascontiguousarray(steps, dtype=np.int32).reshape(-1)
        n = np.ascontiguousarray(sourceSamples, dtype=np.int64).reshape(-1)
        rates = np.ascontiguousarray(sourceRates, dtype=np.float64).reshape(-1)
        if off.size != self.count or stp.size != self.count or n.size != self.count or rates.size != self.count:
            raise ValueError("one offset, length and rate (and step) per recording")
        if self.count and (off.min() < 0 or stp.min() < 1 or n.min() < 0 or
                           int((off + np.maximum(n - 1, 0) * stp)[n > 0].max(initial=-1)) >= src.numel()):
            raise ValueError("a recording reaches outside src")
        if out is None:
            out = torch.empty((det.channels, self.rowSamples), dtype=torch.float32, device=src.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == det.channels and out.shape[1] >= self.rowSamples
                  and out.stride(1) == 1 and out.device == src.device):
            raise ValueError("out must be float32 [channels, >= rowSamples] on src's device, rows contiguous")
        z, b, r = _sinc_quality(zeroCrossings, beta, rolloff)
        fn = _abi.lib.syldet_recordings_load_sinc_device_s16 if src.dtype == torch.int16 else _abi.lib.syldet_recordings_load_sinc_device
        stride = int(out.stride(0)) if det.channels > 1 else int(out.shape[1])
        check(fn(self._h, src.data_ptr(), off.ctypes.data_as(_abi.c_int64_p), stp.ctypes.data_as(_abi.c_int32_p), n.ctypes.data_as(_abi.c_int64_p),
                 rates.ctypes.data_as(_abi.c_double_p), z, b, r, out.data_ptr(), stride, det._stream_ptr(stream)))
        return out

    def _pcm_args(self, src, byteOffsets, byteSteps, formats, out):
        torch = _torch()
        det = self.detector
        if not (src.is_cuda and src.dim() == 1 and src.is_contiguous() and src.dtype == torch.uint8 and src.device.index == det.device):
            raise ValueError("src must be a contiguous 1-D uint8 CUDA tensor on the detector's device")
        off = np.ascontiguousarray(byteOffsets, dtype=np.int64).reshape(-1)
        fmt = np.ascontiguousarray(formats, dtype=np.int32).reshape(-1)
        if fmt.size != self.count or off.size != self.count:
            raise ValueError("one byte offset and format (and byte step) per recording")
        stp = (np.array([pcmSampleBytes(f) for f in fmt], np.int32) if byteSteps is None
               else np.ascontiguousarray(byteSteps, dtype=np.int32).reshape(-1))
        if stp.size != self.count:
            raise ValueError("one byte offset and format (and byte step) per recording")
        if out is None:
            out = torch.empty((det.channels, self.rowSamples), dtype=torch.float32, device=src.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == det.channels and out.shape[1] >= self.rowSamples
                  and out.stride(1) == 1 and out.device == src.device):
            raise ValueError("out must be float32 [channels, >= rowSamples] on src's device, rows contiguous")
        stride = int(out.stride(0)) if det.channels > 1 else int(out.shape[1])
        return off, stp, fmt, out, stride

    def loadPCM(self, src, byteOffsets, byteSteps, formats, out=None, stream=None):
        """load() from the files' own bytes (syldet_recordings_load_pcm_device): `src` a 1-D uint8 CUDA tensor, sample i of recording
        k the formats[k] value (PCM_U8 ... PCM_F64) at byte byteOffsets[k] + i * byteSteps[k] (byteSteps None: contiguous
        recordings; a step of tracks * sample bytes takes one track of an interleaved file).  Returns float32 rows [C, rowSamples]
        with the bits load() gives on pcmDecode's float32 of the same bytes; what the library refuses (an unknown format, a step
        below a sample, a misaligned S16 / S32 / F32 / F64 address, samples beyond src) raises SyllableDetectorError before the
        rows are touched.  One launch; the same layout again makes it a launch only."""
        off, stp, fmt, out, stride = self._pcm_args(src, byteOffsets, byteSteps, formats, out)
        check(_abi.lib.syldet_recordings_load_pcm_device(self._h, src.data_ptr(), int(src.numel()), off.ctypes.data_as(_abi.c_int64_p),
                                                         stp.ctypes.data_as(_abi.c_int32_p), fmt.ctypes.data_as(_abi.c_int32_p), out.data_ptr(), stride,
                                                         self.detector._stream_ptr(stream)))
        return out

    def loadSincPCM(self, src, byteOffsets, byteSteps, formats, sourceSamples, sourceRates, zeroCrossings=None, beta=None, rolloff=None, out=None,
                    stream=None):
        """loadSinc() from the files' own bytes (syldet_recordings_load_sinc_pcm_device): the layout of loadPCM, recording k with
        sourceSamples[k] samples at sourceRates[k]; the bits of loadSinc() on pcmDecode's float32 of the same bytes."""
        from .resampler import _sinc_quality
        off, stp, fmt, out, stride = self._pcm_args(src, byteOffsets, byteSteps, formats, out)
        n = np.ascontiguousarray(sourceSamples, dtype=np.int64).reshape(-1)
        rates = np.ascontiguousarray(sourceRates, dtype=np.float64).reshape(-1)
        if n.size != self.count or rates.size != self.count:
            raise ValueError("one length and rate per recording")
        z, b, r = _sinc_quality(zeroCrossings, beta, rolloff)
        check(_abi.lib.syldet_recordings_load_sinc_pcm_device(self._h, src.data_ptr(), int(src.numel()), off.ctypes.data_as(_abi.c_int64_p),
                                                              stp.ctypes.data_as(_abi.c_int32_p), fmt.ctypes.data_as(_abi.c_int32_p),
                                                              n.ctypes.data_as(_abi.c_int64_p), rates.ctypes.data_as(_abi.c_double_p), z, b, r,
                                                              out.data_ptr(), stride, self.detector._stream_ptr(stream)))
        return out

    def view(self, tensor, k: int):
        """The part of a [C, rowEvaluations, ...] result (outputs, flags) that belongs to recording k: [n_evals, ...], no copy."""
        row, _, first, n_evals, _ = self.slots[k]
        return tensor[row, first:first + n_evals]

    def events(self, outputs, flags, debounce: float = 0.0, capacity: Optional[int] = None, stream=None):
        """outputs [C, rowEvaluations, n_out] (or None), flags [C, rowEvaluations] as run() wrote them for the loaded rows ->
        (indices [K, capacity] i64, values [K, capacity, n_out] f32 or None, counts [K] i64): each recording's detections as
        detections() gives them on its flags alone -- sample numbers from the recording's start, debounce restarting with it --
        and the outputs of each detection's evaluation.  counts may exceed capacity (default: the longest recording's
        evaluations)."""
        torch = _torch()
        det = self.detector
        E, n_out = self.rowEvaluations, det.geometry.outputs
        if not (flags.is_cuda and flags.dtype == torch.uint8 and tuple(flags.shape) == (det.channels, E) and flags.is_contiguous()
                and flags.device.index == det.device):
            raise ValueError("flags must be a contiguous uint8 CUDA tensor [channels, rowEvaluations] on the detector's device")
        if outputs is not None and not (outputs.is_cuda and outputs.dtype == torch.float32 and tuple(outputs.shape) == (det.channels, E, n_out)
                                        and outputs.is_contiguous() and outputs.device == flags.device):
            raise ValueError("outputs must be a contiguous float32 CUDA tensor [channels, rowEvaluations, outputs] on the flags' device")
        cap = max([s[3] for s in self.slots], default=0) if capacity is None else int(capacity)
        idx = torch.empty((self.count, max(cap, 1)), dtype=torch.int64, device=flags.device)
        val = None if outputs is None else torch.empty((self.count, max(cap, 1), n_out), dtype=torch.float32, device=flags.device)
        cnt = torch.zeros((self.count,), dtype=torch.int64, device=flags.device)
        check(_abi.lib.syldet_recordings_events_device(self._h, None if outputs is None else outputs.data_ptr(), flags.data_ptr(), float(debounce),
                                                       idx.data_ptr(), None if val is None else val.data_ptr(), cap, cnt.data_ptr(),
                                                       det._stream_ptr(stream)))
        return idx, val, cnt

    # ---- every recording's output track and trigger track (syldet_recordings_trace_device*, syldet_recordings_trigger*_device*) ----
    def _track_steps(self, steps):
        stp = np.ones(self.count, np.int32) if steps is None else np.ascontiguousarray(steps, dtype=np.int32).reshape(-1)
        if stp.size != self.count:
            raise ValueError("one step per recording")
        if self.count and stp.min() < 1:
            raise ValueError("steps must be at least 1")
        return stp

    def trackLayout(self, steps=None, align: int = 8):
        """The default destination of the tracks: the recordings end to end in the caller's order, each from a multiple of
        `align` elements (8 int16 elements are 16 bytes).  Recording k of n_k samples takes (n_k - 1) * steps[k] + 1 elements
        (steps None: all 1, so n_k).  Returns (offsets, total): offsets an int64 array [K], total the elements in all.  Host only."""
        a = int(align)
        if a < 1:
            raise ValueError("align must be at least 1")
        stp = self._track_steps(steps)
        off, pos = np.zeros(self.count, np.int64), 0
        for k, s in enumerate(self.slots):
            pos = (pos + a - 1) // a * a
            off[k] = pos
            pos += (s[4] - 1) * int(stp[k]) + 1 if s[4] > 0 else 0
        return off, pos

    def _track_dst(self, dtype, offsets, steps, out, device):
        torch = _torch()
        dt = SyllableDetector._trace_dtype(dtype, False)
        tdt = torch.float32 if dt == np.dtype(np.float32) else torch.int16
        stp = self._track_steps(steps)
        if offsets is None:
            off, total = self.trackLayout(stp)
        else:
            off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
            if off.size != self.count:
                raise ValueError("one offset per recording")
            if self.count and off.min() < 0:
                raise ValueError("offsets must not be negative")
            n = np.array([s[4] for s in self.slots], np.int64)
            total = int((off + np.maximum(n - 1, 0) * stp + 1)[n > 0].max(initial=0))
        if out is None:
            out = torch.zeros((total,), dtype=tdt, device=device)
        elif not (out.is_cuda and out.dtype == tdt and out.dim() == 1 and out.is_contiguous() and out.device == device):
            raise ValueError("out must be a contiguous 1-D CUDA tensor of the track's dtype on the detector's device")
        elif out.numel() < total:
            raise ValueError("a recording's track reaches outside out")
        return dt, off, stp, out

    def trace(self, outputs, output: int = 0, dtype=np.int16, offsets=None, steps=None, out=None, stream=None):
        """Every recording's output track in one launch (syldet_recordings_trace_device*): outputs [C, rowEvaluations, n_out] as
        run() wrote them for the loaded rows -> a 1-D tensor in which element i of recording k lies at offsets[k] + i * steps[k],
        with the values SyllableDetector.trace() gives on that recording alone.  offsets None: trackLayout(steps); steps None:
        all 1; step n with offsets base + t writes track t of an n-track file's frames.  `out`: the tensor to write into (only the
        recordings' own elements are written); None: a new one, zero elsewhere.  dtype np.int16 or np.float32."""
        torch = _torch()
        det = self.detector
        E, n_out = self.rowEvaluations, det.geometry.outputs
        if not (outputs.is_cuda and outputs.dtype == torch.float32 and tuple(outputs.shape) == (det.channels, E, n_out)
                and outputs.is_contiguous() and outputs.device.index == det.device):
            raise ValueError("outputs must be a contiguous float32 CUDA tensor [channels, rowEvaluations, outputs] on the detector's device")
        dt, off, stp, out = self._track_dst(dtype, offsets, steps, out, outputs.device)
        fn = _abi.lib.syldet_recordings_trace_device if dt == np.dtype(np.float32) else _abi.lib.syldet_recordings_trace_device_s16
        check(fn(self._h, outputs.data_ptr() if E > 0 else None, int(output), out.data_ptr() if out.numel() else None, int(out.numel()),
                 off.ctypes.data_as(_abi.c_int64_p), stp.ctypes.data_as(_abi.c_int32_p), det._stream_ptr(stream)))
        return out

    def _track_flags(self, flags, bufferLength, width, latency):
        torch = _torch()
        det = self.detector
        if not (flags.is_cuda and flags.dtype == torch.uint8 and tuple(flags.shape) == (det.channels, self.rowEvaluations)
                and flags.is_contiguous() and flags.device.index == det.device):
            raise ValueError("flags must be a contiguous uint8 CUDA tensor [channels, rowEvaluations] on the detector's device")
        N = det.triggerWidth() if width is None else int(width)
        return int(bufferLength), N, int(latency)

    def triggerTrack(self, flags, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0, dtype=np.int16, offsets=None,
                     steps=None, out=None, stream=None):
        """Every recording's TTL trigger track (syldet_recordings_trigger_device*: a scan and an expansion): flags
        [C, rowEvaluations] as run() wrote them -> the destination of trace(), with the values SyllableDetector.triggerTrack()
        gives on that recording's flags alone; a pulse never reaches the next recording of a row."""
        det = self.detector
        L, N, lat = self._track_flags(flags, bufferLength, width, latency)
        dt, off, stp, out = self._track_dst(dtype, offsets, steps, out, flags.device)
        fn = _abi.lib.syldet_recordings_trigger_device if dt == np.dtype(np.float32) else _abi.lib.syldet_recordings_trigger_device_s16
        check(fn(self._h, flags.data_ptr() if self.rowEvaluations > 0 else None, L, N, lat, out.data_ptr() if out.numel() else None,
                 int(out.numel()), off.ctypes.data_as(_abi.c_int64_p), stp.ctypes.data_as(_abi.c_int32_p), det._stream_ptr(stream)))
        return out

    def triggerOnsets(self, flags, bufferLength: int = 32, width: Optional[int] = None, latency: int = 0, capacity: Optional[int] = None,
                      stream=None):
        """The rising edges of every recording's trigger track (syldet_recordings_trigger_onsets_device): (indices [K, capacity]
        i64, counts [K] i64), sample numbers from each recording's own start, in order; counts may exceed capacity (default: the
        most a recording can have)."""
        torch = _torch()
        det = self.detector
        L, N, lat = self._track_flags(flags, bufferLength, width, latency)
        if L < 1:
            raise ValueError("bufferLength must be a power of two in [8, 4096]")
        cap = max([min(s[3], s[4] // L + 1) for s in self.slots], default=0) if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError("capacity must not be negative")
        idx = torch.empty((self.count, cap), dtype=torch.int64, device=flags.device)       # (capacity 0: counts only, no index is written)
        cnt = torch.zeros((self.count,), dtype=torch.int64, device=flags.device)
        check(_abi.lib.syldet_recordings_trigger_onsets_device(self._h, flags.data_ptr() if self.rowEvaluations > 0 else None, L, N, lat,
                                                               idx.data_ptr() if idx.numel() else None, cap, cnt.data_ptr() if self.count else None,
                                                               det._stream_ptr(stream)))
        return idx, cnt

    def trackView(self, tensor, k: int, offsets=None, steps=None):
        """Recording k's elements of a track tensor (or array) written with these offsets and steps: [n_k], no copy."""
        stp = self._track_steps(steps)
        off = self.trackLayout(stp)[0] if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        n, o, s = self.slots[k][4], int(off[k]), int(stp[k])
        return tensor[o:o + (n - 1) * s + 1:s] if n > 0 else tensor[o:o]

    # ---- every recording's level meters (syldet_recordings_levels_device*, syldet_recordings_output_levels_device) ----
    def _levels_pair(self, bufferLength, buffersPerReading):
        L = int(bufferLength)
        P = self.detector.defaultBuffersPerReading(L) if buffersPerReading is None else int(buffersPerReading)
        if int(_abi.lib.syldet_levels_count(0, L, P)) < 0:
            raise ValueError("bufferLength must be a power of two in [8, 4096] and buffersPerReading >= 1")
        return L, P

    def levelsLayout(self, bufferLength: int = 32, buffersPerReading: Optional[int] = None):
        """Where every recording's readings lie in the flat tables of levels() and outputLevels() (the arithmetic of
        syldet_recordings_levels_layout): an int64 array [K + 1], recording k's syldet_levels_count(n_k, L, P) readings are
        elements [first[k], first[k + 1]), first[K] the readings in all.  buffersPerReading None: the 0.1 s timer
        (SyllableDetector.defaultBuffersPerReading).  Host only."""
        L, P = self._levels_pair(bufferLength, buffersPerReading)
        kept = self.__dict__.setdefault("_levels_first", {})       # (a pair's prefix is made once: the calls below ask for it every time)
        if (L, P) not in kept:
            first = np.zeros(self.count + 1, np.int64)
            for k, s in enumerate(self.slots):
                first[k + 1] = first[k] + int(_abi.lib.syldet_levels_count(int(s[4]), L, P))
            first.setflags(write=False)
            kept[(L, P)] = first
        return kept[(L, P)]

    def _levels_out(self, dtype, total, out, device):
        torch = _torch()
        if out is None:
            return torch.empty((total,), dtype=dtype, device=device)
        if not (out.is_cuda and out.dtype == dtype and out.dim() == 1 and out.is_contiguous() and out.device == device):
            raise ValueError("out must be a contiguous 1-D CUDA tensor of the table's dtype on the detector's device")
        return out

    def levels(self, rows, bufferLength: int = 32, buffersPerReading: Optional[int] = None, out=None, stream=None):
        """Every recording's input meter (syldet_recordings_levels_device*): rows [C, >= rowSamples] float32 or int16 as load() /
        loadSinc() wrote them -> the fp64 MEAN SQUARES of the readings, flat over the recordings as levelsLayout() lays them,
        with the bits SyllableDetector.levels() / levelsPCM16() gives on each recording alone.  `out`: a float64 tensor of at
        least that many elements to write into.  Asynchronous on `stream`; the same pair again is launches only."""
        torch = _torch()
        det = self.detector
        if not (rows.is_cuda and rows.dtype in (torch.float32, torch.int16) and rows.dim() == 2 and rows.shape[0] == det.channels
                and rows.shape[1] >= self.rowSamples and rows.stride(1) == 1 and rows.device.index == det.device):
            raise ValueError("rows must be a float32 or int16 CUDA tensor [channels, >= rowSamples] on the detector's device, rows contiguous")
        L, P = self._levels_pair(bufferLength, buffersPerReading)
        total = int(self.levelsLayout(L, P)[-1])
        out = self._levels_out(torch.float64, total, out, rows.device)
        if total > 0:                                          # (a table too small is the library's refusal)
            fn = _abi.lib.syldet_recordings_levels_device_s16 if rows.dtype == torch.int16 else _abi.lib.syldet_recordings_levels_device
            stride = int(rows.stride(0)) if det.channels > 1 else int(rows.shape[1])
            check(fn(self._h, rows.data_ptr(), stride, L, P, out.data_ptr() if out.numel() else None, int(out.numel()), det._stream_ptr(stream)))
        return out

    def outputLevels(self, outputs, output: int = 0, bufferLength: int = 32, buffersPerReading: Optional[int] = None, out=None, stream=None):
        """Every recording's output meter (syldet_recordings_output_levels_device): outputs [C, rowEvaluations, n_out] as run()
        wrote them for the loaded rows -> float32, flat as levelsLayout() lays them, with the values
        SyllableDetector.outputLevels() gives on each recording's evaluations alone (0 for a reading without one)."""
        torch = _torch()
        det = self.detector
        E, n_out = self.rowEvaluations, det.geometry.outputs
        if not (outputs.is_cuda and outputs.dtype == torch.float32 and tuple(outputs.shape) == (det.channels, E, n_out)
                and outputs.is_contiguous() and outputs.device.index == det.device):
            raise ValueError("outputs must be a contiguous float32 CUDA tensor [channels, rowEvaluations, outputs] on the detector's device")
        L, P = self._levels_pair(bufferLength, buffersPerReading)
        total = int(self.levelsLayout(L, P)[-1])
        out = self._levels_out(torch.float32, total, out, outputs.device)
        if total > 0:                                          # (a table too small is the library's refusal)
            check(_abi.lib.syldet_recordings_output_levels_device(self._h, outputs.data_ptr() if E > 0 else None, int(output), L, P,
                                                                  out.data_ptr() if out.numel() else None, int(out.numel()),
                                                                  det._stream_ptr(stream)))
        return out

    def levelsView(self, tensor, k: int, bufferLength: int = 32, buffersPerReading: Optional[int] = None):
        """Recording k's readings of a table levels() or outputLevels() made with this pair (tensor or array): [M_k], no copy."""
        first = self.levelsLayout(bufferLength, buffersPerReading)
        return tensor[int(first[k]):int(first[k + 1])]

    def scorer(self, thresholds, labels, tolerance: int, debounce: float = 0.0) -> "Scorer":
        """A Scorer whose detectors are these recordings: labels[k], the labelled sample numbers of recording k, count from its
        own start (SyllableDetector.scorer)."""
        return Scorer(self.detector, thresholds, labels, tolerance, debounce, recordings=self)

    # ---- the packed rows' columns, and windows of them at every recording's events ----
    def spectrogram(self, rows, stream=None):
        """rows [C, >= rowSamples] float32 as load*() wrote them -> columns [C, countFrames(rowSamples), bins]
        (syldet_spectrogram_device on the packed rows): recording k's columns are columnsView(cols, k), bit for bit its
        spectrogram alone on the fold kernel and the generic engine; row frames between recordings mean nothing."""
        det = self.detector
        if not (rows.dim() == 2 and rows.shape[1] >= self.rowSamples):
            raise ValueError("rows must be [channels, >= rowSamples]")
        return det.spectrogram(rows[:, :self.rowSamples], stream=stream)

    def columnsView(self, cols, k: int):
        """The part of spectrogram()'s columns that belongs to recording k: [countFrames(n_samples), bins], no copy."""
        row, _, first, _, n = self.slots[k]
        return cols[row, first:first + max(self.detector.countFrames(n), 0)]

    def aligner(self, source="columns", before: Optional[int] = None, after: Optional[int] = None) -> "Aligner":
        """An Aligner whose detectors are these recordings: events count from each recording's own start, and a window never
        reads beyond its recording (SyllableDetector.aligner).  The arrays are those of the packed rows: spectrogram(rows),
        the detector's run(rows) outputs, or the rows themselves."""
        return Aligner(self.detector, source, before, after, recordings=self)

    def trainer(self) -> "Trainer":
        """A Trainer whose detectors are these recordings: labels count from each recording's own start, and whatever lies
        between two recordings or behind the last one gets weight 0 and is never read (SyllableDetector.trainer).  The columns
        are spectrogram(rows)."""
        return Trainer(self.detector, recordings=self)

    def multiTrainer(self) -> "MultiTrainer":
        """A MultiTrainer whose detectors are these recordings: a recording trains the network of the row it was planned onto
        (SyllableDetector.multiTrainer, trainer)."""
        return MultiTrainer(self.detector, recordings=self)

    def matcher(self, template, anchor: Optional[int] = None) -> "Matcher":
        """A Matcher whose detectors are these recordings: a window never reaches beyond its recording, matches are never
        suppressed across two recordings of a row, and events count from each recording's own start (SyllableDetector.matcher).
        The columns are spectrogram(rows)."""
        return Matcher(self.detector, template, anchor, recordings=self)

    def matcherBank(self, templates, classes=None, anchor=None, ragged: Optional[bool] = None) -> "MatcherBank":
        """A MatcherBank whose detectors are these recordings (SyllableDetector.matcherBank, Recordings.matcher); ragged as there."""
        return MatcherBank(self.detector, templates, classes, anchor, recordings=self, ragged=ragged)


def _score_args(thresholds, labels):
    thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    labels = [np.ascontiguousarray(t, dtype=np.int64).reshape(-1) for t in labels]
    begin = np.zeros(len(labels) + 1, np.int64)
    np.cumsum([t.size for t in labels], out=begin[1:])
    flat = np.concatenate(labels) if labels else np.zeros(0, np.int64)
    return thr, np.ascontiguousarray(flat, dtype=np.int64), begin


class Scorer:
    """Threshold calibration (syldet_scorer_*, include/syldet.h "threshold calibration"): thresholds, labels and tolerance kept
    on the device, so that score() is one launch over outputs that are there already.  A detector is a channel of the bank, or
    (made by Recordings.scorer) a recording.  labels: a list of arrays, one per detector, of sorted sample numbers; tolerance in
    samples; debounce in seconds.  The detector (and the Recordings) must outlive it."""

    def __init__(self, detector: SyllableDetector, thresholds, labels, tolerance: int, debounce: float = 0.0, recordings: Optional[Recordings] = None):
        self.detector = detector
        self.recordings = recordings
        labels = list(labels)
        D = recordings.count if recordings is not None else detector.channels
        if len(labels) != D:
            raise ValueError("one array of labels per detector (%d given, %d detectors)" % (len(labels), D))
        thr, flat, begin = _score_args(thresholds, labels)
        self.thresholds = thr.copy()
        self.labelCounts = np.diff(begin)
        self.tolerance, self.debounce = int(tolerance), float(debounce)
        self._h = _abi.Handle()
        check(_abi.lib.syldet_scorer_create(detector._h, None if recordings is None else recordings._h, thr.ctypes.data_as(_abi.c_double_p), thr.size,
                                            flat.ctypes.data_as(_abi.c_int64_p), begin.ctypes.data_as(_abi.c_int64_p), self.tolerance, self.debounce,
                                            C.byref(self._h)))
        d, k, n = C.c_int32(), C.c_int32(), C.c_int64()
        check(_abi.lib.syldet_scorer_shape(self._h, C.byref(d), C.byref(k), C.byref(n)))
        self.count, self.thresholdCount, self.labelCount = d.value, k.value, n.value

    def close(self):
        if getattr(self, "_h", None):
            _abi.lib.syldet_scorer_destroy(self._h)
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

    def score(self, outputs, output: int = 0, out=None, stream=None):
        """outputs [C, n_evals, n_out] as run() wrote them (for recordings: of the packed rows, n_evals = rowEvaluations) ->
        table [D, K, 6] int64 on the device: per detector and threshold (detections, hits, false positives, repeats, the sum of
        the hits' offsets in samples, the sum of their squares), scoring output `output`.  Asynchronous on `stream`."""
        torch = _torch()
        det = self.detector
        n_out = det.geometry.outputs
        if not (outputs.is_cuda and outputs.dtype == torch.float32 and outputs.dim() == 3 and outputs.shape[0] == det.channels
                and outputs.shape[2] == n_out and outputs.is_contiguous() and outputs.device.index == det.device):
            raise ValueError("outputs must be a contiguous float32 CUDA tensor [channels, n_evals, outputs] on the detector's device")
        if self.recordings is not None and outputs.shape[1] != self.recordings.rowEvaluations:
            raise ValueError("outputs must hold the packed rows' %d evaluations" % self.recordings.rowEvaluations)
        if not 0 <= int(output) < n_out:
            raise ValueError("output must be in [0, %d)" % n_out)
        want = (self.count, self.thresholdCount, _abi.SCORE_COLUMNS)
        if out is None:
            out = torch.zeros(want, dtype=torch.int64, device=outputs.device)
        elif not (out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == want and out.is_contiguous() and out.device == outputs.device):
            raise ValueError("out must be a contiguous int64 CUDA tensor of shape %s on the outputs' device" % (want,))
        check(_abi.lib.syldet_score_device(self._h, outputs.data_ptr(), int(outputs.shape[1]), int(output), out.data_ptr(), det._stream_ptr(stream)))
        return out

    def choose(self, table, falsePositiveCost: float = 1.0):
        """(k, threshold, totals [K, 6], costs [K]) of a table of score(): the tables summed over the detectors, cost_k = misses_k
        + falsePositiveCost (false positives_k + repeats_k), and the lowest k of the smallest cost (syldet_score_choose).  A
        device table is waited for and downloaded."""
        if hasattr(table, "is_cuda"):
            table = table.cpu().numpy()
        k, totals, costs = chooseThreshold(table, self.labelCounts, falsePositiveCost)
        return k, float(self.thresholds[k]), totals, costs


def scoreHost(values, thresholds, labels, tolerance: int, firstIndex: int, hop: int, debounceFrames: int = 0) -> np.ndarray:
    """syldet_score_host: one detector scored on the host, no device needed.  values: a 1-D float32 array (a strided view such as
    outputs[c, :, o] is read in place), labels: its sorted labelled sample numbers -> table [K, 6] int64."""
    v = np.asarray(values)
    if v.dtype != np.float32 or v.ndim != 1:
        raise ValueError("values must be a 1-D float32 array")
    if v.size > 1 and (v.strides[0] <= 0 or v.strides[0] % 4):
        v = np.ascontiguousarray(v)
    stride = v.strides[0] // 4 if v.size > 1 else 1
    thr, flat, _ = _score_args(thresholds, [labels])
    table = np.zeros((thr.size, _abi.SCORE_COLUMNS), np.int64)
    check(_abi.lib.syldet_score_host(C.cast(v.ctypes.data, _abi.c_float_p), v.size, stride, thr.ctypes.data_as(_abi.c_double_p), thr.size,
                                     flat.ctypes.data_as(_abi.c_int64_p), flat.size, int(tolerance), int(firstIndex), int(hop), int(debounceFrames),
                                     table.ctypes.data_as(_abi.c_int64_p)))
    return table


def chooseThreshold(table, labelCounts, falsePositiveCost: float = 1.0):
    """syldet_score_choose: table [D, K, 6] (or [K, 6]: one detector) and each detector's label count -> (k, totals [K, 6] int64,
    costs [K] float64): the lowest k of the smallest misses + falsePositiveCost (false positives + repeats)."""
    t = np.ascontiguousarray(table, dtype=np.int64)
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3 or t.shape[2] != _abi.SCORE_COLUMNS:
        raise ValueError("table must be [detectors, thresholds, %d]" % _abi.SCORE_COLUMNS)
    n = np.ascontiguousarray(labelCounts, dtype=np.int64).reshape(-1)
    if n.size != t.shape[0]:
        raise ValueError("one label count per detector")
    best = C.c_int32()
    totals = np.zeros((t.shape[1], _abi.SCORE_COLUMNS), np.int64)
    costs = np.zeros(t.shape[1], np.float64)
    check(_abi.lib.syldet_score_choose(t.ctypes.data_as(_abi.c_int64_p), t.shape[0], t.shape[1], n.ctypes.data_as(_abi.c_int64_p), float(falsePositiveCost),
                                       C.byref(best), totals.ctypes.data_as(_abi.c_int64_p), costs.ctypes.data_as(_abi.c_double_p)))
    return int(best.value), totals, costs


_ALIGN_SOURCES = {"columns": _abi.ALIGN_COLUMNS, "outputs": _abi.ALIGN_OUTPUTS, "samples": _abi.ALIGN_SAMPLES}


def _align_source(source) -> int:
    if isinstance(source, str):
        if source not in _ALIGN_SOURCES:
            raise ValueError("source must be one of %s" % sorted(_ALIGN_SOURCES))
        return _ALIGN_SOURCES[source]
    return int(source)


class Aligner:
    """Event-aligned windows (syldet_aligner_*, include/syldet.h "event-aligned windows"): for every event -- a detection index, a
    label, any sample number counted from its detector's start -- the units of a source around the event's anchor unit, one window
    an event, and the stack statistics of groups of windows.  A detector is a channel of the bank, or (made by Recordings.aligner)
    a recording.  shape = (detectors, units a window, width).  The detector (and the Recordings) must outlive it."""

    def __init__(self, detector: SyllableDetector, source="columns", before: Optional[int] = None, after: Optional[int] = None,
                 recordings: Optional[Recordings] = None):
        self.detector = detector
        self.recordings = recordings
        self.source = _align_source(source)
        T = int(detector.config.timeRange)
        self.before = T - 1 if before is None else int(before)
        self.after = T - 1 if after is None else int(after)
        self._h = _abi.Handle()
        check(_abi.lib.syldet_aligner_create(detector._h, None if recordings is None else recordings._h, self.source, self.before, self.after,
                                             C.byref(self._h)))
        d, n, w = C.c_int32(), C.c_int64(), C.c_int32()
        check(_abi.lib.syldet_aligner_shape(self._h, C.byref(d), C.byref(n), C.byref(w)))
        self.shape = (d.value, n.value, w.value)
        self.count = d.value
        self._begin = None               # the event prefix of the last windows() call: what stats() describes

    def close(self):
        if getattr(self, "_h", None):
            _abi.lib.syldet_aligner_destroy(self._h)
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

    def _source_args(self, array):
        """(n_units, row_stride in elements) of a source array, checked against the source's layout"""
        torch = _torch()
        det, width = self.detector, self.shape[2]
        if not (array.is_cuda and array.dtype == torch.float32 and array.device.index == det.device):
            raise ValueError("the source must be a float32 CUDA tensor on the detector's device")
        if self.source == _abi.ALIGN_SAMPLES:
            if not (array.dim() == 2 and array.shape[0] == det.channels and (array.shape[1] == 0 or array.stride(1) == 1)):
                raise ValueError("samples must be [channels, n_samples], rows contiguous")
            n_units = int(array.shape[1]) if self.recordings is None else self.recordings.rowSamples
            if array.shape[1] < n_units:
                raise ValueError("samples must hold the packed rows' %d samples" % n_units)
            return n_units, (int(array.stride(0)) if det.channels > 1 else max(int(array.shape[1]), n_units))
        if not (array.dim() == 3 and array.shape[0] == det.channels and array.shape[2] == width and array.is_contiguous()):
            raise ValueError("the source must be a contiguous tensor [channels, units, %d]" % width)
        return int(array.shape[1]), 0

    def windows(self, array, events, counts=None, fill: float = float("nan"), out=None, stream=None):
        """array: the source on the device -- columns [C, n_frames, bins], outputs [C, n_evals, n_out] or samples [C, S], for
        recordings those of the packed rows.  events: the (indices [D, capacity], counts [D]) pair of detections() / events()
        (pass counts=; a count beyond the capacity means the capacity), or a list of D arrays of sample numbers, or one flat
        int64 CUDA tensor with counts.  -> windows [N, n, width] float32 on the device, detector d's j-th event at
        eventBegin[d] + j; elements outside a detector's units are `fill`.  One launch; the same counts again make it a launch
        only.  Asynchronous on `stream` (a counts tensor on the device is waited for and downloaded)."""
        torch = _torch()
        det = self.detector
        n_units, row_stride = self._source_args(array)
        D, n, width = self.shape
        if counts is None:
            if hasattr(events, "is_cuda"):
                raise ValueError("an events tensor needs counts")
            parts = [np.ascontiguousarray(e, dtype=np.int64).reshape(-1) for e in events]
            if len(parts) != D:
                raise ValueError("one array of events per detector (%d given, %d detectors)" % (len(parts), D))
            cnt = np.array([p.size for p in parts], np.int64)
            flat = np.concatenate(parts) if parts else np.zeros(0, np.int64)
            ev = torch.from_numpy(np.ascontiguousarray(flat, dtype=np.int64)).to(array.device)
            stride = 0
        else:
            cnt = (counts.cpu().numpy() if hasattr(counts, "is_cuda") else np.asarray(counts)).astype(np.int64).reshape(-1)
            ev = events
            if not (hasattr(ev, "is_cuda") and ev.is_cuda and ev.dtype == torch.int64 and ev.is_contiguous() and ev.device == array.device
                    and ev.dim() in (1, 2)):
                raise ValueError("events must be a contiguous int64 CUDA tensor [detectors, capacity] (or flat) on the source's device")
            if cnt.size != D or (cnt.size and cnt.min() < 0):
                raise ValueError("one count per detector, none negative")
            if ev.dim() == 2:
                if ev.shape[0] != D:
                    raise ValueError("events must have one row per detector")
                stride = int(ev.shape[1])
                cnt = np.minimum(cnt, stride)
            else:
                stride = 0
                if int(cnt.sum()) > ev.numel():
                    raise ValueError("the counts reach beyond the events")
        begin = np.zeros(D + 1, np.int64)
        np.cumsum(cnt, out=begin[1:])
        N = int(begin[-1])
        want = (N, n, width)
        if out is None:
            out = torch.empty(want, dtype=torch.float32, device=array.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == want and out.is_contiguous() and out.device == array.device):
            raise ValueError("out must be a contiguous float32 CUDA tensor of shape %s on the source's device" % (want,))
        check(_abi.lib.syldet_align_device(self._h, array.data_ptr(), n_units, row_stride, ev.data_ptr(), stride, begin.ctypes.data_as(_abi.c_int64_p),
                                           float(fill), out.data_ptr(), det._stream_ptr(stream)))
        self._begin = begin
        self.eventBegin = begin.copy()
        # the launch may still be reading the events when this returns: they stay with the aligner until the next call, and a stream
        # other than torch's current one is told to the allocator
        self._events = ev
        if stream is not None:
            ev.record_stream(stream)
        return out

    def stats(self, windows, groups=None, groupCount: Optional[int] = None, stream=None):
        """The stack statistics of the windows the last windows() call made: (count int64, sum float64, sumsq float64), each
        [G, n, width] on the device.  groups: the stack of every detector (default: one stack of all), G = groupCount or
        max(groups) + 1.  Sums run in blocks of 256 events in a fixed order, so they are the same bits every time, and those of
        alignStatsHost; the mean is sum / count.  Presence is what the LAST windows() call found: call stats() before the next
        windows() -- with the same counts but other events or another array that call replaces the spans, and statistics of an
        earlier call's tensor would go by them without an error."""
        torch = _torch()
        if self._begin is None:
            raise ValueError("stats() describes the windows of the last windows() call: there has been none")
        D, n, width = self.shape
        grp = np.zeros(D, np.int32) if groups is None else np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        if grp.size != D:
            raise ValueError("one group per detector")
        G = int(groupCount) if groupCount is not None else (int(grp.max()) + 1 if D else 1)
        want = (int(self._begin[-1]), n, width)
        if not (windows.is_cuda and windows.dtype == torch.float32 and tuple(windows.shape) == want and windows.is_contiguous()
                and windows.device.index == self.detector.device):
            raise ValueError("windows must be the contiguous float32 CUDA tensor of shape %s the last windows() call made" % (want,))
        count = torch.empty((max(G, 0), n, width), dtype=torch.int64, device=windows.device)
        total = torch.empty((max(G, 0), n, width), dtype=torch.float64, device=windows.device)
        squares = torch.empty((max(G, 0), n, width), dtype=torch.float64, device=windows.device)
        check(_abi.lib.syldet_align_stats_device(self._h, windows.data_ptr(), self._begin.ctypes.data_as(_abi.c_int64_p),
                                                 grp.ctypes.data_as(_abi.c_int32_p), G, count.data_ptr(), total.data_ptr(), squares.data_ptr(),
                                                 self.detector._stream_ptr(stream)))
        return count, total, squares


def alignHost(source, events, before: int, after: int, origin: int, step: int, fill: float = float("nan")):
    """syldet_align_host: one detector's windows on the host, no device needed.  source: the detector's own units, [units, width]
    (or [units]: width 1) float32; events: sample numbers; origin, step: the source's anchor rule u0 = floor((s - origin) / step)
    -> (windows [n_events, before + after + 1, width] float32, present [n_events, 2] int64: each window's first present element
    and the number of present elements)."""
    a = np.asarray(source)
    if a.dtype != np.float32 or a.ndim not in (1, 2):
        raise ValueError("source must be a float32 array [units] or [units, width]")
    a = np.ascontiguousarray(a if a.ndim == 2 else a[:, None])
    width = int(a.shape[1])
    ev = np.ascontiguousarray(events, dtype=np.int64).reshape(-1)
    n = int(before) + int(after) + 1
    windows = np.empty((ev.size, max(n, 0), max(width, 1)), np.float32)
    present = np.zeros((ev.size, 2), np.int64)
    check(_abi.lib.syldet_align_host(a.ctypes.data_as(_abi.c_float_p), a.shape[0], width, int(origin), int(step), int(before), int(after),
                                     ev.ctypes.data_as(_abi.c_int64_p), ev.size, float(fill), windows.ctypes.data_as(_abi.c_float_p),
                                     present.ctypes.data_as(_abi.c_int64_p)))
    return windows, present


def alignStatsHost(windows, present):
    """syldet_align_stats_host: one stack on the host.  windows [events, ...] float32 and present [events, 2] as alignHost gave
    them, in the stack's order -> (count int64, sum float64, sumsq float64), each of a window's shape."""
    w = np.ascontiguousarray(windows, dtype=np.float32)
    if w.ndim < 2:
        raise ValueError("windows must be [events, ...]")
    shape = w.shape[1:]
    L = int(np.prod(shape))
    pr = np.ascontiguousarray(present, dtype=np.int64).reshape(-1, 2)
    if pr.shape[0] != w.shape[0]:
        raise ValueError("one present pair per window")
    count, total, squares = np.zeros(L, np.int64), np.zeros(L, np.float64), np.zeros(L, np.float64)
    check(_abi.lib.syldet_align_stats_host(w.ctypes.data_as(_abi.c_float_p), pr.ctypes.data_as(_abi.c_int64_p), w.shape[0], L,
                                           count.ctypes.data_as(_abi.c_int64_p), total.ctypes.data_as(_abi.c_double_p),
                                           squares.ctypes.data_as(_abi.c_double_p)))
    return count.reshape(shape), total.reshape(shape), squares.reshape(shape)


class Matcher:
    """Template matching (syldet_matcher_*, include/syldet.h "template matching"): the cosine between one normalised template and
    the window at every position of the columns, and the matches among the scores.  A detector is a channel of the bank, or (made
    by Recordings.matcher) a recording.  shape = (detectors, frames of the template, bins, anchor frame); template: the
    normalised template t^ the scores are taken with; form: "matrix" or "plain", the score kernel this shape runs on.  The
    detector (and the Recordings) must outlive it."""

    def __init__(self, detector: SyllableDetector, template, anchor: Optional[int] = None, recordings: Optional[Recordings] = None):
        self.detector = detector
        self.recordings = recordings
        t = np.asarray(template)
        if t.ndim != 2 or t.dtype.kind != "f":
            raise ValueError("the template must be a float array [frames, bins]")
        t = np.ascontiguousarray(t, dtype=np.float32)
        self._h = _abi.Handle()
        check(_abi.lib.syldet_matcher_create(detector._h, None if recordings is None else recordings._h, t.ctypes.data_as(_abi.c_float_p),
                                             t.shape[0], t.shape[1], -1 if anchor is None else int(anchor), C.byref(self._h)))
        d, n, b, a, mf = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(_abi.lib.syldet_matcher_shape(self._h, C.byref(d), C.byref(n), C.byref(b), C.byref(a), C.byref(mf)))
        self.shape = (d.value, n.value, b.value, a.value)
        self.count, self.frames, self.bins, self.anchor = self.shape
        self.form = "matrix" if mf.value else "plain"
        self.template = np.empty((n.value, b.value), np.float32)
        check(_abi.lib.syldet_matcher_template(self._h, self.template.ctypes.data_as(_abi.c_float_p)))

    def close(self):
        if getattr(self, "_h", None):
            _abi.lib.syldet_matcher_destroy(self._h)
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

    def scores(self, cols, out=None, stream=None):
        """cols [C, n_frames, bins] float32 on the device as spectrogram() wrote them (rows may be a view with a larger stride)
        -> scores [C, n_frames] float32: a detector's position p at its first frame + p, NaN wherever no window begins.  One
        launch; a score has the same bits wherever its window lies.  Asynchronous on `stream`."""
        torch = _torch()
        det = self.detector
        if not (cols.is_cuda and cols.dtype == torch.float32 and cols.device.index == det.device and cols.dim() == 3
                and cols.shape[0] == det.channels and cols.shape[2] == self.bins):
            raise ValueError("cols must be a float32 CUDA tensor [channels, n_frames, %d] on the detector's device" % self.bins)
        J = int(cols.shape[1])
        if J > 0 and not (cols.stride(2) == 1 and cols.stride(1) == self.bins):
            raise ValueError("the frames of a row of cols must be contiguous")
        row_stride = int(cols.stride(0)) if (det.channels > 1 and J > 0) else 0
        want = (det.channels, J)
        if out is None:
            out = torch.empty(want, dtype=torch.float32, device=cols.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == want and out.is_contiguous() and out.device == cols.device):
            raise ValueError("out must be a contiguous float32 CUDA tensor of shape %s on the columns' device" % (want,))
        check(_abi.lib.syldet_match_scores_device(self._h, cols.data_ptr() if J else None, J, row_stride, out.data_ptr() if J else None,
                                                  det._stream_ptr(stream)))
        return out

    def peaks(self, scores, threshold: float, separation: int, capacity: Optional[int] = None, withScores: bool = True, stream=None):
        """scores [C, n_frames] as scores() made them -> (events [D, capacity] int64 ascending, counts [D] int64, eventScores
        [D, capacity] float32 or None) on the device, the tables detections() makes: position p is a match iff its score is at
        least `threshold`, above every score up to `separation` positions before it and not below any up to `separation` behind
        it, NaN left out; its event is the sample number of frame p + anchor.  A count may exceed the capacity (default 1024).
        One launch."""
        torch = _torch()
        det = self.detector
        if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2 and scores.shape[0] == det.channels and scores.is_contiguous()
                and scores.device.index == det.device):
            raise ValueError("scores must be a contiguous float32 CUDA tensor [channels, n_frames] on the detector's device")
        cap = 1024 if capacity is None else int(capacity)
        D = self.count
        events = torch.empty((D, max(cap, 0)), dtype=torch.int64, device=scores.device)
        counts = torch.empty((D,), dtype=torch.int64, device=scores.device)
        ev_scores = torch.empty((D, max(cap, 0)), dtype=torch.float32, device=scores.device) if withScores else None
        J = int(scores.shape[1])
        check(_abi.lib.syldet_match_peaks_device(self._h, scores.data_ptr() if J else None, J, float(threshold), int(separation),
                                                 events.data_ptr() if events.numel() else None, cap, counts.data_ptr() if D else None,
                                                 ev_scores.data_ptr() if (withScores and ev_scores.numel()) else None, det._stream_ptr(stream)))
        return events, counts, ev_scores

    def find(self, cols, threshold: float, separation: int, stream=None):
        """scores() and peaks() -> (events, eventScores): two lists with one int64 and one float32 array a detector, every match
        of it (the tables are made again with the largest count as capacity where the first capacity was too small)."""
        s = self.scores(cols, stream=stream)
        ev, cnt, es = self.peaks(s, threshold, separation, stream=stream)
        c = cnt.cpu().numpy()
        if c.size and int(c.max()) > ev.shape[1]:
            ev, cnt, es = self.peaks(s, threshold, separation, capacity=int(c.max()), stream=stream)
            c = cnt.cpu().numpy()
        ev, es = ev.cpu().numpy(), es.cpu().numpy()
        return [ev[d, :c[d]].copy() for d in range(self.count)], [es[d, :c[d]].copy() for d in range(self.count)]


class MatcherBank:
    """A bank of templates (syldet_matcher_bank_*, include/syldet.h "template matching: a bank of templates"): K templates [K, n,
    bins] in C classes matched in one pass.  Template k's score has the bits of Matcher(template k)'s; a class's score is the
    greatest of its templates', `which` the lowest template that attains it (-1 where the score is NaN).  classes: the class of
    each template (None: template k is class k).  shape = (detectors, templates, classes, frames, bins, anchor); templates: the
    normalised templates; classes: the class table; form: "matrix" or "plain".  The detector (and the Recordings) must outlive
    it.
    A RAGGED bank ("template matching: a ragged bank"): `templates` a list of arrays [n_k, bins] of differing lengths (or any list
    of 2-D arrays with ragged=True), lined up at their anchors -- None: each template's last frame; one int for all; or one per
    template.  Its planes are indexed by the ANCHOR frame: element u holds the scores of the windows whose anchor is frame u, and an
    event is the sample of frame u.  ragged: is it one; lengths, anchors: every template's frames and anchor frame (a uniform
    bank: K times the same); templates is then a list, frames the greatest length and anchor 0."""

    def __init__(self, detector: SyllableDetector, templates, classes=None, anchor=None, recordings: Optional[Recordings] = None,
                 ragged: Optional[bool] = None):
        self.detector = detector
        self.recordings = recordings
        rec = None if recordings is None else recordings._h
        parts = None
        if isinstance(templates, (list, tuple)) and len(templates) and all(np.ndim(t) == 2 for t in templates):
            parts = [np.asarray(t) for t in templates]
            per_template = anchor is not None and np.ndim(anchor) > 0
            if ragged is None:
                ragged = len({p.shape[0] for p in parts}) > 1 or per_template
        if ragged and parts is None:
            raise ValueError("a ragged bank takes a list of arrays [frames, bins]")
        K = len(parts) if ragged else None
        if ragged:
            if any(p.dtype.kind != "f" for p in parts) or len({p.shape[1] for p in parts}) != 1:
                raise ValueError("the templates must be float arrays [frames, bins] of the same bins")
            t = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in parts]))
            lens = np.array([p.shape[0] for p in parts], np.int32)
            anc = None
            if anchor is not None:
                anc = np.ascontiguousarray(anchor, dtype=np.int32).reshape(-1)
                if anc.size == 1:
                    anc = np.full(K, anc[0], np.int32)                    # one frame: every template's
                if anc.size != K:
                    raise ValueError("one anchor, or one per template")
        else:
            t = np.asarray(templates)
            if t.ndim != 3 or t.dtype.kind != "f":
                raise ValueError("the templates must be a float array [templates, frames, bins]")
            t = np.ascontiguousarray(t, dtype=np.float32)
            K = t.shape[0]
            if anchor is not None and np.ndim(anchor) > 0:
                raise ValueError("a bank of one length has one anchor")
        cls, n_classes = None, 0
        if classes is not None:
            cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1)
            if cls.size != K:
                raise ValueError("one class per template")
            n_classes = int(cls.max()) + 1 if cls.size else 0
        self._h = _abi.Handle()
        if ragged:
            check(_abi.lib.syldet_matcher_bank_create_ragged(detector._h, rec, t.ctypes.data_as(_abi.c_float_p), K, lens.ctypes.data_as(_abi.c_int32_p),
                                                             parts[0].shape[1], None if anc is None else anc.ctypes.data_as(_abi.c_int32_p),
                                                             None if cls is None else cls.ctypes.data_as(_abi.c_int32_p), n_classes, C.byref(self._h)))
        else:
            check(_abi.lib.syldet_matcher_bank_create(detector._h, rec, t.ctypes.data_as(_abi.c_float_p),
                                                      t.shape[0], t.shape[1], t.shape[2], -1 if anchor is None else int(anchor),
                                                      None if cls is None else cls.ctypes.data_as(_abi.c_int32_p), n_classes, C.byref(self._h)))
        d, k, c, n, b, a, mf = (C.c_int32() for _ in range(7))
        check(_abi.lib.syldet_matcher_bank_shape(self._h, C.byref(d), C.byref(k), C.byref(c), C.byref(n), C.byref(b), C.byref(a), C.byref(mf)))
        self.shape = (d.value, k.value, c.value, n.value, b.value, a.value)
        self.count, self.nTemplates, self.nClasses, self.frames, self.bins, self.anchor = self.shape
        self.form = "matrix" if mf.value else "plain"
        self.lengths, self.anchors, rg = np.empty(k.value, np.int32), np.empty(k.value, np.int32), C.c_int32()
        check(_abi.lib.syldet_matcher_bank_lengths(self._h, self.lengths.ctypes.data_as(_abi.c_int32_p), self.anchors.ctypes.data_as(_abi.c_int32_p),
                                                   C.byref(rg)))
        self.ragged = bool(rg.value)
        flat = np.empty(int(self.lengths.sum()) * b.value, np.float32)
        self.classes = np.empty(k.value, np.int32)
        check(_abi.lib.syldet_matcher_bank_templates(self._h, flat.ctypes.data_as(_abi.c_float_p), self.classes.ctypes.data_as(_abi.c_int32_p)))
        if self.ragged:
            ends = np.cumsum(self.lengths.astype(np.int64)) * b.value
            self.templates = [flat[e - nk * b.value:e].reshape(nk, b.value) for e, nk in zip(ends, self.lengths)]
        else:
            self.templates = flat.reshape(k.value, n.value, b.value)

    def close(self):
        if getattr(self, "_h", None):
            _abi.lib.syldet_matcher_bank_destroy(self._h)
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

    def _thresholds(self, thresholds):
        t = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
        if t.size == 1:
            t = np.full(self.nClasses, t[0], np.float32)             # a scalar: the same value for every class
        if t.size != self.nClasses:
            raise ValueError("one threshold, or one per class")
        return t

    def _separations(self, separation):
        """None where one separation serves every class (the shared call), else one int32 per class"""
        if np.ndim(separation) == 0:
            return None
        s = np.ascontiguousarray(separation, dtype=np.int32).reshape(-1)
        if s.size != self.nClasses:
            raise ValueError("one separation, or one per class")
        return s

    def scores(self, cols, which: bool = False, out=None, stream=None):
        """cols [channels, n_frames, bins] as Matcher.scores takes them -> the class scores [C, channels, n_frames] float32, or with
        which=True (scores, which [C, channels, n_frames] int32).  out: a tensor for the scores, or with which=True a pair.  One
        launch for any K and C.  Asynchronous on `stream`."""
        torch = _torch()
        det = self.detector
        if not (cols.is_cuda and cols.dtype == torch.float32 and cols.device.index == det.device and cols.dim() == 3
                and cols.shape[0] == det.channels and cols.shape[2] == self.bins):
            raise ValueError("cols must be a float32 CUDA tensor [channels, n_frames, %d] on the detector's device" % self.bins)
        J = int(cols.shape[1])
        if J > 0 and not (cols.stride(2) == 1 and cols.stride(1) == self.bins):
            raise ValueError("the frames of a row of cols must be contiguous")
        row_stride = int(cols.stride(0)) if (det.channels > 1 and J > 0) else 0
        want = (self.nClasses, det.channels, J)
        out_s, out_w = (out if which else (out, None)) if out is not None else (None, None)
        if out_s is None:
            out_s = torch.empty(want, dtype=torch.float32, device=cols.device)
        elif not (out_s.is_cuda and out_s.dtype == torch.float32 and tuple(out_s.shape) == want and out_s.is_contiguous() and out_s.device == cols.device):
            raise ValueError("out must be a contiguous float32 CUDA tensor of shape %s on the columns' device" % (want,))
        if which:
            if out_w is None:
                out_w = torch.empty(want, dtype=torch.int32, device=cols.device)
            elif not (out_w.is_cuda and out_w.dtype == torch.int32 and tuple(out_w.shape) == want and out_w.is_contiguous() and out_w.device == cols.device):
                raise ValueError("which must be a contiguous int32 CUDA tensor of shape %s on the columns' device" % (want,))
        check(_abi.lib.syldet_match_bank_scores_device(self._h, cols.data_ptr() if J else None, J, row_stride, out_s.data_ptr() if J else None,
                                                       out_w.data_ptr() if (which and J) else None, det._stream_ptr(stream)))
        return (out_s, out_w) if which else out_s

    def peaks(self, scores, thresholds, separation, capacity: Optional[int] = None, which=None, withScores: bool = True, stream=None):
        """scores [C, channels, n_frames] as scores() made them -> (events [C, D, capacity] int64, counts [C, D] int64, eventScores
        [C, D, capacity] float32 or None, eventTemplates [C, D, capacity] int32 or None): every class's tables as Matcher.peaks makes
        them from that class's plane with that class's threshold (a scalar: the same for all); classes do not suppress each other.
        which: scores()'s second tensor, for eventTemplates.  separation: one int, or one per class
        (syldet_match_bank_peaks_each_device).  One launch."""
        torch = _torch()
        det = self.detector
        Cn = self.nClasses
        if not (scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 3 and scores.shape[0] == Cn and scores.shape[1] == det.channels
                and scores.is_contiguous() and scores.device.index == det.device):
            raise ValueError("scores must be a contiguous float32 CUDA tensor [classes, channels, n_frames] on the detector's device")
        if which is not None and not (which.is_cuda and which.dtype == torch.int32 and tuple(which.shape) == tuple(scores.shape) and which.is_contiguous()
                                      and which.device == scores.device):
            raise ValueError("which must be a contiguous int32 CUDA tensor of the scores' shape on their device")
        thr = self._thresholds(thresholds)
        seps = self._separations(separation)
        cap = 1024 if capacity is None else int(capacity)
        D = self.count
        events = torch.empty((Cn, D, max(cap, 0)), dtype=torch.int64, device=scores.device)
        counts = torch.empty((Cn, D), dtype=torch.int64, device=scores.device)
        ev_scores = torch.empty((Cn, D, max(cap, 0)), dtype=torch.float32, device=scores.device) if withScores else None
        ev_templ = torch.empty((Cn, D, max(cap, 0)), dtype=torch.int32, device=scores.device) if which is not None else None
        J = int(scores.shape[2])
        call, sep = ((_abi.lib.syldet_match_bank_peaks_device, int(separation)) if seps is None
                     else (_abi.lib.syldet_match_bank_peaks_each_device, seps.ctypes.data_as(_abi.c_int32_p)))
        check(call(self._h, scores.data_ptr() if J else None, which.data_ptr() if (which is not None and J) else None,
                   J, thr.ctypes.data_as(_abi.c_float_p), sep,
                   events.data_ptr() if events.numel() else None, cap, counts.data_ptr() if D else None,
                   ev_scores.data_ptr() if (withScores and ev_scores.numel()) else None,
                   ev_templ.data_ptr() if (ev_templ is not None and ev_templ.numel() and J) else None,
                   det._stream_ptr(stream)))
        return events, counts, ev_scores, ev_templ

    def find(self, cols, thresholds, separation, stream=None):
        """scores() and peaks() -> (events, eventScores, eventTemplates): three lists with, a class, a list with one array a
        detector (int64, float32, int32), every match of it (the tables are made again with the largest count as capacity where the
        first capacity was too small)."""
        s, w = self.scores(cols, which=True, stream=stream)
        ev, cnt, es, et = self.peaks(s, thresholds, separation, which=w, stream=stream)
        c = cnt.cpu().numpy()
        if c.size and int(c.max()) > ev.shape[2]:
            ev, cnt, es, et = self.peaks(s, thresholds, separation, capacity=int(c.max()), which=w, stream=stream)
            c = cnt.cpu().numpy()
        ev, es, et = ev.cpu().numpy(), es.cpu().numpy(), et.cpu().numpy()
        per = lambda a: [[a[k, d, :c[k, d]].copy() for d in range(self.count)] for k in range(self.nClasses)]
        return per(ev), per(es), per(et)


def matchClassesHost(templateScores, classes=None):
    """syldet_match_classes_host: template scores [K, positions] float32 -> (class scores [C, positions] float32, which [C,
    positions] int32): a class's score is the greatest of its templates', taken in ascending k and replaced only where greater, so
    which is the lowest template that attains it, -1 where every one is NaN.  classes None: template k is class k."""
    s = np.ascontiguousarray(templateScores, dtype=np.float32)
    if s.ndim != 2:
        raise ValueError("templateScores must be [templates, positions]")
    cls, Cn = None, s.shape[0]
    if classes is not None:
        cls = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1)
        if cls.size != s.shape[0]:
            raise ValueError("one class per template")
        Cn = int(cls.max()) + 1 if cls.size else 0
    out = np.empty((max(Cn, 0), s.shape[1]), np.float32)
    which = np.empty((max(Cn, 0), s.shape[1]), np.int32)
    check(_abi.lib.syldet_match_classes_host(s.ctypes.data_as(_abi.c_float_p), s.shape[1], s.shape[0],
                                             None if cls is None else cls.ctypes.data_as(_abi.c_int32_p), Cn if cls is not None else 0,
                                             out.ctypes.data_as(_abi.c_float_p), which.ctypes.data_as(_abi.c_int32_p)))
    return out, which


def matchNormalizeHost(template):
    """syldet_match_normalize_host: t^ = float32(t / ||t||_2) of a template [frames, bins], norm and division in float64."""
    t = np.ascontiguousarray(template, dtype=np.float32)
    if t.ndim != 2:
        raise ValueError("the template must be [frames, bins]")
    out = np.empty_like(t)
    check(_abi.lib.syldet_match_normalize_host(t.ctypes.data_as(_abi.c_float_p), t.shape[0], t.shape[1], out.ctypes.data_as(_abi.c_float_p)))
    return out


def matchScoresHost(templateHat, cols):
    """syldet_match_scores_host: one detector's scores on the host, no device needed.  templateHat [n, bins] (a Matcher's
    .template, or matchNormalizeHost's), cols [n_frames, bins] float32 -> scores [n_frames] float32, NaN in the last n - 1."""
    t = np.ascontiguousarray(templateHat, dtype=np.float32)
    x = np.ascontiguousarray(cols, dtype=np.float32)
    if t.ndim != 2 or x.ndim != 2 or x.shape[1] != t.shape[1]:
        raise ValueError("templateHat must be [n, bins] and cols [n_frames, bins]")
    out = np.empty(x.shape[0], np.float32)
    check(_abi.lib.syldet_match_scores_host(t.ctypes.data_as(_abi.c_float_p), t.shape[0], t.shape[1], x.ctypes.data_as(_abi.c_float_p), x.shape[0],
                                            out.ctypes.data_as(_abi.c_float_p)))
    return out


def matchPeaksHost(scores, threshold: float, separation: int, origin: int, hop: int, anchor: int, capacity: Optional[int] = None):
    """syldet_match_peaks_host: one detector's matches on the host, no device needed.  scores [positions] float32 -> (events
    int64 [min(count, capacity)], count, eventScores float32): the rule and the event number the kernel runs."""
    s = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    cap = s.size if capacity is None else int(capacity)
    events = np.zeros(max(cap, 0), np.int64)
    ev_scores = np.zeros(max(cap, 0), np.float32)
    n = C.c_int64()
    check(_abi.lib.syldet_match_peaks_host(s.ctypes.data_as(_abi.c_float_p), s.size, float(threshold), int(separation), int(origin), int(hop), int(anchor),
                                           events.ctypes.data_as(_abi.c_int64_p), cap, C.byref(n), ev_scores.ctypes.data_as(_abi.c_float_p)))
    k = min(int(n.value), max(cap, 0))
    return events[:k], int(n.value), ev_scores[:k]


def _train_label_args(labels, labelOutputs):
    """(flat labels, begin, flat outputs or None) of per-detector lists"""
    _, flat, begin = _score_args([0.0], labels)
    if labelOutputs is None:
        return flat, begin, None
    outs = [np.ascontiguousarray(o, dtype=np.int32).reshape(-1) for o in labelOutputs]
    if len(outs) != len(begin) - 1 or any(o.size != n for o, n in zip(outs, np.diff(begin))):
        raise ValueError("labelOutputs must hold one output per label, detector by detector")
    return flat, begin, np.ascontiguousarray(np.concatenate(outs) if outs else np.zeros(0, np.int32), dtype=np.int32)


class _TrainerHandle:
    """What Trainer and MultiTrainer share: the handle's life, the targets and the checks of the device arrays.  A subclass sets
    detector, recordings, _h, count, paramCount, outputs and _paramsShape."""

    def close(self):
        if getattr(self, "_h", None):
            _abi.lib.syldet_trainer_destroy(self._h)
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

    def _shape(self):
        d, p, o, tile = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
        check(_abi.lib.syldet_trainer_shape(self._h, C.byref(d), C.byref(p), C.byref(o), C.byref(tile)))
        self.count, self.paramCount, self.outputs, self.tile = d.value, p.value, o.value, tile.value

    # ---- targets ----
    def _n_evals(self, n_evals):
        if self.recordings is not None:
            return self.recordings.rowEvaluations
        if n_evals is None:
            raise ValueError("n_evals is needed on a bank's channels")
        return int(n_evals)

    def targets(self, labels, halfWidth: int, weightPositive: float, weightNegative: float, labelOutputs=None, n_evals: Optional[int] = None,
                stream=None):
        """labels: a list of arrays, one per detector, of sorted labelled sample numbers (the scorer's); labelOutputs: each label's
        output (default all 0) -> (targets [C, n_evals, O], weights [C, n_evals]) float32 on the device: a target is 1 within
        halfWidth samples of a label of its output, an evaluation's weight weightPositive where any target is 1, else
        weightNegative, and 0 wherever no detector is.  n_evals: evaluations a row (recordings: theirs).  One launch."""
        torch = _torch()
        det = self.detector
        labels = list(labels)
        if len(labels) != self.count:
            raise ValueError("one array of labels per detector (%d given, %d detectors)" % (len(labels), self.count))
        flat, begin, outs = _train_label_args(labels, labelOutputs)
        E = self._n_evals(n_evals)
        dev = "cuda:%d" % det.device
        t = torch.empty((det.channels, E, self.outputs), dtype=torch.float32, device=dev)
        w = torch.empty((det.channels, E), dtype=torch.float32, device=dev)
        check(_abi.lib.syldet_train_targets_device(self._h, flat.ctypes.data_as(_abi.c_int64_p), begin.ctypes.data_as(_abi.c_int64_p),
                                                   None if outs is None else outs.ctypes.data_as(_abi.c_int32_p), int(halfWidth), float(weightPositive),
                                                   float(weightNegative), E, t.data_ptr(), w.data_ptr(), det._stream_ptr(stream)))
        return t, w

    # ---- the device arrays of a gradient or a fit ----
    def _check(self, cols, params, targets, weights):
        torch = _torch()
        det = self.detector
        bins = det.geometry.bins

        def ok(x, dims):
            return x.is_cuda and x.dtype == torch.float32 and x.dim() == dims and x.is_contiguous() and x.device.index == det.device

        if not (ok(cols, 3) and cols.shape[0] == det.channels and cols.shape[2] == bins):
            raise ValueError("cols must be a contiguous float32 CUDA tensor [channels, n_frames, %d] on the detector's device" % bins)
        if not (ok(params, len(self._paramsShape)) and tuple(params.shape) == self._paramsShape):
            raise ValueError("params must be a contiguous float32 CUDA tensor %s" % (list(self._paramsShape),))
        if not (ok(weights, 2) and weights.shape[0] == det.channels):
            raise ValueError("weights must be a contiguous float32 CUDA tensor [channels, n_evals]")
        if not (ok(targets, 3) and tuple(targets.shape) == (det.channels, weights.shape[1], self.outputs)):
            raise ValueError("targets must be a contiguous float32 CUDA tensor [channels, n_evals, %d]" % self.outputs)


class Trainer(_TrainerHandle):
    """Training (syldet_trainer_*, include/syldet.h "training"): loss and gradient of a two-layer network's parameters over
    weighted, labelled evaluations, straight from the columns.  A detector is a channel of the bank, or (made by
    Recordings.trainer) a recording.  shape = (detectors, parameters, outputs); the parameters are one flat float32 vector,
    layer0.weights [H][I], layer0.biases [H], layer1.weights [O][H], layer1.biases [O]; everything else of the network is the
    bank's configuration's.  The optimiser is torch's.  The detector (and the Recordings) must outlive it."""

    def __init__(self, detector: SyllableDetector, recordings: Optional[Recordings] = None):
        self.detector = detector
        self.recordings = recordings
        self._h = _abi.Handle()
        check(_abi.lib.syldet_trainer_create(detector._h, None if recordings is None else recordings._h, C.byref(self._h)))
        self._shape()
        self.shape = (self.count, self.paramCount, self.outputs)
        self._paramsShape = (self.paramCount,)

    # ---- parameters <-> configuration ----
    def params(self, config: Optional[SyllableDetectorConfig] = None):
        """The flat float32 parameter vector of a configuration's two layers (default: the bank's), on the detector's device."""
        torch = _torch()
        layers = (config or self.detector.config).net.layers
        flat = np.concatenate([np.asarray(a, np.float32).reshape(-1) for L in layers for a in (L.weights, L.biases)])
        if len(layers) != 2 or flat.size != self.paramCount:
            raise ValueError("the configuration's layers do not have the trainer's %d parameters" % self.paramCount)
        return torch.from_numpy(flat).to("cuda:%d" % self.detector.device)

    def configWith(self, params) -> SyllableDetectorConfig:
        """A deep copy of the bank's configuration with the two layers' weights and biases replaced by `params`."""
        import copy
        p = (params.detach().cpu().numpy() if hasattr(params, "detach") else np.asarray(params)).astype(np.float32).reshape(-1)
        if p.size != self.paramCount:
            raise ValueError("params must hold %d values" % self.paramCount)
        cfg = copy.deepcopy(self.detector.config)
        at = 0
        for L in cfg.net.layers:
            L.weights = p[at:at + L.outputs * L.inputs].reshape(L.outputs, L.inputs).copy()
            at += L.outputs * L.inputs
            L.biases = p[at:at + L.outputs].copy()
            at += L.outputs
        return cfg

    # ---- loss and gradient ----
    def gradient(self, cols, params, targets, weights, out=None, stream=None):
        """cols [C, n_frames, bins] as spectrogram() wrote them, params [P], targets and weights as targets() made them (or any
        others of those shapes) -> (loss, weightSum, grad): two 0-dim float64 tensors -- the sum over the selected evaluations
        (weight > 0) of w sum_o (y - t)^2, and the sum of their weights -- and dloss/dparams [P] float32, on the device.  Launches
        only, the same bits for the same arrays.  out: a (float64 [2], float32 [P]) pair to write into.  Asynchronous on `stream`."""
        torch = _torch()
        self._check(cols, params, targets, weights)
        if out is None:
            out = (torch.empty(2, dtype=torch.float64, device=cols.device), torch.empty(self.paramCount, dtype=torch.float32, device=cols.device))
        loss, grad = out
        if not (loss.is_cuda and loss.dtype == torch.float64 and loss.numel() == 2 and loss.is_contiguous() and grad.is_cuda
                and grad.dtype == torch.float32 and grad.numel() == self.paramCount and grad.is_contiguous()):
            raise ValueError("out must be a (float64 [2], float32 [%d]) pair of contiguous CUDA tensors" % self.paramCount)
        check(_abi.lib.syldet_train_gradient_device(self._h, cols.data_ptr(), int(cols.shape[1]), 0, params.data_ptr(), targets.data_ptr(),
                                                    weights.data_ptr(), int(weights.shape[1]), loss.data_ptr(), grad.data_ptr(),
                                                    self.detector._stream_ptr(stream)))
        return loss[0], loss[1], grad

    def fit(self, cols, targets, weights, params, steps: int, lr: float = 0.01):
        """`steps` full-batch steps of torch.optim.Adam on the mean loss L / Wsum, from `params`: a leaf tensor whose .grad the
        library fills.  -> (params [P] float32 on the device, the mean loss in front of every step as a list of floats)."""
        torch = _torch()
        p = params.detach().clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=lr)
        out = (torch.empty(2, dtype=torch.float64, device=cols.device), torch.empty(self.paramCount, dtype=torch.float32, device=cols.device))
        history = []
        for _ in range(int(steps)):
            loss, wsum, grad = self.gradient(cols, p.detach(), targets, weights, out=out)
            scale = torch.where(wsum > 0, 1.0 / wsum, torch.zeros_like(wsum))
            history.append(loss * scale)
            p.grad = (grad * scale.to(torch.float32))
            opt.step()
        history = torch.stack(history).cpu().tolist() if history else []
        return p.detach(), history

    # ---- training from the tool: the input map, the optimiser, the fit (include/syldet.h "training from the tool") ----
    def inputRange(self, cols, weights, stream=None):
        """syldet_train_input_range_device: per input position the least and the greatest value behind the input functions in front
        of the first mapminmax, over the evaluations with weight > 0 whose values there are all finite -> (range [2, I] float32,
        count: a 0-dim int64 tensor), on the device.  Two launches."""
        torch = _torch()
        det = self.detector
        I = det.geometry.inputs
        ok = lambda x, dims: x.is_cuda and x.dtype == torch.float32 and x.dim() == dims and x.is_contiguous() and x.device.index == det.device
        if not (ok(cols, 3) and cols.shape[0] == det.channels and cols.shape[2] == det.geometry.bins):
            raise ValueError("cols must be a contiguous float32 CUDA tensor [channels, n_frames, %d] on the detector's device" % det.geometry.bins)
        if not (ok(weights, 2) and weights.shape[0] == det.channels):
            raise ValueError("weights must be a contiguous float32 CUDA tensor [channels, n_evals]")
        rng = torch.empty((2, I), dtype=torch.float32, device=cols.device)
        count = torch.empty(1, dtype=torch.int64, device=cols.device)
        check(_abi.lib.syldet_train_input_range_device(self._h, cols.data_ptr(), int(cols.shape[1]), 0, weights.data_ptr(), int(weights.shape[1]),
                                                       rng.data_ptr(), count.data_ptr(), det._stream_ptr(stream)))
        return rng, count[0]

    def setInputMap(self, xOffsets, gains, y: float = -1.0) -> None:
        """syldet_trainer_set_input_map: replaces the first mapminmax's parameters in the trainer's own tables (host arrays [I]);
        later gradient, range and fit calls use them.  Waits for the trainer's last call."""
        I = self.detector.geometry.inputs
        xo = np.ascontiguousarray(xOffsets, dtype=np.float32).reshape(-1)
        g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        if xo.size != I or g.size != I:
            raise ValueError("xOffsets and gains must hold %d values each" % I)
        check(_abi.lib.syldet_trainer_set_input_map(self._h, xo.ctypes.data_as(_abi.c_float_p), g.ctypes.data_as(_abi.c_float_p), float(y)))

    def inputMap(self):
        """syldet_trainer_input_map -> (xOffsets [I], gains [I], y, the function's index in the input chain)"""
        I = self.detector.geometry.inputs
        xo, g = np.zeros(I, np.float32), np.zeros(I, np.float32)
        y, at = C.c_float(), C.c_int32()
        check(_abi.lib.syldet_trainer_input_map(self._h, C.byref(at), xo.ctypes.data_as(_abi.c_float_p), g.ctypes.data_as(_abi.c_float_p), C.byref(y)))
        return xo, g, float(y.value), int(at.value)

    def adamStep(self, params, loss, grad, step: int, lr: float = 0.01, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, stream=None):
        """syldet_train_adam_device: step number `step` (from 1) of Adam on params [P] IN PLACE, on the moments the trainer keeps,
        from loss (float64 [2]: L, Wsum) and grad [P] as gradient(out=...) left them -> the mean loss L / Wsum, a 0-dim float64
        tensor.  One launch."""
        torch = _torch()
        ok = lambda x, dt, n: x.is_cuda and x.dtype == dt and x.numel() == n and x.is_contiguous() and x.device.index == self.detector.device
        if not (ok(params, torch.float32, self.paramCount) and ok(grad, torch.float32, self.paramCount) and ok(loss, torch.float64, 2)):
            raise ValueError("params and grad must be contiguous float32 CUDA tensors of %d values, loss float64 [2]" % self.paramCount)
        mean = torch.empty(1, dtype=torch.float64, device=params.device)
        check(_abi.lib.syldet_train_adam_device(self._h, params.data_ptr(), loss.data_ptr(), grad.data_ptr(), int(step), float(lr), float(beta1), float(beta2),
                                                float(eps), mean.data_ptr(), self.detector._stream_ptr(stream)))
        return mean[0]

    def fitDevice(self, cols, targets, weights, params, steps: int, lr: float = 0.01, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                  stream=None):
        """syldet_train_fit_device: `steps` full-batch Adam steps on the mean loss, enqueued as 3 x steps launches -> (params [P]: a
        copy of `params` after the steps, history: float64 [steps] on the device, the mean loss in front of every step)."""
        torch = _torch()
        self._check(cols, params, targets, weights)
        p = params.detach().clone()
        history = torch.empty(max(int(steps), 0), dtype=torch.float64, device=cols.device)
        check(_abi.lib.syldet_train_fit_device(self._h, cols.data_ptr(), int(cols.shape[1]), 0, targets.data_ptr(), weights.data_ptr(), int(weights.shape[1]),
                                               p.data_ptr(), int(steps), float(lr), float(beta1), float(beta2), float(eps), history.data_ptr(),
                                               self.detector._stream_ptr(stream)))
        return p, history

    def fitInputMap(self, cols, events, chunk: int = 1 << 16) -> SyllableDetectorConfig:
        """Refits the configuration's first mapminmax input function to data, as the MATLAB side does before it trains: the
        network inputs at `events` (a list of arrays of sample numbers, one per detector; an event's input is the evaluation it
        anchors, and an event whose input is not whole is left out) are cut with an Aligner (before = timeRange - 1, after = 0,
        `chunk` events at a time), the functions in front of the map are applied with torch, and per input position
        xOffsets = min, gains = 2 / (max - min) (1 where they are equal), yMin = -1.  -> a new configuration."""
        import copy
        torch = _torch()
        det = self.detector
        cfg = copy.deepcopy(det.config)
        fns = cfg.net.inputProcessing
        at = next((k for k, f in enumerate(fns) if f.function == "mapminmax"), None)
        if at is None:
            raise ValueError("the configuration has no mapminmax input function")
        events = [np.ascontiguousarray(e, dtype=np.int64).reshape(-1) for e in events]
        if len(events) != self.count:
            raise ValueError("one array of events per detector (%d given, %d detectors)" % (len(events), self.count))
        T = int(cfg.timeRange)
        lo = hi = None
        with Aligner(det, "columns", T - 1, 0, recordings=self.recordings) as al:
            longest = max([e.size for e in events] + [0])
            for c0 in range(0, longest, max(int(chunk) // max(self.count, 1), 1)):
                part = [e[c0:c0 + max(int(chunk) // max(self.count, 1), 1)] for e in events]
                x = al.windows(cols, part, fill=float("nan")).reshape(-1, T * det.geometry.bins)
                x = x[~torch.isnan(x).any(dim=1)]
                if x.shape[0] == 0:
                    continue
                if cfg.spectrogramScaling == "log":
                    x = torch.log(x)
                elif cfg.spectrogramScaling == "db":
                    x = 20.0 * torch.log10(x)
                for f in fns[:at]:
                    if f.function == "l2normalize":
                        x = x / torch.sqrt((x * x).sum(dim=1, keepdim=True))
                    elif f.function == "normalize":
                        mn, mx = x.min(dim=1, keepdim=True).values, x.max(dim=1, keepdim=True).values
                        x = torch.where(mx > mn, (x - mn) * (2.0 / (mx - mn)) - 1.0, torch.full_like(x, -1.0))
                    elif f.function == "normalizestd":
                        x = (x - x.mean(dim=1, keepdim=True)) / x.std(dim=1, unbiased=False, keepdim=True)
                    else:
                        x = (x - torch.from_numpy(np.asarray(f.xOffsets, np.float32)).to(x.device)) * torch.from_numpy(np.asarray(f.gains, np.float32)).to(x.device) + float(f.y)
                x = x[torch.isfinite(x).all(dim=1)]
                if x.shape[0] == 0:
                    continue
                mn, mx = x.min(dim=0).values, x.max(dim=0).values
                lo = mn if lo is None else torch.minimum(lo, mn)
                hi = mx if hi is None else torch.maximum(hi, mx)
        if lo is None:
            raise ValueError("no event has a whole network input")
        lo, hi = lo.cpu().numpy().astype(np.float32), hi.cpu().numpy().astype(np.float32)
        rng = hi - lo
        fns[at].xOffsets = lo
        fns[at].gains = np.where(rng > 0, np.float32(2.0) / np.where(rng > 0, rng, 1), np.float32(1.0)).astype(np.float32)
        fns[at].y = -1.0
        return cfg


class MultiTrainer(_TrainerHandle):
    """A network per channel (syldet_trainer_create_multi, include/syldet.h "training a network per channel"): ONE trainer for the
    N networks of a SyllableDetector.multi bank (or of a plain bank, N = 1).  Row r trains network rowNetwork[r] -- with
    Recordings, a recording the network of the row it was planned onto -- and network n's loss, gradient, range, Adam step and
    fit are bit for bit a plain Trainer's on a plain bank of that network over those rows alone.  shape = (detectors, networks,
    parameters, outputs); params, gradients and moments are [N, P].  The detector (and the Recordings) must outlive it."""

    def __init__(self, detector: SyllableDetector, recordings: Optional[Recordings] = None):
        self.detector = detector
        self.recordings = recordings
        self._h = _abi.Handle()
        check(_abi.lib.syldet_trainer_create_multi(detector._h, None if recordings is None else recordings._h, C.byref(self._h)))
        self._shape()
        n = C.c_int32()
        rows = np.zeros(detector.channels, np.int32)
        check(_abi.lib.syldet_trainer_networks(self._h, C.byref(n), rows.ctypes.data_as(_abi.c_int32_p)))
        self.networks, self.rowNetwork = int(n.value), rows
        self.shape = (self.count, self.networks, self.paramCount, self.outputs)
        self._paramsShape = (self.networks, self.paramCount)
        self.configs = list(getattr(detector, "configs", None) or [detector.config])
        if len(self.configs) != self.networks:
            raise ValueError("the detector holds %d configurations for %d networks" % (len(self.configs), self.networks))

    def groups(self, n_evals: int) -> np.ndarray:
        """syldet_trainer_groups: the workgroups G_n each network gets for n_evals evaluations a row, int32 [N] (host only)."""
        g = np.zeros(self.networks, np.int32)
        check(_abi.lib.syldet_trainer_groups(self._h, int(n_evals), g.ctypes.data_as(_abi.c_int32_p)))
        return g

    # ---- parameters <-> configurations ----
    def params(self, configs=None):
        """The networks' flat float32 parameter vectors [N, P] (default: the bank's own configurations), on the detector's device."""
        torch = _torch()
        configs = list(configs) if configs is not None else self.configs
        if len(configs) != self.networks:
            raise ValueError("one configuration per network (%d given, %d networks)" % (len(configs), self.networks))
        flat = []
        for cfg in configs:
            flat.append(np.concatenate([np.asarray(a, np.float32).reshape(-1) for L in cfg.net.layers for a in (L.weights, L.biases)]))
            if len(cfg.net.layers) != 2 or flat[-1].size != self.paramCount:
                raise ValueError("a configuration's layers do not have the trainer's %d parameters" % self.paramCount)
        return torch.from_numpy(np.stack(flat)).to("cuda:%d" % self.detector.device)

    def configsWith(self, params) -> List[SyllableDetectorConfig]:
        """One syldet_train_config_with per network: network n's configuration with its two layers replaced by params[n] and,
        where it has a mapminmax input function, that function's parameters by the trainer's own (inputMap(n))."""
        p = np.ascontiguousarray((params.detach().cpu().numpy() if hasattr(params, "detach") else np.asarray(params)), dtype=np.float32)
        if p.shape != (self.networks, self.paramCount):
            raise ValueError("params must be [%d, %d]" % (self.networks, self.paramCount))
        has_map = any(f.function == "mapminmax" for f in self.configs[0].net.inputProcessing)
        out = []
        fp = lambda a: a.ctypes.data_as(_abi.c_float_p)
        for n, cfg in enumerate(self.configs):
            c, keep = cfg.to_abi()
            made = _abi.Config_p()
            if has_map:
                xo, g, y, _ = self.inputMap(n)
                check(_abi.lib.syldet_train_config_with(C.byref(c), fp(p[n]), self.paramCount, fp(xo), fp(g), float(y), C.byref(made)))
            else:
                check(_abi.lib.syldet_train_config_with(C.byref(c), fp(p[n]), self.paramCount, None, None, 0.0, C.byref(made)))
            del keep
            try:
                out.append(SyllableDetectorConfig._from_abi(made.contents))
            finally:
                _abi.lib.syldet_config_free(made)
        return out

    # ---- loss and gradient ----
    def gradient(self, cols, params, targets, weights, out=None, stream=None):
        """Trainer.gradient for every network at once: params [N, P] -> (loss [N], weightSum [N]) float64 and grad [N, P] float32 on
        the device, network n's over its own rows alone.  out: a (float64 [N, 2], float32 [N, P]) pair.  Two launches."""
        torch = _torch()
        self._check(cols, params, targets, weights)
        N, P = self.networks, self.paramCount
        if out is None:
            out = (torch.empty((N, 2), dtype=torch.float64, device=cols.device), torch.empty((N, P), dtype=torch.float32, device=cols.device))
        loss, grad = out
        if not (loss.is_cuda and loss.dtype == torch.float64 and tuple(loss.shape) == (N, 2) and loss.is_contiguous() and grad.is_cuda
                and grad.dtype == torch.float32 and tuple(grad.shape) == (N, P) and grad.is_contiguous()):
            raise ValueError("out must be a (float64 [%d, 2], float32 [%d, %d]) pair of contiguous CUDA tensors" % (N, N, P))
        check(_abi.lib.syldet_train_gradient_device(self._h, cols.data_ptr(), int(cols.shape[1]), 0, params.data_ptr(), targets.data_ptr(),
                                                    weights.data_ptr(), int(weights.shape[1]), loss.data_ptr(), grad.data_ptr(),
                                                    self.detector._stream_ptr(stream)))
        return loss[:, 0], loss[:, 1], grad

    def inputRange(self, cols, weights, stream=None):
        """Trainer.inputRange per network -> (range [N, 2, I] float32, count [N] int64), on the device.  Two launches."""
        torch = _torch()
        det = self.detector
        I = det.geometry.inputs
        ok = lambda x, dims: x.is_cuda and x.dtype == torch.float32 and x.dim() == dims and x.is_contiguous() and x.device.index == det.device
        if not (ok(cols, 3) and cols.shape[0] == det.channels and cols.shape[2] == det.geometry.bins):
            raise ValueError("cols must be a contiguous float32 CUDA tensor [channels, n_frames, %d] on the detector's device" % det.geometry.bins)
        if not (ok(weights, 2) and weights.shape[0] == det.channels):
            raise ValueError("weights must be a contiguous float32 CUDA tensor [channels, n_evals]")
        rng = torch.empty((self.networks, 2, I), dtype=torch.float32, device=cols.device)
        count = torch.empty(self.networks, dtype=torch.int64, device=cols.device)
        check(_abi.lib.syldet_train_input_range_device(self._h, cols.data_ptr(), int(cols.shape[1]), 0, weights.data_ptr(), int(weights.shape[1]),
                                                       rng.data_ptr(), count.data_ptr(), det._stream_ptr(stream)))
        return rng, count

    def setInputMap(self, net: int, xOffsets, gains, y: float = -1.0) -> None:
        """syldet_trainer_set_input_map_of: Trainer.setInputMap for network `net`."""
        I = self.detector.geometry.inputs
        xo = np.ascontiguousarray(xOffsets, dtype=np.float32).reshape(-1)
        g = np.ascontiguousarray(gains, dtype=np.float32).reshape(-1)
        if xo.size != I or g.size != I:
            raise ValueError("xOffsets and gains must hold %d values each" % I)
        check(_abi.lib.syldet_trainer_set_input_map_of(self._h, int(net), xo.ctypes.data_as(_abi.c_float_p), g.ctypes.data_as(_abi.c_float_p), float(y)))

    def inputMap(self, net: int = 0):
        """syldet_trainer_input_map_of -> (xOffsets [I], gains [I], y, the function's index in the input chain) of network `net`"""
        I = self.detector.geometry.inputs
        xo, g = np.zeros(I, np.float32), np.zeros(I, np.float32)
        y, at = C.c_float(), C.c_int32()
        check(_abi.lib.syldet_trainer_input_map_of(self._h, int(net), C.byref(at), xo.ctypes.data_as(_abi.c_float_p), g.ctypes.data_as(_abi.c_float_p),
                                                   C.byref(y)))
        return xo, g, float(y.value), int(at.value)

    def adamStep(self, params, loss, grad, step: int, lr: float = 0.01, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, stream=None):
        """syldet_train_adam_device on params [N, P] IN PLACE from loss (float64 [N, 2]) and grad [N, P] as gradient(out=...) left
        them; 1 / Wsum is each network's own -> the mean losses, float64 [N].  One launch."""
        torch = _torch()
        N, P = self.networks, self.paramCount
        ok = lambda x, dt, n: x.is_cuda and x.dtype == dt and x.numel() == n and x.is_contiguous() and x.device.index == self.detector.device
        if not (ok(params, torch.float32, N * P) and ok(grad, torch.float32, N * P) and ok(loss, torch.float64, 2 * N)):
            raise ValueError("params and grad must be contiguous float32 CUDA tensors [%d, %d], loss float64 [%d, 2]" % (N, P, N))
        mean = torch.empty(N, dtype=torch.float64, device=params.device)
        check(_abi.lib.syldet_train_adam_device(self._h, params.data_ptr(), loss.data_ptr(), grad.data_ptr(), int(step), float(lr), float(beta1), float(beta2),
                                                float(eps), mean.data_ptr(), self.detector._stream_ptr(stream)))
        return mean

    def fitDevice(self, cols, targets, weights, params, steps: int, lr: float = 0.01, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                  stream=None):
        """syldet_train_fit_device for every network at once: 3 x steps launches -> (params [N, P]: a copy of `params` after the
        steps, history: float64 [steps, N] on the device, each network's mean loss in front of every step)."""
        torch = _torch()
        self._check(cols, params, targets, weights)
        p = params.detach().clone()
        history = torch.empty((max(int(steps), 0), self.networks), dtype=torch.float64, device=cols.device)
        check(_abi.lib.syldet_train_fit_device(self._h, cols.data_ptr(), int(cols.shape[1]), 0, targets.data_ptr(), weights.data_ptr(), int(weights.shape[1]),
                                               p.data_ptr(), int(steps), float(lr), float(beta1), float(beta2), float(eps), history.data_ptr(),
                                               self.detector._stream_ptr(stream)))
        return p, history


def trainInputMapHost(rng):
    """syldet_train_input_map_host: range [2, I] -> (xOffsets [I], gains [I]) float32: xOffsets = least, gains = 2 / (greatest - least)
    in float32, 1 where they are equal; yMin is -1."""
    r = np.ascontiguousarray(rng, dtype=np.float32)
    if r.ndim != 2 or r.shape[0] != 2:
        raise ValueError("range must be [2, I]")
    I = r.shape[1]
    xo, g = np.zeros(I, np.float32), np.zeros(I, np.float32)
    check(_abi.lib.syldet_train_input_map_host(r.ctypes.data_as(_abi.c_float_p), I, xo.ctypes.data_as(_abi.c_float_p), g.ctypes.data_as(_abi.c_float_p)))
    return xo, g


def trainAdamHost(params, m, v, grad, loss, step: int, lr: float = 0.01, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
    """syldet_train_adam_host: one Adam step in the kernel's own text on float32 host arrays -> (params, m, v, mean loss); the
    arguments are not changed."""
    p, m, v = (np.array(a, dtype=np.float32).reshape(-1) for a in (params, m, v))
    g = np.ascontiguousarray(grad, dtype=np.float32).reshape(-1)
    l = np.ascontiguousarray(loss, dtype=np.float64).reshape(-1)
    if not (p.size == m.size == v.size == g.size) or l.size != 2:
        raise ValueError("params, m, v and grad must have one size, loss two values")
    mean = C.c_double()
    fp = lambda a: a.ctypes.data_as(_abi.c_float_p)
    check(_abi.lib.syldet_train_adam_host(fp(p), fp(m), fp(v), fp(g), p.size, l.ctypes.data_as(_abi.c_double_p), int(step), float(lr), float(beta1), float(beta2),
                                          float(eps), C.byref(mean)))
    return p, m, v, float(mean.value)


def trainInitHost(seed: int, inputs: int, hidden: int, outputs: int) -> np.ndarray:
    """syldet_train_init_host: the seeded starting parameters [H I + H + O H + O] float32 of an (I, H, O) network."""
    theta = np.zeros(max(int(hidden) * int(inputs) + int(hidden) + int(outputs) * int(hidden) + int(outputs), 1), np.float32)
    check(_abi.lib.syldet_train_init_host(int(seed) & 0xFFFFFFFFFFFFFFFF, int(inputs), int(hidden), int(outputs), theta.ctypes.data_as(_abi.c_float_p)))
    return theta


def trainParamCount(config: SyllableDetectorConfig) -> int:
    """syldet_train_param_count: the parameters H I + H + O H + O of a configuration of two layers, no device needed."""
    c, keep = config.to_abi()
    n = C.c_int64()
    check(_abi.lib.syldet_train_param_count(C.byref(c), C.byref(n)))
    del keep
    return int(n.value)


def trainTargetsHost(labels, n_evals: int, halfWidth: int, weightPositive: float, weightNegative: float, firstIndex: int, hop: int, outputs: int = 1,
                     labelOutputs=None):
    """syldet_train_targets_host: one detector's targets on the host, no device needed -> (targets [n_evals, outputs],
    weights [n_evals]) float32."""
    flat, _, outs = _train_label_args([labels], None if labelOutputs is None else [labelOutputs])
    t = np.zeros((max(int(n_evals), 0), max(int(outputs), 0)), np.float32)
    w = np.zeros(max(int(n_evals), 0), np.float32)
    check(_abi.lib.syldet_train_targets_host(flat.ctypes.data_as(_abi.c_int64_p), flat.size, None if outs is None else outs.ctypes.data_as(_abi.c_int32_p),
                                             int(outputs), int(halfWidth), float(weightPositive), float(weightNegative), int(firstIndex), int(hop),
                                             int(n_evals), t.ctypes.data_as(_abi.c_float_p), w.ctypes.data_as(_abi.c_float_p)))
    return t, w


def _pcm16(data) -> np.ndarray:
    """16-bit PCM as given: an int16 array (never a cast -- a float recording is not PCM)."""
    a = np.asarray(data)
    if a.dtype != np.int16:
        raise ValueError("16-bit PCM must be an int16 array (got %s)" % a.dtype)
    return a


def configsCompatible(a: SyllableDetectorConfig, b: SyllableDetectorConfig) -> Tuple[bool, Optional[str]]:
    """syldet_config_compatible: may a and b share one SyllableDetector.multi bank?  (True, None), or (False, the first field
    that differs)."""
    ca, ka = a.to_abi()
    cb, kb = b.to_abi()
    field = C.c_char_p()
    r = check(_abi.lib.syldet_config_compatible(C.byref(ca), C.byref(cb), C.byref(field)))
    del ka, kb
    return (True, None) if r == 1 else (False, field.value.decode() if field.value else None)


def configsShareClock(a: SyllableDetectorConfig, b: SyllableDetectorConfig) -> Tuple[bool, Optional[str]]:
    """syldet_config_same_clock: may a and b share one SyllableDetector.mixed bank?  (True, None), or (False, the first clock
    field that differs)."""
    ca, ka = a.to_abi()
    cb, kb = b.to_abi()
    field = C.c_char_p()
    r = check(_abi.lib.syldet_config_same_clock(C.byref(ca), C.byref(cb), C.byref(field)))
    del ka, kb
    return (True, None) if r == 1 else (False, field.value.decode() if field.value else None)


def fusedFormOfConfig(configs, channels: int, n_samples: int, channelNetworks=None, s16: bool = False, spectrogram: bool = False,
                      engine: int = _abi.ENGINE_AUTO):
    """syldet_fused_form_of_config: (kernel, template arguments) of the fused kernel instantiation a detector of `configs` (one
    configuration, or a list with channelNetworks: SyllableDetector.multi's) would run for a batch of n_samples per channel --
    from the host alone, no device needed; raises SyllableDetectorError (unsupported) for what is not on the fused engine."""
    configs = [configs] if isinstance(configs, SyllableDetectorConfig) else list(configs)
    abi = [cfg.to_abi() for cfg in configs]
    ptrs = (_abi.Config_p * max(1, len(abi)))(*[C.pointer(c) for c, _ in abi])
    nets = None if channelNetworks is None else np.ascontiguousarray(channelNetworks, dtype=np.int32).reshape(-1)
    kernel, params = C.c_int32(), (C.c_int32 * 10)()
    check(_abi.lib.syldet_fused_form_of_config(ptrs, len(abi), None if nets is None else nets.ctypes.data_as(_abi.c_int32_p), int(channels),
                                               int(n_samples), 1 if s16 else 0, 1 if spectrogram else 0, int(engine), C.byref(kernel), params))
    del abi
    return int(kernel.value), tuple(int(v) for v in params)
