"""The numpy model of the files' own sample formats (include/syldet.h, "packed recordings: the files' own sample formats"; the
table of csrc/pcm_values.hpp), a maker of test bytes for every format, and a writer of the WAV files the library's own writer does
not make (8-, 24- and 32-bit PCM, 32- and 64-bit float).  Nothing here calls the library."""
import struct

import numpy as np

U8, S16, S24, S32, F32, F64 = 1, 2, 3, 4, 5, 6
FORMATS = (U8, S16, S24, S32, F32, F64)
BYTES = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4, F64: 8}
NAMES = {U8: "u8", S16: "s16", S24: "s24", S32: "s32", F32: "f32", F64: "f64"}


def decode(raw, fmt, n=None, step=None, offset=0):
    """float32 [n]: sample i is the `fmt` value at raw[offset + i * step] (raw: uint8; step None: contiguous; n None: all)."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    size = BYTES[fmt]
    step = size if step is None else step
    if n is None:
        n = 0 if raw.size - offset < size else (raw.size - offset - size) // step + 1
    if n == 0:
        return np.zeros(0, np.float32)
    at = offset + np.arange(n, dtype=np.int64)[:, None] * step + np.arange(size)[None, :]
    assert at.max() < raw.size
    b = raw[at]                                                   # [n, size]
    if fmt == U8:
        return ((b[:, 0].astype(np.int32) - 128).astype(np.float32) * np.float32(2.0 ** -7)).astype(np.float32)
    if fmt == S16:
        return (np.ascontiguousarray(b).view("<i2")[:, 0].astype(np.float32) * np.float32(2.0 ** -15)).astype(np.float32)
    if fmt == S24:
        v = b[:, 0].astype(np.int32) | b[:, 1].astype(np.int32) << 8 | b[:, 2].astype(np.int32) << 16
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return (v.astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    if fmt == S32:
        v = np.ascontiguousarray(b).view("<i4")[:, 0]
        # (float32)((double)v / 2^31), as the tool's WAV reader writes it: the division is exact, the rounding is fp64 -> fp32
        return (v.astype(np.float64) / 2147483648.0).astype(np.float32)
    if fmt == F32:
        return np.ascontiguousarray(b).view("<f4")[:, 0].copy()
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.ascontiguousarray(b).view("<f8")[:, 0].astype(np.float32)


def same(a, b):
    """equal by bits, but for NaNs, which only have to be NaNs in the same places (a conversion may quieten one)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def samples(fmt, n, rng, special=True):
    """uint8 [n * size]: n contiguous samples of the format -- random bits for the integers, finite values of every magnitude for
    the floats -- with the format's own edge cases in front where there is room (F32: NaNs with payloads, an infinity, a
    subnormal; F64: 1e-40 (an fp32 subnormal), +-0, +-inf, a value that rounds to the fp32 infinity, a NaN)"""
    size = BYTES[fmt]
    if fmt in (U8, S16, S24, S32):
        raw = rng.integers(0, 256, size=n * size, dtype=np.uint8)
        edge = {U8: [0, 128, 255], S16: [-32768, 32767, -1], S24: [-(1 << 23), (1 << 23) - 1, -1], S32: [-(1 << 31), -(1 << 31) + 1, (1 << 31) - 1]}[fmt]
        if special:
            for i, v in enumerate(edge[:n]):
                raw[i * size:(i + 1) * size] = np.frombuffer(int(v & ((1 << 8 * size) - 1)).to_bytes(size, "little"), np.uint8)
        return raw
    if fmt == F32:
        x = (rng.uniform(0.1, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)).astype("<f4")
        bits = x.view("<u4")
        edge = [0x7FC12345, 0xFFA00001, 0x7F800001, 0x7F800000, 0x00000001, 0x80000000]      # quiet and signalling NaNs, inf, subnormal, -0
        if special:
            bits[:min(n, len(edge))] = edge[:n]
        return bits.view(np.uint8).copy()
    x = (rng.uniform(0.1, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.integers(-30, 1, size=n)).astype("<f8")
    edge = [1e-40, 0.0, -0.0, np.inf, -np.inf, 3.5e38, 1e-46, np.nan, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24]
    if special:
        x[:min(n, len(edge))] = edge[:n]
    return x.view(np.uint8).copy()


def interleave(tracks, fmt):
    """uint8 [frames * tracks * size]: the tracks' samples (each uint8 [frames * size]) as a file's data chunk stores them"""
    size = BYTES[fmt]
    frames = tracks[0].size // size
    return np.stack([t.reshape(frames, size) for t in tracks], axis=1).reshape(-1).copy()


def write_wav(path, raw, fmt, tracks, rate, extensible=False):
    """A RIFF/WAVE file whose data chunk is `raw` (uint8: frames * tracks samples of the format, interleaved)."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    size = BYTES[fmt]
    tag = 3 if fmt in (F32, F64) else 1
    assert raw.size % (size * tracks) == 0
    fmt_chunk = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, tracks, int(rate), int(rate) * tracks * size, tracks * size, 8 * size)
    if extensible:
        fmt_chunk += struct.pack("<HHIH", 22, 8 * size, 0, tag) + bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt_chunk)) + fmt_chunk + b"data" + struct.pack("<I", raw.size) + raw.tobytes()
    if raw.size % 2:
        body += b"\0"
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
