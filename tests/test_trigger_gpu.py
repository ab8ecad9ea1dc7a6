"""The TTL trigger track on the device (syldet_trigger*; kernels_trigger.hip) against tests/trigger_ref.py, bit for bit, no
tolerance.  Flags are planted arrays on a network's geometry -- no network quality is involved -- except in the end-to-end and
streaming cases, which take them from the library's own, separately tested run()."""
import numpy as np
import pytest

import trigger_ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets, synth

pytestmark = pytest.mark.gpu

SPAN16 = 8192                        # samples of an int16 row a workgroup of trigger_kernel writes (16 KiB; fp32: 4096)
S_LONG = 3 * SPAN16 + 4321           # three spans and an odd remainder
WIDTHS = lambda L: [1, L - 1, L, 44, 20 * L, 10000]     # the last one is longer than a span: a pulse that begins two workgroups earlier
LATENCIES = [0, 1, 221, 9000]
CANARY16, CANARY32, CANARY64 = -21846, 0x7FC0BEEF, -0x0123456789ABCDEF


def _torch():
    import torch
    return torch


def _same(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d differences, first at %s: %s != %s" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def _geometries():
    base = util.sample_net()
    return {"hop 132": base,
            "hop 1": nets.variant(base, windowOverlap=base.windowLength - 1),
            "gap 20": nets.variant(base, windowOverlap=-20)}


def _clock(cfg):
    return (cfg.windowLength, cfg.windowOverlap, cfg.timeRange)


def _pair(D, hop, L, E, k):
    """two evaluations whose buffers lie exactly k apart, well inside the recording; None if the geometry has none"""
    b = trigger_ref.buffer_of(np.arange(E), D, hop, L)
    for e1 in range(E // 3, min(E, E // 3 + 50)):
        hit = np.nonzero(b == b[e1] + k)[0]
        if len(hit):
            return e1, int(hit[0])
    return None


def _planted(kind, E, D, hop, L, N, rng):
    """one channel's flags; `kind` falls back to sparse random flags where the geometry cannot make it"""
    f = np.zeros(E, np.uint8)
    if kind == "ones":
        f[:] = 1
    elif kind == "first" and E:
        f[0] = 1
    elif kind == "last" and E:
        f[E - 1] = 1
    elif kind in ("abut", "miss"):
        k, r = divmod(N + (kind == "miss"), L)             # abut: (b2 - b1) L == N; miss by one sample: (b2 - b1) L == N + 1
        pair = _pair(D, hop, L, E, k) if r == 0 and k >= 1 else None
        if pair is None:
            return _planted("sparse", E, D, hop, L, N, rng)
        f[list(pair)] = 1
    elif kind == "sparse":
        f[:] = rng.random(E) < 0.03
    elif kind == "dense":
        f[:] = rng.random(E) < 0.5
    return f, kind


def _canaried(C, n, stride, shift, dtype, device):
    """rows [C][stride] `shift` elements behind a 16-byte line inside a filled buffer"""
    torch = _torch()
    pad = 16
    if dtype == np.int16:
        flat = torch.full((C * stride + 2 * pad,), CANARY16, dtype=torch.int16, device=device)
    else:
        flat = torch.empty((C * stride + 2 * pad,), dtype=torch.float32, device=device)
        flat.view(torch.int32).fill_(CANARY32)
    assert flat.data_ptr() % 16 == 0
    rows = flat[pad + shift:pad + shift + C * stride].view(C, stride)
    return flat, rows


def _check_canaries(flat, C, n, stride, shift, dtype, what):
    rest = flat.cpu().numpy().copy()
    body = rest[16 + shift:16 + shift + C * stride].reshape(C, stride)
    if dtype == np.int16:
        body[:, :n] = CANARY16
        assert (rest == CANARY16).all(), what + ": bytes outside the first n_samples of a row were written"
    else:
        body.view(np.int32)[:, :n] = CANARY32
        assert (rest.view(np.int32) == CANARY32).all(), what + ": bytes outside the first n_samples of a row were written"


def _onsets_with_canaries(det, fl, n, L, N, lat, cap):
    torch = _torch()
    C = det.channels
    flat = torch.full((C * cap + 2 * C + 32,), CANARY64, dtype=torch.int64, device=fl.device)
    idx, cnt = flat[8:8 + C * cap], flat[16 + C * cap:16 + C * cap + C]
    src = fl if fl.shape[1] else torch.zeros(1, dtype=torch.uint8, device=fl.device)
    st = _abi.lib.syldet_trigger_onsets_device(det._h, src.data_ptr(), int(fl.shape[1]), L, N, lat, n, idx.data_ptr(), cap, cnt.data_ptr(),
                                               det._stream_ptr(None))
    assert st == 0, _abi.last_error()
    torch.cuda.synchronize()
    host = flat.cpu().numpy()
    idx_h, cnt_h = host[8:8 + C * cap].reshape(C, cap).copy(), host[16 + C * cap:16 + C * cap + C].copy()
    host[8:8 + C * cap] = CANARY64
    host[16 + C * cap:16 + C * cap + C] = CANARY64
    assert (host == CANARY64).all(), "onsets: written outside indices [C][capacity] and counts [C]"
    return idx_h, cnt_h


def _check_onsets(idx_h, cnt_h, flags, D, hop, L, N, lat, n, cap, what):
    for c in range(len(flags)):
        want = trigger_ref.onsets(flags[c], D, hop, L, N, lat, n)
        assert cnt_h[c] == len(want), (what, c, cnt_h[c], len(want))
        k = min(len(want), cap)
        assert np.array_equal(idx_h[c, :k], want[:k]), (what, c)
        assert (idx_h[c, k:] == CANARY64).all(), (what, c, "written past the onsets")


@pytest.mark.parametrize("L", [32, 256])
@pytest.mark.parametrize("geometry", list(_geometries()))
def test_planar_tracks_and_onsets_equal_the_closed_form(geometry, L):
    """every width x every latency on three channels of planted flags (zeros / ones / first / last in turn, abutting or
    missing-by-one pairs where the width allows them, random flags), rows 0 .. 3 elements behind a 16-byte line with odd strides,
    canaries around every row and behind the onsets"""
    torch = _torch()
    cfg = _geometries()[geometry]
    rng = np.random.default_rng(L)
    S = S_LONG
    seen = {"abut": 0, "miss": 0, "ones": 0, "zeros": 0, "first": 0, "last": 0}
    with sd.SyllableDetector(cfg, channels=3) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        # the recording ends with the sample that makes its last evaluation available (that evaluation's pulse starts beyond it),
        # at a length that is no multiple of 8
        E = det.countEvaluations(S)
        while (D + (E - 1) * hop) % 8 == 0:
            E -= 1
        S = D + (E - 1) * hop
        assert E == det.countEvaluations(S) == trigger_ref.count_evals(S, *_clock(cfg)) and E > 50 and S > SPAN16 + 4000
        combo = 0
        for N in WIDTHS(L):
            for lat in LATENCIES:
                kinds = [["zeros", "ones", "first", "last"][(combo + combo // 4) % 4], "abut" if N % L == 0 else "miss", ["sparse", "dense"][(combo // 4) % 2]]
                planted = [_planted(k, E, D, hop, L, N, rng) for k in kinds]
                flags = np.stack([p[0] for p in planted])
                for _, k in planted:
                    if k in seen:
                        seen[k] += 1
                what = "%s L %d N %d latency %d %s" % (geometry, L, N, lat, [k for _, k in planted])
                want = trigger_ref.closed_form_bank(flags, D, hop, L, N, lat, S)
                fl = torch.from_numpy(flags).cuda()
                shift, stride = combo % 4, (S | 1) + 2 + 2 * (combo % 3)   # (odd strides)
                for dtype, conv in ((np.float32, trigger_ref.as_f32), (np.int16, trigger_ref.as_s16)):
                    flat, rows = _canaried(3, S, stride, shift, dtype, fl.device)
                    got = det.triggerTrack(fl, S, L, N, lat, dtype=dtype, out=rows[:, :S])
                    torch.cuda.synchronize()
                    assert got.data_ptr() == rows.data_ptr() and rows.data_ptr() % 16 == (shift * rows.element_size()) % 16
                    _same(rows[:, :S].cpu().numpy(), conv(want), what)
                    _check_canaries(flat, 3, S, stride, shift, dtype, what)
                cap = E
                idx_h, cnt_h = _onsets_with_canaries(det, fl, S, L, N, lat, cap)
                _check_onsets(idx_h, cnt_h, flags, D, hop, L, N, lat, S, cap, what)
                for c in range(3):                                     # the onsets are the track's rising edges
                    assert np.array_equal(idx_h[c, :cnt_h[c]], trigger_ref.rising_edges(want[c])), what
                if kinds[0] == "last":                                 # its pulse starts beyond S: nothing written, no onset
                    assert not want[0].any() and cnt_h[0] == 0
                if planted[1][1] in ("abut", "miss"):                 # one pulse of 2 N samples, or two with one sample between them
                    t1, t2 = [(int(b) + 1) * L + lat for b in trigger_ref.seen_buffers(flags[1], D, hop, L)]
                    assert t2 - t1 == N + (planted[1][1] == "miss")
                    assert cnt_h[1] == ((t1 < S) if planted[1][1] == "abut" else (t1 < S) + (t2 < S)), what
                    if t2 + N <= S:
                        assert want[1].sum() == 2 * N and want[1][t2 - 1] == (planted[1][1] == "abut")
                combo += 1
    print("%s, L %d: %d samples, %d evaluations, %d combinations, planted %s" % (geometry, L, S, E, combo, seen))
    assert combo == 24 and seen["ones"] and seen["zeros"] and seen["first"] and seen["last"], seen
    if geometry != "gap 20" or L == 256:
        assert seen["abut"], seen                                      # (hop 276 puts no two evaluations 1 or 20 buffers of 32 apart)
    if L == 256 or geometry == "hop 1":
        assert seen["miss"], seen                                      # N = L - 1 between neighbouring buffers


CHUNK = 2048                         # buffers a workgroup of trigger_scan_kernel / trigger_onsets_kernel takes a step


def _straddling_pair(b, edge):
    """the last evaluation whose buffer lies in front of buffer `edge` and the first one at or behind it"""
    e2 = int(np.nonzero(b >= edge)[0][0])
    assert e2 >= 1 and b[e2 - 1] < edge <= b[e2]
    return e2 - 1, e2


@pytest.mark.parametrize("geometry", ["hop 132", "hop 1"])
def test_tables_longer_than_the_scans_chunk(geometry):
    """L = 8 (the length that sizes the kernels' table slices) and three chunks of 2048 buffers plus an odd remainder: the scan's
    and the onsets' carries from chunk to chunk.  Flags on both sides of each chunk edge, pairs of pulses that abut or miss by one
    sample across an edge, a single flag in the first chunk whose pulse runs through the second and third, ones, random flags --
    the planar rows, the frames, the mux and the onsets against tests/trigger_ref.py."""
    torch = _torch()
    cfg = _geometries()[geometry]
    L, C = 8, 8
    S = 3 * CHUNK * L + 4321
    rng = np.random.default_rng(77)
    with sd.SyllableDetector(cfg, channels=C) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        E = det.countEvaluations(S)
        b = trigger_ref.buffer_of(np.arange(E), D, hop, L)
        assert b[-1] >= 3 * CHUNK and (S + 2 * L - 2) // L > 3 * CHUNK          # B' spans four chunks
        p1, p2 = _straddling_pair(b, CHUNK), _straddling_pair(b, 2 * CHUNK)
        gap1, gap2 = int(b[p1[1]] - b[p1[0]]), int(b[p2[1]] - b[p2[0]])
        audio = rng.integers(-32768, 32768, (C, S), dtype=np.int16)
        xa = torch.from_numpy(audio).cuda()
        # (width, latency): the pair at the first edge abuts / misses by one sample; then the same at the second edge; 1 ms; a
        # pulse longer than two chunks of buffers
        for N, lat in [(gap1 * L, 0), (gap1 * L - 1, 3), (gap2 * L, 221), (gap2 * L - 1, 0), (44, 1), (2 * CHUNK * L + 777, 0), (1, 0)]:
            flags = np.zeros((C, E), np.uint8)
            flags[0, list(p1)] = 1                                     # a pair across the first chunk edge
            flags[1, list(p2)] = 1                                     # ... and across the second
            flags[2, [p1[0], p2[1]]] = 1                               # the last buffer of chunk 0 and the first of chunk 2: nothing in chunk 1
            flags[3, 3] = 1                                            # one flag in the first chunk
            flags[4] = 1
            flags[5] = rng.random(E) < 0.02
            flags[6] = rng.random(E) < 0.5
            flags[7, -1] = 1                                           # the last chunk alone
            what = "%s N %d latency %d" % (geometry, N, lat)
            want = trigger_ref.closed_form_bank(flags, D, hop, L, N, lat, S)
            fl = torch.from_numpy(flags).cuda()
            t32 = det.triggerTrack(fl, S, L, N, lat)
            t16 = det.triggerTrackPCM16(fl, S, L, N, lat)
            fr = det.triggerTrackInterleavedPCM16(fl, S, L, N, lat)
            mx = det.triggerMuxPCM16(fl, xa, L, N, lat)
            idx_h, cnt_h = _onsets_with_canaries(det, fl, S, L, N, lat, 300)
            torch.cuda.synchronize()
            _same(t32.cpu().numpy(), trigger_ref.as_f32(want), what)
            _same(t16.cpu().numpy(), trigger_ref.as_s16(want), what)
            _same(fr.cpu().numpy(), trigger_ref.as_s16(want).T, what + " frames")
            m = mx.cpu().numpy()
            _same(m[:, 0::2], audio.T, what + " audio lanes")
            _same(m[:, 1::2], trigger_ref.as_s16(want).T, what + " trigger lanes")
            _check_onsets(idx_h, cnt_h, flags, D, hop, L, N, lat, S, 300, what)
            for c in range(C):
                edges = trigger_ref.rising_edges(want[c])
                assert cnt_h[c] == len(edges) and np.array_equal(idx_h[c, :min(300, len(edges))], edges[:300]), (what, c)
            # what the planted rows are there for
            if N == gap1 * L:
                assert cnt_h[0] == 1 and want[0].sum() == 2 * N
            if N == gap1 * L - 1:
                assert cnt_h[0] == 2
            if N == gap2 * L:
                assert cnt_h[1] == 1 and want[1].sum() == 2 * N
            if N == gap2 * L - 1:
                assert cnt_h[1] == 2
            if N > 2 * CHUNK * L:
                t3 = (int(b[3]) + 1) * L + lat
                assert cnt_h[3] == 1 and want[3][t3:t3 + N].all() and want[3].sum() == N and t3 + N > 2 * CHUNK * L
                assert cnt_h[2] == 1                                   # the second flag lands inside the first one's pulse, a chunk later
            assert cnt_h[2] >= 1 and cnt_h[4] >= 1 and cnt_h[7] == (1 if (int(b[-1]) + 1) * L + lat < S else 0)


@pytest.mark.parametrize("C", [1, 3])
def test_short_recordings_on_every_form(C):
    """S in {0, 1, L - 1, D - 1, D, D + hop}: nothing, less than a buffer, no evaluation, one, two"""
    torch = _torch()
    cfg = util.sample_net()
    L, N = 32, 44
    rng = np.random.default_rng(9)
    with sd.SyllableDetector(cfg, channels=C) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        for S in (0, 1, L - 1, D - 1, D, D + hop, D + hop + 2 * L + N):
            E = max(det.countEvaluations(S), 0)
            assert E == (0 if S < D else (S - D) // hop + 1)
            flags = np.ones((C, E), np.uint8)
            fl = torch.from_numpy(flags).cuda()
            audio = rng.integers(-32768, 32768, (C, S), dtype=np.int16)
            for lat in (0, 1):
                what = "C %d S %d latency %d" % (C, S, lat)
                want = trigger_ref.closed_form_bank(flags, D, hop, L, N, lat, S)
                t32 = det.triggerTrack(fl, S, L, N, lat)
                t16 = det.triggerTrackPCM16(fl, S, L, N, lat)
                fr = det.triggerTrackInterleavedPCM16(fl, S, L, N, lat)
                mux = det.triggerMuxPCM16(fl, torch.from_numpy(audio).cuda(), L, N, lat)
                idx_h, cnt_h = _onsets_with_canaries(det, fl, S, L, N, lat, 4)
                torch.cuda.synchronize()
                _same(t32.cpu().numpy(), trigger_ref.as_f32(want), what)
                _same(t16.cpu().numpy(), trigger_ref.as_s16(want), what)
                _same(fr.cpu().numpy(), trigger_ref.as_s16(want).T, what)
                m = mux.cpu().numpy()
                assert m.shape == (S, 2 * C)
                _same(m[:, 0::2], audio.T, what + " audio lanes")
                _same(m[:, 1::2], trigger_ref.as_s16(want).T, what + " trigger lanes")
                _check_onsets(idx_h, cnt_h, flags, D, hop, L, N, lat, S, 4, what)
            # the first pulse starts with the buffer behind the one that holds sample D - 1: at D at the earliest
            assert want.any() == (S > ((D - 1) // L + 1) * L + 1)


@pytest.mark.parametrize("C", [1, 3, 65, 130])
def test_interleaved_and_mux_frames(C):
    """one tile, a partial tile and three tiles of channels; frames [n][C] are the int16 rows transposed, frames [n][2 C] carry the
    input's bits in the audio lanes and the int16 track in the trigger lanes; nothing behind the last frame"""
    torch = _torch()
    cfg = util.sample_net()
    S, L = 12007, 32
    rng = np.random.default_rng(C)
    with sd.SyllableDetector(cfg, channels=C) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        E = det.countEvaluations(S)
        audio = rng.integers(-32768, 32768, (C, S + 3), dtype=np.int16)
        xa = torch.from_numpy(audio).cuda()[:, :S]                     # rows with an odd stride
        for i, (N, lat) in enumerate([(1, 0), (L - 1, 1), (L, 221), (44, 0), (20 * L, 1), (10000, 0), (44, 9000)]):
            flags = (rng.random((C, E)) < [0.03, 0.4][i % 2]).astype(np.uint8)
            flags[0] = [1, 0][i % 2]                                   # (ones under the latency of 9000: its first pulses are inside S)
            what = "C %d N %d latency %d" % (C, N, lat)
            want = trigger_ref.as_s16(trigger_ref.closed_form_bank(flags, D, hop, L, N, lat, S))
            fl = torch.from_numpy(flags).cuda()
            planar = det.triggerTrackPCM16(fl, S, L, N, lat)
            fr_buf = torch.full((S + 8, C), CANARY16, dtype=torch.int16, device="cuda")
            mx_buf = torch.full((S + 8, 2 * C), CANARY16, dtype=torch.int16, device="cuda")
            fr = det.triggerTrackInterleavedPCM16(fl, S, L, N, lat, out=fr_buf[:S])
            mx = det.triggerMuxPCM16(fl, xa, L, N, lat, out=mx_buf[:S])
            torch.cuda.synchronize()
            _same(planar.cpu().numpy(), want, what + " planar")
            _same(fr.cpu().numpy(), want.T, what + " frames")
            m = mx.cpu().numpy()
            _same(m[:, 0::2], audio[:, :S].T, what + " audio lanes")
            _same(m[:, 1::2], want.T, what + " trigger lanes")
            assert (fr_buf[S:].cpu().numpy() == CANARY16).all() and (mx_buf[S:].cpu().numpy() == CANARY16).all(), what
            assert want[0].any() == (i % 2 == 0) and (C == 1 or want.any())


def test_onsets_beyond_the_capacity_are_counted_not_written():
    torch = _torch()
    cfg = util.sample_net()
    S, L, N = S_LONG, 32, 44
    with sd.SyllableDetector(cfg, channels=3) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        E = det.countEvaluations(S)
        flags = np.zeros((3, E), np.uint8)
        flags[0, ::3] = 1
        flags[1, 5] = 1
        flags[2] = 1
        fl = torch.from_numpy(flags).cuda()
        full = [len(trigger_ref.onsets(flags[c], D, hop, L, N, 0, S)) for c in range(3)]
        assert full[0] > 60 and full[1] == 1 and full[2] > 200
        for cap in (0, 1, 7, full[0], full[2] + 5):
            idx_h, cnt_h = _onsets_with_canaries(det, fl, S, L, N, 0, cap)
            _check_onsets(idx_h, cnt_h, flags, D, hop, L, N, 0, S, cap, "capacity %d" % cap)
        idx, cnt = det.triggerOnsets(fl, S, L, N)
        got = det.triggerOnsetsHost(flags, S, L, N)
        torch.cuda.synchronize()
        for c in range(3):
            want = trigger_ref.onsets(flags[c], D, hop, L, N, 0, S)
            assert np.array_equal(idx[c, :int(cnt[c])].cpu().numpy(), want) and np.array_equal(got[c], want)


def test_end_to_end_rehearse_on_planted_syllables():
    torch = _torch()
    cfg = util.sample_net()
    S = 44100
    x = np.stack([synth.syllable_channel(S, util.template(), seed=11), synth.channel(S, 0), synth.syllable_channel(S, util.template(), seed=12)])
    with sd.SyllableDetector(cfg, channels=3) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        xd = torch.from_numpy(x.astype(np.float32)).cuda()
        out, fl = det.run(xd)
        track, onsets, counts, out2, fl2 = det.rehearse(xd)
        t32 = det.rehearse(xd, bufferLength=256, width=20 * 256, latency=221, dtype=np.float32)[0]
        torch.cuda.synchronize()
        flags = fl.cpu().numpy()
        assert torch.equal(fl, fl2) and torch.equal(out, out2) and flags[0].sum() > 0 and flags[2].sum() > 0
        N = det.triggerWidth()
        assert N == 44 and track.dtype == torch.int16 and track.shape == (3, S)
        want = trigger_ref.closed_form_bank(flags, D, hop, 32, N, 0, S)
        _same(track.cpu().numpy(), trigger_ref.as_s16(want), "rehearse")
        _same(t32.cpu().numpy(), trigger_ref.as_f32(trigger_ref.closed_form_bank(flags, D, hop, 256, 5120, 221, S)), "rehearse, the Arduino form")
        for c in range(3):
            w = trigger_ref.onsets(flags[c], D, hop, 32, N, 0, S)
            assert int(counts[c]) == len(w) and np.array_equal(onsets[c, :len(w)].cpu().numpy(), w)
        assert int(counts[0]) >= 1 and want[0].any()
        _same(det.triggerTrackHost(flags, S), trigger_ref.as_f32(want), "host form")
        _same(det.triggerTrackHost(flags, S, dtype=np.int16), trigger_ref.as_s16(want), "host form, int16")
        assert det.triggerTrackHost(flags[:, :0], 500).shape == (3, 500) and not det.triggerTrackHost(flags[:, :0], 500).any()
        assert det.triggerTrackHost(flags, 0).shape == (3, 0)


def test_the_streaming_twin_gives_the_batch_track():
    """the rig itself: append a buffer, seenSyllable, arm, render the following buffer"""
    torch = _torch()
    cfg = util.sample_net()
    S, L = 30000, 32
    x = synth.syllable_channel(44100, util.template(), seed=11)[:S].astype(np.float32)
    with sd.SyllableDetector(cfg, channels=1) as det:
        N = det.triggerWidth()
        _, fl = det.run(torch.from_numpy(x[None]).cuda())
        batch = det.triggerTrack(fl, S, L, N, 0)
        torch.cuda.synchronize()
        assert fl.sum() > 0
        assert not det.renderTrigger(0, L).any()                       # never armed: zeros
        out = np.zeros(S + 2 * L, np.float32)
        for b in range((S + L - 1) // L):
            det.appendAudioData(x[b * L:(b + 1) * L])
            if det.seenSyllable():
                det.armTrigger(0)
            out[(b + 1) * L:(b + 2) * L] = det.renderTrigger(0, L)
        _same(out[:S], batch.cpu().numpy()[0], "streaming")
        assert out[:S].any()


@pytest.mark.parametrize("kind", ["multi", "mixed"])
def test_bank_kinds(kind):
    torch = _torch()
    base = util.sample_net()
    if kind == "multi":
        cfgs = [base, nets.perturbed(base, 5), nets.perturbed(base, 6)]
        net_of = [0, 1, 2, 1, 0]
        det = sd.SyllableDetector.multi(cfgs, net_of)
    else:
        f0, f1 = sd.frequencyIndexRange(base.fourierLength, base.samplingRate, 2000.0, 5000.0)
        narrow = nets.variant(base, freqRange=(2000.0, 5000.0), thresholds=[0.1],
                              net=nets.random_net(np.random.default_rng(1), (f1 - f0) * base.timeRange, (4,), 1))
        cfgs = [base, narrow, nets.perturbed(base, 5)]
        net_of = [1, 0, 2, 1, 0, 2]
        det = sd.SyllableDetector.mixed(cfgs, net_of)
    C, S, L, N, lat = len(net_of), 15013, 32, 44, 1
    rng = np.random.default_rng(3)
    with det:
        D, hop = det.geometry.first_index, det.geometry.hop
        E = det.countEvaluations(S)
        flags = (rng.random((C, E)) < 0.1).astype(np.uint8)
        fl = torch.from_numpy(flags).cuda()
        want = trigger_ref.closed_form_bank(flags, D, hop, L, N, lat, S)
        t32, t16 = det.triggerTrack(fl, S, L, N, lat), det.triggerTrackPCM16(fl, S, L, N, lat)
        fr = det.triggerTrackInterleavedPCM16(fl, S, L, N, lat)
        idx, cnt = det.triggerOnsets(fl, S, L, N, lat)
        torch.cuda.synchronize()
        _same(t32.cpu().numpy(), trigger_ref.as_f32(want), kind)
        _same(t16.cpu().numpy(), trigger_ref.as_s16(want), kind)
        _same(fr.cpu().numpy(), trigger_ref.as_s16(want).T, kind)
        for c in range(C):
            w = trigger_ref.onsets(flags[c], D, hop, L, N, lat, S)
            assert int(cnt[c]) == len(w) and np.array_equal(idx[c, :len(w)].cpu().numpy(), w)
        # a run on the bank, then its rehearsal
        x = torch.from_numpy(np.stack([synth.channel(S, c) for c in range(C)]).astype(np.float32)).cuda()
        track, _, _, _, fl2 = det.rehearse(x)
        torch.cuda.synchronize()
        _same(track.cpu().numpy(), trigger_ref.as_s16(trigger_ref.closed_form_bank(fl2.cpu().numpy(), D, hop, 32, det.triggerWidth(), 0, S)), kind + " rehearse")


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_one_scan_gives_the_track_and_the_onsets_of_the_two_calls(dtype):
    """syldet_trigger_rehearse_device*: rows at an odd stride one element behind a 16-byte line, a capacity below the count, canaries"""
    torch = _torch()
    cfg = util.sample_net()
    S, L, C = S_LONG, 32, 3
    rng = np.random.default_rng(12)
    conv = trigger_ref.as_f32 if dtype == np.float32 else trigger_ref.as_s16
    with sd.SyllableDetector(cfg, channels=C) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        E = det.countEvaluations(S)
        flags = (rng.random((C, E)) < 0.2).astype(np.uint8)
        flags[1] = 0
        fl = torch.from_numpy(flags).cuda()
        for N, lat, cap in [(44, 0, None), (20 * L, 221, 5), (10000, 1, 0)]:
            what = "N %d latency %d capacity %s" % (N, lat, cap)
            flat, rows = _canaried(C, S, S + 3, 1, dtype, fl.device)
            track, idx, cnt = det.triggerRehearse(fl, S, L, N, lat, dtype=dtype, capacity=cap, out=rows[:, :S])
            torch.cuda.synchronize()
            want = trigger_ref.closed_form_bank(flags, D, hop, L, N, lat, S)
            _same(rows[:, :S].cpu().numpy(), conv(want), what)
            _check_canaries(flat, C, S, S + 3, 1, dtype, what)
            for c in range(C):
                w = trigger_ref.onsets(flags[c], D, hop, L, N, lat, S)
                k = len(w) if cap is None else min(cap, len(w))
                assert int(cnt[c]) == len(w) and np.array_equal(idx[c, :k].cpu().numpy(), w[:k]), (what, c)
        assert det.triggerRehearse(fl, 0, L, 44, 0, dtype=dtype)[0].shape == (C, 0)
        lib, bad = _abi.lib, _abi.ERR_INVALID_ARGUMENT
        t = torch.zeros((C, 64), dtype=torch.int16, device="cuda")
        i = torch.zeros((C, 4), dtype=torch.int64, device="cuda")
        assert lib.syldet_trigger_rehearse_device_s16(det._h, fl.data_ptr(), E, L, 44, 0, t.data_ptr(), 64, 63, i.data_ptr(), 4, i.data_ptr(), None) == bad
        assert lib.syldet_trigger_rehearse_device_s16(det._h, fl.data_ptr(), E, L, 44, 0, t.data_ptr(), 64, 64, None, 4, i.data_ptr(), None) == bad
        assert lib.syldet_trigger_rehearse_device_s16(det._h, fl.data_ptr(), E, L, 44, 0, t.data_ptr(), 64, 64, i.data_ptr(), 4, None, None) == bad
        assert lib.syldet_trigger_rehearse_device_s16(det._h, fl.data_ptr(), E, 33, 44, 0, t.data_ptr(), 64, 64, i.data_ptr(), 4, i.data_ptr(), None) == bad


def test_deinterleave_s16_gives_the_rows():
    torch = _torch()
    rng = np.random.default_rng(4)
    for C, n in ((1, 1001), (3, 10007), (70, 2777)):
        frames = rng.integers(-32768, 32768, (n, C), dtype=np.int16)
        f = torch.from_numpy(frames).cuda()
        rows = torch.full((C, n + 5), CANARY16, dtype=torch.int16, device="cuda")
        st = _abi.lib.syldet_deinterleave_device_s16(f.data_ptr(), n, C, C, rows.data_ptr(), n + 5, int(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert st == 0, _abi.last_error()
        got = rows.cpu().numpy()
        assert np.array_equal(got[:, :n], frames.T) and (got[:, n:] == CANARY16).all(), (C, n)


def test_b_of_e_is_the_librarys_levels_eval_range():
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=1) as det:
        D, hop = det.geometry.first_index, det.geometry.hop
        for L, S in ((8, 3001), (32, 9001), (256, 20011)):
            E = det.countEvaluations(S)
            b = trigger_ref.buffer_of(np.arange(E), D, hop, L)
            for m in range(det.levelsCount(S, L, 1)):
                first, count = det.levelsEvalRange(S, E, m, L, 1)
                assert list(np.nonzero(b == m)[0]) == list(range(first, first + count)), (L, m)


def test_the_launches_are_listed_under_profiling():
    torch = _torch()
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=3) as det:
        det.profile(True)
        S = 9000
        fl = torch.ones((3, det.countEvaluations(S)), dtype=torch.uint8, device="cuda")
        audio = torch.zeros((3, S), dtype=torch.int16, device="cuda")
        det.triggerTrack(fl, S)
        torch.cuda.synchronize()
        assert util.launched(det) == ["trigger_scan_kernel", "trigger_kernel"]
        det.triggerTrackPCM16(fl, S)
        torch.cuda.synchronize()
        assert util.launched(det) == ["trigger_scan_kernel", "trigger_kernel"]
        det.triggerTrackInterleavedPCM16(fl, S)
        torch.cuda.synchronize()
        assert util.launched(det) == ["trigger_scan_kernel", "trigger_interleaved_s16_kernel"]
        det.triggerMuxPCM16(fl, audio)
        torch.cuda.synchronize()
        assert util.launched(det) == ["trigger_scan_kernel", "trigger_interleaved_s16_kernel"]
        det.triggerOnsets(fl, S)
        torch.cuda.synchronize()
        names = det.lastTimings()
        assert [n for n, _ in names] == ["trigger_scan_kernel", "trigger_onsets_kernel"] and all(ms > 0 for _, ms in names)
        det.triggerRehearse(fl, S)                                     # one scan for both
        torch.cuda.synchronize()
        assert util.launched(det) == ["trigger_scan_kernel", "trigger_kernel", "trigger_onsets_kernel"]


def test_argument_statuses_with_a_live_handle():
    torch = _torch()
    cfg = util.sample_net()
    with sd.SyllableDetector(cfg, channels=2) as det:
        f = torch.ones((2, 10), dtype=torch.uint8, device="cuda")
        t = torch.full((2, 4000), 7.0, device="cuda")
        q = torch.full((2, 8000), 7, dtype=torch.int16, device="cuda")
        a = torch.zeros((2, 4000), dtype=torch.int16, device="cuda")
        i = torch.full((2, 8), 7, dtype=torch.int64, device="cuda")
        n = torch.full((2,), 7, dtype=torch.int64, device="cuda")
        lib, bad, h = _abi.lib, _abi.ERR_INVALID_ARGUMENT, det._h
        fp, tp, qp, ap, ip, np_ = f.data_ptr(), t.data_ptr(), q.data_ptr(), a.data_ptr(), i.data_ptr(), n.data_ptr()
        for L, N, lat in [(33, 44, 0), (4, 44, 0), (8192, 44, 0), (0, 44, 0), (-32, 44, 0), (32, 0, 0), (32, -1, 0), (32, (1 << 24) + 1, 0),
                          (32, 44, -1), (32, 44, (1 << 24) + 1)]:
            assert lib.syldet_trigger_device(h, fp, 10, L, N, lat, tp, 4000, 4000, None) == bad, (L, N, lat)
            assert lib.syldet_trigger_device_s16(h, fp, 10, L, N, lat, qp, 4000, 4000, None) == bad, (L, N, lat)
            assert lib.syldet_trigger_interleaved_device_s16(h, fp, 10, L, N, lat, qp, 4000, None) == bad, (L, N, lat)
            assert lib.syldet_trigger_mux_device_s16(h, fp, 10, L, N, lat, ap, 4000, qp, 4000, None) == bad, (L, N, lat)
            assert lib.syldet_trigger_onsets_device(h, fp, 10, L, N, lat, 4000, ip, 8, np_, None) == bad, (L, N, lat)
        assert lib.syldet_trigger_device(h, fp, 10, 32, 1 << 24, 1 << 24, tp, 4000, 4000, None) == 0      # the bounds themselves are taken
        torch.cuda.synchronize()
        assert not t.any()
        t.fill_(7.0)
        assert lib.syldet_trigger_device(h, fp, -1, 32, 44, 0, tp, 4000, 4000, None) == bad
        assert lib.syldet_trigger_device(h, fp, 10, 32, 44, 0, tp, -1, 4000, None) == bad
        assert lib.syldet_trigger_device(h, fp, 10, 32, 44, 0, tp, 4000, 3999, None) == bad
        assert lib.syldet_trigger_device_s16(h, fp, 10, 32, 44, 0, qp, 4000, 3999, None) == bad
        assert lib.syldet_trigger_mux_device_s16(h, fp, 10, 32, 44, 0, ap, 3999, qp, 4000, None) == bad
        assert lib.syldet_trigger_device(h, None, 10, 32, 44, 0, tp, 4000, 4000, None) == bad
        assert lib.syldet_trigger_device(h, fp, 10, 32, 44, 0, None, 4000, 4000, None) == bad
        assert lib.syldet_trigger_interleaved_device_s16(h, fp, 10, 32, 44, 0, None, 4000, None) == bad
        assert lib.syldet_trigger_mux_device_s16(h, fp, 10, 32, 44, 0, None, 4000, qp, 4000, None) == bad
        assert lib.syldet_trigger_mux_device_s16(h, fp, 10, 32, 44, 0, ap, 4000, None, 4000, None) == bad
        assert lib.syldet_trigger_onsets_device(h, fp, 10, 32, 44, 0, 4000, None, 8, np_, None) == bad
        assert lib.syldet_trigger_onsets_device(h, fp, 10, 32, 44, 0, 4000, ip, 8, None, None) == bad
        assert lib.syldet_trigger_onsets_device(h, fp, 10, 32, 44, 0, 4000, ip, -1, np_, None) == bad
        assert lib.syldet_trigger_onsets_device(h, fp, 10, 32, 44, 0, -1, ip, 8, np_, None) == bad
        assert lib.syldet_trigger_arm(h, 2, 44) == bad and lib.syldet_trigger_arm(h, -1, 44) == bad and lib.syldet_trigger_arm(h, 0, -1) == bad
        assert lib.syldet_trigger_render(h, 2, None, 0) == bad and lib.syldet_trigger_render(h, 0, None, 8) == bad
        # n_samples == 0 writes nothing
        assert lib.syldet_trigger_device(h, fp, 10, 32, 44, 0, tp, 0, 0, None) == 0
        assert lib.syldet_trigger_device_s16(h, fp, 10, 32, 44, 0, qp, 0, 0, None) == 0
        assert lib.syldet_trigger_mux_device_s16(h, fp, 10, 32, 44, 0, ap, 0, qp, 0, None) == 0
        torch.cuda.synchronize()
        assert (t == 7.0).all() and (q == 7).all() and (i == 7).all() and (n == 7).all()     # refused before the device was touched
        # n_evals == 0 writes zeros
        assert lib.syldet_trigger_device(h, fp, 0, 32, 44, 0, tp, 4000, 4000, None) == 0
        assert lib.syldet_trigger_onsets_device(h, fp, 0, 32, 44, 0, 4000, ip, 8, np_, None) == 0
        torch.cuda.synchronize()
        assert not t.any() and not n.any() and (i == 7).all()
        with pytest.raises(ValueError):
            det.triggerTrack(f, 100, dtype=np.float64)
        with pytest.raises(ValueError):
            det.triggerTrack(f, 100, interleaved=True)                 # frames are int16
        with pytest.raises(ValueError):
            det.triggerTrack(f, 100, bufferLength=33)
        with pytest.raises(ValueError):
            det.triggerTrack(f, 100, width=0)
        with pytest.raises(ValueError):
            det.triggerTrack(f, 100, out=torch.zeros((2, 99), device="cuda"))
        with pytest.raises(ValueError):
            det.triggerWidth(1e-6)
