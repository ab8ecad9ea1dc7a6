"""The TTL trigger track (Processor.swift:128-148, ProcessorAudio :217-221, AudioInterface.swift:13-40, :442-445) restated in
numpy, twice: the closed form the library's header states (a union of pulses), and the rig's callback loop -- walk buffers of L,
collect the evaluations the buffer makes available, `seen`, arm, render the next buffer -- as its witness."""
import numpy as np

from trace_ref import count_evals, geometry  # noqa: F401  (the clock is the trace's)


def buffer_of(e, D, hop, L):
    """b(e) = (D + e hop - 1) / L: the callback buffer that makes evaluation e available"""
    return (D + np.asarray(e, np.int64) * hop - 1) // L


def seen_buffers(flags, D, hop, L):
    """the seen buffers of one channel's flags [n_evals], ascending"""
    f = np.asarray(flags).reshape(-1)
    return np.unique(buffer_of(np.nonzero(f)[0], D, hop, L))


def closed_form(flags, D, hop, L, N, latency, n_samples):
    """flags [n_evals] of one channel -> track [n_samples] uint8: 1 iff some seen buffer b has t_b <= s < t_b + N, t_b = (b + 1) L + latency"""
    edge = np.zeros(n_samples + 1, np.int64)
    for b in seen_buffers(flags, D, hop, L):
        t = (int(b) + 1) * L + latency
        if t < n_samples:
            edge[t] += 1
            edge[min(t + N, n_samples)] -= 1
    return (np.cumsum(edge)[:n_samples] > 0).astype(np.uint8)


def closed_form_bank(flags, D, hop, L, N, latency, n_samples):
    """flags [C, n_evals] -> [C, n_samples] uint8"""
    C = len(flags)
    return np.stack([closed_form(flags[c], D, hop, L, N, latency, n_samples) for c in range(C)]) if C else np.zeros((0, n_samples), np.uint8)


def onsets(flags, D, hop, L, N, latency, n_samples):
    """the onset rule: a seen buffer b with no seen buffer in [b - N / L, b); its sample t_b; those at t_b >= n_samples dropped"""
    out, prev = [], None
    for b in (int(x) for x in seen_buffers(flags, D, hop, L)):
        if prev is None or prev < b - N // L:
            t = (b + 1) * L + latency
            if t < n_samples:
                out.append(t)
        prev = b
    return np.asarray(out, np.int64)


def rising_edges(track):
    """the samples where a 0/1 track goes from 0 (or the start) to 1"""
    t = np.asarray(track).astype(np.int8)
    return np.nonzero(np.diff(np.concatenate([[0], t])) == 1)[0].astype(np.int64)


def as_f32(track):
    return np.asarray(track, np.float32)              # 1.0 / 0.0: the reference's floats


def as_s16(track):
    return (np.asarray(track, np.int16) * np.int16(32767)).astype(np.int16)


def rig_loop(flags, window, overlap, time_range, L, N, latency, n_samples):
    """The rig, callback by callback.  Input buffer b hands the detector its samples; the evaluations processNewValue then has
    (the rule of syldet_count_evals on what was fed so far) are consumed and `seen` is set if one of them is flagged
    (Processor.swift:128-148); a seen buffer arms: high = N (createHighOutput: set, not added).  Then the next render buffer is
    written with renderOutput's arithmetic -- frame i is 1 for i < high, high goes down by min(high, frames) -- at the output's
    position (b + 1) L + latency.  Samples no render buffer covers (the first one's, and the latency) are 0."""
    f = np.asarray(flags).reshape(-1)
    out = np.zeros(n_samples + L + latency + 1, np.uint8)
    high = done = fed = b = 0
    while fed < n_samples:
        fed = min(fed + L, n_samples)
        seen = False
        avail = min(count_evals(fed, window, overlap, time_range), len(f))
        while done < avail:
            seen = seen or f[done] != 0
            done += 1
        if seen:
            high = N
        pos = (b + 1) * L + latency
        h = high
        if 0 < h:
            high = h - min(h, L)
        for i in range(L):
            if pos + i < len(out):
                out[pos + i] = 1 if i < h else 0
        b += 1
    return out[:n_samples]
