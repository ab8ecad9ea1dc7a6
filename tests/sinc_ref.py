"""The fp64 model of the band-limited rate converter (the sinc convention of include/syldet.h), written from that text with
numpy.i0 and numpy.sinc: every coefficient evaluated directly, no table.

    s      = min(1, rate_out / rate_in) * rolloff
    H      = Z / s
    p_i    = i * rate_in / rate_out
    h(t)   = s * sinc(s t) * I0(beta sqrt(1 - (t / H)^2)) / I0(beta)   for |t| < H, else 0
    out[i] = sum over k = ceil(p_i - H) .. floor(p_i + H) of x[k] * h(p_i - k),   x[k] = 0 outside [0, n_in)

`convert` returns, for every output of a stretch, the value and the three sums the device's error bound is made of."""
import numpy as np

DEFAULTS = (32, 12.0, 0.9)                                      # zero crossings, beta, rolloff


def count(n_in, rate_in, rate_out):
    """syldet_convert_rate_count: the positions i * rate_in / rate_out <= n_in - 1."""
    return int((n_in - 1) * float(rate_out) / float(rate_in)) + 1 if n_in > 0 else 0


def design(rate_in, rate_out, rolloff, Z):
    s = min(1.0, float(rate_out) / float(rate_in)) * float(rolloff)
    return s, Z / s


def coefficient(t, rate_in, rate_out, Z=DEFAULTS[0], beta=DEFAULTS[1], rolloff=DEFAULTS[2]):
    """h(t), t in input samples (any shape)."""
    t = np.asarray(t, np.float64)
    s, H = design(rate_in, rate_out, rolloff, Z)
    inside = np.abs(t) < H
    u = np.where(inside, t / H, 0.0)
    h = s * np.sinc(s * t) * np.i0(beta * np.sqrt(1.0 - u * u)) / np.i0(beta)
    return np.where(inside, h, 0.0)


def taps(rate_in, rate_out, Z=DEFAULTS[0], rolloff=DEFAULTS[2]):
    return 2 * int(np.floor(design(rate_in, rate_out, rolloff, Z)[1])) + 1


def convert(x, rate_in, rate_out, Z=DEFAULTS[0], beta=DEFAULTS[1], rolloff=DEFAULTS[2], start=0, stop=None, rows=2048):
    """x [n_in] -> (out, A, X, T) for outputs start .. stop - 1 (default: all of them), each fp64 [stop - start] (T int64):
    out the converted samples, A = sum |h x|, X = sum |x| over the taps inside the row, T the number of k in
    [ceil(p - H), floor(p + H)] before the row cuts them."""
    x = np.asarray(x)                                            # (widened stretch by stretch: a long row stays as it is)
    n_in = x.size
    n_out = count(n_in, rate_in, rate_out)
    stop = n_out if stop is None else min(int(stop), n_out)
    s, H = design(rate_in, rate_out, rolloff, Z)
    out, A, X, T = (np.zeros(max(stop - start, 0)) for _ in range(4))
    span = 2 * int(np.floor(H)) + 2                              # ceil(p - H) + span > floor(p + H)
    for a in range(start, stop, rows):
        i = np.arange(a, min(a + rows, stop), dtype=np.float64)
        p = i * float(rate_in) / float(rate_out)
        k_lo, k_hi = np.ceil(p - H).astype(np.int64), np.floor(p + H).astype(np.int64)
        k = k_lo[:, None] + np.arange(span, dtype=np.int64)[None, :]
        live = (k <= k_hi[:, None]) & (k >= 0) & (k < n_in)
        xs = np.where(live, x[np.clip(k, 0, n_in - 1)].astype(np.float64), 0.0)
        h = coefficient(p[:, None] - k, rate_in, rate_out, Z, beta, rolloff)
        sl = slice(a - start, a - start + i.size)
        out[sl] = (xs * h).sum(axis=1)
        A[sl] = np.abs(xs * h).sum(axis=1)
        X[sl] = np.abs(xs).sum(axis=1)
        T[sl] = k_hi - k_lo + 1
    return out, A, X, T.astype(np.int64)


def bound(A, X, T):
    """The device's contract: T 2^-24 A for a T-term fp32 dot product, 2^-21 X for coefficients each 2^-21 from the exact one."""
    return T * 2.0 ** -24 * A + 2.0 ** -21 * X
