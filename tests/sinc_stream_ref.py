"""The emission rule of the streaming band-limited resampler (the streaming sinc convention of include/syldet.h), restated with
numpy from that text:

    output i is ready once floor(p_i + H) <= N - 1,   p_i = i * rate_in / rate_out   (fp64, in that order)
    ready(N) = the number of outputs that are

The predicate is monotone in i, so around (N - H) * rate_out / rate_in a window of candidates holds the one place where it turns
false; the window's ends are asserted to be on either side of it."""
import numpy as np

import sinc_ref


def is_ready(i, n_total, rate_in, rate_out, H):
    p = np.asarray(i, np.int64).astype(np.float64) * np.float64(rate_in) / np.float64(rate_out)
    return np.floor(p + np.float64(H)).astype(np.int64) <= n_total - 1


def ready(n_total, rate_in, rate_out, Z=sinc_ref.DEFAULTS[0], rolloff=sinc_ref.DEFAULTS[2], window=8):
    if n_total <= 0:
        return 0
    _, H = sinc_ref.design(rate_in, rate_out, rolloff, Z)
    est = int(max((n_total - H) * float(rate_out) / float(rate_in), 0.0))
    i = np.arange(max(est - window, 0), est + window + 1, dtype=np.int64)
    ok = is_ready(i, n_total, rate_in, rate_out, H)
    assert not ok[-1] and (ok[0] or i[0] == 0), (n_total, rate_in, rate_out, Z)
    assert not (ok[1:] & ~ok[:-1]).any(), "the predicate is monotone"
    return int(i[0] + np.count_nonzero(ok))


def history(rate_in, rate_out, Z=sinc_ref.DEFAULTS[0], rolloff=sinc_ref.DEFAULTS[2]):
    """ceil(2 H) + 2: the samples per channel a handle keeps."""
    return int(np.ceil(2.0 * sinc_ref.design(rate_in, rate_out, rolloff, Z)[1])) + 2
