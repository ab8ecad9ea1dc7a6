#!/usr/bin/env python3
"""Measurement (CPU, no device): what the band-limited converter buys the detector over the linear one.

Syllable audio at 44.1 kHz is brought to 48 kHz with scipy.signal.resample_poly(x, 160, 147) -- a recording at another rate of
the same sound -- and converted back to 44.1 kHz with each converter's fp64 model: the linear one (positions i * rate_in /
rate_out, two neighbours) and the sinc one (tests/sinc_ref.py, default quality).  The sample network's outputs on each are
compared with its outputs on the original audio (oracle/pyoracle.py, fp64): the greatest and the mean deviation over all
evaluations, and the evaluations whose detection flag differs.  Prints one JSON line.

    python tools/sinc_benefit.py [seconds] [seed]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def linear_model(x, rate_in, rate_out):
    import numpy as np
    n = x.size
    m = int((n - 1) * rate_out / rate_in) + 1
    pos = np.arange(m, dtype=np.float64) * (rate_in / rate_out)
    k = np.minimum(pos.astype(np.int64), n - 1)
    return (x[k].astype(np.float64) + (pos - k) * (x[np.minimum(k + 1, n - 1)].astype(np.float64) - x[k])).astype(np.float32)


def main(argv):
    import numpy as np
    from scipy.signal import resample_poly
    import pyoracle as po
    import sinc_ref
    import util
    from syllable_detector_swift_amd import synth

    seconds, seed = (int(argv[0]) if argv else 8), (int(argv[1]) if len(argv) > 1 else 43)
    cfg = util.sample_net()
    fs = int(cfg.samplingRate)
    x = synth.syllable_channel(seconds * fs, util.template(), seed=seed).astype(np.float32)
    x48 = resample_poly(x.astype(np.float64), 160, 147).astype(np.float32)
    back = {"linear": linear_model(x48, 48000.0, float(fs)),
            "sinc": sinc_ref.convert(x48, 48000.0, float(fs))[0].astype(np.float32)}
    o = util.oracle_for(cfg)
    thr = np.asarray(cfg.thresholds)[None, :]
    want = o.run(x, po.F64, po.RULE_ANY)[2]
    rows = {}
    for name, y in back.items():
        got = o.run(y, po.F64, po.RULE_ANY)[2]
        E = min(got.shape[0], want.shape[0])                     # (the way there and back may cost the last evaluation)
        d = np.abs(got[:E] - want[:E])
        rows[name] = {"evaluations": int(E), "greatest_deviation": float(d.max()), "mean_deviation": float(d.mean()),
                      "flags_that_differ": int(((got[:E] >= thr).any(axis=1) != (want[:E] >= thr).any(axis=1)).sum()),
                      "detections_in_original": int((want[:E] >= thr).any(axis=1).sum()),
                      "audio_rms_difference": float(np.sqrt(np.mean((y[:min(y.size, x.size)].astype(np.float64) - x[:min(y.size, x.size)]) ** 2)))}
    doc = {"audio": "%d s of planted syllables at %d Hz, seed %d; to 48 kHz by resample_poly(160, 147) and back" % (seconds, fs, seed),
           "network": "tests/golden/sample_net.npz", "results": rows}
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
