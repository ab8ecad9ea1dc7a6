"""Debug: the wide GEMM's arithmetic restated on the host for tools/debug/wide_blame.py and wide_trace.py -- upload_wide's
folded tables (csrc/syldet_api.cpp) in numpy, the kernel front's bf16 operands from the |X| columns, float64 sums.  The bf16
conversion and the folding are the suite's one restatement, tests/wide_ref.py; this module keeps the shapes its callers use
(BASELINE configs[4]: tables padded to 320 inputs, one output)."""
import os
import sys

import numpy as np
from syllable_detector_swift_amd import nets

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
import wide_ref                                                                    # noqa: E402
from wide_ref import bf16                                                          # noqa: E402,F401

cfg = nets.wide_mlp(nets.from_npz())
I, F = cfg.net.inputs, 29
T = I // F
L0, L1 = cfg.net.layers
H = L0.outputs

_plan = wide_ref.plan(cfg, F)
assert _plan.front and _plan.l2 and _plan.sig and not _plan.poly
Wq = np.zeros((H, 320))
Wq[:, :I] = _plan.Wq
bias = _plan.bias
w1q = _plan.w1[0]
NCH = H // 32


def operands(cols, c, e0, n):
    """bf16 operands of evaluations e0 .. e0 + n - 1 of channel c, [n][320] float64, as the kernel's front makes them"""
    frames = cols[c, e0:e0 + n + T - 1, :].cpu().numpy().astype(np.float32)          # [n + T - 1][F]
    out = np.zeros((n, 320))
    with np.errstate(all="ignore"):
        out[:, :I] = bf16(wide_ref._front_values(_plan, frames)).astype(np.float64)
    return out


def r_of(acc):
    return 1.0 / (np.exp2(acc) + 1.0)
