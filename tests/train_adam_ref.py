"""The numpy model of training from the tool (include/syldet.h, "training from the tool"): one Adam step with float32 scalars and
arrays, one numpy operation per stated operation, math.pow / math.sqrt for the step's constants; the seeded starting weights with
Python integers for SplitMix64; the input map of a range.

    adam_step(p, m, v, grad, loss, t, ...) -> (p, m, v, mean loss)     loss = (L, Wsum)
    init(seed, I, H, O)                    -> theta [P] float32
    input_map(range [2, I])                -> (xOffsets, gains) float32
"""
import math

import numpy as np

f32 = np.float32
MASK = (1 << 64) - 1


def adam_step(p, m, v, grad, loss, t, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8):
    p, m, v, grad = (np.array(a, dtype=f32) for a in (p, m, v, grad))
    L, wsum = float(loss[0]), float(loss[1])
    s = f32(1.0 / wsum) if wsum > 0 else f32(0)
    c1 = f32(lr / (1.0 - math.pow(beta1, t)))
    c2 = f32(1.0 / math.sqrt(1.0 - math.pow(beta2, t)))
    b1, omb1, b2, omb2, e = f32(beta1), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps)
    if t == 1:                                         # the old moments are not read
        m, v = np.zeros_like(m), np.zeros_like(v)
    with np.errstate(all="ignore"):
        g = grad * s
        gg = g * g
        m = b1 * m + omb1 * g
        v = b2 * v + omb2 * gg
        if wsum > 0:
            root = np.sqrt(v)
            den = root * c2 + e
            q = m / den
            p = p - c1 * q
    assert p.dtype == m.dtype == v.dtype == f32
    return p, m, v, (L / wsum if wsum > 0 else 0.0)


def splitmix64(seed):
    state = int(seed) & MASK
    while True:
        state = (state + 0x9E3779B97F4A7C15) & MASK
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        yield z ^ (z >> 31)


def init(seed, I, H, O):
    draws = splitmix64(seed)

    def u(n):
        return np.array([f32(next(draws) >> 40) * f32(2.0 ** -23) - f32(1) for _ in range(n)], dtype=f32)

    w1, w2 = f32(math.sqrt(3.0 / I)), f32(math.sqrt(3.0 / H))
    theta = np.concatenate([u(H * I) * w1, u(H) * f32(0.35), u(O * H) * w2, np.zeros(O, f32)])
    assert theta.dtype == f32
    return theta


def input_map(rng):
    rng = np.asarray(rng, f32)
    lo, hi = rng[0], rng[1]
    with np.errstate(all="ignore"):
        width = hi - lo
        gains = np.where(width > 0, f32(2) / np.where(width > 0, width, f32(1)), f32(1)).astype(f32)
    return lo.copy(), gains
