"""The numpy model of training (include/syldet.h, "training"): loss and gradient of a two-layer network over one detector's
selected evaluations, in float64 or with every array and operation in float32; and the targets in Python integers.

    net_of(cfg, bins)                  what the model needs of a configuration
    gradient(net, cols, theta, t, w, dtype)   -> L, Wsum, g [P], A [P]: A_p = sum_e |w_e dl_e / dtheta_p|, the sum of the absolute
                                       per-evaluation contributions (for the loss: L itself)
    bars(net, cols, theta, t, w)       -> the float64 result and r32, the float32 model's worst |g32 - g64| / A (gradient, loss)
    targets(...), packed_targets(...)  the targets rule over Python integers
"""
import numpy as np

TF = {"TanSig": 0, "LogSig": 1, "PureLin": 2, "SatLin": 3}


class Net:
    pass


def net_of(cfg, bins):
    n = Net()
    L0, L1 = cfg.net.layers
    n.F, n.T = int(bins), int(cfg.timeRange)
    n.I, n.H, n.O = int(L0.inputs), int(L0.outputs), int(L1.outputs)
    assert n.I == n.F * n.T and L1.inputs == n.H
    n.tf0, n.tf1 = TF[L0.transferFunction], TF[L1.transferFunction]
    n.scaling = cfg.spectrogramScaling
    n.in_fns = [(f.function, None if f.xOffsets is None else np.asarray(f.xOffsets, np.float32), None if f.gains is None else np.asarray(f.gains, np.float32),
                 np.float32(f.y)) for f in cfg.net.inputProcessing]
    n.out_fns = [(np.asarray(f.xOffsets, np.float32), np.asarray(f.gains, np.float32), np.float32(f.y)) for f in cfg.net.outputProcessing]
    n.P = n.H * n.I + n.H + n.O * n.H + n.O
    return n


def split(net, theta):
    H, I, O = net.H, net.I, net.O
    a = H * I
    return theta[:a].reshape(H, I), theta[a:a + H], theta[a + H:a + H + O * H].reshape(O, H), theta[a + H + O * H:]


def _transfer(tf, a):
    if tf == 0:
        return np.tanh(a)
    if tf == 1:
        return 1 / (np.exp(-a) + 1)
    if tf == 3:
        return np.clip(a, 0, 1)
    return a


def _slope(tf, a, h):
    if tf == 0:
        return 1 - h * h
    if tf == 1:
        return h * (1 - h)
    if tf == 3:
        return ((a > 0) & (a < 1)).astype(h.dtype)
    return np.ones_like(h)


def inputs(net, cols, sel, dtype):
    """the processed inputs [n, I] of the selected evaluations `sel` (indices) of one detector's columns [J, F]"""
    J = cols.shape[0]
    win = np.lib.stride_tricks.sliding_window_view(np.ascontiguousarray(cols, np.float32).reshape(-1), net.I)[::net.F]
    assert win.shape[0] == J - net.T + 1
    x = win[sel].astype(dtype)
    if net.scaling == "log":
        x = np.log(x)
    elif net.scaling == "db":
        x = dtype(20) * np.log10(x)
    for name, xo, g, y in net.in_fns:
        if name == "l2normalize":
            x = x / np.sqrt((x * x).sum(axis=1, keepdims=True, dtype=dtype))
        elif name == "normalize":
            mn, mx = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
            rng = mx - mn
            safe = np.where(rng == 0, dtype(1), rng)
            x = np.where(rng == 0, dtype(-1), x * (dtype(2) / safe) + (dtype(0) - mn - mx) / safe)
        elif name == "normalizestd":
            mean = x.sum(axis=1, keepdims=True, dtype=dtype) / dtype(net.I)
            d = x - mean
            x = d / np.sqrt((d * d).sum(axis=1, keepdims=True, dtype=dtype) / dtype(net.I))
        else:
            x = (x - xo.astype(dtype)) * g.astype(dtype) + dtype(y)
    return x.astype(dtype)


def gradient(net, cols, theta, targets, weights, dtype=np.float64, order="matmul"):
    """cols [J, F] float32, theta [P] float32, targets [E, O], weights [E] float32 -> (L, Wsum, g [P], A [P]) in `dtype`; in
    float32 the sums over the evaluations run in evaluation order.  order (float32 only): how the first layer's I products are
    added -- "matmul" (numpy's), "forward" (one after another from input 0) or "reverse" (from input I - 1)."""
    f32 = dtype == np.float32
    w_all = np.asarray(weights, np.float32)
    with np.errstate(invalid="ignore"):
        sel = np.nonzero(w_all > 0)[0]
    w = w_all[sel].astype(dtype)
    t = np.asarray(targets, np.float32)[sel].astype(dtype)
    W1, b1, W2, b2 = (a.astype(dtype) for a in split(net, np.asarray(theta, np.float32)))
    x = inputs(net, cols, sel, dtype)
    if f32 and order != "matmul":
        products = x[:, None, :] * W1[None, :, :]
        a1 = np.add.accumulate(products if order == "forward" else products[:, :, ::-1], axis=2, dtype=np.float32)[:, :, -1] + b1
    else:
        a1 = x @ W1.T + b1
    h1 = _transfer(net.tf0, a1)
    a2 = h1 @ W2.T + b2
    h2 = _transfer(net.tf1, a2)
    y, scale = h2, np.ones(net.O, dtype)
    for xo, g, yk in net.out_fns:
        y = (y - dtype(yk)) / g.astype(dtype) + xo.astype(dtype)
        scale = scale / g.astype(dtype)
    diff = y - t
    terms = w * (diff * diff).sum(axis=1, dtype=dtype)
    d2 = dtype(2) * w[:, None] * diff * scale * _slope(net.tf1, a2, h2)
    d1 = (d2 @ W2) * _slope(net.tf0, a1, h1)

    def total(rows):                                   # the sum over the evaluations of rows [n, ...]
        if not f32:
            return rows.sum(axis=0, dtype=dtype)
        if rows.shape[0] == 0:
            return np.zeros(rows.shape[1:], np.float32)
        return np.add.accumulate(rows.astype(np.float32), axis=0, dtype=np.float32)[-1]      # (accumulate adds one after another)

    def outer(a, b):                                   # sum_e a_e b_e^T
        if not f32:
            return a.T @ b
        return total(a[:, :, None] * b[:, None, :])

    g = np.concatenate([outer(d1, x).reshape(-1), total(d1), outer(d2, h1).reshape(-1), total(d2)]).astype(dtype)
    A = np.concatenate([(np.abs(d1).T @ np.abs(x)).reshape(-1), np.abs(d1).sum(axis=0), (np.abs(d2).T @ np.abs(h1)).reshape(-1), np.abs(d2).sum(axis=0)])
    L = total(terms[:, None])[0] if sel.size else dtype(0)
    Wsum = total(w[:, None])[0] if sel.size else dtype(0)
    return dtype(L), dtype(Wsum), g, A.astype(np.float64)


def bars(net, cols, theta, targets, weights):
    """-> (L64, Wsum64, g64, A, r32 of the gradient, r32 of the loss): the float64 model and the float32 model's worst ratios"""
    L, Ws, g, A = gradient(net, cols, theta, targets, weights, np.float64)
    L32, _, g32, _ = gradient(net, cols, theta, targets, weights, np.float32)
    nz = A > 0
    r = float((np.abs(g32.astype(np.float64) - g)[nz] / A[nz]).max()) if nz.any() else 0.0
    rl = abs(float(L32) - float(L)) / float(L) if L > 0 else 0.0
    return float(L), float(Ws), g, A, r, rl


def within(dev, want, A, r32, margin=8.0):
    """the gradient bar: |dev - want| <= margin max(r32, 2^-24) A, and exactly 0 where A is 0 -> (ok, worst ratio |dev - want| / A)"""
    dev, want, A = np.asarray(dev, np.float64), np.asarray(want, np.float64), np.asarray(A, np.float64)
    nz = A > 0
    err = np.abs(dev - want)
    ratio = float((err[nz] / A[nz]).max()) if nz.any() else 0.0
    ok = bool((err[nz] <= margin * max(r32, 2.0 ** -24) * A[nz]).all()) and bool((dev[~nz] == 0).all())
    return ok, ratio


# ---- the targets, in Python integers ----
def targets(labels, label_outputs, n_evals, half_width, wp, wn, first_index, hop, n_out):
    labels = [int(v) for v in labels]
    outs = [0] * len(labels) if label_outputs is None else [int(v) for v in label_outputs]
    t = np.zeros((n_evals, n_out), np.float32)
    w = np.zeros(n_evals, np.float32)
    for e in range(n_evals):
        idx = int(first_index) + e * int(hop)
        hit = {o for s, o in zip(labels, outs) if abs(idx - s) <= int(half_width)}
        for o in hit:
            t[e, o] = 1.0
        w[e] = np.float32(wp) if hit else np.float32(wn)
    return t, w


def packed_targets(slots, rows, row_evals, labels, label_outputs, half_width, wp, wn, first_index, hop, n_out):
    """slots: (row, offset, first_eval, n_evals, n_samples) per recording -> targets [rows, row_evals, n_out], weights [rows, row_evals]:
    zeros wherever no recording's evaluation is"""
    t = np.zeros((rows, row_evals, n_out), np.float32)
    w = np.zeros((rows, row_evals), np.float32)
    for k, (row, _, first, n, _) in enumerate(slots):
        tk, wk = targets(labels[k], None if label_outputs is None else label_outputs[k], int(n), half_width, wp, wn, first_index, hop, n_out)
        t[row, first:first + n] = tk
        w[row, first:first + n] = wk
    return t, w
