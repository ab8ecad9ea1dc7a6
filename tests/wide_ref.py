"""The wide bf16 engine's arithmetic (csrc/kernels_wide.hip, upload_wide in csrc/syldet_api.cpp) restated in numpy as a plain
model: NeuralNet.apply (Common/NeuralNet.swift:294-326) with the engine's rounding points and nothing else -- everything that is
not on the list below is float64.  It takes the fp32 columns [J][F] of one channel and a configuration and returns the outputs
[E][n_out] in float64.  No product code is imported; a configuration is read by attribute (the plain-data classes of config.py).

Where the engine rounds:
  bf16          round to nearest even, NaN stays NaN (upload_wide's to_bf16, v_cvt_pk_bf16_f32)
  front route   (the chain is [l2normalize,] affine maps, linear columns, every folded offset |o_i| <= 4, the band fits the stage in
                LDS: front_fits) the operand is bf16(fl32(v * rinv)), rinv = fl32(1 / fl32(sqrt(ss))), ss the fp32 sum in frame
                order of the T column sums of squares, each an fp32 fma chain over the bins in order; without l2normalize bf16(v).
                Weights bf16(fl32(sc W0[u,i] a_i)), first-layer bias fl32(sc (b0 + W0 . o)), a and o the composed maps in fp64.
  prepared      (every other chain, log / dB columns, SYLDET_WIDE_NO_FRONT, SYLDET_WIDE_SHAPE32) the operand is bf16(u), u the chain
                in fp32 as the preparation kernels make it (the reference's operations; sums a lane's five elements first, then a
                balanced tree over the 64 lanes; multiply-adds contracted as the built kernels have them: x inv - xoff is one
                fma in wide_prep_chain_kernel).  Weights bf16(fl32(sc W0)), bias fl32(sc b0).
  hidden layer  TanSig / LogSig folded: acc = sc (W0 x + b0), r = 1 / (2^acc + 1), y = b1' + sum w1' r with w1' = fl32(w1s w1) and
                b1' = fl32(b1 + sum w1) for tanh; any other transfer function exact.  SYLDET_WIDE_TANH_POLY: the kernel's clamped
                seven-term odd polynomial from the kernel's fp32 coefficients, evaluated in float64.
  then          the second layer in float64, f1, the output maps (v - y) / gain + xoff.

An operand whose fp32 value lies within `w` ulps of a bf16 rounding boundary may round the other way in the engine if the engine's
fp32 value differs in its last place: evaluate() reports such operands per evaluation and returns, for an evaluation with one to
three of them, the outputs of every combination of roundings (an evaluation with more is left out and counted).  compare() is the
rule the tests hold the engine to.

Two points of the prepared route describe the kernels AS BUILT, not the engine's contract: that a lane's sum of squares starts
from its second product (_lane_dot's first_two_swapped) and that `x inv - xoff` is one fma in wide_prep_chain_kernel.  Both are
the compiler's contraction choices, read from the kernels' ISA; another compiler may choose otherwise.  Either way the values
differ in an operand's last place only, which is what the prepared route's window of 8 ulps and the alternative roundings are
for: a change there shows as evaluations that need another rounding, not as a wrong GEMM."""
import itertools
from types import SimpleNamespace

import numpy as np

K = 320                       # kWideK: network inputs the engine takes
TOL = 1e-5                    # the suite's bar (tests/util.py)
W_FRONT, W_PREPARED = 2, 8    # near-tie windows in fp32 ulps: the front's arithmetic is restated operation for operation, the
#                               preparation kernels' up to the order of a sum's last additions
MAX_NEAR = 3
FAULTS = ("kstep_missing", "k_tail_missing_in_chunk", "bias_rotated", "unit_term_lost", "product_lost_3pct", "truncation",
          "last_frame_late", "norm_T_minus_1", "input_missing")
# tanh_poly's coefficients as the kernel holds them (fp32), and its clamp
POLY = [float(np.float32(c)) for c in (0.9934016466140747, -0.30040496587753296, 0.08361941576004028, -0.015534450300037861,
                                       0.0017269821837544441, -0.00010273736552335322, 2.5018941869348055e-06)]
POLY_CLAMP = float(np.float32(3.3))

f32, f64 = np.float32, np.float64


# ---- bf16 ----------------------------------------------------------------------------------------------------------------
def _bits(v):
    a = np.asarray(v, f32)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64), a.shape


def bf16(v, truncate=False):
    """float32 array -> float32 array of the bf16 values: round to nearest even (truncate: toward zero); NaN stays NaN"""
    u, shape = _bits(v)
    r = (u >> 16 << 16) if truncate else ((u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = np.where(nan, (u >> 16 << 16) | 0x400000, r)
    return (r & 0xffffffff).astype(np.uint32).view(f32).reshape(shape)


def near_boundary(v, w):
    """finite float32 values within w fp32 ulps of the midpoint of two bf16 neighbours"""
    u, shape = _bits(v)
    lo = (u & 0xffff).astype(np.int64)
    finite = (u & 0x7f800000) != 0x7f800000
    return ((np.abs(lo - 0x8000) <= w) & finite).reshape(shape)


def bf16_other(v):
    """the bf16 neighbour that bf16() did not choose"""
    u, shape = _bits(v)
    up = (u + 0x7fff + ((u >> 16) & 1)) >> 16
    r = np.where(up == (u >> 16), (u >> 16) + 1, u >> 16) << 16
    return (r & 0xffffffff).astype(np.uint32).view(f32).reshape(shape)


def _fma(a, b, c):
    """fp32 fma through float64: the product of two floats is exact there, the sum is rounded once more on the way back (a double
    rounding that needs the float64 sum to land on a float32 tie: about 2^-29 an operation)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


# ---- the tables: upload_wide restated ----------------------------------------------------------------------------------------
def front_stage_floats(F, I, tile=512):
    return (tile - 1) * F + I + 32 + tile + I // max(F, 1)


def front_fits(F, I):
    """wide_front_fits: the columns under 512 evaluations and their sums of squares behind two chunk buffers in 150 KB of LDS"""
    return front_stage_floats(F, I) * 4 + 2 * 21 * 64 * 16 <= 150 * 1024


def _fn_params(f):
    return np.asarray(f.xOffsets, f32).astype(f64), np.asarray(f.gains, f32).astype(f64), float(f32(f.y))


def plan(cfg, F, no_front=False, shape32=False, tanh_poly=False, exact=False):
    """The route and the folded tables for a band of F bins.  exact: no rounding anywhere (the folding alone, for the host test)."""
    net = cfg.net
    assert len(net.layers) == 2
    L0, L1 = net.layers
    I, H, n_out = int(L0.inputs), int(L0.outputs), int(L1.outputs)
    assert I <= K and I % F == 0 and H >= 32 and n_out <= 4
    p = SimpleNamespace(I=I, F=int(F), T=I // F, H=H, n_out=n_out, exact=exact, scaling=cfg.spectrogramScaling,
                        chain=list(net.inputProcessing), tf0=L0.transferFunction, tf1=L1.transferFunction)
    front = (not shape32) and (not no_front) and cfg.spectrogramScaling == "linear" and front_fits(F, I)
    l2 = False
    fa, fo = np.ones(I), np.zeros(I)
    for k, f in enumerate(net.inputProcessing):
        if not front:
            break
        if f.function == "l2normalize" and k == 0:
            l2 = True
            continue
        if f.function not in ("mapminmax", "mapstd"):
            front = False
            break
        xo, ga, y = _fn_params(f)
        fo = (fo - xo) * ga + y
        fa = fa * ga
    if front and not (np.abs(fo).max(initial=0.0) <= 4.0):
        front = False
    p.front, p.l2 = front, bool(l2 and front)
    p.sig = p.tf0 in ("TanSig", "LogSig")
    tansig = p.tf0 == "TanSig"
    p.poly = bool(p.sig and (not shape32) and front and n_out == 1 and tanh_poly)
    sc = 1.0 if not p.sig else ((1.0 if tansig else 0.5) if p.poly else (2.8853900817779268 if tansig else -1.4426950408889634))
    w1s = 1.0 if not p.sig else ((1.0 if tansig else 0.5) if p.poly else (-2.0 if tansig else 1.0))
    rnd = (lambda a: np.asarray(a, f64)) if exact else (lambda a: np.asarray(a, f64).astype(f32).astype(f64))
    W = np.asarray(L0.weights, f32).reshape(H, I).astype(f64)
    Wf = sc * W * (fa[None, :] if front else 1.0)
    p.Wq = Wf if exact else bf16(Wf.astype(f32)).astype(f64)
    b = np.asarray(L0.biases, f32).astype(f64).copy()
    if front:
        for i in range(I):
            b = b + W[:, i] * fo[i]
    p.bias = rnd(sc * b)
    W1 = np.asarray(L1.weights, f32).reshape(n_out, H).astype(f64)
    p.w1 = rnd(w1s * W1)
    b1 = np.asarray(L1.biases, f32).astype(f64)
    if p.sig and not p.poly and tansig:
        b1 = np.array([np.cumsum(np.concatenate([[b1[o]], W1[o]]))[-1] for o in range(n_out)])
    if p.poly and not tansig:
        b1 = np.array([np.cumsum(np.concatenate([[b1[o]], 0.5 * W1[o]]))[-1] for o in range(n_out)])
    p.b1 = rnd(b1)
    p.out_maps = [_fn_params(f) for f in net.outputProcessing]
    return p


# ---- operands ---------------------------------------------------------------------------------------------------------------
def _frames(J, T, late=False):
    idx = np.arange(J - T + 1)[:, None] + np.arange(T)[None, :]
    if late:
        idx[:, -1] = np.minimum(idx[:, -1] + 1, J - 1)
    return idx


def _front_values(p, cols, fault=None):
    """fl32(v * rinv) [E][I]: the kernel front's values before the bf16 conversion"""
    J = cols.shape[0]
    idx = _frames(J, p.T)
    v = cols[_frames(J, p.T, late=fault == "last_frame_late")].reshape(-1, p.I)
    if p.exact:
        v = v.astype(f64)
        return v / np.sqrt((v * v).sum(axis=1, keepdims=True)) if p.l2 else v
    if not p.l2:
        return v
    css = np.zeros(J, f32)
    for b in range(p.F):                                          # a = fmaf(x, x, a)
        css = _fma(cols[:, b], cols[:, b], css)
    ss = np.zeros(idx.shape[0], f32)
    for tt in range(p.T - 1 if fault == "norm_T_minus_1" else p.T):
        ss = ss + css[idx[:, tt]]
    rinv = f32(1.0) / np.sqrt(ss)                                 # (silence: 0 * inf = NaN, as the reference's 0 / 0)
    return v * rinv[:, None]


def _lanes(x):
    """[E][320] -> [E][5][64]: element i in lane i % 64, register i / 64"""
    return x.reshape(x.shape[0], K // 64, 64)


def _tree(s):
    while s.shape[1] > 1:
        s = s[:, 0::2] + s[:, 1::2]
    return s[:, 0]


def _lane_dot(a, b, first_two_swapped=False):
    """a lane's five products added by fma in register order, then the tree over the lanes.  first_two_swapped: the sum starts
    from the SECOND product (the compiler's choice for `s = 0; s += x0 x0; s += x1 x1`: fl(x1 x1) first, x0 x0 fused onto it)"""
    s = np.zeros((a.shape[0], 64), f32)
    for k in ((1, 0, 2, 3, 4) if first_two_swapped else range(K // 64)):
        s = _fma(_lanes(a)[:, k], _lanes(b)[:, k], s)
    return _tree(s)


def _chain_values(p, cols):
    """u [E][I]: scaling and the input chain as wide_prep_kernel / wide_prep_chain_kernel make them, in fp32 (exact: the
    reference's definitions in float64)"""
    J = cols.shape[0]
    I = p.I
    v = cols[_frames(J, p.T)].reshape(-1, I)
    names = [f.function for f in p.chain]
    if p.exact:
        x = v.astype(f64)
        x = np.log(x) if p.scaling == "log" else 20.0 * np.log10(x) if p.scaling == "db" else x
        for f in p.chain:
            if f.function == "l2normalize":
                x = x / np.sqrt((x * x).sum(axis=1, keepdims=True))
            elif f.function == "normalize":
                mn, mx = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
                x = np.where(mx == mn, -1.0, 2 * (x - mn) / (mx - mn) - 1)
            elif f.function == "normalizestd":
                x = (x - x.mean(axis=1, keepdims=True)) / x.std(axis=1, keepdims=True)
            else:
                xo, ga, y = _fn_params(f)
                x = (x - xo) * ga + y
        return x
    E = v.shape[0]
    x = np.zeros((E, K), f32)
    x[:, :I] = v
    valid = np.arange(K) < I
    if p.scaling == "log":                                       # logf / log10f as the correctly rounded values (the device's are within an ulp of them)
        x[:, :I] = np.log(v.astype(f64)).astype(f32)
    elif p.scaling == "db":
        x[:, :I] = f32(20.0) * np.log10(v.astype(f64)).astype(f32)
    affine = lambda n: n in ("mapminmax", "mapstd")
    special = (len(names) == 2 and names[0] == "l2normalize" and affine(names[1])) or (len(names) == 1 and affine(names[0]))
    for q, f in enumerate(p.chain):
        if f.function == "l2normalize":
            s = np.sqrt(_lane_dot(x, x, first_two_swapped=True))
            if special:                                           # x inv - xoff is ONE fma there (contracted), then the gain's
                xo, ga, y = _fn_params(p.chain[1])
                pad = lambda a: np.concatenate([a, np.zeros(K - I)]).astype(f32)
                x = _fma(pad(ga), _fma((f32(1.0) / s)[:, None], x, -pad(xo)), f32(y))
                x = np.where(valid, x, f32(0.0)).astype(f32)
                break
            x = x / s[:, None]
        elif f.function == "normalize":
            mn = np.where(valid, x, np.inf).min(axis=1).astype(f32)
            mx = np.where(valid, x, -np.inf).max(axis=1).astype(f32)
            rng = mx - mn
            slope, icpt = f32(2.0) / rng, (f32(0.0) - mn - mx) / rng
            x = np.where((rng == 0)[:, None], f32(-1.0), _fma(x, slope[:, None], icpt[:, None]))
        elif f.function == "normalizestd":
            s = np.zeros((E, 64), f32)
            for k in range(K // 64):
                s = s + _lanes(x)[:, k]
            mean = _tree(s) / f32(I)
            d = np.where(valid, x - mean[:, None], f32(0.0)).astype(f32)
            sd = np.sqrt(_lane_dot(d, d) / f32(I))
            x = (x - mean[:, None]) / sd[:, None]
        else:
            xo, ga, y = _fn_params(f)
            pad = lambda a: np.concatenate([a, np.zeros(K - I)]).astype(f32)
            x = _fma(x - pad(xo), pad(ga), f32(y))
        x = np.where(valid, x, f32(0.0)).astype(f32)
    return x[:, :I]


# ---- the network behind the operands -------------------------------------------------------------------------------------
def _transfer(tf, x):
    if tf == "TanSig":
        return np.tanh(x)
    if tf == "LogSig":
        return 1.0 / (1.0 + np.exp(-x))
    if tf == "SatLin":
        return np.where(np.isnan(x), x, np.clip(x, 0.0, 1.0))
    return x


def _poly(x):
    x = np.where(np.isnan(x), x, np.clip(x, -POLY_CLAMP, POLY_CLAMP))
    u = x * x
    q = np.full_like(x, POLY[6])
    for c in POLY[5::-1]:
        q = q * u + c
    return q * x


def _tables(p, fault):
    Wq, bias, w1 = p.Wq, p.bias, p.w1
    ch = min(1, (p.H + 31) // 32 - 1)                            # the chunk the chunk faults hit: the second, or the only one
    u0, u1 = 32 * ch, min(32 * ch + 32, p.H)
    unit = u0 + int(np.argsort(np.abs(p.w1[0, u0:u1]))[(u1 - u0) // 4])   # the unit the unit faults hit: the chunk's lower-quartile |w1|
    if fault == "k_tail_missing_in_chunk":
        Wq = Wq.copy()
        Wq[u0:u1, p.I - (p.I % 32 or 32):] = 0.0                 # (I = 290: inputs 288, 289)
    elif fault == "input_missing":
        Wq = Wq.copy()
        Wq[unit, p.I // 2] = 0.0
    elif fault == "bias_rotated":
        bias = bias.copy()
        bias[u0:u1] = np.roll(bias[u0:u1], 1)
    elif fault == "unit_term_lost":
        w1 = w1.copy()
        w1[:, unit] = 0.0
    return Wq, bias, w1, unit


def _forward(p, X, fault=None, rows=None):
    """operands X [n][I] (float64 holding bf16 values) -> outputs [n][n_out]; rows: the evaluation number of every row"""
    Wq, bias, w1, unit = _tables(p, fault)
    if fault == "kstep_missing":
        X = X.copy()
        X[:, 32:64] = 0.0
    with np.errstate(all="ignore"):
        acc = bias[None, :] + X @ Wq.T
        if p.poly:
            h = _poly(acc)
        elif p.sig:
            h = 1.0 / (np.exp2(acc) + 1.0)
        else:
            h = _transfer(p.tf0, acc)
        y = h @ w1.T + p.b1[None, :]
        if fault == "product_lost_3pct":
            hit = (np.arange(len(X)) if rows is None else np.asarray(rows)) % 33 == 0
            y = y - np.where(hit[:, None], h[:, unit:unit + 1] * w1[None, :, unit], 0.0)
        y = _transfer(p.tf1, y)
        for yy, ga, xo in [(m[2], m[1], m[0]) for m in p.out_maps]:
            y = (y - yy) / ga[None, :] + xo[None, :]
    return y


def evaluate(cfg, cols, no_front=False, shape32=False, tanh_poly=False, exact=False, fault=None, w=None):
    """cols [J][F] float32, one channel -> the model's result:
         out [E][n_out] float64   the outputs with every operand rounded to nearest even
         near [E]                 operands within w ulps of a bf16 boundary
         alts {e: [2^k - 1][n_out]}  for 1 <= near[e] <= 3: the outputs of every other combination of roundings
         left_out [E] bool        near[e] > 3: no statement about this evaluation
         operands [E][I] float64, values [E][I] float32 (the operands before the conversion), plan, route ("front" | "prepared"), w"""
    cols = np.ascontiguousarray(cols, f32)
    assert fault is None or fault in FAULTS, fault
    p = plan(cfg, cols.shape[1], no_front, shape32, tanh_poly, exact)
    E = cols.shape[0] - p.T + 1
    assert E >= 1
    with np.errstate(all="ignore"):
        val = _front_values(p, cols, fault) if p.front else _chain_values(p, cols)
    w = (W_FRONT if p.front else W_PREPARED) if w is None else w
    res = SimpleNamespace(plan=p, route="front" if p.front else "prepared", w=w, alts={})
    if exact:
        res.operands, res.near, res.left_out = val, np.zeros(E, int), np.zeros(E, bool)
        res.out = _forward(p, val, fault)
        return res
    X = bf16(val, truncate=fault == "truncation").astype(f64)
    res.operands, res.values = X, val
    res.out = _forward(p, X, fault)
    near = near_boundary(val, w)
    res.near = near.sum(axis=1)
    res.left_out = res.near > MAX_NEAR
    todo = np.nonzero((res.near >= 1) & ~res.left_out)[0]
    if len(todo):
        other = bf16_other(val).astype(f64)
        rows, owner = [], []
        for e in todo:
            at = np.nonzero(near[e])[0]
            for pick in itertools.product((0, 1), repeat=len(at)):
                if any(pick):
                    r = X[e].copy()
                    sel = at[np.array(pick, bool)]
                    r[sel] = other[e, sel]
                    rows.append(r)
                    owner.append(e)
        alt = _forward(p, np.array(rows), fault, rows=owner)
        owner = np.array(owner)
        res.alts = {int(e): alt[owner == e] for e in todo}
    return res


def evaluate32(res):
    """The same model with fp32 sums in one fixed order, [E][n_out]: a k-step of 32 inputs summed exactly and added to an fp32
    accumulator that starts at the bias, in k order; the hidden values in fp32; a unit's second-layer term by fp32 fma, four running
    sums (units 4g .. 4g + 3 of every 16) in unit order, added pairwise at the end; f1 and the output maps in fp32.  The polynomial
    by fp32 Horner.  |evaluate32 - evaluate| is `own`: what fp32 sums cost the model itself."""
    p, X = res.plan, res.operands
    n = X.shape[0]
    Hp = (p.H + 31) // 32 * 32
    Wq = np.zeros((Hp, p.I))
    Wq[:p.H] = p.Wq
    bias, w1 = np.zeros(Hp), np.zeros((p.n_out, Hp))
    bias[:p.H], w1[:, :p.H] = p.bias, p.w1
    one = f32(1.0)
    with np.errstate(all="ignore"):
        acc = np.broadcast_to(bias.astype(f32), (n, Hp)).copy()
        for k0 in range(0, p.I, 32):
            acc = (acc.astype(f64) + X[:, k0:k0 + 32] @ Wq[:, k0:k0 + 32].T).astype(f32)
        if p.poly:
            x = np.where(np.isnan(acc), acc, np.clip(acc, f32(-POLY_CLAMP), f32(POLY_CLAMP))).astype(f32)
            u = x * x
            q = np.full_like(x, f32(POLY[6]))
            for c in POLY[5::-1]:
                q = _fma(q, u, f32(c))
            h = q * x
        elif p.sig:
            h = one / (np.exp2(acc) + one)
        else:
            h = _transfer(p.tf0, acc.astype(f64)).astype(f32)
        order = lambda a: a.reshape(a.shape[:-1] + (Hp // 16, 4, 4)).swapaxes(-3, -2).reshape(a.shape[:-1] + (4, Hp // 4))
        hg = order(h)                                             # [n][g][its units in order]
        y = np.zeros((n, p.n_out), f32)
        for o in range(p.n_out):
            wg = order(w1[o].astype(f32))
            s = np.zeros((n, 4), f32)
            for j in range(Hp // 4):
                s = _fma(wg[None, :, j], hg[:, :, j], s)
            y[:, o] = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
        y = y + p.b1.astype(f32)[None, :]
        y = _transfer(p.tf1, y.astype(f64)).astype(f32)
        for xo, ga, yy in p.out_maps:
            y = (y - f32(yy)) / ga.astype(f32)[None, :] + xo.astype(f32)[None, :]
    return y.astype(f64)


def own_of(res):
    """the model's own fp32 spread per evaluation, relative to max(1, |model|)"""
    y32 = evaluate32(res)
    ok = np.isfinite(res.out).all(axis=1) & np.isfinite(y32).all(axis=1)
    own = np.zeros(len(res.out))
    own[ok] = (np.abs(y32[ok] - res.out[ok]) / np.maximum(1.0, np.abs(res.out[ok]))).max(axis=1)
    return own


# ---- the rule --------------------------------------------------------------------------------------------------------------
def bar_of(own, tol=TOL):
    """the suite's bar per evaluation: 1e-5 relative to max(1, |model|), or 4x the model's own fp32 spread AT THAT EVALUATION
    where that is larger"""
    return np.maximum(tol, 4.0 * np.asarray(own, f64))


def compare(res, got, bar):
    """One channel's engine outputs `got` [E][n_out] against the model under the rule: per evaluation |got - model| <=
    bar max(1, |model|) for the nearest-even roundings or, where the model names near ties, for one of their combinations; NaN / inf
    exactly where the model has them; left-out evaluations are not judged.
    -> dict: worst (relative error over the judged evaluations, the best combination taken), bad (evaluations that fail),
       alt_needed (evaluations that needed another rounding), left_out, judged"""
    got = np.asarray(got, f64).reshape(res.out.shape)
    bars = np.broadcast_to(np.asarray(bar, f64), (len(got),))          # one bar, or one per evaluation
    rel = lambda a, m: float((np.abs(a - m) / np.maximum(1.0, np.abs(m))).max())
    worst, bad, alt_needed = 0.0, [], 0
    finite_m, finite_g = np.isfinite(res.out), np.isfinite(got)
    with np.errstate(all="ignore"):
        err = np.abs(got - res.out) / np.maximum(1.0, np.abs(res.out))
    for e in range(len(got)):
        if res.left_out[e]:
            continue
        bar = float(bars[e])
        if not finite_m[e].all() or not finite_g[e].all():
            m, g = res.out[e], got[e]
            inf = np.isinf(m)
            ok = np.array_equal(np.isnan(m), np.isnan(g)) and np.array_equal(inf, np.isinf(g)) and bool((m[inf] == g[inf]).all())
            if ok and finite_m[e].any():
                ok = rel(g[finite_m[e]], m[finite_m[e]]) <= bar
            if not ok:
                bad.append(e)
            continue
        ee = float(err[e].max())
        if ee > bar and e in res.alts:
            cand = [rel(got[e], a) for a in res.alts[e] if np.isfinite(a).all()]
            if cand and min(cand) <= bar:
                ee = min(cand)
                alt_needed += 1
        worst = max(worst, ee)
        if ee > bar:
            bad.append(e)
    return {"worst": worst, "bad": bad, "alt_needed": alt_needed, "left_out": int(res.left_out.sum()),
            "judged": int((~res.left_out).sum()), "near_evaluations": int((res.near >= 1).sum())}


def decisions(res, thresholds, rule, bar):
    """-> (want [E] uint8, safe [E] bool): the model's decision (output >= threshold: output 0 under rule 0, any under rule 1; a NaN
    never hits), and where it binds the engine: every rounding combination the model names gives the same decision and lies
    farther than twice the bar from the threshold, and the evaluation is not left out"""
    thr = np.asarray(thresholds, f64)[None, :]
    cols = slice(0, 1) if int(rule) == 0 else slice(None)
    bars = np.broadcast_to(np.asarray(bar, f64), (len(res.out),))      # one bar, or one per evaluation

    def judge(o, b):
        with np.errstate(invalid="ignore"):
            hit = (o >= thr)[:, cols].any(axis=1)
            far = ((np.abs(o - thr) > 2 * np.reshape(b, (-1, 1)) * np.maximum(1.0, np.abs(o))) | np.isnan(o))[:, cols].all(axis=1)
        return hit, far
    want, safe = judge(res.out, bars)
    safe = safe & ~res.left_out
    for e, alt in res.alts.items():
        h, f = judge(alt, bars[e])
        safe[e] = safe[e] and bool(f.all()) and bool((h == want[e]).all())
    return want.astype(np.uint8), safe


def near_shares(res):
    """(share of evaluations with a near tie, share left out)"""
    E = len(res.near)
    return float((res.near >= 1).sum()) / E, float(res.left_out.sum()) / E


NEAR_LIMIT = {"front": 0.05, "prepared": 0.15}
LEFT_OUT_LIMIT = 0.01
