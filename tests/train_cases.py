"""The networks the training tests share (tests/test_train_host.py, tests/test_train_gpu.py): a small 7-bin network (timeRange 3,
21 -> 3 -> 2) with any transfer functions, chain and scaling, and variants of the sample network."""
import copy

import numpy as np

import util
from syllable_detector_swift_amd import NeuralNet, NeuralNetLayer, SyllableDetectorConfig, nets

SMALL_BINS, SMALL_T, SMALL_H, SMALL_O = 7, 3, 3, 2


def small_net(tf0="TanSig", tf1="PureLin", in_fns=("l2normalize", "mapminmax"), out_fns=("mapminmax",), scaling="linear", seed=0):
    """7 bins (1000 .. 2100 Hz of 256-point frames), timeRange 3, 21 -> 3 -> 2"""
    rng = np.random.default_rng(seed)
    net = nets.random_net(rng, SMALL_BINS * SMALL_T, [SMALL_H], SMALL_O, transfer=(tf0, tf1), in_fns=tuple(in_fns), out_fns=tuple(out_fns))
    cfg = SyllableDetectorConfig(44100.0, 256, 256, 124, (1000.0, 2100.0), SMALL_T, scaling, [0.5] * SMALL_O, net)
    assert cfg.geometry().bins == SMALL_BINS
    return cfg


def sample_wide(hidden=16, outputs=4, tf0="SatLin", tf1="PureLin", seed=3):
    """the sample front with `hidden` units and `outputs` outputs"""
    base = util.sample_net()
    rng = np.random.default_rng(seed)
    cfg = copy.deepcopy(base)
    I = base.net.inputs
    new = nets.random_net(rng, I, [hidden], outputs, transfer=(tf0, tf1), in_fns=(), out_fns=("mapminmax",))
    # (SatLin is flat outside (0, 1): biases of a half put the units' sums inside it for about half the evaluations)
    new.layers[0].biases = (0.5 + 0.2 * rng.standard_normal(hidden)).astype(np.float32)
    cfg.net = NeuralNet(new.layers, copy.deepcopy(base.net.inputProcessing), new.outputProcessing)
    cfg.thresholds = [0.5] * outputs
    return cfg


def fit_map(cfg, bins, cols_list):
    """refits cfg's first mapminmax input function to the windows of the columns in cols_list (each [J, F]), from the float64 model
    of the functions in front of it: xOffsets = min, gains = 2 / (max - min), yMin = -1 -- so that the mapped inputs fill [-1, 1] and
    the units behind them are not saturated, as on the data a network is trained on"""
    import train_ref as ref
    fns = cfg.net.inputProcessing
    at = next(k for k, f in enumerate(fns) if f.function == "mapminmax")
    front = copy.deepcopy(cfg)
    front.net.inputProcessing = fns[:at]
    net = ref.net_of(front, bins)
    x = np.concatenate([ref.inputs(net, c, np.arange(c.shape[0] - net.T + 1), np.float64) for c in cols_list if c.shape[0] >= net.T])
    lo, hi = x.min(axis=0), x.max(axis=0)
    assert (hi > lo).all()
    fns[at].xOffsets, fns[at].gains, fns[at].y = lo.astype(np.float32), (2.0 / (hi - lo)).astype(np.float32), -1.0
    return cfg


def spread_first_layer(cfg, net, cols):
    """scales and centres cfg's first layer so that over the windows of cols [J, F] every unit's sum has mean 0.5 and deviation 0.4
    (float64, the model's input chain) -> the share of those windows in which each unit lies inside (0, 1)"""
    import train_ref as ref
    x = ref.inputs(net, cols, np.arange(cols.shape[0] - net.T + 1), np.float64)
    L0 = cfg.net.layers[0]
    z = x @ np.asarray(L0.weights, np.float64).T
    L0.weights = (np.asarray(L0.weights, np.float64) * (0.4 / z.std(axis=0))[:, None]).astype(np.float32)
    z = x @ np.asarray(L0.weights, np.float64).T
    L0.biases = (0.5 - z.mean(axis=0)).astype(np.float32)
    a = z + L0.biases
    return ((a > 0) & (a < 1)).mean(axis=0)


def columns(rng, frames, bins, rows=None):
    """positive columns of the size a spectrogram's are, a few decades apart"""
    shape = (frames, bins) if rows is None else (rows, frames, bins)
    return (np.abs(rng.standard_normal(shape)) * 10.0 ** rng.uniform(-2, 1, shape) + 1e-3).astype(np.float32)


def planted_channel(seed, n=6 * 44100, every=11000, jitter=3000, noise=0.01):
    """-> (samples [n] float32, positions): 0.01 noise plus the template syllable about every 11 000 +- 3000 samples at amplitudes
    0.05 .. 0.6; the positions are the syllables' first samples"""
    from syllable_detector_swift_amd import synth
    rng = np.random.default_rng(seed)
    x = noise * rng.standard_normal(n)
    pos, at = int(rng.integers(0, every)), []
    while True:
        s = synth.syllable(util.template(), 132, 256, 12, 256, rng, amplitude=float(rng.uniform(0.05, 0.6)))
        if pos + s.size > n:
            break
        x[pos:pos + s.size] += s
        at.append(pos)
        pos += every + int(rng.integers(-jitter, jitter + 1))
    return np.clip(x, -1.0, 1.0).astype(np.float32), np.array(at, np.int64)


def seeded_theta(rng, I, H, O):
    """1 / sqrt(fan-in) weights, hidden biases 0.2 N(0, 1), output biases 0"""
    return np.concatenate([(rng.standard_normal((H, I)) / np.sqrt(I)).reshape(-1), 0.2 * rng.standard_normal(H),
                           (rng.standard_normal((O, H)) / np.sqrt(H)).reshape(-1), np.zeros(O)]).astype(np.float32)


def theta_of(cfg):
    return np.concatenate([np.asarray(a, np.float32).reshape(-1) for L in cfg.net.layers for a in (L.weights, L.biases)])
