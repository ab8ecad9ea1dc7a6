"""Every compiled instantiation ("leaf") of the three fused kernels, and a case that reaches it.

- `leaves()` reads the launchers' source (the `launch_one<...>` lines of kernels_fused.hip, kernels_fused_r.hip and
  kernels_fused_s.hip, their SD_* macros expanded, diagnostic builds' blocks dropped) and returns the set of
  (kernel, ten template arguments) tuples the shipped library compiles -- the shape syldet_last_fused_form reports.
- `CASES` holds one entry per leaf: a configuration, the environment switches it needs (none where a public configuration
  reaches the leaf) and the leaf.  tests/test_forms_host.py holds the table to the scan (a new or changed leaf fails there until a
  case reaches it); tests/test_forms_gpu.py runs every entry against the fp64 anchor and asks the library which leaf ran.
- `UNREACHABLE`: leaves no configuration and no switch of the shipped build reaches, each with the reason from the code.
- `BAND_CASES`: the band edges of the fold kernel's host-built tables (DC in the band, odd / even first bins, 1 .. 64 bins, a band
  that ends at N/2 - 1) on its once- and twice-folded forms.
"""
import os
import re
from collections import namedtuple

import numpy as np

import util
from syllable_detector_swift_amd import nets
from syllable_detector_swift_amd.config import SyllableDetectorConfig, frequencyIndexRange

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "syllable_detector_swift_amd", "csrc")
FILES = {0: "kernels_fused.hip", 1: "kernels_fused_r.hip", 2: "kernels_fused_s.hip"}       # kernel numbers as in fused_choice
FS = 44100.0

# positions of the fold kernel's template arguments in a leaf's parameter tuple
S_K2, S_GEN, S_HQ, S_NW, S_PADP, S_F2, S_NT, S_SPECT, S_MN, S_S16 = range(10)


# ---- the scanner ---------------------------------------------------------------------------------------------------------------
def _constants():
    """The named integer constants of kernels.hpp (a launcher passes kFusedMaxLoads as a template argument)."""
    text = open(os.path.join(CSRC, "kernels.hpp")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (k\w+) = (\d+);", text)}


def _logical_lines(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out, cur = [], ""
    for line in text.split("\n"):
        line = re.sub(r"//.*$", "", line).rstrip()
        if line.endswith("\\"):
            cur += line[:-1] + " "
            continue
        out.append(cur + line)
        cur = ""
    return out


def _condition(directive, expr):
    """Is a conditional block compiled into the shipped library?  No SYLDET_* build macro is defined there."""
    if directive == "ifdef":
        return False
    if directive == "ifndef":
        return True
    py = re.sub(r"defined\s*\(\s*\w+\s*\)|defined\s+\w+", "False", expr).replace("&&", " and ").replace("||", " or ").replace("!", " not ")
    return bool(eval(py, {"__builtins__": {}}, {}))            # (what is left of an #if over SYLDET_* macros: booleans)


def _expand(text, macros):
    """Function-like SD_* macros of the file, expanded until none is left (SD_EXACT_ALL invokes SD_EXACT)."""
    for _ in range(16):
        hit = False
        for name, (params, body) in macros.items():
            def sub(m):
                args = [a.strip() for a in m.group(1).split(",")]
                if len(args) != len(params):
                    return m.group(0)
                r = body
                for p, a in zip(params, args):
                    r = re.sub(r"\b%s\b" % re.escape(p), a, r)
                return r
            new = re.sub(r"\b%s\s*\(([^()]*)\)" % re.escape(name), sub, text)
            hit |= new != text
            text = new
        if not hit:
            return text
    raise AssertionError("macro expansion does not end")


def scan(path):
    """-> list of parameter tuples (ten integers each) of the launch_one<...> instantiations `path` compiles."""
    consts = _constants()
    macros, stack, taken, body = {}, [], [], []         # taken: has a branch of the open conditional been compiled?
    for line in _logical_lines(open(path).read()):
        m = re.match(r"\s*#\s*(ifdef|ifndef|if|else|elif|endif|define|undef)\b\s*(.*)$", line)
        if m:
            d, rest = m.group(1), m.group(2)
            if d in ("ifdef", "ifndef", "if"):
                stack.append(_condition(d, rest))
                taken.append(stack[-1])
            elif d == "else":
                stack[-1] = not taken[-1]
            elif d == "elif":
                stack[-1] = not taken[-1] and _condition("if", rest)
                taken[-1] = taken[-1] or stack[-1]
            elif d == "endif":
                stack.pop()
                taken.pop()
            elif all(stack):
                if d == "define":
                    dm = re.match(r"(SD_\w+)\(([^)]*)\)\s*(.*)$", rest)
                    if dm and "launch_one" in dm.group(3) or dm and re.search(r"\bSD_\w+\s*\(", dm.group(3)):
                        macros[dm.group(1)] = ([p.strip() for p in dm.group(2).split(",")], dm.group(3))
                else:
                    macros.pop(rest.strip(), None)
            continue
        if all(stack):
            body.append(_expand(line, macros) if macros else line)
    assert not stack, "unbalanced conditionals in %s" % path
    text = "\n".join(body)
    # the defaulted template arguments of launch_one
    tm = re.search(r"template\s*<([^>]*)>\s*hipError_t\s+launch_one\s*\(", text)
    assert tm, "no launch_one in %s" % path
    defaults = []
    for p in tm.group(1).split(","):
        defaults.append(p.split("=")[1].strip() if "=" in p else None)
    n_params = len(defaults)
    word = {"true": 1, "false": 0}

    def value(tok):
        tok = tok.strip()
        if tok in word:
            return word[tok]
        if tok in consts:
            return consts[tok]
        return int(tok) if re.fullmatch(r"-?\d+", tok) else None

    out = []
    for stmt in re.split(r"[;{}]", text):
        if "d.stamps" in stmt:                                  # the stamped diagnostic instantiation: never without its build
            continue
        for m in re.finditer(r"launch_one\s*<([^<>]*)>\s*\(", stmt):
            args = [value(t) for t in m.group(1).split(",")]
            if any(a is None for a in args):                    # launch_one's own recursion into its multi-network twin
                continue
            args += [value(d) for d in defaults[len(args):]]
            assert len(args) == n_params and None not in args, (path, m.group(0))
            out.append(tuple(args + [0] * (10 - n_params)))
    return out


def leaves():
    """The set of (kernel, (p0 .. p9)) the shipped library compiles, single-network forms."""
    return {(k, p) for k, name in FILES.items() for p in scan(os.path.join(CSRC, name))}


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# cfg: a SyllableDetectorConfig; env: the SYLDET_FUSED_* switches the handle is created under; leaf: what it must run;
# spect: the leaf is a spectrogram instantiation (syldet_spectrogram_device); s16: the batch is 16-bit PCM; cls: how to draw
# another network of the case's class (a multi-network bank's second network)
Case = namedtuple("Case", "name cfg env leaf spect s16 cls")


def band(N, f0, F):
    """A freqRange that gives bins [f0, f0 + F) of N-point frames (as draw() of tests/test_fuzz_gpu.py makes one)."""
    lo, hi = max((f0 - 0.4) * FS / N, 0.0), (f0 + F - 1 + 0.4) * FS / N
    r = frequencyIndexRange(N, FS, lo, hi)
    assert (r[0], r[1] - r[0]) == (f0, F), (N, f0, F, r)
    return lo, hi


EXAMPLE = dict(transfer=("TanSig", "PureLin"), in_fns=("l2normalize", "mapminmax"), out_fns=("mapminmax",))   # the reference's example class
RUNTIME = dict(transfer=("LogSig", "PureLin"), in_fns=("l2normalize", "mapstd"), out_fns=())                    # ... with run-time network facts


def make(seed, N, W, hop, f0, F, T, H, n_out=1, rule=0, **cls):
    """A configuration of the given framing and band with a random network of the given class, from a fixed seed."""
    cls = dict(EXAMPLE, **cls)
    rng = np.random.default_rng(seed)
    net = nets.random_net(rng, F * T, (H,), n_out, **cls)
    return SyllableDetectorConfig(FS, N, W, W - hop, band(N, f0, F), T, "linear", [0.0] * n_out, net, rule=rule)


def sibling(case, seed):
    """Another network of the case's class (compatible with it: the second network of a two-network bank)."""
    c = case.cfg
    L = c.net.layers
    rng = np.random.default_rng(seed)
    net = nets.random_net(rng, L[0].inputs, (L[0].outputs,), L[-1].outputs, **case.cls)
    return nets.variant(c, net=net)


def _cases():
    out, seed = [], [5000]

    def add(name, leaf, N, W, hop, f0, F, T, H, env=None, spect=False, s16=False, n_out=1, rule=0, **cls):
        seed[0] += 1
        full = dict(EXAMPLE, **cls)
        out.append(Case(name, make(seed[0], N, W, hop, f0, F, T, H, n_out, rule, **cls), dict(env or {}), leaf, spect, s16, full))

    # ---- kernels_fused_s.hip (kernel 2): <K2, GEN, HQ, NW, PADP, F2, NT, SPECT, MN, S16> ----
    def s(K2, GEN, HQ, NW, PADP=0, F2=0, NT=1, SPECT=0, MN=0, S16=0):
        return (2, (K2, GEN, HQ, NW, PADP, F2, NT, SPECT, MN, S16))
    # the once-folded forms, SD_S_GO(K2): W = 64 K2 (W = 256 under zero padding, N = 512: the twice-folded form needs W == N)
    for K2 in (1, 2, 3, 4):
        W = 64 * K2
        N = {64: 64, 128: 128, 192: 256, 256: 512}[W]
        f0 = {64: 3, 128: 6, 192: 11, 256: 24}[W]
        F = {64: 13, 128: 22, 192: 29, 256: 30}[W]
        hop = {64: 52, 128: 100, 192: 132, 256: 132}[W]
        add("s_go%d_h16" % K2, s(K2, 1, 4, 4), N, W, hop, f0, F, 5, 16)
        add("s_go%d_h11" % K2, s(K2, 1, 3, 4), N, W, hop, f0, F, 4, 11, n_out=2, rule=1, **RUNTIME)
        add("s_go%d_h7_w8" % K2, s(K2, 1, 2, 8), N, W, hop, f0, F, 3, 7)
        # (timeRange 12 under a hop of 116: the rows of tap products leave no room for eight waves' rings)
        add("s_go%d_h6_w4" % K2, s(K2, 1, 2, 4), N, W, 116, f0, F, 12, 6, **RUNTIME)
        add("s_go%d_exact" % K2, s(K2, 0, 1, 8), N, W, hop, f0, F, 6, 4)
        add("s_go%d_gen" % K2, s(K2, 1, 1, 8), N, W, hop, f0, F, 7, 3, n_out=3, rule=1, **RUNTIME)
    # hops that are multiples of 64 under a 256-sample window: the padded rings, once-folded (N = 512) and twice-folded (N = 256)
    add("s_pad64_exact", s(4, 0, 1, 8, 64), 512, 256, 64, 24, 30, 5, 4)
    add("s_pad64_gen", s(4, 1, 1, 8, 64), 512, 256, 64, 24, 30, 5, 2, **RUNTIME)
    add("s_pad128_exact", s(4, 0, 1, 8, 128), 512, 256, 128, 24, 30, 5, 4)
    add("s_pad128_gen", s(4, 1, 1, 8, 128), 512, 256, 128, 24, 30, 5, 2, **RUNTIME)
    add("s_pad64_f2_exact", s(4, 0, 1, 8, 64, 1), 256, 256, 64, 12, 29, 5, 4)
    add("s_pad64_f2_gen", s(4, 1, 1, 8, 64, 1), 256, 256, 64, 12, 29, 5, 3, **RUNTIME)
    # (hop 128 takes the staggered chunks below; the twice-folded padded-128 ring is public at hop 256, whose ring fits for timeRange <= 2)
    add("s_pad128_f2_exact", s(4, 0, 1, 8, 128, 1), 256, 256, 256, 12, 29, 2, 4)
    add("s_pad128_f2_gen", s(4, 1, 1, 8, 128, 1), 256, 256, 256, 12, 29, 2, 3, **RUNTIME)
    add("s_cs8_exact", s(4, 0, 1, 8, 1, 1), 256, 256, 128, 12, 29, 10, 4)
    add("s_cs8_gen", s(4, 1, 1, 8, 1, 1), 256, 256, 128, 12, 29, 4, 1, **RUNTIME)
    # bands of 33 .. 64 bins: two row tiles per parity
    add("s_nt2_exact", s(4, 0, 1, 4, 0, 1, 2), 256, 256, 132, 7, 45, 4, 4)
    add("s_nt2_gen", s(4, 1, 1, 4, 0, 1, 2), 256, 256, 100, 10, 64, 3, 2, n_out=2, **RUNTIME)
    # the twice-folded form, W == N == 256
    add("s_f2_h13", s(4, 1, 4, 4, 0, 1), 256, 256, 132, 12, 29, 5, 13)
    add("s_f2_h9", s(4, 1, 3, 4, 0, 1), 256, 256, 120, 12, 29, 4, 9, **RUNTIME)
    add("s_f2_h8_w8_hop64", s(4, 1, 2, 8, 0, 1), 256, 256, 64, 12, 29, 3, 8)
    add("s_f2_h5_w4", s(4, 1, 2, 4, 0, 1), 256, 256, 116, 12, 29, 12, 5)
    add("s_f2_exact", s(4, 0, 1, 8, 0, 1), 256, 256, 132, 12, 29, 10, 4)
    add("s_f2_gen", s(4, 1, 1, 8, 0, 1), 256, 256, 132, 12, 29, 8, 3, n_out=4, rule=1, **RUNTIME)
    # 16-bit PCM read natively
    add("s_s16_exact", s(4, 0, 1, 8, 0, 1, 1, 0, 0, 1), 256, 256, 132, 12, 29, 10, 4, s16=True)
    add("s_s16_gen", s(4, 1, 1, 8, 0, 1, 1, 0, 0, 1), 256, 256, 100, 12, 29, 5, 2, s16=True, **RUNTIME)
    # the transform alone
    add("s_spect", s(4, 0, 1, 8, 0, 1, 1, 1), 256, 256, 132, 12, 29, 3, 2, spect=True)
    add("s_spect_pad64", s(4, 0, 1, 8, 64, 1, 1, 1), 256, 256, 64, 12, 29, 3, 2, spect=True)
    add("s_spect_pad128", s(4, 0, 1, 8, 128, 1, 1, 1), 256, 256, 256, 12, 29, 2, 2, spect=True)
    add("s_spect_cs8", s(4, 0, 1, 8, 1, 1, 1, 1), 256, 256, 128, 12, 29, 3, 2, spect=True)

    # ---- kernels_fused_r.hip (kernel 1): <KS, TMAX, NL, SKEW, STAMP, GEN> -- windows that are no multiple of 64 samples keep
    # the fold kernel out, at most 4 hidden units behind l2normalize bring this one in ----
    def r(KS, NL, SKEW, GEN):
        return (1, (KS, 12, NL, SKEW, 0, GEN, 0, 0, 0, 0))
    for KS, N, W, f0, F in ((4, 128, 100, 6, 22), (8, 256, 200, 12, 29)):
        for hop, NL, SKEW in ((48, 6, 1), (96, 9, 1), (16, 2, 16), (32, 3, 32), (64, 5, 64)):
            add("r_ks%d_hop%d" % (KS, hop), r(KS, NL, SKEW, 1), N, W, hop, f0, F, 4 + hop // 32, 1 + hop // 32, **(RUNTIME if hop % 32 else {}))
    add("r_ks4_hop128", r(4, 9, 128, 1), 128, 100, 128, 6, 22, 6, 4)                      # (a gap of 28 samples between windows)
    add("r_ks4_plain", r(4, 9, 0, 1), 128, 100, 84, 6, 22, 9, 3)
    add("r_ks8_hop128_exact", r(8, 9, 128, 0), 256, 200, 128, 12, 29, 10, 4)
    add("r_ks8_hop128_gen", r(8, 9, 128, 1), 256, 200, 128, 12, 29, 5, 2, n_out=2, **RUNTIME)
    add("r_ks8_plain_exact", r(8, 9, 0, 0), 256, 200, 132, 12, 29, 10, 4)
    add("r_ks8_plain_gen", r(8, 9, 0, 1), 256, 200, 132, 12, 29, 12, 2, n_out=4, rule=1, **RUNTIME)

    # ---- kernels_fused.hip (kernel 0): <KS, TMAX, NL, EXACT, SKEW, LEAN, STAMP, KNOCK, SPECT> -- the same windows with more
    # than 4 hidden units or a normalize chain keep the other two out ----
    def c(KS, TMAX, NL, EXACT, SKEW, LEAN=0, SPECT=0):
        return (0, (KS, TMAX, NL, EXACT, SKEW, LEAN, 0, 0, SPECT, 0))
    classes = ({}, RUNTIME, dict(in_fns=("normalize", "mapminmax")), dict(in_fns=("normalizestd", "mapstd"), transfer=("TanSig", "TanSig")))
    for KS, N, W, f0, F in ((8, 256, 200, 12, 29), (4, 128, 100, 6, 22)):
        for T in range(1, 13):
            for skew, hop in ((0, 132 if KS == 8 else 84), (1, 128 if KS == 8 else 96)):
                cls = classes[(T + skew) % 4]
                # (behind l2normalize only five or more hidden units keep the register-resident-basis kernel out)
                H = 1 + T % 4 if cls.get("in_fns", ("l2normalize",))[0] != "l2normalize" else 5 + (5 * T + skew) % 12
                add("c_exact_ks%d_t%d_%s" % (KS, T, "skew" if skew else "plain"), c(KS, T, 9, 1, skew), N, W, hop, f0, F, T, H,
                    n_out=1 + T % 3, rule=T % 2, **cls)
        # hops of 148 .. 160 stage ten quads a thread: the instantiations with run-time sizes (four k-steps only: UNREACHABLE below)
        for TM, T in ((4, 3), (8, 7), (12, 11)):
            for skew, hop in ((0, 148), (1, 160)) if KS == 4 else ():
                add("c_generic_ks%d_tm%d_%s" % (KS, TM, "skew" if skew else "plain"), c(KS, TM, 10, 0, skew), N, W, hop, f0, F, T, 6 + TM // 4,
                    **classes[(TM // 4 + skew) % 2])
        for skew, hop in ((0, 132 if KS == 8 else 84), (1, 128 if KS == 8 else 96)):
            add("c_spect_ks%d_%s" % (KS, "skew" if skew else "plain"), c(KS, 4, 10, 0, skew, 0, 1), N, W, hop, f0, F, 3, 2, spect=True)
    # the example shape's `lean` forms: its class is the other two kernels' too, so only SYLDET_FUSED_CLASSIC=1 brings it here
    add("c_lean_plain", c(8, 10, 9, 1, 0, 1), 256, 256, 132, 12, 29, 10, 4, env={"SYLDET_FUSED_CLASSIC": "1"})
    add("c_lean_skew", c(8, 10, 9, 1, 1, 1), 256, 256, 128, 12, 29, 10, 4, env={"SYLDET_FUSED_CLASSIC": "1"})
    return out


CASES = _cases()

# leaf -> the reason no configuration and no switch of the shipped build reaches it
UNREACHABLE = {
    (0, (8, TM, 10, 0, skew, 0, 0, 0, 0, 0)):
        "SD_GENERIC(8, %d): every timeRange 1 .. 12 has an SD_EXACT form while a thread stages at most 9 quads, and with 8 k-steps the tenth "
        "comes at hop 144, where the basis (64 KB), the staged samples (>= 74.5 KB) and the columns no longer fit 160 KB of LDS: "
        "make_fused_plan clears classic_ok (\"LDS budget exceeded\")" % TM
    for TM in (4, 8, 12) for skew in (0, 1)}


# ---- band edges of the fold kernel's tables ------------------------------------------------------------------------------------
BandCase = namedtuple("BandCase", "name cfg f0 F leaf")


def _band_cases():
    out, seed = [], 7000
    forms = (("fold1_w128", 128, 128, 100, 2, (2, (2, 0, 1, 8, 0, 0, 1, 0, 0, 0))),
             ("fold1_w256_n512", 512, 256, 132, 4, (2, (4, 0, 1, 8, 0, 0, 1, 0, 0, 0))),
             ("fold2_w256", 256, 256, 132, 4, (2, (4, 0, 1, 8, 0, 1, 1, 0, 0, 0))))
    for name, N, W, hop, K2, leaf in forms:
        bands = [(0, 16), (0, 1), (0, 32), (7, 1), (8, 2), (5, 15), (6, 16), (9, 17), (4, 31), (3, 32), (N // 2 - 20, 20), (N // 2 - 1, 1)]
        if name == "fold2_w256":
            bands += [(0, 33), (5, 33), (0, 64), (11, 64), (N // 2 - 64, 64), (N // 2 - 33, 33)]
        for f0, F in bands:
            seed += 1
            lf = leaf
            if F > 32:
                lf = (2, (4, 0, 1, 4, 0, 1, 2, 0, 0, 0))
            out.append(BandCase("%s_f0_%d_F%d" % (name, f0, F), make(seed, N, W, hop, f0, F, 2, 3), f0, F, lf))
    return out


BAND_CASES = _band_cases()


# ---- what a case runs on -------------------------------------------------------------------------------------------------------
def geometry(cfg):
    gap = max(0, -cfg.windowOverlap)
    return gap, gap + cfg.windowLength - max(0, cfg.windowOverlap)


def samples_for(cfg, frames, extra=5):
    gap, hop = geometry(cfg)
    return gap + cfg.windowLength + (frames - 1) * hop + extra


def sizes(cfg, leaf):
    """The two batch lengths of a case, in frames: (a) a partial first tile or pass, timeRange + 2 frames; (b) one that spans more
    wave segments than a workgroup has waves and ends in a ragged tile (the fold kernel: fused_plan.cpp cuts a short row into
    segments of four 16-frame tiles, rounded to whole workgroups of NW waves -- 64 NW frames fill one workgroup), for the older
    two kernels three 64-frame passes plus nine frames."""
    kernel, p = leaf
    T = cfg.timeRange
    return T + 2, (64 * p[S_NW] + 64 + 9 if kernel == 2 else 3 * 64 + 9)


def apply_env(monkeypatch, env):
    for k in ("SYLDET_FUSED_CLASSIC", "SYLDET_FUSED_NOFOLD", "SYLDET_FUSED_NOFOLD2", "SYLDET_FUSED_PAD128"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
