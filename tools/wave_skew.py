#!/usr/bin/env python3
"""Diagnostic: when each wave of the fold kernel starts and ends, for the benchmark batch -- do the two waves of a SIMD end together?

    tools/variant_libs.sh kernels_fused_s.hip stamps "-DSYLDET_S_STAMPS"
    python tools/wave_skew.py [lib_stamps] [NAME:VAR=VAL[,VAR=VAL...] ...]      e.g.  pair nopair:SYLDET_FUSED_PAIRSTEP=0

Needs a stamped build of the library (-DSYLDET_S_STAMPS; a directory under syllable_detector_swift_amd/): every wave then leaves
a record -- its SIMD and CU from the hardware-id register, the 100 MHz clock at its entry and after its last tile, its tiles
(syldet_run.cpp writes them to SYLDET_FUSED_STAMPS_FILE).  Each variant runs in a child process of its own: 100 launches for
the clock governor's ramp, then three that are recorded.  Prints, per recorded launch: which wave indices share a SIMD, the
distribution of (end of the pair's first wave) / (end of its second) over all SIMD pairs, the spread of the workgroups' ends
over CUs and XCDs, and the start ramp.  The stamped kernel carries two clock reads a wait more than the shipped one: the shape
of the picture is what it shows, the timings belong to tools/ab_kernel.py.
"""
import collections, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys
sys.path.insert(0, %r)
import torch
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import nets, synth, _abi
base = nets.from_npz()
C, S = 64, 1 << 24
x = synth.channels_on_device(C, S, torch.device("cuda", 0), fs=base.samplingRate)
with sd.SyllableDetector(base, channels=C, engine=_abi.ENGINE_FUSED) as det:
    E = det.countEvaluations(S)
    out = torch.empty((C, E, det.geometry.outputs), dtype=torch.float32, device="cuda")
    fl = torch.empty((C, E), dtype=torch.uint8, device="cuda")
    for i in range(100):                                   # (the clock governor's ramp, MEASUREMENTS R3.8)
        det.run(x, out, fl)
    for k in range(3):
        os.environ["SYLDET_FUSED_STAMPS_FILE"] = os.environ["WAVE_SKEW_OUT"] + ".%%d" %% k
        det.run(x, out, fl)
    torch.cuda.synchronize()
''' % ROOT


def pct(v, qs=(0, 5, 25, 50, 75, 95, 100)):
    v = sorted(v)
    return "  ".join("p%d %.4g" % (q, v[min(len(v) - 1, int(round(q / 100.0 * (len(v) - 1))))]) for q in qs)


def report(path):
    rec = [tuple(int(t) for t in l.split()) for l in open(path) if l.strip() and not l.startswith("#")]
    if not rec:
        print("   no records (is the library a -DSYLDET_S_STAMPS build?)")
        return
    t_first = min(r[5] for r in rec)
    t_last = max(r[6] for r in rec)
    us = lambda ticks: ticks * 0.01                        # the clock counts 10 ns
    print("   %d waves, %d workgroups, launch %.1f us from the first wave's entry to the last wave's end" %
          (len(rec), len({r[0] for r in rec}), us(t_last - t_first)))
    life = [r[6] - r[5] for r in rec]
    print("   wave lifetime / launch: mean %.3f   (%s)" % (sum(life) / len(life) / (t_last - t_first), pct([l / (t_last - t_first) for l in life])))
    print("   tiles a wave: %s" % pct([r[7] for r in rec], (0, 50, 100)))
    by_wg = collections.defaultdict(list)
    for r in rec:
        by_wg[r[0]].append(r)
    # ---- which wave indices share a SIMD
    pairing = collections.Counter()
    split_cu = 0
    pairs = []                                             # (wg, wave a, wave b, begin of the workgroup, end a, end b, tiles a, tiles b)
    for wg, rs in by_wg.items():
        place = {(r[4], (r[3] >> 13) & 7, (r[3] >> 12) & 1, (r[3] >> 8) & 15) for r in rs}       # (XCD, SE, SH, CU)
        split_cu += len(place) > 1
        simd = collections.defaultdict(list)
        for r in rs:
            simd[(r[3] >> 4) & 3].append(r)
        begin = min(r[5] for r in rs)
        for sid, ws in simd.items():
            ws.sort(key=lambda r: r[1])
            pairing[tuple(r[1] for r in ws)] += 1
            if len(ws) == 2:
                pairs.append((wg, ws[0][1], ws[1][1], begin, ws[0][6], ws[1][6], ws[0][7], ws[1][7]))
    print("   waves that share a SIMD (wave indices: SIMDs of all workgroups):  " + "  ".join("%s: %d" % (k, v) for k, v in sorted(pairing.items())))
    print("   w and w ^ 4 in every pair: %s;   workgroups spread over more than one CU: %d" %
          ("yes" if all(len(k) != 2 or k[1] == k[0] ^ 4 for k in pairing) else "NO", split_cu))
    # ---- the pairs' ends
    full = [p for p in pairs if p[6] == p[7]]             # (both waves with the same number of tiles: the ragged last segment apart)
    ratio = [(min(p[4], p[5]) - p[3]) / max(1, max(p[4], p[5]) - p[3]) for p in full]
    gap = [us(abs(p[4] - p[5])) for p in full]
    tile_us = [us(max(p[4], p[5]) - p[3]) / p[6] for p in full]
    print("   SIMD pairs with equal tile counts: %d" % len(full))
    print("   (end of first) / (end of second), from the workgroup's start:  mean %.4f   %s" % (sum(ratio) / len(ratio), pct(ratio)))
    print("   gap between the two ends, us:     mean %.2f   %s" % (sum(gap) / len(gap), pct(gap)))
    print("   ... in tiles of the later wave:   mean %.2f   %s" % (sum(g / t for g, t in zip(gap, tile_us)) / len(gap), pct([g / t for g, t in zip(gap, tile_us)])))
    print("   the lower wave index ends first in %.1f %% of the pairs" % (100.0 * sum(p[4] < p[5] for p in full) / len(full)))
    # ---- workgroup ends over CUs and XCDs, the start ramp
    wg_end = {wg: max(r[6] for r in rs) for wg, rs in by_wg.items()}
    wg_beg = {wg: min(r[5] for r in rs) for wg, rs in by_wg.items()}
    print("   workgroup start after the launch's first wave, us:  %s" % pct([us(b - t_first) for b in wg_beg.values()]))
    print("   workgroup end, us:                                  %s" % pct([us(e - t_first) for e in wg_end.values()]))
    print("   workgroup end / launch:                             %s" % pct([(e - t_first) / (t_last - t_first) for e in wg_end.values()]))
    by_xcd = collections.defaultdict(list)
    for wg, rs in by_wg.items():
        by_xcd[rs[0][4]].append(wg)
    for x in sorted(by_xcd):
        ends = [us(wg_end[w] - t_first) for w in by_xcd[x]]
        begs = [us(wg_beg[w] - t_first) for w in by_xcd[x]]
        cus = {((r[3] >> 13) & 7, (r[3] >> 12) & 1, (r[3] >> 8) & 15) for w in by_xcd[x] for r in by_wg[w]}
        print("      XCD %d: %3d workgroups on %2d CUs   start mean %6.1f max %6.1f   end min %6.1f mean %6.1f max %6.1f us" %
              (x, len(ends), len(cus), sum(begs) / len(begs), max(begs), min(ends), sum(ends) / len(ends), max(ends)))


def main():
    args = sys.argv[1:]
    lib = "lib_stamps"
    if args and ":" not in args[0] and os.path.isdir(os.path.join(ROOT, "syllable_detector_swift_amd", args[0])):
        lib = args.pop(0)
    variants = args or ["default"]
    for v in variants:
        name, _, envs = v.partition(":")
        with tempfile.TemporaryDirectory() as tmp:
            env = dict(os.environ, SYLDET_LIB=os.path.join(ROOT, "syllable_detector_swift_amd", lib, "libsyldet.so"),
                       SYLDET_FUSED_STAMPS="1", WAVE_SKEW_OUT=os.path.join(tmp, "records"))
            for kv in filter(None, envs.split(",")):
                k, _, val = kv.partition("=")
                env[k] = val
            r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True)
            if r.returncode != 0:
                print("%s: the child ended with %d\n%s" % (name, r.returncode, r.stderr.strip()[-600:]), flush=True)
                return r.returncode
            for k in range(3):
                print("== %s (%s)  recorded launch %d" % (name, lib, k), flush=True)
                report(os.path.join(tmp, "records.%d" % k))
            print("   " + r.stderr.strip().split("\n")[-1][:240], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
