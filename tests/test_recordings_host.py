"""Packed recordings on the host (no GPU): the plan (syldet_recordings_plan_of_config, the device-free form of
syldet_recordings_plan) against the numpy model, its invariants and its layout guarantee, the statuses of every refused
argument, eligibility on a two-network bank, and the tool's --batch usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recordings_ref as ref
import util
import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi, nets
from test_multinet_host import _base

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "syllable_detector_swift_amd", "lib", "syllable-detector-cli")

# shorter than a window, one sample short of the first evaluation (first_index 1444 = need of the sample network) and exactly it,
# one short of the second and exactly it, a multiple of hop, a long one, duplicates
LENGTHS = [0, 100, 1443, 1444, 1575, 1576, 132 * 40, 131 * 40, 20011, 1444, 100, 20011, 0, 7777]


def _hop131():
    base = _base()
    return nets.variant(base, windowOverlap=base.windowLength - 131)


def _check(cfg, lengths, Cn, channel_net=None, networks=None):
    hop, need, T, _ = ref.clock(cfg)
    slots, rs, re_, fill = sd.planRecordings(cfg, Cn, lengths, channel_net, networks)
    want = ref.plan(lengths, hop, need, T, Cn, channel_net, networks)
    assert (slots, rs, re_) == want[:3] and fill == want[3]
    assert rs % 8 == 0
    by_row = {}
    for k, (row, offset, first, n_evals, n) in enumerate(slots):
        assert 0 <= row < Cn and offset % hop == 0 and first == offset // hop and n == lengths[k]
        assert n_evals == ref.count_evals(n, hop, need, T)
        assert offset + n <= rs
        # (a recording without an evaluation may lie behind the row's last one: nothing of it is ever read)
        assert n_evals == 0 or first + n_evals <= re_
        if channel_net is not None:
            assert channel_net[row] == networks[k]
        by_row.setdefault(row, []).append((offset, -(-n // hop) * hop))
    for spans in by_row.values():                           # no two slots of a row overlap (their padded lengths included)
        spans.sort()
        for (a, la), (b, _) in zip(spans, spans[1:]):
            assert a + la <= b
    return slots, rs, re_, fill


@pytest.mark.parametrize("make,hop", [(_base, 132), (_hop131, 131)])
@pytest.mark.parametrize("Cn", [1, 3, 7])
def test_plan_equals_the_model_and_keeps_its_guarantee(make, hop, Cn):
    cfg = make()
    assert ref.clock(cfg)[0] == hop
    if hop == 132:
        assert ref.clock(cfg)[1:] == (256, cfg.timeRange, 1444) and cfg.timeRange == 10
    _, rs, _, fill = _check(cfg, LENGTHS, Cn)
    P = [-(-n // hop) * hop for n in LENGTHS]
    assert rs <= -(-sum(P) // Cn) + max(P) + 7              # greedy placement: no row is more than the longest ahead of the mean
    assert 0.0 < fill <= 1.0


def test_fewer_recordings_than_rows_and_none():
    cfg = _base()
    slots, rs, re_, fill = _check(cfg, [5000, 20011], 7)
    assert sorted(s[0] for s in slots) == [0, 1] and all(s[1] == 0 for s in slots) and rs == 20064         # ceil(20011 / 132) 132, already whole quads
    assert _check(cfg, [], 3) == ([], 0, 0, 0.0)
    assert _check(cfg, [0, 0], 3)[1:] == (0, 0, 0.0)


def test_eligibility_on_a_two_network_bank():
    base = _base()
    other = nets.perturbed(base, 1)
    assert sd.configsCompatible(base, other) == (True, None)
    channel_net = [0, 1, 1, 0, 1]
    networks = [k % 2 for k in range(len(LENGTHS))]
    slots, rs, _, _ = _check(base, LENGTHS, 5, channel_net, networks)
    # the guarantee holds for each network's own rows and recordings
    for net in (0, 1):
        P = [-(-n // 132) * 132 for n, w in zip(LENGTHS, networks) if w == net]
        most = max(o + -(-n // 132) * 132 for (row, o, _, _, n) in slots if channel_net[row] == net)
        assert most <= -(-sum(P) // channel_net.count(net)) + max(P)
    # a network that no row runs
    with pytest.raises(sd.SyllableDetectorError) as ei:
        sd.planRecordings(base, 3, [1000, 2000], [0, 0, 2], [0, 1])
    assert ei.value.status == _abi.ERR_UNSUPPORTED and "network 1" in str(ei.value)


def _plan_status(cfg, Cn, channel_net, lengths, networks, K=None, null_lengths=False, null_cfg=False):
    c, keep = cfg.to_abi()
    n = np.ascontiguousarray(lengths, np.int64)
    cn = None if channel_net is None else np.ascontiguousarray(channel_net, np.int32)
    net = None if networks is None else np.ascontiguousarray(networks, np.int32)
    st = _abi.lib.syldet_recordings_plan_of_config(None if null_cfg else C.byref(c), Cn, None if cn is None else cn.ctypes.data_as(_abi.c_int32_p),
                                                   None if null_lengths else n.ctypes.data_as(_abi.c_int64_p),
                                                   None if net is None else net.ctypes.data_as(_abi.c_int32_p), n.size if K is None else K,
                                                   None, None, None, None)
    del keep
    return st


def test_refused_arguments():
    cfg = _base()
    bad, unsupported = _abi.ERR_INVALID_ARGUMENT, _abi.ERR_UNSUPPORTED
    assert _plan_status(cfg, 3, None, [100, 200], None) == _abi.OK              # (every result pointer may be NULL)
    assert _plan_status(cfg, 3, None, [100, -1], None) == bad                    # a negative length
    assert _plan_status(cfg, 3, None, [100], None, K=-1) == bad                  # a negative count
    assert _plan_status(cfg, 3, None, [100], None, null_lengths=True) == bad     # NULL array with recordings
    assert _plan_status(cfg, 3, None, [], None, null_lengths=True) == _abi.OK    # ... without any it is legal
    assert _plan_status(cfg, 3, None, [100, 200], [0, 0]) == _abi.OK             # a plain bank: NULL or all zeros
    assert _plan_status(cfg, 3, None, [100, 200], [0, 1]) == bad
    assert _plan_status(cfg, 3, [0, 1, 0], [100, 200], None) == bad              # several networks: every recording needs one
    assert _plan_status(cfg, 3, [0, 1, 0], [100, 200], [0, -1]) == bad
    assert _plan_status(cfg, 3, [0, 1, 0], [100, 200], [0, 2]) == unsupported    # a network no row runs
    assert "network 2" in _abi.last_error()
    assert _plan_status(cfg, 3, [0, -1, 0], [100], [0]) == bad
    assert _plan_status(cfg, 0, None, [100], None) == bad                        # no channel
    assert _plan_status(cfg, 3, None, [100], None, null_cfg=True) == bad
    # a configuration syldet_create refuses: its status
    assert _plan_status(nets.variant(cfg, thresholds=[0.5, 0.5]), 3, None, [100], None) == _abi.ERR_THRESHOLD_MISMATCH
    # the handle forms refuse a NULL handle before anything else
    n = np.array([100], np.int64)
    h = _abi.Handle()
    assert _abi.lib.syldet_recordings_plan(None, n.ctypes.data_as(_abi.c_int64_p), None, 1, None, None, None, None) == bad
    assert _abi.lib.syldet_recordings_create(None, n.ctypes.data_as(_abi.c_int64_p), None, 1, C.byref(h)) == bad and not h.value
    assert _abi.lib.syldet_recordings_destroy(None) == _abi.OK
    assert _abi.lib.syldet_recordings_slots(None, None) == bad and _abi.lib.syldet_recordings_shape(None, None, None, None, None) == bad
    assert _abi.lib.syldet_recordings_load_device(None, None, None, None, None, 0, None) == bad
    assert _abi.lib.syldet_recordings_events_device(None, None, None, 0.0, None, None, 0, None, None) == bad


def test_a_sharded_bank_has_no_packed_form():
    bank = sd.ShardedSyllableDetectorBank.__new__(sd.ShardedSyllableDetectorBank)   # (no device: the answer needs none)
    bank._h = None
    with pytest.raises(sd.SyllableDetectorError) as ei:
        bank.recordings([100, 200])
    assert ei.value.status == _abi.ERR_UNSUPPORTED


def test_the_handles_block_layout_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "recordings_blob"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "syllable_detector_swift_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "recordings_blob_test.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and not r.stderr, (r.returncode, r.stdout, r.stderr)
    # the handle's block is that header's
    text = open(os.path.join(ROOT, "syllable_detector_swift_amd", "csrc", "syldet_recordings.cpp")).read()
    assert "RecBlob " in text and "up16(" not in text


@pytest.mark.parametrize("extra,needle", [
    (["--simulate", "x.wav"], b"--batch"), (["--levels", "x.tsv"], b"--batch"), (["--ttl", "x.wav"], b"--batch"),
    (["--ttl-onsets", "x.tsv"], b"--batch")])
def test_batch_refuses_the_one_file_options(extra, needle):
    r = subprocess.run([CLI, "-n", "net.txt", "-a", "a.wav", "--batch", *extra], capture_output=True, timeout=60)
    assert r.returncode == 64 and needle in r.stderr and b"exactly one file" in r.stderr and r.stdout.startswith(b"Usage:")


def test_batch_option_errors():
    for args, msg in [(["--batch-rows", "4"], b"need --batch"), (["--batch-bytes", "4"], b"need --batch"),
                      (["--batch", "--batch-rows", "0"], b"--batch-rows takes"), (["--batch", "--batch-rows", "x"], b"--batch-rows takes"),
                      (["--batch", "--batch-bytes", "0"], b"--batch-bytes takes"), (["--batch", "--batch-rows"], b"Missing value")]:
        r = subprocess.run([CLI, "-n", "net.txt", "-a", "a.wav", *args], capture_output=True, timeout=60)
        assert r.returncode == 64 and msg in r.stderr, (args, r.stderr)
    assert b"--batch" in subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
