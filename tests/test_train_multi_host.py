"""Training a network per channel, the host side (no GPU): the entry points of syldet_trainer_create_multi are declared in the
header and in _abi under ABI 1, the header still compiles as strict C99, the header states the convention, and every status
that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import syllable_detector_swift_amd as sd
from syllable_detector_swift_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = _abi.lib
NEW = ("syldet_trainer_create_multi", "syldet_trainer_networks", "syldet_trainer_groups", "syldet_trainer_set_input_map_of", "syldet_trainer_input_map_of")


def test_symbols_exist_and_the_abi_is_still_1():
    with open(os.path.join(ROOT, "include", "syldet.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _abi.SIGNATURES and getattr(LIB, name).argtypes == _abi.SIGNATURES[name][1]
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert LIB.syldet_abi_version() == 1 == _abi.ABI_VERSION and "#define SYLDET_ABI_VERSION 1" in header
    section = header[header.index("---- training a network per channel"):header.index("---- template matching")]
    for word in ("in ascending order", "G_n = min(tiles_n", "g, g + G_n", "THE BITS", "always runs the multi form", "1 / Wsum is per network",
                 "d_params [N][P]", "d_history [steps][N]", "SYLDET_ERR_OUT_OF_MEMORY", "--train keeps taking one network", "mixed and sharded banks"):
        assert word in section, word
    assert callable(sd.SyllableDetector.multiTrainer) and callable(sd.Recordings.multiTrainer)
    for name in ("groups", "params", "configsWith", "targets", "gradient", "inputRange", "setInputMap", "inputMap", "adamStep", "fitDevice"):
        assert callable(getattr(sd.MultiTrainer, name)), name


def test_the_header_is_still_strict_c99(tmp_path):
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                    os.path.join(ROOT, "tests", "c", "header_is_c.c"), "-o", str(tmp_path / "header_is_c.o")], check=True)


def test_null_handles_are_refused_without_a_device():
    h = _abi.Handle()
    n, groups = C.c_int32(7), np.full(4, 7, np.int32)
    x = np.zeros(4, np.float32)
    fp = x.ctypes.data_as(_abi.c_float_p)
    assert LIB.syldet_trainer_create_multi(None, None, C.byref(h)) == _abi.ERR_INVALID_ARGUMENT and not h
    assert LIB.syldet_trainer_create_multi(None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_trainer_networks(None, C.byref(n), None) == _abi.ERR_INVALID_ARGUMENT and n.value == 7
    assert LIB.syldet_trainer_groups(None, 100, groups.ctypes.data_as(_abi.c_int32_p)) == _abi.ERR_INVALID_ARGUMENT and (groups == 7).all()
    assert LIB.syldet_trainer_set_input_map_of(None, 0, fp, fp, -1.0) == _abi.ERR_INVALID_ARGUMENT
    assert LIB.syldet_trainer_input_map_of(None, 0, None, fp, fp, None) == _abi.ERR_INVALID_ARGUMENT and not x.any()
    assert "NULL" in _abi.last_error()
