"""The scratch carver (overlapnet_amd/csrc/ovn_scratch.h) on the host: tests/ovn_scratch_check.cpp includes only that header, is built
with AddressSanitizer + UBSan and run as a child process.  It checks that the measuring pass and the placing pass of a sample layout
(optional and zero-count regions included) give the same offsets and total, that every region starts on a 256-byte boundary, and that
the first and last byte of every region of a heap block of exactly bytes() bytes can be written."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "overlapnet_amd", "csrc")


@pytest.mark.skipif(not shutil.which("g++"), reason="needs g++")
def test_carver_measures_what_it_places(tmp_path):
    exe = tmp_path / "ovn_scratch_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "ovn_scratch_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ovn_scratch ok" in r.stdout, r.stdout + r.stderr


def test_no_hand_rounding_outside_the_carver():
    """Every scratch consumer goes through the carver: no other file of csrc/ rounds to 256 by hand."""
    for name in sorted(os.listdir(CSRC)):
        if name == "ovn_scratch.h" or not name.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(CSRC, name)).read()
        assert "+ 255) & ~(size_t)255" not in text and "auto al = [](size_t b)" not in text, name
