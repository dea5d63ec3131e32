"""The tile enumeration and the pair counts of the scan from first_new without a GPU: csrc/ke_scan_region.h -- the header the
kernel and the host's closed form share -- compiled with the host C++ compiler into a stand-alone program
(tests/_scan_region_cpu.cpp), with AddressSanitizer and UBSan on, and run.

The program walks every n in {1, 2, 1023, 1024, 1025, 2048, 2049, 3000, 5121, 2^20 + 1}, every first_new in
{0, 1, 15, 16, 17, 1023, 1024, 1025, n - 1, n} that is <= n and part_count in {1, 3, 8}: the map t -> (rb, cc) hits every
tile of the region exactly once and no other, the shards' pair counts are the sums over their tiles and add up to
n (n - 1) / 2 - f (f - 1) / 2, and every n up to 5 121 is enumerated pair by pair against a double loop.  This is where the
sqrt inversion and its integer fix-up can go wrong."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def test_the_region_arithmetic_holds_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "scan_region_cpu")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "_scan_region_cpu.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    assert res.stdout.strip().splitlines()[-1] == "ok cases=85", res.stdout[-2000:]
