"""What a pair scan reserves and launches, without a GPU: csrc/ke_scan_plan.h -- the header ke_launch_scan follows -- compiled
with the host C++ compiler into a stand-alone program (tests/_scan_plan_cpu.cpp), with AddressSanitizer and UBSan on, and run.

The program plans every n in {2, 1023, 1024, 1025, 2049, 5000, 49 999, 50 000, 4 193 280, 4 193 281, 2^32} x kind x first_new in
{0, 1, 1024, 1025, n - 1, n} x shard in {0/1, 0/3, 2/3, 7/8} x bands in {16x4, 17x3, 24x2, 25x2, 1x64} x KE_SCAN_MODE x cap in
{0, 5} x want_bucket_pairs x exact x buckets_allowed (2^32: a handful of them) and holds each plan to expectations written out
from the rules: region, shard and yardstick, which of histogram, bucket kernels, hist-pairs and wide sort run, the buffer sizes,
the refusals.  Slices of 1, 3, 8, the default and 2^40 tiles are walked slot by slot.  The boundaries -- kBucketMinN, 2^18 bins,
the re-plan without buckets, 2^32 hashes, both tile refusals at their first failing size -- are then checked by name."""
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


def test_the_scan_plan_follows_its_rules_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "scan_plan_cpu")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "_scan_plan_cpu.cpp"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    assert res.stdout.strip().splitlines()[-1] == "ok cases=122451", res.stdout[-2000:]
