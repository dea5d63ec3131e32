"""The restart-interval split without a GPU: csrc/ke_jpeg_restarts.h -- the header the kernels and the host share -- compiled
with the host C++ compiler into a stand-alone program (tests/_jpeg_rst_cpu.cpp), with AddressSanitizer and UBSan on, and run
on the files of tests/_jpeg_rst_cases.py and the sequential members of the restarts_ family.

For every file the program walks the entropy-coded segment once as a whole and once lane by lane (marker index, plan, a lane's
range: all from the header) and compares every coefficient and the status; a file the rule declines must be declined for the
reason named here.  Then the plan arithmetic, exhaustively: mcus in 1..300, every interval up to mcus + 1, minimum MCUs per lane
in {1, 2, 7, 64}, at most 5 lanes -- the lanes' MCU ranges tile [0, mcus) exactly once, a lane's next_rst is the ordinal of
its first interval mod 8, and g is the smallest count the definition allows."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

import _jpeg_rst_cases as R
import _jpeg_stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kobato-eyes_amd", "csrc")


def _cxx():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def _expected(data: bytes, min_mcus: int, verdict: str = "split") -> str:
    if verdict == "refused":
        return verdict
    mcus, ri, progressive, _ = R.header(data)
    assert not progressive
    return verdict if ri and R.plan(mcus, ri, min_mcus)[2] >= 2 else "one_lane"


def test_lane_by_lane_equals_the_walk_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "jpeg_rst_cpu")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "_jpeg_rst_cpu.cpp"), "-o", exe])
    rows = []                                                     # (name, file, min MCUs, expected verdict)
    for name, data in R.handwritten():
        for min_mcus in (1, 2, R.DEFAULT_MIN_MCUS):
            rows.append((name, data, min_mcus, _expected(data, min_mcus)))
    for name, data, _ in S.family("restarts"):
        if not R.header(data)[2]:
            rows.append((name, data, 1, _expected(data, 1)))
    for name, data, verdict, _ in R.deviants():
        rows.append((name, data, 1, _expected(data, 1, verdict)))
    lines = []
    for k, (name, data, min_mcus, expected) in enumerate(rows):
        path = tmp_path / f"{k:04d}_{name}.jpg"
        path.write_bytes(data)
        lines.append(f"{path} {min_mcus} {expected}")
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(manifest)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    out = res.stdout.strip().splitlines()
    plans = sum(4 * (mcus + 1) for mcus in range(1, 301))
    assert out[-1] == f"ok files={len(rows)} plans={plans}", res.stdout[-2000:]
    # the cases cover what they are there for: every verdict, many lanes, and files the default minimum still splits
    verdicts = {e for _, _, _, e in rows}
    assert verdicts == {"split", "one_lane", "numbers", "few", "many", "refused"}
    split_lines = [line for line in out if " split lanes=" in line]
    assert any("lanes=140 " in line for line in split_lines) and sum(e == "split" for *_, m, e in rows if m == R.DEFAULT_MIN_MCUS) >= 2
    assert any(line.endswith("status=2") for line in split_lines) and sum(line.endswith("status=0") for line in split_lines) >= 60
