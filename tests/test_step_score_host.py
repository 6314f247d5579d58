"""csrc/step_score.h holds the plain arithmetic of a branch-rollout launch (qs_score):
the steps one launch takes from the LDS figures, the byte sizes of its buffers over
C * E virtual envs with their overflow checks, and the overlap test over outputs and
action buffers.  tests/step_score_check.cpp exercises them as a stand-alone program
built with the address and undefined-behaviour sanitizers (no GPU, nothing loaded
into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_score_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "step_score_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "step_score_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "step_score ok" in out.stdout
