"""csrc/step_branch.h holds the plain arithmetic of a branch set (qs_branch_*): the
sizes of its blocks over C * E virtual envs with their overflow checks, how a rollout
of any length is cut into launches of at most the depth, and the live / first-done
rule of the accumulators as a reference function.  tests/step_branch_check.cpp
exercises them as a stand-alone program built with the address and
undefined-behaviour sanitizers (no GPU, nothing loaded into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_branch_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "step_branch_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "step_branch_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "step_branch ok" in out.stdout
