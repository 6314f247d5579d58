"""csrc/step_trunc.h (the smallest step counter at which an episode is truncated, so
that the step kernel compares integers instead of dividing doubles) is plain C++:
tests/step_trunc_check.cpp checks it against the division form as a stand-alone
program built with the address and undefined-behaviour sanitizers (no GPU, nothing
loaded into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trunc_threshold_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "step_trunc_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "step_trunc_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "step_trunc ok" in out.stdout
