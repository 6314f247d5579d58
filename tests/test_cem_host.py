"""csrc/cem_sizes.h holds the plain arithmetic of the CEM planner (qs_cem_*): the byte sizes
of its buffers with every refusal bound, the choice between the two select + refit
variants, and the launch grids.  tests/cem_check.cpp exercises them as a stand-alone
program built with the address and undefined-behaviour sanitizers (no GPU, nothing loaded
into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cem_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "cem_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cem_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cem_sizes ok" in out.stdout
