"""csrc/prior_sizes.h holds the plain arithmetic of the policy prior (qs_prior_act,
qs_prior_mppi_* / qs_prior_cem_*): every refusal of a prior spec, the byte sizes of its
buffers with the 32-bit-offset bounds, and the row tile, grid and LDS plan of the actor
launch.  tests/prior_check.cpp exercises them as a stand-alone program built with the
address and undefined-behaviour sanitizers (no GPU, nothing loaded into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prior_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "prior_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "prior_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "prior_sizes ok" in out.stdout
