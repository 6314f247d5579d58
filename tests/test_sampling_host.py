"""csrc/sampling_sizes.h holds the plain arithmetic of the sampling spec (qs_sampling_mppi_set /
qs_sampling_cem_set / qs_sampling_smc_set): every refusal at its boundary values, the noise
scale, the byte size of `kept` with its 32-bit-offset bound, and the grids of the serial
sample launch and of the elite memory's launches.  tests/sampling_check.cpp exercises them as
a stand-alone program built with the address and undefined-behaviour sanitizers (no GPU,
nothing loaded into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sampling_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "sampling_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sampling_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sampling_sizes ok" in out.stdout
