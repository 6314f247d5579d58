"""csrc/track_sizes.h holds the plain arithmetic of the tracking cost (qs_track_score /
qs_track_fold / qs_track_mppi_set / qs_track_cem_set): every refusal at its boundary values,
the byte sizes of the reference and of cost_agent with the 32-bit-offset bound, the row clamp
and the fold's grid.  tests/track_check.cpp exercises them as a stand-alone program built
with the address and undefined-behaviour sanitizers (no GPU, nothing loaded into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_track_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "track_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "track_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "track_sizes ok" in out.stdout
