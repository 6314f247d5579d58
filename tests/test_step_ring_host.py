"""qs::FuseGroup::can_wrap and qs::ring_shape_ok (csrc/step_fuse.h), the host's decision whether
a step that writes an output set of the launch again may stay in it, are plain C++:
tests/step_ring_check.cpp walks the first wrap and the later positions of rings of 2, 3, 7 and
32 sets, every refusal (a set out of turn, one pointer that differs, a partial overlap, one set
reused every step, a group that is not live), the step cap and the bound of the period by the
fusion depth, and ring_shape_ok on the flagship shape and deviations from it, as a stand-alone
program built with the address and undefined-behaviour sanitizers (no GPU, nothing loaded into
Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_predicates_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "step_ring_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "step_ring_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "step_ring ok" in out.stdout
