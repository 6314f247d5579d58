"""qs::hot_shape_ok (csrc/step_fuse.h), the host's decision whether a multi-step launch may run
the shape-specialised kernel instance, is plain C++: tests/step_hot_check.cpp calls it on the
flagship shape and on each single deviation from it (other drone counts, a partial workgroup,
a step without a reward or with terminal_obs, a misaligned obs, other tasks, action types and
flags, a reset queue, the LDS reduction, a run-time control frequency, a single step), as a
stand-alone program built with the address and undefined-behaviour sanitizers (no GPU,
nothing loaded into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hot_shape_predicate_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "step_hot_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "step_hot_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "step_hot ok" in out.stdout
