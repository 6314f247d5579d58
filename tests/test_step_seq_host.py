"""csrc/step_fuse.h's SeqGroup (which steps of a caller-supplied action sequence may
share a launch: a step's actions against the other steps' outputs, both ways) and
seq_depth_cap (how many steps' action rows a launch may hold in LDS) are plain C++:
tests/step_seq_check.cpp exercises them as a stand-alone program built with the
address and undefined-behaviour sanitizers (no GPU, nothing loaded into Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_seq_rule_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "step_seq_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "step_seq_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "step_seq ok" in out.stdout
