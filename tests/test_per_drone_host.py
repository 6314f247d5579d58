"""The per-drone planner modes (qs_pd_mppi_create, qs_pd_cem_create) and qs_score_agents
add plain arithmetic to csrc/planner_sizes.h, csrc/cem_sizes.h and csrc/step_score.h:
the byte sizes of ret_agent and of the buffers that grow by a drone axis, with their
overflow refusals, the shape the update / refit kernels run over and the variant and
grids taken from it.  tests/per_drone_check.cpp exercises them as a stand-alone program
built with the address and undefined-behaviour sanitizers (no GPU, nothing loaded into
Python)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_per_drone_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or "c++"
    exe = tmp_path / "per_drone_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "marl-gym-pybullet-drones_amd", "csrc"),
                    os.path.join(ROOT, "tests", "per_drone_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "per_drone sizes ok" in out.stdout
