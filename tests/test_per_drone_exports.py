"""The per-drone entry points (qs_score_agents, qs_pd_mppi_create, qs_pd_mppi_ret_agent,
qs_pd_cem_create, qs_pd_cem_ret_agent) are declared in include/quadswarm.h, listed in
`_lib.EXPORTS`, exported by the library and bound with prototypes; null arguments are
refused on the host; and the records the planners are created from keep their size (no
GPU calls)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["qs_pd_cem_create", "qs_pd_cem_ret_agent", "qs_pd_mppi_create", "qs_pd_mppi_ret_agent", "qs_score_agents"]


def test_per_drone_symbols_are_declared_listed_and_bound():
    from gym_pybullet_drones_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "quadswarm.h")).read()
    declared = sorted(set(re.findall(r"^int\s+(qs_pd_\w+|qs_score_agents)\s*\(", header, re.M)))
    assert declared == NAMES
    assert sorted(n for n in L.EXPORTS if n.startswith("qs_pd_") or n == "qs_score_agents") == NAMES
    lib = L.load()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    want = {
        "qs_score_agents": [vp, i32, i32, ctypes.POINTER(vp), ctypes.POINTER(L.QsStepOut), ctypes.POINTER(L.QsScoreOut), vp, vp],
        "qs_pd_mppi_create": [vp, ctypes.POINTER(L.QsMppiSpec), ctypes.POINTER(vp)],
        "qs_pd_mppi_ret_agent": [vp, ctypes.POINTER(vp)],
        "qs_pd_cem_create": [vp, ctypes.POINTER(L.QsCemSpec), ctypes.POINTER(vp)],
        "qs_pd_cem_ret_agent": [vp, ctypes.POINTER(vp)],
    }
    for n in NAMES:
        fn = getattr(lib, n)
        assert list(fn.argtypes) == want[n] and fn.restype is ctypes.c_int, n
    # the ABI number stays, as with qs_step_seq
    assert lib.qs_abi_version() == L.ABI_VERSION == 4


def test_null_arguments_are_refused_on_the_host():
    from gym_pybullet_drones_amd import _lib as L
    lib = L.load()
    assert lib.qs_score_agents(None, 1, 1, None, None, None, None, None) == -1
    assert b"qs_score_agents: null handle" in lib.qs_last_error()
    assert lib.qs_score(None, 1, 1, None, None, None, None) == -1 and b"qs_score: null handle" in lib.qs_last_error()
    for name, spec in (("qs_pd_mppi_create", L.QsMppiSpec()), ("qs_pd_cem_create", L.QsCemSpec())):
        out = ctypes.c_void_p(0x55)
        assert getattr(lib, name)(None, None, None) == -1 and name.encode() in lib.qs_last_error()
        assert getattr(lib, name)(None, ctypes.byref(spec), ctypes.byref(out)) == -1 and out.value == 0x55
        assert name.encode() + b": null argument" in lib.qs_last_error()
    for name in ("qs_pd_mppi_ret_agent", "qs_pd_cem_ret_agent"):
        out = ctypes.c_void_p(0x55)
        assert getattr(lib, name)(None, ctypes.byref(out)) == -1 and out.value == 0x55
        assert name.encode() + b": null argument" in lib.qs_last_error()
        assert getattr(lib, name)(None, None) == -1


def test_the_planner_records_keep_their_size(tmp_path):
    """qs_pd_*_create take qs_mppi_spec / qs_cem_spec as they are: the sizes the existing export
    tests assert, in the mirrors and in the header."""
    from gym_pybullet_drones_amd import _lib as L
    want = {"qs_mppi_spec": (L.QsMppiSpec, 56), "qs_mppi_bufs": (L.QsMppiBufs, 64), "qs_cem_spec": (L.QsCemSpec, 80),
            "qs_cem_bufs": (L.QsCemBufs, 72), "qs_score_out": (L.QsScoreOut, 16), "qs_step_out": (L.QsStepOut, 56)}
    lines = ["#include <stdio.h>", '#include "quadswarm.h"', "int main(void) {"]
    lines += [f'  printf("{rec} %zu\\n", sizeof({rec}));' for rec in want]
    lines += ["  return 0;", "}"]
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for rec, (cls, size) in want.items():
        assert int(got[rec]) == size == ctypes.sizeof(cls), rec
