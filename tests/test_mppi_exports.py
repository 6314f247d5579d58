"""The ctypes mirrors of the planner's C-ABI records (qs_mppi_spec, qs_mppi_bufs) have the
header's size and field offsets: a C program built with gcc against include/quadswarm.h
prints them (no GPU calls)."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_records_match_the_header(tmp_path):
    from gym_pybullet_drones_amd import _lib as L
    recs = {"qs_mppi_spec": L.QsMppiSpec, "qs_mppi_bufs": L.QsMppiBufs}
    c_name = {"lambda_": "lambda"}   # Python keyword renamed in the mirror
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "quadswarm.h"', "int main(void) {"]
    for rec, cls in recs.items():
        lines.append(f'  printf("{rec} size %zu\\n", sizeof({rec}));')
        for f in cls._fields_:
            lines.append(f'  printf("{rec} {f[0]} %zu\\n", offsetof({rec}, {c_name.get(f[0], f[0])}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        rec, field, val = line.split()
        got[(rec, field)] = int(val)
    for rec, cls in recs.items():
        assert got[(rec, "size")] == ctypes.sizeof(cls), rec
        assert len(cls._fields_) == len([k for k in got if k[0] == rec]) - 1
        for f in cls._fields_:
            assert got[(rec, f[0])] == getattr(cls, f[0]).offset, (rec, f[0])
    assert ctypes.sizeof(L.QsMppiSpec) == 56 and ctypes.sizeof(L.QsMppiBufs) == 64


def test_planner_symbols_are_bound():
    """Every qs_mppi_* entry point the header declares is exported and has its prototype."""
    from gym_pybullet_drones_amd import _lib as L
    lib = L.load()
    names = [n for n in L.EXPORTS if n.startswith("qs_mppi_")]
    assert sorted(names) == ["qs_mppi_buffers", "qs_mppi_create", "qs_mppi_destroy", "qs_mppi_plan", "qs_mppi_reset",
                             "qs_mppi_sample", "qs_mppi_update"]
    for n in names:
        fn = getattr(lib, n)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, n
    # null arguments are refused on the host, before any device work
    assert lib.qs_mppi_create(None, None, None) == -1 and b"qs_mppi_create" in lib.qs_last_error()
    assert lib.qs_mppi_plan(None, None) == -1 and lib.qs_mppi_buffers(None, None) == -1
    assert lib.qs_mppi_destroy(None) == 0
