"""The ctypes mirrors of the CEM planner's C-ABI records (qs_cem_spec, qs_cem_bufs) have the
header's size and field offsets: a C program built with gcc against include/quadswarm.h
prints them; every qs_cem_* entry point the header declares is bound (no GPU calls)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cem_records_match_the_header(tmp_path):
    from gym_pybullet_drones_amd import _lib as L
    recs = {"qs_cem_spec": L.QsCemSpec, "qs_cem_bufs": L.QsCemBufs}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "quadswarm.h"', "int main(void) {"]
    for rec, cls in recs.items():
        lines.append(f'  printf("{rec} size %zu\\n", sizeof({rec}));')
        for f in cls._fields_:
            lines.append(f'  printf("{rec} {f[0]} %zu\\n", offsetof({rec}, {f[0]}));')
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
    assert ctypes.sizeof(L.QsCemSpec) == 80 and ctypes.sizeof(L.QsCemBufs) == 72
    # the header's records have no field the mirrors lack: the same names, in the same order
    header = open(os.path.join(ROOT, "include", "quadswarm.h")).read()
    for rec, cls in recs.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (rec, rec), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") if decl.strip()
                 for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip().split(None, 1)[1].replace("*", " "))]
        assert names == [f[0] for f in cls._fields_], rec


def test_cem_symbols_are_bound():
    """Every qs_cem_* entry point the header declares is exported and has its prototype."""
    from gym_pybullet_drones_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "quadswarm.h")).read()
    declared = sorted(set(re.findall(r"^int\s+(qs_cem_\w+)\s*\(", header, re.M)))
    names = sorted(n for n in L.EXPORTS if n.startswith("qs_cem_"))
    assert names == declared == ["qs_cem_begin", "qs_cem_buffers", "qs_cem_create", "qs_cem_destroy", "qs_cem_finish",
                                 "qs_cem_plan", "qs_cem_refit", "qs_cem_reset", "qs_cem_sample"]
    for n in names:
        fn = getattr(lib, n)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, n
    assert len(lib.qs_cem_sample.argtypes) == 3 and len(lib.qs_cem_refit.argtypes) == 3   # (planner, iteration, stream)
    # null arguments are refused on the host, before any device work
    assert lib.qs_cem_create(None, None, None) == -1 and b"qs_cem_create" in lib.qs_last_error()
    assert lib.qs_cem_buffers(None, None) == -1 and lib.qs_cem_reset(None, None, None) == -1
    for fn in (lib.qs_cem_begin, lib.qs_cem_finish, lib.qs_cem_plan):
        assert fn(None, None) == -1
    assert lib.qs_cem_sample(None, 0, None) == -1 and lib.qs_cem_refit(None, 0, None) == -1
    assert b"qs_cem_refit" in lib.qs_last_error()
    assert lib.qs_cem_destroy(None) == 0
    assert lib.qs_abi_version() == 4
