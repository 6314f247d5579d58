"""The avoidance entry points (qs_avoid_*) are declared in include/quadswarm.h, listed in
_lib.EXPORTS and bound with the header's argument types; null arguments come back as
QS_E_INVALID before any device work; the ctypes mirror of qs_avoid_spec has the header's
layout (24 bytes); the ABI version is still 4 and the earlier spec records, qs_track_spec's
96 bytes included, have kept their sizes.  No GPU calls."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qs_avoid_score", "qs_avoid_mppi_set", "qs_avoid_mppi_buffers", "qs_avoid_mppi_score",
         "qs_avoid_cem_set", "qs_avoid_cem_buffers", "qs_avoid_cem_score")
SPEC_FIELDS = ["obstacles", "M", "sep_radius", "sep_weight", "sep_z_scale"]
RECORDS = dict(qs_mppi_spec=("QsMppiSpec", 56), qs_cem_spec=("QsCemSpec", 80), qs_smc_spec=("QsSmcSpec", 72),
               qs_value_spec=("QsValueSpec", 104), qs_sampling_spec=("QsSamplingSpec", 24),
               qs_track_spec=("QsTrackSpec", 96))
QS_E_INVALID = -1


def src_header():
    return open(os.path.join(ROOT, "include", "quadswarm.h")).read()


def test_avoid_symbols_are_declared_listed_and_bound():
    from gym_pybullet_drones_amd import _lib as L
    src = src_header()
    declared = set(re.findall(r"^int\s+(qs_avoid_\w+)\s*\(", src, re.M))
    assert declared == set(NAMES) and len(NAMES) == 7
    assert sorted(n for n in L.EXPORTS if n.startswith("qs_avoid_")) == sorted(NAMES)
    lib = L.load()
    vp, i32, P = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER
    want = {"qs_avoid_score": [vp, i32, i32, P(vp), P(L.QsStepOut), P(L.QsScoreOut), vp, P(L.QsTrackSpec),
                               P(L.QsAvoidSpec), vp, vp]}
    for who in ("mppi", "cem"):
        want[f"qs_avoid_{who}_set"] = [vp, P(L.QsAvoidSpec)]
        want[f"qs_avoid_{who}_buffers"] = [vp, P(vp), P(vp)]
        want[f"qs_avoid_{who}_score"] = [vp, vp]
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want[name], name
        assert fn.restype is i32, name
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", src, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(want[name]), name   # the argument counts are the header's


def test_abi_4_and_the_earlier_records_are_unchanged():
    from gym_pybullet_drones_amd import _lib as L
    assert re.search(r"#define\s+QS_ABI_VERSION\s+4\b", src_header())
    lib = L.load()
    assert lib.qs_abi_version() == L.ABI_VERSION == 4
    assert hasattr(lib, "qs_avoid_score") and hasattr(lib, "qs_track_score")
    for mirror, size in RECORDS.values():
        assert ctypes.sizeof(getattr(L, mirror)) == size, mirror
    assert ctypes.sizeof(L.QsCemBufs) == 72 and ctypes.sizeof(L.QsMppiBufs) == 64


def test_null_arguments_are_refused_without_device_work():
    from gym_pybullet_drones_amd import _lib as L
    lib = L.load()
    spec, track = L.QsAvoidSpec(), L.QsTrackSpec()
    cost = ctypes.c_void_p(4096)
    for tr in (None, ctypes.byref(track)):
        assert lib.qs_avoid_score(None, 1, 1, None, None, None, None, tr, ctypes.byref(spec), cost, None) == QS_E_INVALID
        assert b"qs_avoid_score" in lib.qs_last_error()
    for who in ("mppi", "cem"):
        fn = getattr(lib, f"qs_avoid_{who}_set")
        assert fn(None, ctypes.byref(spec)) == QS_E_INVALID
        assert f"qs_avoid_{who}_set".encode() in lib.qs_last_error()
        assert fn(None, None) == QS_E_INVALID
        a, o = ctypes.c_void_p(12345), ctypes.c_void_p(6789)
        assert getattr(lib, f"qs_avoid_{who}_buffers")(None, ctypes.byref(a), ctypes.byref(o)) == QS_E_INVALID
        assert f"qs_avoid_{who}_buffers".encode() in lib.qs_last_error()
        assert (a.value, o.value) == (12345, 6789)   # untouched
        assert getattr(lib, f"qs_avoid_{who}_score")(None, None) == QS_E_INVALID
        assert f"qs_avoid_{who}_score".encode() in lib.qs_last_error()


def test_avoid_spec_matches_the_header(tmp_path):
    """gcc's sizeof / offsetof of qs_avoid_spec, and the sizes of the earlier spec records,
    against the ctypes mirrors (the way of tests/test_track_exports.py)."""
    from gym_pybullet_drones_amd import _lib as L
    assert [f[0] for f in L.QsAvoidSpec._fields_] == SPEC_FIELDS
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "quadswarm.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(qs_avoid_spec));']
    for name in SPEC_FIELDS:
        lines.append(f'  printf("{name} %zu\\n", offsetof(qs_avoid_spec, {name}));')
    for rec in RECORDS:
        lines.append(f'  printf("{rec} %zu\\n", sizeof({rec}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict((k, int(v)) for k, v in (line.split() for line in
                                        subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()))
    assert got["size"] == ctypes.sizeof(L.QsAvoidSpec) == 24
    for name in SPEC_FIELDS:
        assert got[name] == getattr(L.QsAvoidSpec, name).offset, name
    assert [got[k] for k in SPEC_FIELDS] == [0, 8, 12, 16, 20]
    for rec, (mirror, size) in RECORDS.items():
        assert got[rec] == ctypes.sizeof(getattr(L, mirror)) == size, rec
    # the header's record has no field the mirror lacks: the same names, in the same order
    body = re.search(r"typedef struct qs_avoid_spec \{(.*?)\} qs_avoid_spec;", src_header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.match(r"(?:const\s+)?\w+\s*\*?\s*(\w+)", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert names == SPEC_FIELDS
