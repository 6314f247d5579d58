"""The policy-prior entry points (qs_prior_*) are declared in include/quadswarm.h, listed in
_lib.EXPORTS and bound with the header's argument types; null arguments come back as
QS_E_INVALID before any device work; the ctypes mirror of qs_prior_spec has the header's
layout; the ABI version is still 4 and no earlier name list has grown.  No GPU calls."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qs_prior_act", "qs_prior_mppi_set", "qs_prior_mppi_buffers", "qs_prior_mppi_rollout", "qs_prior_cem_set",
         "qs_prior_cem_buffers", "qs_prior_cem_rollout")
SPEC_FIELDS = ["in_dim", "hidden", "act_dim", "w1", "b1", "w2", "b2", "w3", "b3", "logstd", "action_scale", "std_scale",
               "obs_mean", "obs_var", "obs_eps", "obs_clip", "count", "obs"]
QS_E_INVALID = -1


def test_prior_symbols_are_declared_listed_and_bound():
    from gym_pybullet_drones_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "quadswarm.h")).read()
    declared = set(re.findall(r"^int\s+(qs_prior_\w+)\s*\(", src, re.M))
    assert declared == set(NAMES)
    assert sorted(n for n in L.EXPORTS if n.startswith("qs_prior_")) == sorted(NAMES)
    lib = L.load()
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    P = ctypes.POINTER
    want = {"qs_prior_act": [P(L.QsPriorSpec), i32, i32, i32, i32, f32, f32, ctypes.c_uint64, i64, vp, vp, i32, vp, vp, vp]}
    for who in ("mppi", "cem"):
        want[f"qs_prior_{who}_set"] = [vp, P(L.QsPriorSpec)]
        want[f"qs_prior_{who}_buffers"] = [vp, P(vp), P(vp)]
        want[f"qs_prior_{who}_rollout"] = [vp, vp]
    for name in NAMES:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want[name], name
        assert fn.restype is i32, name
        decl = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", src, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(want[name]), name   # the argument counts are the header's


def test_abi_4_is_unchanged():
    """The version is 4 and the name lists the earlier export tests pin hold no new name."""
    from gym_pybullet_drones_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "quadswarm.h")).read()
    assert re.search(r"#define\s+QS_ABI_VERSION\s+4\b", src)
    lib = L.load()
    assert lib.qs_abi_version() == L.ABI_VERSION == 4
    declared = set(re.findall(r"^int\s+(qs_\w+)\s*\(", src, re.M))
    count = {p: sum(n.startswith(p) for n in declared) for p in ("qs_mppi_", "qs_cem_", "qs_pd_", "qs_smc_", "qs_branch_",
                                                                 "qs_value_")}
    assert count == {"qs_mppi_": 7, "qs_cem_": 9, "qs_pd_": 4, "qs_smc_": 11, "qs_branch_": 8, "qs_value_": 7}
    # the records the earlier entry points take have kept their sizes
    assert ctypes.sizeof(L.QsMppiSpec) == 56 and ctypes.sizeof(L.QsCemSpec) == 80 and ctypes.sizeof(L.QsValueSpec) == 104


def test_null_arguments_are_refused_without_device_work():
    from gym_pybullet_drones_amd import _lib as L
    lib = L.load()
    spec = L.QsPriorSpec()
    assert lib.qs_prior_act(None, 0, 1, 1, 1, -1.0, 1.0, 0, 0, None, None, 0, None, None, None) == QS_E_INVALID
    assert b"qs_prior_act" in lib.qs_last_error()
    assert lib.qs_prior_act(ctypes.byref(spec), 0, 1, 1, 1, -1.0, 1.0, 0, 0, None, None, 0, None, None, None) == QS_E_INVALID
    a, o = ctypes.c_void_p(12345), ctypes.c_void_p(6789)
    for who in ("mppi", "cem"):
        assert getattr(lib, f"qs_prior_{who}_set")(None, ctypes.byref(spec)) == QS_E_INVALID
        assert f"qs_prior_{who}_set".encode() in lib.qs_last_error()
        assert getattr(lib, f"qs_prior_{who}_set")(None, None) == QS_E_INVALID
        assert getattr(lib, f"qs_prior_{who}_buffers")(None, ctypes.byref(a), ctypes.byref(o)) == QS_E_INVALID
        assert (a.value, o.value) == (12345, 6789)   # untouched
        assert getattr(lib, f"qs_prior_{who}_rollout")(None, None) == QS_E_INVALID
        assert f"qs_prior_{who}_rollout".encode() in lib.qs_last_error()


def test_prior_spec_matches_the_header(tmp_path):
    """gcc's sizeof / offsetof of qs_prior_spec against the ctypes mirror (the way of
    tests/test_exports.py)."""
    from gym_pybullet_drones_amd import _lib as L
    assert [f[0] for f in L.QsPriorSpec._fields_] == SPEC_FIELDS
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "quadswarm.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(qs_prior_spec));']
    for name in SPEC_FIELDS:
        lines.append(f'  printf("{name} %zu\\n", offsetof(qs_prior_spec, {name}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict((k, int(v)) for k, v in (line.split() for line in
                                        subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()))
    assert got["size"] == ctypes.sizeof(L.QsPriorSpec)
    for name in SPEC_FIELDS:
        assert got[name] == getattr(L.QsPriorSpec, name).offset, name
