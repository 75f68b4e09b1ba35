"""CPU: the A/B switches as a closed list.  Every switch whose contract (dsml_thesis_amd/switches.py, fourth field) is "bits" or
"tolerance" names, in the arm registries of tests/test_switch_arms_gpu.py / tests/test_switch_arms_model_gpu.py, the tests that
run its other arm -- a switch added without one fails here; the library's switch table (csrc/ldmk_common.h) answers through
ldmk_switch_value / ldmk_switch_override with the defaults this table documents, and still reads the environment."""
import ctypes
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from dsml_thesis_amd.build import build_lib
    so = ctypes.CDLL(build_lib(verbose=False))
    so.ldmk_switch_value.argtypes = [ctypes.c_char_p]
    so.ldmk_switch_override.argtypes = [ctypes.c_char_p, ctypes.c_int]
    return so


def _registries():
    import test_switch_arms_gpu as A
    import test_switch_arms_model_gpu as B
    assert not set(A.ARMS) & set(B.ARMS)
    return {**A.ARMS, **B.ARMS}


def test_every_ab_switch_names_the_tests_of_its_other_arm():
    from dsml_thesis_amd import switches as S
    arms = _registries()
    want = {n for n, e in S.SWITCHES.items() if e[3] in ("bits", "tolerance")}
    assert want - set(arms) == set(), f"A/B switches without an arm test: {sorted(want - set(arms))}"
    assert set(arms) - want == set(), f"registered arms of switches that state no contract: {sorted(set(arms) - want)}"
    for name, tests in arms.items():
        assert tests, name
        for tid in tests:
            mod, fn = tid.split("::")
            assert callable(getattr(importlib.import_module(mod), fn, None)), (name, tid)
    # the arms this work added state their switch by name in the test that runs them
    for modname in ("test_switch_arms_gpu", "test_switch_arms_model_gpu"):
        src = open(os.path.join(ROOT, "tests", modname + ".py")).read()
        for name, tests in arms.items():
            if any(t.startswith(modname + "::") for t in tests):
                assert src.count(f'"{name}"') >= 2, (name, modname)      # (the registry line and the test's own use)


def test_library_switch_table_reports_the_documented_defaults(lib):
    from dsml_thesis_amd import switches as S
    names = [n for n, e in S.SWITCHES.items() if e[1] == "library"]
    assert len(names) == 9
    for name in names:
        if name in os.environ:
            continue
        assert lib.ldmk_switch_value(name.encode()) == int(S.SWITCHES[name][0] or 0), name
    for name in ("LDMK_PS", "LDMK_PS_DEBUG", "LDMK_IG_NFAS", "", "LDMK_IG_NFAST "):
        assert lib.ldmk_switch_value(name.encode()) == -1 and lib.ldmk_switch_override(name.encode(), 1) == -1
    assert lib.ldmk_switch_value(None) == -1


def test_library_switch_override_round_trips(lib):
    from dsml_thesis_amd import switches as S
    for name, e in S.SWITCHES.items():
        if e[1] != "library" or name in os.environ:
            continue
        key, default = name.encode(), int(e[0] or 0)
        for value in (0, 1, 2, 7):
            before = lib.ldmk_switch_value(key)
            assert lib.ldmk_switch_override(key, value) == before
            assert lib.ldmk_switch_value(key) == value
        assert lib.ldmk_switch_override(key, -1) == 7 and lib.ldmk_switch_value(key) == default
        assert lib.ldmk_switch_override(key, -5) == default and lib.ldmk_switch_value(key) == default      # (no override to take back)
    # one entry's override leaves the others alone
    lib.ldmk_switch_override(b"LDMK_IG_LEAN", 0)
    try:
        assert lib.ldmk_switch_value(b"LDMK_PS_LEAN") == 1 and lib.ldmk_switch_value(b"LDMK_IG_NFAST") == 1
    finally:
        lib.ldmk_switch_override(b"LDMK_IG_LEAN", -1)


def test_library_switches_still_read_the_environment(lib):
    """A child process with LDMK_IG_LEAN=0 LDMK_ATTN_PIPE=1 in its environment loads the library through ctypes only (no GPU use)
    and reports those values; an override stands in front of them and gives way to them again."""
    code = ("import ctypes, sys\n"
            "so = ctypes.CDLL(sys.argv[1])\n"
            "so.ldmk_switch_value.argtypes = [ctypes.c_char_p]\n"
            "so.ldmk_switch_override.argtypes = [ctypes.c_char_p, ctypes.c_int]\n"
            "v = lambda n: so.ldmk_switch_value(n.encode())\n"
            "a = [v(n) for n in ('LDMK_IG_LEAN', 'LDMK_ATTN_PIPE', 'LDMK_PS_LEAN', 'LDMK_ATTN_QB', 'LDMK_WGRAD_TR')]\n"
            "so.ldmk_switch_override(b'LDMK_IG_LEAN', 1)\n"
            "b = v('LDMK_IG_LEAN')\n"
            "so.ldmk_switch_override(b'LDMK_IG_LEAN', -1)\n"
            "print(a, b, v('LDMK_IG_LEAN'))\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LDMK_")}
    env.update(LDMK_IG_LEAN="0", LDMK_ATTN_PIPE="1", LDMK_WGRAD_TR="junk")
    out = subprocess.run([sys.executable, "-c", code, lib._name], env=env, check=True, capture_output=True, text=True).stdout
    assert out.strip() == "[0, 1, 1, 0, 0] 1 0", out
