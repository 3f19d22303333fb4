"""Black-box candidate rollouts (fgx_rollout_bb, include/fgx.h): the boundary, without a GPU.

Both entry points are declared in the header, bound in ``_lib.EXPORTS`` with as many arguments as the
declaration has, and exported by the built library; the ABI version is still 9 (the call adds to the
ABI, as fgx_rollout_raw did)."""
import os
import re
import subprocess

from fancy_gym_crowd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fgx_rollout_bb_workspace", "fgx_rollout_bb")


def _header():
    with open(os.path.join(ROOT, "include", "fgx.h")) as f:
        return f.read()


def test_declared_and_bound_with_matching_arity():
    header = _header()
    for name in NAMES:
        m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", header, re.S | re.M)
        assert m, f"{name} is not declared in include/fgx.h"
        params = [p for p in m.group(1).split(",") if p.strip()]
        assert name in _lib.EXPORTS, f"{name} is not bound in _lib.EXPORTS"
        res, args = _lib.EXPORTS[name]
        assert len(params) == len(args), (name, len(params), len(args))
    assert len(_lib.EXPORTS["fgx_rollout_bb_workspace"][1]) == 3
    assert len(_lib.EXPORTS["fgx_rollout_bb"][1]) == 11


def test_exported_by_the_built_library():
    from fancy_gym_crowd_amd import _build
    _build.build()   # no-op when the library's build id matches the sources
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NAMES) <= exported, set(NAMES) - exported


def test_abi_version_is_still_9():
    assert re.search(r"^#define FGX_ABI_VERSION 9\s*$", _header(), re.M)
    assert _lib.FGX_ABI_VERSION == 9
