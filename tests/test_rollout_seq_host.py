"""Black-box sequence rollouts (fgx_rollout_bb_seq, include/fgx.h): the boundary, without a GPU.

The entry point is declared in the header, bound in ``_lib.EXPORTS`` with the declaration's fifteen
arguments and a ``c_int`` result, and exported by the built library; the ABI version is still 9 (the
call adds to the ABI, as the two rollouts before it did)."""
import ctypes
import os
import re
import subprocess

from fancy_gym_crowd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fgx_rollout_bb_seq"


def _header():
    with open(os.path.join(ROOT, "include", "fgx.h")) as f:
        return f.read()


def test_declared_and_bound_with_fifteen_arguments():
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header(), re.S | re.M)
    assert m, f"{NAME} is not declared in include/fgx.h"
    params = [p.strip() for p in m.group(1).split(",") if p.strip()]
    assert len(params) == 15, params
    assert NAME in _lib.EXPORTS, f"{NAME} is not bound in _lib.EXPORTS"
    res, args = _lib.EXPORTS[NAME]
    assert res is ctypes.c_int
    assert len(args) == 15
    # the two counts are the only 32-bit integers, the workspace size the only 64-bit one
    for decl, arg in zip(params, args):
        want = ctypes.c_int32 if decl.startswith("int32_t ") else ctypes.c_int64 if decl.startswith("int64_t ") \
            else ctypes.c_void_p
        assert arg is want, (decl, arg)


def test_exported_by_the_built_library():
    from fancy_gym_crowd_amd import _build
    _build.build()   # no-op when the library's build id matches the sources
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert NAME in exported


def test_abi_version_is_still_9():
    assert re.search(r"^#define FGX_ABI_VERSION 9\s*$", _header(), re.M)
    assert _lib.FGX_ABI_VERSION == 9
