"""Step-based rollouts on the CPU: the C ABI entry point is declared, bound and exported, and the
LDS sizing of k_rollout_raw (csrc/fgx_rollout_lds.h, one statement for the kernel and its launch)
gives the chunk and region sizes worked out by hand below.

Sizing rule: a lane's share of the action staging is 20 floats (160 KiB of LDS per CU / 8 workgroups
of 256 lanes / 4 B), rows have the odd stride dof | 1, so the chunk is 20 // (dof | 1) steps (at most
16); a wave's region is the larger of chunk * 64 * (dof | 1) and, when observations leave through it,
64 * (obs_dim | 1) floats; a workgroup has four waves."""
import ctypes
import os
import re
import subprocess

from fancy_gym_crowd_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_entry_point_is_declared_and_bound():
    res, args = _lib.EXPORTS["fgx_rollout_raw"]
    assert res is ctypes.c_int and len(args) == 12
    assert [a for a in args if a is ctypes.c_int32] == [ctypes.c_int32] * 3   # horizon, n_cand, commit
    assert args[2] is ctypes.c_int32 and args[3] is ctypes.c_int32 and args[10] is ctypes.c_int32
    header = open(os.path.join(ROOT, "include", "fgx.h")).read()
    m = re.search(r"^int\s+fgx_rollout_raw\s*\(([^)]*)\)\s*;", header, re.S | re.M)
    assert m, "fgx_rollout_raw is not declared in include/fgx.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["void* handle", "const float* actions", "int32_t horizon", "int32_t n_cand", "double* returns",
                      "int32_t* lengths", "uint8_t* terminated", "uint8_t* truncated", "float* obs", "double* rewards",
                      "int32_t commit", "void* stream"]
    assert "base_reacher.py:98-119" in header
    assert _lib.FGX_ABI_VERSION == 9 and "#define FGX_ABI_VERSION 9" in header


# (dof, obs_dim): chunk, stride, floats of a wave's region, bytes of a workgroup
#   obs_dim = 3 dof + 3 (SimpleReacher), + 4 (HoleReacher), + 5 (ViaPointReacher); 0: no observations
SIZES = {
    (1, 6): (16, 1, 1024, 16384),       # 16 * 64 * 1 = 1024 > 64 * 7
    (2, 9): (6, 3, 1152, 18432),        # 6 * 64 * 3 = 1152 > 64 * 9
    (2, 10): (6, 3, 1152, 18432),       # 64 * 11 = 704
    (2, 11): (6, 3, 1152, 18432),
    (5, 18): (4, 5, 1280, 20480),       # 4 * 64 * 5 = 1280 > 64 * 19 = 1216
    (5, 19): (4, 5, 1280, 20480),
    (5, 20): (4, 5, 1344, 21504),       # 64 * 21 = 1344: the observation rows are the larger
    (8, 27): (2, 9, 1728, 27648),       # 2 * 64 * 9 = 1152 < 64 * 27
    (8, 28): (2, 9, 1856, 29696),       # 64 * 29
    (8, 29): (2, 9, 1856, 29696),
    (5, 0): (4, 5, 1280, 20480),        # no observations: the action chunk alone
    (8, 0): (2, 9, 1152, 18432),
}


def test_lds_sizing(tmp_path):
    exe = str(tmp_path / "rollout_lds_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wno-unused-result",
                    os.path.join(HERE, "host", "rollout_lds_check.hip"), "-o", exe], check=True)
    argv = [str(x) for key in SIZES for x in key]
    out = subprocess.run([exe, *argv], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {tuple(v[:2]): tuple(v[2:]) for v in (list(map(int, line.split())) for line in out if line)}
    assert got == SIZES
    for (dof, od), (chunk, stride, floats, lds) in SIZES.items():
        assert stride % 2 == 1 and chunk * stride <= 20 and lds == 16 * floats
        # the action staging alone never takes more than 1/8 of a CU's LDS; with the widest
        # observation rows five workgroups still fit
        assert 4 * 4 * chunk * 64 * stride <= 160 * 1024 // 8 and 5 * lds <= 160 * 1024
