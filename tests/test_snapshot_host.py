"""The snapshot blob layout on the CPU (csrc/fgx_snapshot.h: snapshot_layout, the one function
fgx_snapshot_bytes, k_snapshot and k_restore place their sections by): tests/host/snapshot_layout.hip
runs it over env kind x link count x aux / cond present or absent x env count, checks the invariants
itself and prints every section; the numbers are checked here again against the formula written out
in Python.  Also the C ABI's version and the five ABI-9 names in the ctypes table."""
import os
import re
import shutil
import subprocess

import pytest

from fancy_gym_crowd_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ORDER = ["q", "qd", "goal", "hole", "aux", "steps", "plans", "flags", "rng", "cond", "start"]


def _bytes_per_env(nl):
    # f64 [nl][N] x 2, f64 [2][N], f64 [3][N] x 2, i32 / u32 [N] x 3, u64 [5][N], f32 [2][nl][N], f64 [N]
    return dict(q=8 * nl, qd=8 * nl, goal=16, hole=24, aux=24, steps=4, plans=4, flags=4, rng=40, cond=8 * nl, start=8)


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_snapshot_layout(tmp_path):
    exe = str(tmp_path / "snapshot_layout")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-Wno-unused-result",
                    os.path.join(HERE, "host", "snapshot_layout.hip"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == 3 * 4 * 2 * 2 * 3
    seen = set()
    for ln in lines:
        m = re.match(r"(simple|hole|via) nl=(\d+) aux=([01]) cond=([01]) N=(\d+) bytes=(\d+) (.*)$", ln)
        assert m, ln
        kind, nl, aux, cond, N, total = m.group(1), *map(int, m.group(2, 3, 4, 5, 6))
        seen.add((kind, nl, aux, cond, N))
        secs = [re.match(r"(\w+)=(\d+):(\d+):([01])$", s).groups() for s in m.group(7).split()]
        assert [s[0] for s in secs] == ORDER, ln          # the stated order
        bpe = _bytes_per_env(nl)
        end, want_total = 0, 0
        for name, off, b, present in secs:
            off, b, present = int(off), int(b), int(present)
            assert present == {"aux": aux, "cond": cond}.get(name, 1), (ln, name)
            assert off % 256 == 0, (ln, name)
            assert off >= end, (ln, name)                  # no overlap, offsets never decrease
            if not present:
                assert b == 0                              # an absent section takes no space:
                continue                                   # `end` stays, the next one may start at `off`
            assert b == bpe[name], (ln, name)
            assert off == -(-end // 256) * 256, (ln, name)   # and no gap beyond the alignment
            end = off + b * N
            want_total += -(-b * N // 256) * 256
        assert total == want_total == -(-end // 256) * 256, ln
    assert seen == {(k, nl, a, c, N) for k in ("simple", "hole", "via") for nl in (1, 2, 5, 8) for a in (0, 1)
                    for c in (0, 1) for N in (1, 67, 256)}


def test_abi_9_exports():
    assert _lib.FGX_ABI_VERSION == 9
    for name in ("fgx_snapshot_bytes", "fgx_snapshot", "fgx_restore", "fgx_fingerprint", "fgx_copy_envs"):
        assert name in _lib.EXPORTS, name
        assert _lib.EXPORTS[name][0] is _lib.ctypes.c_int   # values come back through out-parameters
