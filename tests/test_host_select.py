"""The episode-kernel selection table on the CPU (csrc/fgx_select.h: select_episode_kernel, the one
function fgx_step launches by and fgx_episode_kernel reports): tests/host/select_table.hip runs it over
a grid of synthetic configurations, step requests and FGX_EPISODE_KERNEL / FGX_V2 / FGX_HP settings
(the CU count is an input, fixed at 256) and prints one line per case; the output must equal
tests/host/select_table.expected byte for byte.  That file was recorded from the selection code before
it was gathered into one function, so a change of it is a change of which kernel runs: a new rule or
threshold changes the expected lines it is meant to change and no others.  (The on-device statement of
the same table is tests/test_gpu_ws.py::test_episode_kernel_selection.)"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_selection_table_is_unchanged(tmp_path):
    exe = str(tmp_path / "select_table")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-Wno-unused-result",
                    os.path.join(HERE, "host", "select_table.hip"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("FGX_EPISODE_KERNEL", "FGX_V2", "FGX_HP")}
    got = subprocess.run([exe], check=True, capture_output=True, env=env).stdout
    with open(os.path.join(HERE, "host", "select_table.expected"), "rb") as f:
        want = f.read()
    if got != want:
        g, w = got.decode().splitlines(), want.decode().splitlines()
        diff = [f"want {a!r}\n got {b!r}" for a, b in zip(w, g) if a != b]
        pytest.fail(f"{len(diff)} of {len(w)} lines differ ({len(g)} printed); first:\n" + "\n".join(diff[:10]))
    kernels = {ln.rsplit(b" ", 1)[1] for ln in want.splitlines() if not ln.startswith(b"#")}
    assert len(kernels) == 9, kernels   # every EK_* value occurs
