"""bench.py --dump-outputs (no GPU): dump_outputs writes one float .npy per output array, and
past its size bound every array keeps the same fixed, seeded sample of rows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs(n):
    rng = np.random.default_rng(5)
    return {"observations": torch.from_numpy(rng.standard_normal((n, 19), dtype=np.float32)),
            "returns": torch.from_numpy(rng.standard_normal(n)),
            "terminated": torch.from_numpy(rng.integers(0, 2, n).astype(np.uint8)),
            "trajectory_length": torch.from_numpy(rng.integers(1, 201, n).astype(np.int32))}


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_whole_arrays(tmp_path):
    outs = _outputs(257)
    bench.dump_outputs(str(tmp_path / "d"), outs)
    got = _load(str(tmp_path / "d"))
    assert sorted(got) == sorted(outs)
    assert got["observations"].dtype == np.float32 and got["returns"].dtype == np.float64
    assert got["terminated"].dtype == np.float32 and got["trajectory_length"].dtype == np.float32
    for k, t in outs.items():
        np.testing.assert_array_equal(got[k], t.numpy().astype(got[k].dtype))


def test_dump_samples_rows_past_the_bound(tmp_path, monkeypatch):
    outs = _outputs(1000)
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 20000)
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == sorted(list(outs) + ["sample_rows"])
    assert sum(v.nbytes for v in a.values()) <= 20000
    rows = a["sample_rows"].astype(np.int64)
    assert 100 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
    for k, t in outs.items():
        np.testing.assert_array_equal(a[k], t.numpy()[rows].astype(a[k].dtype))
        np.testing.assert_array_equal(a[k], b[k])
