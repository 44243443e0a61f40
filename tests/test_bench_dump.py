"""CPU: bench.py --dump-outputs writes float32 .npy files named after the arrays, and a dump over its byte budget becomes a fixed, seeded sample."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_writes_float32_arrays_by_name(tmp_path):
    w = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    bench.dump_outputs(str(tmp_path), {"loss_dice": np.array([0.5, 0.25], np.float32), "c1a/kernel": w})
    assert sorted(os.listdir(tmp_path)) == ["c1a.kernel.npy", "loss_dice.npy"]
    k = np.load(tmp_path / "c1a.kernel.npy")
    assert k.dtype == np.float32 and k.shape == (2, 3, 4) and np.array_equal(k, w.astype(np.float32))


def test_dump_over_budget_is_a_fixed_sample(tmp_path):
    arrays = {"a": np.arange(10000, dtype=np.float32), "b": np.arange(3000, dtype=np.float32) * 2}
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=13000 * 4 // 10)
    a, b = np.load(tmp_path / "x" / "a.npy"), np.load(tmp_path / "x" / "b.npy")
    assert a.nbytes + b.nbytes <= 13000 * 4 // 10 and a.size == 1000 and b.size == 300
    assert np.all(np.diff(a) > 0) and np.isin(a, arrays["a"]).all() and np.isin(b, arrays["b"]).all()
    assert np.array_equal(a, np.load(tmp_path / "y" / "a.npy")) and np.array_equal(b, np.load(tmp_path / "y" / "b.npy"))
