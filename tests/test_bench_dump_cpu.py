"""bench.py's dump_outputs (--dump-outputs): float64 files, and above the size cap the same fixed, seeded sample of problems
taken from every per-problem array."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_float64_and_sampled_above_the_cap(tmp_path, monkeypatch):
    bench = _bench()
    B = 1000
    rng = np.random.default_rng(1)
    arrays = {"X": rng.standard_normal((B, 30)), "stats": rng.integers(0, 100, (B, 6)), "flag": rng.random(B) < 0.5, "loop_iters": 7}
    assert bench.dump_outputs(str(tmp_path / "all"), arrays, B) == sorted(arrays)
    for k, a in arrays.items():
        got = np.load(tmp_path / "all" / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, np.asarray(a, dtype=np.float64)), k
    # room for 100 problems: 30 + 6 + 1 doubles each, plus 8 bytes of index
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", (1 << 20) + 100 * (37 * 8 + 8))
    for d in ("s1", "s2"):
        assert bench.dump_outputs(str(tmp_path / d), arrays, B) == sorted(list(arrays) + ["problem_index"])
    idx = np.load(tmp_path / "s1" / "problem_index.npy")
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "problem_index.npy"))       # fixed seed: the same sample every run
    assert idx.dtype == np.float64 and len(idx) == 100 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < B
    i = idx.astype(np.int64)
    for k in ("X", "stats", "flag"):
        assert np.array_equal(np.load(tmp_path / "s1" / (k + ".npy")), np.asarray(arrays[k], dtype=np.float64)[i]), k
    assert float(np.load(tmp_path / "s1" / "loop_iters.npy")) == 7.0
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= bench.DUMP_BYTES_MAX
