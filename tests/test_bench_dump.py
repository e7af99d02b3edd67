"""bench.py --dump-outputs on the host: the files it writes (world-major float64) and the fixed, seeded sample of worlds above its size cap."""
import numpy as np

import bench


def test_dump_outputs_writes_world_major_float64(tmp_path):
    rng = np.random.default_rng(0)
    nxt, st = rng.normal(size=(6, 10)), np.arange(10, dtype=np.int32)
    bench.dump_outputs(str(tmp_path), {"next_state": nxt, "status": st}, {"shared_action_grad": np.ones(3)})
    got = {f.stem: np.load(f) for f in tmp_path.glob("*.npy")}
    assert set(got) == {"next_state", "status", "shared_action_grad"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["next_state"], nxt.T) and np.array_equal(got["status"], np.arange(10.0))
    assert np.array_equal(got["shared_action_grad"], np.ones(3))


def test_dump_outputs_samples_the_same_worlds_of_every_array_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    B = 1000
    a = np.arange(4 * B, dtype=np.float64).reshape(4, B)             # [dof][B]
    b = np.arange(B, dtype=np.float64)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b}, {"g": np.zeros(2)})
    got = {f.stem: np.load(f) for f in (tmp_path / "one").glob("*.npy")}
    idx = got["world_index"].astype(np.int64)
    assert sum(x.nbytes for x in got.values()) <= 4096 and len(idx) > 0 and np.all(np.diff(idx) > 0)
    assert np.array_equal(got["a"], a.T[idx]) and np.array_equal(got["b"], b[idx])
    again = {f.stem: np.load(f) for f in (tmp_path / "two").glob("*.npy")}
    assert all(np.array_equal(got[k], again[k]) for k in got)          # fixed seed: the same sample every run
