"""bench.py --dump-outputs: what the last timed step computed, as <name>.npy in float32 / float64, at most 64 MB in all (over the
limit a fixed, seeded sample of the rows, the same rows for arrays of the same length).  No device involved."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_arrays_are_written_whole_under_the_limit(tmp_path):
    g = np.linspace(0, 1, 7, dtype=np.float32)
    m = np.arange(21, dtype=np.float32).reshape(7, 3)
    bench.dump_outputs(str(tmp_path), {"global_misfits": g, "misfits": m, "wide": np.arange(3, dtype=np.float64)})
    assert sorted(os.listdir(tmp_path)) == ["global_misfits.npy", "misfits.npy", "wide.npy"]
    assert np.array_equal(np.load(tmp_path / "global_misfits.npy"), g)
    assert np.array_equal(np.load(tmp_path / "misfits.npy"), m)
    assert np.load(tmp_path / "wide.npy").dtype == np.float64


def test_over_the_limit_a_seeded_sample_of_the_same_rows(tmp_path):
    g = np.arange(1000, dtype=np.float32)
    m = np.repeat(g[:, None], 50, axis=1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"global_misfits": g, "misfits": m.astype(np.int32)}, limit=40000)
    ga, ma = np.load(tmp_path / "a" / "global_misfits.npy"), np.load(tmp_path / "a" / "misfits.npy")
    assert ga.dtype == np.float32 and ma.dtype == np.float32
    assert ga.nbytes + ma.nbytes <= 40000 and len(ga) > 100
    assert np.array_equal(ma[:, 0], ga) and np.all(np.diff(ga) > 0)
    assert np.array_equal(ga, np.load(tmp_path / "b" / "global_misfits.npy"))
    assert np.array_equal(ma, np.load(tmp_path / "b" / "misfits.npy"))
    assert bench.DUMP_LIMIT_BYTES == 64 << 20
