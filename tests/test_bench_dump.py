"""bench.py --dump-outputs (CPU): whole arrays under the size limit, one fixed seeded row sample
shared by the arrays over it, float64 files, the same bytes from run to run."""
import os

import numpy as np


def _load(d):
    return {f: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    import bench
    res = np.asfortranarray(np.arange(600, dtype=np.float64).reshape(100, 6))
    bench.dump_outputs(str(tmp_path / "d"), {"results": res})
    got = _load(tmp_path / "d")
    assert list(got) == ["results.npy"]
    assert got["results.npy"].dtype == np.float64 and np.array_equal(got["results.npy"], res)


def test_large_outputs_share_one_seeded_row_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 16)
    jp = np.asfortranarray(np.arange(3000 * 7, dtype=np.float64).reshape(3000, 7))
    modes = np.asfortranarray(np.arange(3000 * 33, dtype=np.float32).reshape(3000, 33))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"jp": jp, "modes": modes})
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert list(a) == ["jp.npy", "jp_rows.npy", "modes.npy", "modes_rows.npy"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 1 << 16
    rows = a["jp_rows.npy"].astype(int)
    assert np.array_equal(rows, a["modes_rows.npy"]) and np.all(np.diff(rows) > 0) and rows[-1] < 3000
    # more than a quarter of the limit is used, and the rows are the arrays' own
    assert sum(v.nbytes for v in a.values()) > 1 << 14
    assert np.array_equal(a["jp.npy"], jp[rows]) and np.array_equal(a["modes.npy"], modes[rows])
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_rank_suffix_in_a_multi_rank_run(tmp_path):
    import bench
    bench.dump_outputs(str(tmp_path), {"results": np.zeros((4, 6))}, rank=1, world=2)
    assert os.listdir(tmp_path) == ["results.rank1.npy"]
