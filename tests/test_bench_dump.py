"""bench.py --dump-outputs / --full without a GPU: the saved sample is fixed by the arguments, float32 / float64, at most 64 MB, and
holds the rows of exactly the drones it names; a plain run's options leave every auxiliary leg off."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import bench  # noqa: E402


class _Env:
    """The parts of fpyv_amd.env._Batch that dump_outputs reads, on CPU tensors."""

    def __init__(self, n, rows=14, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.n, self.rows, self.device = n, rows, torch.device("cpu")
        self.state = torch.randn((rows, n + 64), generator=g)              # padded row stride, like the device state
        self.reward = torch.randn(n, generator=g)
        self.done = torch.rand(n, generator=g) < 0.1

    def rows_f32(self, r0, r1):
        return self.state[r0:r1, :self.n].t()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_samples_large_populations_the_same_way(tmp_path):
    n = (1 << 20) + 3
    e = _Env(n)
    bench.dump_outputs(e, str(tmp_path / "a"))
    bench.dump_outputs(_Env(n, seed=1), str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["done", "drone_index", "reward", "state"]
    assert np.array_equal(a["drone_index"], b["drone_index"]), "the sample depends on the arguments only"
    idx = a["drone_index"]
    k = bench.DUMP_SAMPLE_DRONES
    assert idx.dtype == np.float64 and idx.shape == (k,) and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    ii = idx.astype(np.int64)
    assert a["state"].dtype == np.float32 and a["state"].shape == (k, e.rows)
    assert np.array_equal(a["state"], e.state[:, :n].t().numpy()[ii])
    assert np.array_equal(a["reward"], e.reward.numpy()[ii])
    assert a["done"].dtype == np.float32 and np.array_equal(a["done"], e.done.numpy()[ii].astype(np.float32))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64 << 20


def test_dump_of_a_small_shard_is_whole_and_ranks_are_named(tmp_path):
    e = _Env(5000)
    for r in range(4):
        bench.dump_outputs(e, str(tmp_path), rank=r, world=4)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(f"{x}_rank{r}.npy" for x in ("done", "drone_index", "reward", "state") for r in range(4))
    st = np.load(tmp_path / "state_rank2.npy")
    assert np.array_equal(np.load(tmp_path / "drone_index_rank2.npy"), np.arange(5000, dtype=np.float64))
    assert np.array_equal(st, e.state[:, :5000].t().numpy())


def test_plain_run_options():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
