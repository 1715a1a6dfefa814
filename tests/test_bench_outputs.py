"""bench.py's plain run and its --dump-outputs.

* CPU: dump_outputs on host tensors -- a small output whole, a large one as
  the fixed seeded sample beside the fold sums that cover all of it; float32,
  the same bytes from call to call, a changed element shows.
* GPU: a plain run (no --full) in this process, two timed steps of a 200K-key
  build: the result line carries the headline keys and none of the records
  that --full adds, and the dumped bitmap is the oracle's, byte for byte.
"""
import json
import os

import numpy as np
import pytest

import bench

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "parity", "cpu_baseline", "e2e", "compaction_strong", "headline_with_reader", "probe",
             "varlen", "ms_per_step_kernel_timed"}


def test_parse_defaults_are_plain():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_whole_and_sampled(tmp_path):
    import torch

    rng = np.random.default_rng(7)
    small = torch.from_numpy(rng.integers(0, 256, 1000, dtype=np.uint8))
    n = 100_003  # no multiple of the fold width: a tail sum
    large = torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "large": large}, sample=5000, folds=1000)
    assert sorted(os.listdir(tmp_path / "a")) == ["large.npy", "large_fold.npy", "small.npy"]
    for f in os.listdir(tmp_path / "a"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    got = np.load(tmp_path / "a" / "small.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy())
    samp = np.load(tmp_path / "a" / "large.npy")
    assert samp.dtype == np.float32 and samp.shape == (5000,)
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, 5000))
    assert np.array_equal(samp, large.numpy()[idx])
    fold = np.load(tmp_path / "a" / "large_fold.npy")
    width = 128  # the least power of two >= 64 with ceil(n / width) <= 1000
    assert fold.dtype == np.float32 and fold.shape == ((n + width - 1) // width,)
    want = np.add.reduceat(large.numpy().astype(np.int64), np.arange(0, n, width))
    assert np.array_equal(fold, want)
    # one element changed that the sample may miss: the fold shows it
    large2 = large.clone()
    large2[n - 1] ^= 1
    bench.dump_outputs(str(tmp_path / "c"), {"large": large2}, sample=5000, folds=1000)
    assert not np.array_equal(np.load(tmp_path / "c" / "large_fold.npy"), fold)


def test_dump_outputs_rank_suffix(tmp_path):
    import torch

    bench.dump_outputs(str(tmp_path), {"answers": torch.arange(10, dtype=torch.uint8)}, rank=1, world=2)
    assert os.listdir(tmp_path) == ["answers_rank1.npy"]


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, capsys, oracle):
    n = 200_000
    bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", "--keys", str(n), "--dump-outputs", str(tmp_path)])
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert HEADLINE_KEYS <= set(d) and not (FULL_ONLY & set(d)), sorted(d)
    assert d["metric"] == "Mkeys/s bloom-filter build (device-resident), 16B keys, bits/key=10"
    assert (d["unit"], d["higher_is_better"], d["dtype"], d["steps"], d["warmup"]) == ("Mkeys/s", True, "u32", 2, 1)
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - n / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * d["value"] + 0.1
    assert os.listdir(tmp_path) == ["bitmap.npy"]
    got = np.load(tmp_path / "bitmap.npy")
    want = oracle.keys2block(oracle.splitmix_keys16(0x5EED, n), bits_per_key=bench.BPK)
    assert got.dtype == np.float32 and np.array_equal(got, want)
