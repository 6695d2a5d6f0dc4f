"""bench.py --dump-outputs on the host: an output within its budget is written whole, a larger one as a fixed, seeded
sample of its rows with the row numbers beside it, the same call gives the same files, and the 64 MiB limit holds."""
import os

import numpy as np
import pytest
import torch

import bench


def _arrays():
    g = torch.Generator().manual_seed(7)
    soft = torch.randint(-127, 128, (600, 3072), generator=g, dtype=torch.int32).to(torch.int8)
    crc = torch.randint(0, 2, (50, 12), generator=g, dtype=torch.int32).to(torch.uint8)
    fo = np.linspace(-1e-3, 1e-3, 8, dtype=np.float32)[:, None]
    return soft, crc, fo


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_whole_and_sampled_outputs(tmp_path):
    soft, crc, fo = _arrays()
    budget = 100 * 3072 * 4                                     # room for 100 of the 600 rows
    names = bench.dump_outputs(torch, str(tmp_path / "a"), [("soft_bits", soft, budget), ("crc", crc, 1 << 20),
                                                            ("fo", fo, 1 << 20)])
    assert names == ["crc", "fo", "soft_bits", "soft_bits_rows"]
    out = _load(tmp_path / "a")
    assert out["crc"].dtype == np.float32 and (out["crc"] == crc.numpy()).all()
    assert out["fo"].dtype == np.float32 and (out["fo"] == fo).all()
    rows = out["soft_bits_rows"]
    assert rows.dtype == np.float64 and rows.shape == (100,) and (np.diff(rows) > 0).all()
    assert out["soft_bits"].dtype == np.float32 and (out["soft_bits"] == soft.numpy()[rows.astype(np.int64)]).all()
    bench.dump_outputs(torch, str(tmp_path / "b"), [("soft_bits", soft, budget), ("crc", crc, 1 << 20), ("fo", fo, 1 << 20)])
    again = _load(tmp_path / "b")
    assert all(np.array_equal(out[k], again[k]) for k in out)


def test_dump_refuses_more_than_64_mib(tmp_path):
    big = torch.zeros((4, 5 << 20), dtype=torch.int8)          # 80 MiB as float32, all of it inside its own budget
    with pytest.raises(SystemExit):
        bench.dump_outputs(torch, str(tmp_path), [("big", big, 1 << 30)])
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".npy")]


def test_steps_set_the_timed_steps():
    assert bench.parse_args(["--steps", "7", "--warmup", "0"]).steps == 7
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_full_is_off_by_default_and_the_legs_need_it():
    assert bench.parse_args([]).full is False and bench.parse_args(["--full"]).full is True
    assert bench.parse_args(["--legs", "none"]).legs == "none"
    assert bench.parse_args(["--full", "--legs", "all"]).legs == "all"
    with pytest.raises(SystemExit):
        bench.parse_args(["--legs", "all"])
