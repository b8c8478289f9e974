"""CPU: bench.py's run options -- a plain run is the default, --steps is checked, and --dump-outputs stays within its size bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse_args([])
    assert not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out", "--steps", "5"])
    assert a.full and a.dump_outputs == "out" and a.steps == 5
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_writes_the_frame_or_a_fixed_sample(tmp_path):
    small = np.random.default_rng(1).random((48, 64, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "small"), small)
    assert np.array_equal(np.load(tmp_path / "small" / "framebuffer.npy"), small)
    # a 2048 x 2048 RGBA32F frame (64 MiB) is written as a sample of whole pixels, the same one every time
    big = np.arange(2048 * 2048 * 4, dtype=np.float32).reshape(2048, 2048, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    assert os.listdir(tmp_path / "a") == ["framebuffer_sample.npy"]
    s = np.load(tmp_path / "a" / "framebuffer_sample.npy")
    assert s.dtype == np.float32 and s.shape[1] == 4 and s.nbytes <= bench.MAX_DUMP_BYTES
    assert os.path.getsize(tmp_path / "a" / "framebuffer_sample.npy") < 64e6
    assert np.array_equal(s, np.load(tmp_path / "b" / "framebuffer_sample.npy"))
    assert np.array_equal(s[:, 1:] - s[:, :1], np.broadcast_to(np.float32([1, 2, 3]), (len(s), 3)))
    assert np.all(np.diff(s[:, 0]) > 0)
