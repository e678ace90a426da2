"""bench.py's command line without a GPU: what a plain run leaves out (`--full`), the `--steps` contract and the
`--dump-outputs` files (full image, or a fixed seeded sample above the size cap)."""
import sys

import numpy as np
import pytest

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_leaves_the_extras_to_full(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "2")
    assert (a.full, a.steps, a.warmup, a.dump_outputs) == (False, 3, 2, None)
    a = parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(monkeypatch, argv):
    with pytest.raises(SystemExit):
        parse(monkeypatch, *argv)


def test_dump_writes_the_image_as_it_is(tmp_path):
    img = np.random.default_rng(3).random((36, 64, 3))
    bench.dump_outputs(str(tmp_path / "d"), img)
    got = np.load(tmp_path / "d" / "image.npy")
    assert got.dtype == np.float64 and np.array_equal(got, img)
    bench.dump_outputs(str(tmp_path / "f"), img.astype(np.float32))
    assert np.load(tmp_path / "f" / "image.npy").dtype == np.float32


def test_dump_of_a_large_image_is_a_fixed_sample_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 24 * 1000)
    img = np.arange(100 * 80 * 3, dtype=np.float64).reshape(100, 80, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), img)
    a, b = np.load(tmp_path / "a" / "image_sample.npy"), np.load(tmp_path / "b" / "image_sample.npy")
    assert not (tmp_path / "a" / "image.npy").exists()
    assert a.shape == (1000, 3) and a.nbytes <= bench.DUMP_MAX_BYTES and np.array_equal(a, b)
    pix = a[:, 0] / 3  # (pixel index of each sampled row: the test image counts up)
    assert np.all(np.diff(pix) > 0) and np.array_equal(a, img.reshape(-1, 3)[pix.astype(np.int64)])
