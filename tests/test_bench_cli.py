"""CPU: bench.py's command line (no GPU): a plain run has every side
measurement off, --full turns them back on under their --no-* options, and
--dump-outputs writes uint64 limbs as exact float64 words."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_side_legs(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert all(getattr(a, "no_" + leg) for leg in bench.SIDE_LEGS)
    assert not a.no_table  # the headline's own fixed-base table stays


def test_full_run_keeps_the_no_options(monkeypatch):
    a = _parse(monkeypatch, "--full", "--no-l2", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    assert [leg for leg in bench.SIDE_LEGS if getattr(a, "no_" + leg)] == ["l2"]


def test_dump_outputs_is_exact(tmp_path):
    x = np.array([2**64 - 1, 1, 2**63, 3, 2**32, 5, 6, 2**53 + 1], np.uint64)
    bench.dump_outputs(str(tmp_path / "out"), {"msm_g1_result": x})
    y = np.load(tmp_path / "out" / "msm_g1_result.npy")
    assert y.dtype == np.float64 and y.shape == (16,)
    assert np.array_equal(y.astype("<u4").view("<u8"), x)
