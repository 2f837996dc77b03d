"""bench.py's two forms on a small batch: a plain run prints the headline alone (and writes --dump-outputs), --full adds the
legs that take runs of their own -- overlapped batches, per-kernel times and roofline, host-fed uploads, CPU baseline with
the in-run parity check, parameter sets."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels_ms_per_step", "search_fit", "overlapped_batches_frames_per_s", "host_fed", "cpu_baseline",
             "parity", "settings", "config1", "stream")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "16", "--steps", "2",
                        "--warmup", "1"] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_prints_the_headline_alone(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    assert all(k in line for k in HEADLINE)
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert line["config"]["frames_per_gpu_per_step"] == 16
    assert not [k for k in FULL_ONLY if k in line]
    frames = np.load(os.path.join(str(tmp_path), "frame.npy"))
    assert list(frames) == list(range(16))
    assert np.load(os.path.join(str(tmp_path), "masks_sample.npy")).shape[0] == 8


def test_full_run_adds_the_other_legs():
    line = _bench("--full", "--no-stream")          # (--no-stream: the stream leg and config 1 alone take half a minute)
    assert all(k in line for k in HEADLINE)
    assert line["roofline"]["stage_ms_per_launch"] > 0 and line["kernels_ms_per_step"]["sws_fit"] > 0
    assert line["overlapped_batches_frames_per_s"] > 0 and line["host_fed"]["overlapped_frames_per_s"] > 0
    assert line["parity"]["record_mismatches"] == 0 and line["parity"]["mask_mismatches"] == 0
    assert line["cpu_baseline"]["value"] > 0
    assert set(line["settings"]) >= {"process_defaults", "demo1", "second_try"}
    assert "stream" not in line and "config1" not in line
