"""`python bench.py --dump-outputs DIR` on the device: the timed path's last step lands in DIR as float32 arrays, the uint8 frames
are exactly the conversion of the float prediction beside them (w2l_frames_to_u8 is numpy's `pred * 255.` truncated), and the
result line names what was written."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import datagen_ref

pytestmark = pytest.mark.gpu


def test_bench_dump_outputs_holds_the_last_steps_frames_and_their_prediction(tmp_path):
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--windows", "1", "--sustained-seconds", "0", "--no-cpu-baseline", "--no-train-configs",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-500:], p.stderr[-1500:])
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    d = r["dump_outputs"]
    assert d["files"] == {"frames_u8.npy": [128, 96, 96, 3], "pred_nchw.npy": [128, 3, 96, 96]}
    assert set(d["contents"]) == {"frames_u8", "pred_nchw"}
    assert sorted(os.listdir(out)) == ["frames_u8.npy", "pred_nchw.npy"]
    frames = np.load(out / "frames_u8.npy")
    pred = np.load(out / "pred_nchw.npy")
    assert frames.dtype == np.float32 and pred.dtype == np.float32
    assert np.isfinite(pred).all() and 0.0 <= pred.min() and pred.max() <= 1.0       # the generator ends in a sigmoid
    assert np.array_equal(frames, datagen_ref.frames_to_u8(pred).astype(np.float32))
    assert len(np.unique(frames)) > 16                                                 # real frames, not a cleared buffer


def _bench_line(extra, cwd):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--windows", "1"] + extra, capture_output=True, text=True, timeout=300, env=env, cwd=str(cwd))
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-500:], p.stderr[-1500:])
    return json.loads(lines[0])


def test_plain_bench_run_times_the_steps_and_full_adds_the_rest(tmp_path):
    """a plain run prints the headline line from the timed windows alone; --full (here without the CPU legs) adds the sustained
    window with its clock samples and the dominant kernel's serial pass"""
    r = _bench_line([], tmp_path)
    assert r["config"]["full"] is False and r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert abs(r["value"] - 128 * 1e3 / r["ms_per_step"]) <= 1e-3 * r["value"]
    assert r["roofline"]["frac"] > 0 and r["roofline"]["dominant_kernel"] is None and r["roofline"]["sustained_clock_mhz"] is None
    assert r["windows"]["sustained"] is None
    assert not {"cpu_baseline", "parity", "other_configs", "exact_value", "value_with_mel_and_d2h"} & set(r)
    f = _bench_line(["--full", "--no-cpu-baseline", "--sustained-seconds", "0.2"], tmp_path)
    assert f["config"]["full"] is True and f["roofline"]["dominant_kernel"]["launches_per_step"] > 0
    assert f["roofline"]["serial_ms_per_step"] > 0 and f["roofline"]["sustained_clock_mhz"] > 0
    assert f["windows"]["sustained"]["steps"] >= 3 and f["windows"]["sustained"]["clock_samples"]["n"] >= 1
