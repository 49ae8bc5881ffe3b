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
