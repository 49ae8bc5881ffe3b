"""fp32 against bf16 inference, alternated in one process: frames/s of each generator precision through PipelinedRunner.

    python tools/infer_precision_bench.py [--batch 128] [--depth 4] [--alternations 5] [--min-seconds 1.0]

Both runners (seed-0 synthetic weights, BASELINE cfg2 inputs) are warmed on every shape first.  A sample keeps submitting
batches until at least --min-seconds of device time have passed between two events on the caller's stream; samples of fp32 and
bf16 alternate, --alternations pairs.  Prints one JSON line: per precision the frames/s of every sample, median, min and max
(the spread), the bf16 / fp32 ratio of the medians, and the uint8 difference of the last timed bf16 batch against the fp32 one
(share of bytes that differ, worst level, mean absolute level)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wav2lip_amd import models  # noqa: E402
from wav2lip_amd import synthetic as synth  # noqa: E402
from wav2lip_amd.inference import PipelinedRunner  # noqa: E402


def sample(runner, faces, mels, n, min_s):
    """run batches until >= min_s seconds of device time; returns (frames/s, last batch's uint8 frames)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pending, batches, last = [], 0, None
    e0.record()
    while True:
        pending.append(runner.submit(faces, mels))
        batches += 1
        if len(pending) >= runner.depth:
            last = runner.result(pending.pop(0))
        if batches % runner.depth == 0:
            e1.record()
            e1.synchronize()
            if e0.elapsed_time(e1) >= 1000.0 * min_s:
                break
    while pending:
        last = runner.result(pending.pop(0))
    e1.record()
    e1.synchronize()
    return batches * n / (e0.elapsed_time(e1) / 1000.0), last.cpu().numpy().copy()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    a = ap.parse_args(argv)
    if a.alternations < 1 or a.min_seconds <= 0:
        ap.error("--alternations >= 1 and --min-seconds > 0")
    dev = torch.device("cuda", 0)
    G = models.Wav2Lip()
    G.load_state_dict(synth.synthetic_state_dict({k: tuple(v.shape) for k, v in G.state_dict().items()}, seed=0))
    G = G.to(dev).eval()
    faces = torch.from_numpy(synth.face_crops_u8(a.batch, seed=5)).to(dev)
    mels = torch.from_numpy(synth.mel_windows(a.batch, seed=5)).to(dev)
    runners = {p: PipelinedRunner(G, a.batch, depth=a.depth, precision=p) for p in ("f32", "bf16")}
    for r in runners.values():            # every lane builds its plan (and split-K scratch) before anything is timed
        for t in [r.submit(faces, mels) for _ in range(2 * a.depth)]:
            r.result(t)
    torch.cuda.synchronize()
    fps = {p: [] for p in runners}
    last = {}
    for _ in range(a.alternations):
        for p, r in runners.items():
            f, last[p] = sample(r, faces, mels, a.batch, a.min_seconds)
            fps[p].append(f)
    d = np.abs(last["bf16"].astype(np.int32) - last["f32"].astype(np.int32))
    out = {"batch": a.batch, "depth": a.depth, "alternations": a.alternations, "min_seconds": a.min_seconds,
           "device": torch.cuda.get_device_name(dev)}
    for p, v in fps.items():
        out[p] = {"frames_per_s": [round(x, 1) for x in v], "median": round(float(np.median(v)), 1),
                  "min": round(float(np.min(v)), 1), "max": round(float(np.max(v)), 1)}
    out["speedup_median"] = round(out["bf16"]["median"] / out["f32"]["median"], 3)
    out["speedup_range"] = [round(out["bf16"]["min"] / out["f32"]["max"], 3), round(out["bf16"]["max"] / out["f32"]["min"], 3)]
    out["u8_vs_f32"] = {"bytes_differ": round(float((d != 0).mean()), 5), "worst_level": int(d.max()),
                        "mean_level": round(float(d.mean()), 5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
