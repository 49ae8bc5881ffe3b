"""Packed filelist scoring against the per-clip loop, alternated in one process: clips/s and windows/s of `evaluation.lse_many`
and of `for clip: evaluation.lse_like(syncnet, faces, mel)` over the same seeded clips.

    python tools/score_bench.py [--clips 200] [--alternations 5] [--batch 128] [--seed 0]

The clips are those of tools/filelist_bench.py (160x160 frames, lengths uniform in 30..120 mel chunks, one frame per chunk); their
96x96 face crops (fixed box, w2l_crop_resize_rows_u8) and mel spectrograms are made once, before any timing, and live on the
device: both loops start from crops and mel and end with every clip's scores on the host.  Each loop owns a SyncNet, so the
graphs it builds are its own.  Pass 0 of each loop is its warm-up and is reported separately; then the two loops alternate,
--alternations pairs.  The per-clip loop runs `lse_like` with its default batch of 64 and, because SyncNet_color keeps one
inference graph, rebuilds a graph whenever the window count changes: that is what the loop costs, in every pass.  Prints one
JSON line: per loop the clips/s and windows/s of every pass with median, min and max, the first-pass seconds, the number of
_SyncGraph builds per pass, and torch.cuda.max_memory_allocated after the loop's first pass (the peak since process start for
the packed loop, which runs first, and the peak over everything for the per-clip loop)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filelist_bench import BOX, make_clips  # noqa: E402
from wav2lip_amd import audio, calculate_scores, evaluation, models  # noqa: E402
from wav2lip_amd import synthetic as synth  # noqa: E402
from wav2lip_amd.models import syncnet  # noqa: E402

BUILDS = [0]
_real_graph = syncnet._SyncGraph


def _counting_graph(*a, **k):
    BUILDS[0] += 1
    return _real_graph(*a, **k)


def model(dev):
    S = models.SyncNet_color()
    S.load_state_dict(synth.synthetic_state_dict({k: tuple(v.shape) for k, v in S.state_dict().items()}, seed=2))
    return S.to(dev).eval()


def prepare(clips, dev):
    """[(faces u8 [T,96,96,3] on the device, mel [80,Tm] on the device)]"""
    out = []
    for frames, wav in clips:
        out.append((calculate_scores.face_crops(np.stack(frames), [BOX] * len(frames), dev), audio.melspectrogram_device(wav, dev)))
    torch.cuda.synchronize()
    return out


def run_packed(S, data, batch):
    t0 = time.perf_counter()
    res = evaluation.lse_many(S, (evaluation.ScoreJob(i, f, m) for i, (f, m) in enumerate(data)), batch_size=batch)
    torch.cuda.synchronize()
    return len(res), sum(r["n"] for r in res), time.perf_counter() - t0


def run_loop(S, data, batch):
    t0 = time.perf_counter()
    res = [evaluation.lse_like(S, f, m) for f, m in data]
    torch.cuda.synchronize()
    return len(res), sum(r["n"] for r in res), time.perf_counter() - t0


def stats(v):
    return {"samples": [round(x, 1) for x in v], "median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    data = prepare(make_clips(a.clips, a.seed), dev)
    syncnet._SyncGraph = _counting_graph
    out = {"clips": a.clips, "batch": a.batch, "alternations": a.alternations,
           "distinct_lengths": len({f.shape[0] for f, _ in data})}
    loops = {"packed": (run_packed, model(dev)), "per_clip": (run_loop, model(dev))}
    res = {k: {"clips_per_s": [], "windows_per_s": [], "graph_builds": []} for k in loops}

    def one_pass(name):
        fn, S = loops[name]
        BUILDS[0] = 0
        n, w, t = fn(S, data, a.batch)
        print("%s: %d clips, %d windows, %.2f s, %d graph builds" % (name, n, w, t, BUILDS[0]), file=sys.stderr, flush=True)
        return n, w, t, BUILDS[0]

    for name in loops:                                    # pass 0: warm-up
        n, w, t, b = one_pass(name)
        res[name].update(clips=n, windows=w, first_pass_s=round(t, 2), first_pass_graph_builds=b,
                         max_memory_allocated_gb=round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2))
    for _ in range(a.alternations):
        for name in loops:
            n, w, t, b = one_pass(name)
            res[name]["clips_per_s"].append(n / t)
            res[name]["windows_per_s"].append(w / t)
            res[name]["graph_builds"].append(b)
    for name in loops:
        res[name]["clips_per_s"] = stats(res[name]["clips_per_s"])
        res[name]["windows_per_s"] = stats(res[name]["windows_per_s"])
    out.update(res)
    out["packed_over_per_clip_median"] = round(res["packed"]["clips_per_s"]["median"] / res["per_clip"]["clips_per_s"]["median"], 3)
    out["ahead_by_more_than_the_spread"] = bool(res["packed"]["clips_per_s"]["min"] > res["per_clip"]["clips_per_s"]["max"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
