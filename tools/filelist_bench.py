"""Packed filelist generation against the per-clip loop, alternated in one process: frames/s of `multiclip.lipsync_many` and of
`for clip: inference.lipsync(model, frames, wav, box=...)` over the same seeded clips.

    python tools/filelist_bench.py [--clips 200] [--alternations 5] [--batch 128] [--seed 0] [--blend_feather N] [--blend_top FRACTION]
                                     [--color_match {mean,full}]

The clips are 160x160 with a fixed 110x110 face box (no detection: only the generator path is timed) and lengths uniform in
30..120 mel chunks.  Both loops start from the 16 kHz samples (the mel spectrogram is part of both) and end with every output
frame on the host.  Each loop owns a model, so that the number of cached plans and what they hold is its own.  Pass 0 of each
loop is its warm-up and is reported separately: for the per-clip loop it builds one plan per distinct clip length, which is part
of what that loop costs on a filelist it has not seen.  Then the two loops alternate, --alternations pairs, in steady state
(every plan built).  Prints one JSON line: per loop the frames/s of every pass, median, min and max (the spread), the first-pass
seconds, the number of cached plans, and torch.cuda.max_memory_allocated after the loop's first pass (the device is reset to
the other loop's state in between only as far as the caching allocator allows: the figure is the peak since process start for
the packed loop, which runs first, and the peak over everything for the per-clip loop).  `--blend_feather` / `--blend_top` are
passed to both loops (the feathered mouth-region paste) and recorded in the result, and so is `--color_match`
(colour matching of the prediction).  For an A/B of an option call `main(argv)` with and without it, alternating,
in one process (profiles/blend/, profiles/color_match/)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wav2lip_amd import audio, inference, models, multiclip  # noqa: E402
from wav2lip_amd import synthetic as synth  # noqa: E402

BOX = (30, 140, 25, 135)


def make_clips(n, seed):
    r = np.random.default_rng(seed)
    pool = r.integers(0, 256, (16, 160, 160, 3), dtype=np.uint8)
    clips = []
    for i in range(n):
        chunks = int(r.integers(30, 121))
        wav = synth.noise_wav(synth.filelist_samples(chunks), seed=seed * 100003 + i)
        clips.append(([pool[(i + k) % 16] for k in range(chunks)], wav))
    return clips


def model(dev):
    G = models.Wav2Lip()
    G.load_state_dict(synth.synthetic_state_dict({k: tuple(v.shape) for k, v in G.state_dict().items()}, seed=0))
    return G.to(dev).eval()


def run_packed(G, clips, batch, dev, blend=None, color_match=None):
    def jobs():
        for i, (frames, wav) in enumerate(clips):
            mel = audio.melspectrogram_device(wav, dev)
            yield multiclip.ClipJob(i, frames, mel, multiclip.rows_inference(mel.shape[1], len(frames), [BOX] * len(frames)))
    n = [0]

    def sink(key, frame):
        n[0] += frame is not None
    t0 = time.perf_counter()
    multiclip.lipsync_many(G, jobs(), batch_size=batch, sink=sink, **inference._blend_kw(blend), **inference._color_kw(color_match))
    torch.cuda.synchronize()
    return n[0], time.perf_counter() - t0


def run_loop(G, clips, batch, dev, blend=None, color_match=None):
    n = 0
    t0 = time.perf_counter()
    for frames, wav in clips:
        n += len(inference.lipsync(G, frames, wav, batch_size=batch, box=BOX, **inference._blend_kw(blend),
                                      **inference._color_kw(color_match)))
    torch.cuda.synchronize()
    return n, time.perf_counter() - t0


def stats(v):
    return {"samples": [round(x, 1) for x in v], "median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    inference.add_blend_flags(ap)
    inference.add_color_match_flag(ap)
    a = ap.parse_args(argv)
    blend = inference.blend_from_args(a)
    color_match = inference.color_match_from_args(a)
    dev = torch.device("cuda", 0)
    clips = make_clips(a.clips, a.seed)
    out = {"clips": a.clips, "batch": a.batch, "alternations": a.alternations,
           "distinct_lengths": len({len(f) for f, _ in clips}), "blend": blend, "color_match": color_match}
    loops = {"packed": (run_packed, model(dev)), "per_clip": (run_loop, model(dev))}
    res = {k: {"fps": []} for k in loops}
    for name, (fn, G) in loops.items():                   # pass 0: warm-up, plans built
        n, t = fn(G, clips, a.batch, dev, blend, color_match)
        res[name].update(frames=n, first_pass_s=round(t, 2), first_pass_fps=round(n / t, 1), plans=len(G._graphs),
                         max_memory_allocated_gb=round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2))
    for _ in range(a.alternations):
        for name, (fn, G) in loops.items():
            n, t = fn(G, clips, a.batch, dev, blend, color_match)
            res[name]["fps"].append(n / t)
    for name in loops:
        res[name]["fps"] = stats(res[name]["fps"])
        res[name]["plans"] = len(loops[name][1]._graphs)
    out.update(res)
    out["packed_over_per_clip_median"] = round(res["packed"]["fps"]["median"] / res["per_clip"]["fps"]["median"], 3)
    out["ahead_by_more_than_the_spread"] = bool(res["packed"]["fps"]["min"] > res["per_clip"]["fps"]["max"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
