#!/usr/bin/env python
"""Dataset preprocessing throughput on one MI355X: synthetic 160x160 clips (the LRS2 frame size) written as AVIs, seeded S3FD
weights, then in ONE process
  1. end to end: frames/s of `preprocess.main` (AVI decode, detection in batches, host JPEG pool, audio.wav), best of --repeats
  2. detection only, on the same frames resident on the device, alternating per sample:
       per_image  the previous rect path - detect_from_batch (one index_select + copy back per image) + the host rule
       batched    FaceAlignment.get_detections_for_batch (w2l_s3fd_first_rect: one launch, one [B][5] copy back)
     frames/s per sample, the median of each and whether both paths gave the same rects.
Prints one JSON line.
    python tools/preprocess_bench.py [--clips 8] [--frames 75] [--batch_size 32] [--samples 5] [--face_det_precision fp32|bf16]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def per_image_rects(fa, images):
    """the rect path before w2l_s3fd_first_rect (api.py:61-77 over detect_from_batch)"""
    out = []
    for dets in fa.detect_from_batch(images):
        out.append(None if len(dets) == 0 else tuple(int(v) for v in np.maximum(np.asarray(dets[0][:4]), 0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=75, help="frames per clip (LRS2 clips are a few seconds at 25 fps)")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--face_det_precision", default="fp32", choices=["fp32", "bf16"])
    a = ap.parse_args()
    from wav2lip_amd import container, face_detection, preprocess
    from wav2lip_amd import synthetic as synth
    from wav2lip_amd.inference import CLI_PRECISION
    os.environ.pop("WORLD_SIZE", None)
    sd = synth.s3fd_state_dict()
    clips = [synth.preprocess_frames(a.frames, 1000 + i) for i in range(a.clips)]
    n_frames = a.clips * a.frames
    res = {"clips": a.clips, "frames_per_clip": a.frames, "batch_size": a.batch_size, "precision": a.face_det_precision}
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "data")
        for i, fr in enumerate(clips):
            os.makedirs(os.path.join(data, "spk%d" % (i % 2)), exist_ok=True)
            pcm = np.zeros((a.frames * 16000 // 25, 1), np.int16)
            container.write_avi(os.path.join(data, "spk%d" % (i % 2), "%05d.avi" % i), fr, 25, audio=pcm, audio_sr=16000)
        rates = []
        for r in range(a.repeats + 1):                   # the first run builds the detector graph and is not counted
            args = preprocess.parser.parse_args(["--data_root", data, "--preprocessed_root", os.path.join(tmp, "out%d" % r),
                                                 "--batch_size", str(a.batch_size), "--face_det_precision", a.face_det_precision])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            preprocess.main(args, state_dict=sd if r == 0 else None)
            torch.cuda.synchronize()
            if r:
                rates.append(n_frames / (time.perf_counter() - t0))
        res["main_frames_per_s"] = [round(x, 1) for x in rates]
        res["main_frames_per_s_best"] = round(max(rates), 1)

    fa = face_detection.FaceAlignment(face_detection.LandmarksType._2D, device="cuda", state_dict=sd,
                                      precision=CLI_PRECISION[a.face_det_precision])
    frames = np.concatenate(clips)
    nb = len(frames) // a.batch_size
    dev = torch.from_numpy(frames[:nb * a.batch_size]).cuda().view(nb, a.batch_size, *frames.shape[1:])
    paths = {"per_image": lambda x: per_image_rects(fa, x), "batched": fa.get_detections_for_batch}
    for f in paths.values():
        f(dev[0])                                         # graph build / warm-up
    samples = {k: [] for k in paths}
    outs = {}
    for s in range(a.samples):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[k] = [r for b in range(nb) for r in f(dev[b])]
            torch.cuda.synchronize()
            samples[k].append(nb * a.batch_size / (time.perf_counter() - t0))
    for k in paths:
        res["detect_%s_frames_per_s" % k] = [round(x, 1) for x in samples[k]]
        res["detect_%s_median" % k] = round(float(np.median(samples[k])), 1)
    res["detect_speedup"] = round(res["detect_batched_median"] / res["detect_per_image_median"], 3)
    res["same_rects"] = outs["per_image"] == outs["batched"]
    res["frames_with_face"] = sum(r is not None for r in outs["batched"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
