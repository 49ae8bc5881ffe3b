#!/usr/bin/env python
"""Dataset preprocessing throughput on one MI355X: synthetic 160x160 clips (the LRS2 frame size) written as AVIs, seeded S3FD
weights, then in ONE process
  1. end to end: frames/s of `preprocess.main` (AVI decode, detection in batches, host JPEG pool, audio.wav), best of --repeats
  2. detection only, on the same frames resident on the device, alternating per sample:
       per_image  the previous rect path - detect_from_batch (one index_select + copy back per image) + the host rule
       batched    FaceAlignment.get_detections_for_batch (w2l_s3fd_first_rect: one launch, one [B][5] copy back)
     frames/s per sample, the median of each and whether both paths gave the same rects.
With `--jpeg device` step 1 runs `preprocess.main --jpeg device` (the crops encoded by w2l_jpeg_encode_rows).  With `--jpeg both`
step 1 alternates the two end to end in this one process, host then device, --alternations times each (at least five) after a
warm-up pass of each, and reports median and range of both and whether they wrote the same files; and
  3. the encoder alone, on the detected crops of the same frames, alternating per sample: crops/s of `jpeg.encode_crops` (frames
     resident on the device, the files' bytes back on the host) against the 4-thread PIL pool of the host path (crops in host
     memory, bytes out), median and range of each.
Prints one JSON line.
    python tools/preprocess_bench.py [--clips 8] [--frames 75] [--batch_size 32] [--samples 5] [--face_det_precision fp32|bf16]
                                     [--jpeg host|device|both] [--alternations 5]"""
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


def encoder_alone(frames, dev, rects, batch_size, samples):
    """crops/s of jpeg.encode_crops per detector batch against the host path's 4-thread PIL pool on the same crops"""
    import io
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from wav2lip_amd import jpeg, preprocess
    H, W = frames.shape[1:3]
    batches = []                                          # per detector batch: (boxes, rows), the rects cut at the frame as numpy cuts
    for b in range(dev.shape[0]):
        boxes, rows = [], []
        for j, r in enumerate(rects[b * batch_size:(b + 1) * batch_size]):
            if r is not None and min(r[2], W) > r[0] and min(r[3], H) > r[1]:
                boxes.append((r[0], r[1], min(r[2], W), min(r[3], H)))
                rows.append(j)
        if boxes:
            batches.append((b, boxes, rows))
    n = sum(len(boxes) for _, boxes, _ in batches)

    def pil(crop):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(crop[:, :, ::-1])).save(buf, format="JPEG", quality=preprocess.JPEG_QUALITY,
                                                                      subsampling=preprocess.JPEG_SUBSAMPLING)
        return buf.getvalue()
    pool = ThreadPoolExecutor(preprocess.JPEG_WORKERS)

    def host():
        return [list(pool.map(pil, [frames[b * batch_size + j][y1:y2, x1:x2] for (x1, y1, x2, y2), j in zip(boxes, rows)]))
                for b, boxes, rows in batches]

    def device():
        return [jpeg.encode_crops(dev[b], boxes, preprocess.JPEG_QUALITY, frame_index=rows) for b, boxes, rows in batches]
    paths = {"host_pool": host, "device": device}
    outs = {k: f() for k, f in paths.items()}             # warm-up, and the bytes to compare
    rates = {k: [] for k in paths}
    for s in range(max(5, samples)):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            rates[k].append(n / (time.perf_counter() - t0))
    pool.shutdown()
    res = {"encoder_crops": n, "encoder_same_bytes": outs["host_pool"] == outs["device"]}
    for k in paths:
        res["encoder_%s_crops_per_s_median" % k] = round(float(np.median(rates[k])), 1)
        res["encoder_%s_crops_per_s_range" % k] = [round(min(rates[k]), 1), round(max(rates[k]), 1)]
    res["encoder_device_over_host"] = round(res["encoder_device_crops_per_s_median"] / res["encoder_host_pool_crops_per_s_median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=75, help="frames per clip (LRS2 clips are a few seconds at 25 fps)")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--face_det_precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--jpeg", default="host", choices=["host", "device", "both"])
    ap.add_argument("--alternations", type=int, default=5, help="--jpeg both: timed end-to-end runs of each path (at least 5)")
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
        state = {"first": True}

        def run_main(mode, out):
            """frames/s of one `preprocess.main --jpeg <mode>` into `out`"""
            args = preprocess.main_parser.parse_args(["--data_root", data, "--preprocessed_root", out, "--batch_size", str(a.batch_size),
                                                      "--face_det_precision", a.face_det_precision, "--jpeg", mode])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            preprocess.main(args, state_dict=sd if state["first"] else None)
            torch.cuda.synchronize()
            state["first"] = False
            return n_frames / (time.perf_counter() - t0)

        if a.jpeg != "both":
            rates = []
            for r in range(a.repeats + 1):               # the first run builds the detector graph and is not counted
                rate = run_main(a.jpeg, os.path.join(tmp, "out%d" % r))
                if r:
                    rates.append(rate)
            res["jpeg"] = a.jpeg
            res["main_frames_per_s"] = [round(x, 1) for x in rates]
            res["main_frames_per_s_best"] = round(max(rates), 1)
        else:
            modes = ("host", "device")
            for m in modes:                              # warm-up: the detector graph, the pool, the allocator
                run_main(m, os.path.join(tmp, "warm_" + m))
            rates = {m: [] for m in modes}
            for r in range(max(5, a.alternations)):
                for m in modes:
                    rates[m].append(run_main(m, os.path.join(tmp, "%s%d" % (m, r))))
            res["jpeg"] = "both"
            for m in modes:
                res["main_%s_frames_per_s" % m] = [round(x, 1) for x in rates[m]]
                res["main_%s_median" % m] = round(float(np.median(rates[m])), 1)
                res["main_%s_range" % m] = [round(min(rates[m]), 1), round(max(rates[m]), 1)]
            res["main_device_over_host"] = round(res["main_device_median"] / res["main_host_median"], 3)

            def tree(root):
                return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read()
                        for d, _, fs in os.walk(root) for f in fs}
            res["same_files"] = tree(os.path.join(tmp, "host0")) == tree(os.path.join(tmp, "device0"))

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
    if a.jpeg == "both":
        res.update(encoder_alone(frames[:nb * a.batch_size], dev, outs["batched"], a.batch_size, a.samples))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
