#!/usr/bin/env python
"""S3FD face-detection throughput on one MI355X: batches of uint8 frames resident in HBM ->
dense decoded boxes on device -> candidate gate + greedy NMS on device (w2l_s3fd_nms), survivors to the host.
    python tools/s3fd_bench.py [--batch 16] [--height 480] [--width 640] [--steps 5] [--precision fp32|bf16] [--alternate N]

--precision selects the detector graph (fp32 default: the output line is the one it always was).  --alternate N times N samples
of each precision, fp32 and bf16 alternately in one process (each sample: --steps batches of the network + decode between two
events), and prints one JSON line: the ms per batch of every sample, median / min / max per precision, the ratio of the medians,
the layer -> kernel-family list of the bf16 graph and whether the rects of the last timed batch agree between the precisions."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--alternate", type=int, default=0, metavar="N")
    args = ap.parse_args()
    if args.alternate:
        return alternate(args)
    from wav2lip_amd.synthetic import s3fd_state_dict as seeded_state_dict
    from wav2lip_amd import face_detection as fd
    fa = fd.FaceAlignment(fd.LandmarksType._2D, device="cuda", state_dict=seeded_state_dict())
    net = fa.face_detector
    B, H, W = args.batch, args.height, args.width
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    prec = {"fp32": "f32", "bf16": "bf16"}[args.precision]
    fa.precision = prec
    ms = _time(net, img, args.steps, prec)
    g = net._graph(B, H, W, img.device, prec)
    macs = _macs(g, B)
    t0 = time.perf_counter()
    fa.get_detections_for_batch(img)
    host_ms = (time.perf_counter() - t0) * 1e3 - ms
    print(json.dumps({"what": "S3FD detector, %s, network + decode on device" % args.precision, "batch": B, "frame": [H, W],
                      "ms_per_batch": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1),
                      "gflop_per_frame": round(2 * macs / B / 1e9, 1), "tflops": round(2 * macs / ms / 1e9, 1),
                      "gate_nms_ms_per_batch": round(host_ms, 1), "gate_nms": "device (w2l_s3fd_nms) + the copy of the survivors; round 4: host numpy, 3 570 ms"}))



def _time(net, img, steps, prec):
    """ms per batch of the network + decode (the first call builds the graph; fp32 plans autotune there)"""
    net.dense_boxes(img, precision=prec)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        net.dense_boxes(img, precision=prec)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _macs(g, B):
    if hasattr(g, "plans"):          # bf16 graph: the convb plans (executed FLOPs / 2) and the heads' 3x3 contractions
        macs = sum(fl for p in g.plans for _, fl, _, _ in p.resolved()) // 2
        return macs + sum(op[2].N * op[2].H * op[2].W * op[2].C * 9 * (op[1].ncls + 4) for op in g.ops if op[0] == "head")
    return sum(op[1].macs() for op in g.ops if op[0] == "convs")


def alternate(args):
    from wav2lip_amd.synthetic import s3fd_state_dict as seeded_state_dict
    from wav2lip_amd import face_detection as fd
    # one detector per precision (same weights): each keeps its own live graph, so no sample rebuilds one
    fas = {name: fd.FaceAlignment(fd.LandmarksType._2D, device="cuda", state_dict=seeded_state_dict(), precision=prec)
           for name, prec in (("fp32", "f32"), ("bf16", "bf16"))}
    B, H, W = args.batch, args.height, args.width
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    for fa in fas.values():
        fa.face_detector.dense_boxes(img, precision=fa.precision)       # build (fp32: autotune) before anything is timed
    samples = {name: [] for name in fas}
    for _ in range(args.alternate):
        for name, fa in fas.items():
            samples[name].append(_time(fa.face_detector, img, args.steps, fa.precision))
    rects = {name: fa.get_detections_for_batch(img) for name, fa in fas.items()}
    families = fas["bf16"].face_detector._graph(B, H, W, img.device, "bf16").resolved()
    out = {"what": "S3FD detector, fp32 vs bf16 alternated, network + decode on device", "batch": B, "frame": [H, W],
           "steps_per_sample": args.steps, "device": torch.cuda.get_device_name(0)}
    for name, v in samples.items():
        out[name] = {"ms_per_batch": [round(x, 3) for x in v], "median": round(float(np.median(v)), 3),
                     "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}
    out["speedup_median"] = round(out["fp32"]["median"] / out["bf16"]["median"], 3)
    out["bf16_kernel_families"] = families
    out["rects_agree"] = rects["fp32"] == rects["bf16"]
    out["rects"] = {k: [list(r) if r is not None else None for r in v] for k, v in rects.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
