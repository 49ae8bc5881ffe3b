#!/usr/bin/env python
"""S3FD face-detection throughput on one MI355X: batches of uint8 frames resident in HBM ->
dense decoded boxes on device -> candidate gate + greedy NMS on device (w2l_s3fd_nms), survivors to the host.
    python tools/s3fd_bench.py [--batch 16] [--height 480] [--width 640] [--steps 5] [--precision fp32|bf16] [--alternate N]
                               [--det_scale K] [--pack_only]

--precision selects the detector graph (fp32 default: the output line is the one it always was).  --alternate N times N samples
of each precision, fp32 and bf16 alternately in one process (each sample: --steps batches of the network + decode between two
events), and prints one JSON line: the ms per batch of every sample, median / min / max per precision, the ratio of the medians,
the layer -> kernel-family list of the bf16 graph and whether the rects of the last timed batch agree between the precisions.

--det_scale K (default 1: every output line is the one it was) runs the detector on the frames at 1/K size (`--face_det_scale`).
With --alternate the alternation then covers four detectors in one process - fp32 and bf16 at scale 1 (the baseline: the code
path without the option) and at scale K - and the line carries the ratio of the medians, scale 1 over scale K, per precision.
--pack_only alternates the fused reduced-resolution pack (`w2l_s3fd_pack_rows_scaled[_bf16]`) against the two launches it
replaces (`w2l_resize_rows_u8` into a scratch batch, then `w2l_s3fd_pack_rows[_bf16]`) at --det_scale K, no network."""
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
    ap.add_argument("--det_scale", type=int, default=1, metavar="K")
    ap.add_argument("--pack_only", action="store_true")
    args = ap.parse_args()
    if args.pack_only:
        return pack_only(args)
    if args.alternate:
        return alternate_scales(args) if args.det_scale > 1 else alternate(args)
    from wav2lip_amd.synthetic import s3fd_state_dict as seeded_state_dict
    from wav2lip_amd import face_detection as fd
    k = args.det_scale
    fa = fd.FaceAlignment(fd.LandmarksType._2D, device="cuda", state_dict=seeded_state_dict(), **({} if k == 1 else {"det_scale": k}))
    net = fa.face_detector
    B, H, W = args.batch, args.height, args.width
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    prec = {"fp32": "f32", "bf16": "bf16"}[args.precision]
    fa.precision = prec
    ms = _time(net, img, args.steps, prec, k)
    g = net._graph(B, H // k, W // k, img.device, prec)
    macs = _macs(g, B)
    t0 = time.perf_counter()
    fa.get_detections_for_batch(img)
    host_ms = (time.perf_counter() - t0) * 1e3 - ms
    print(json.dumps({"what": "S3FD detector, %s, network + decode on device" % args.precision, "batch": B, "frame": [H, W],
                      **({} if k == 1 else {"det_scale": k, "detector_frame": [H // k, W // k]}),
                      "ms_per_batch": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1),
                      "gflop_per_frame": round(2 * macs / B / 1e9, 1), "tflops": round(2 * macs / ms / 1e9, 1),
                      "gate_nms_ms_per_batch": round(host_ms, 1), "gate_nms": "device (w2l_s3fd_nms) + the copy of the survivors; round 4: host numpy, 3 570 ms"}))



def _time(net, img, steps, prec, det_scale=1):
    """ms per batch of the network + decode (the first call builds the graph; fp32 plans autotune there)"""
    kw = {} if det_scale == 1 else {"det_scale": det_scale}
    net.dense_boxes(img, precision=prec, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        net.dense_boxes(img, precision=prec, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _macs(g, B):
    if g.precision == "bf16":        # bf16 graph: the convb plans (executed FLOPs / 2) and the heads' 3x3 contractions
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


def _stats(v):
    return {"ms_per_batch": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
            "max": round(float(np.max(v)), 4)}


def alternate_scales(args):
    """fp32 and bf16 at det_scale 1 and K, alternated in one process; each detector keeps its own live graph"""
    from wav2lip_amd.synthetic import s3fd_state_dict as seeded_state_dict
    from wav2lip_amd import face_detection as fd
    K = args.det_scale
    fas = {}
    for k in (1, K):
        for name, prec in (("fp32", "f32"), ("bf16", "bf16")):
            fas["%s@%d" % (name, k)] = fd.FaceAlignment(fd.LandmarksType._2D, device="cuda", state_dict=seeded_state_dict(),
                                                        precision=prec, **({} if k == 1 else {"det_scale": k}))
    B, H, W = args.batch, args.height, args.width
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).cuda()
    for fa in fas.values():
        _time(fa.face_detector, img, 1, fa.precision, fa.det_scale)      # build (fp32: autotune) and warm before anything is timed
    samples = {name: [] for name in fas}
    for _ in range(args.alternate):
        for name, fa in fas.items():
            samples[name].append(_time(fa.face_detector, img, args.steps, fa.precision, fa.det_scale))
    out = {"what": "S3FD detector at det_scale 1 vs %d, fp32 and bf16 alternated, pack + network + decode on device" % K, "batch": B,
           "frame": [H, W], "detector_frame": [H // K, W // K], "det_scale": K, "steps_per_sample": args.steps,
           "device": torch.cuda.get_device_name(0)}
    for name, v in samples.items():
        out[name] = _stats(v)
    for name in ("fp32", "bf16"):
        out["speedup_median_%s" % name] = round(out[name + "@1"]["median"] / out["%s@%d" % (name, K)]["median"], 3)
    rects = {name: fa.get_detections_for_batch(img) for name, fa in fas.items()}
    out["rects"] = {k: [list(r) if r is not None else None for r in v] for k, v in rects.items()}
    print(json.dumps(out))


def pack_only(args):
    """the fused reduced-resolution pack against resize_rows + pack_rows, alternated; both precisions' output formats"""
    from wav2lip_amd import _lib, real_videos_inference as rv
    from wav2lip_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    K, B, H, W = max(2, args.det_scale), args.batch, args.height, args.width
    Hd, Wd = H // K, W // K
    dev = torch.device("cuda")
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    small = torch.empty((B, Hd, Wd, 3), dtype=torch.uint8, device=dev)
    frames = torch.arange(B, dtype=torch.int64, device=dev) * (H * W * 3) + img.data_ptr()
    smalls = torch.arange(B, dtype=torch.int64, device=dev) * (Hd * Wd * 3) + small.data_ptr()
    rows = np.zeros(B, rv.RESIZE_ROW)
    rows["src"] = frames.cpu().numpy().astype(np.uint64)
    rows["dst"] = smalls.cpu().numpy().astype(np.uint64)
    rows["Hs"], rows["Ws"], rows["Hd"], rows["Wd"] = H, W, Hd, Wd
    rows_dev = torch.from_numpy(rows.view(np.uint8)).to(dev)
    ys = {"fp32": torch.empty((B, Hd, Wd, 4), dtype=torch.float32, device=dev),
          "bf16": torch.empty((B, Hd, Wd, 8), dtype=torch.bfloat16, device=dev)}
    y2 = {k: torch.empty_like(v) for k, v in ys.items()}
    s = current_stream()

    def fused(name):
        if name == "fp32":
            check(lib.w2l_s3fd_pack_rows_scaled(s, B, H, W, Hd, Wd, ptr(frames), ptr(ys[name]), 4), "pack_rows_scaled")
        else:
            check(lib.w2l_s3fd_pack_rows_scaled_bf16(s, B, H, W, Hd, Wd, ptr(frames), ptr(ys[name]), 8), "pack_rows_scaled_bf16")

    def composed(name):
        check(lib.w2l_resize_rows_u8(s, B, ptr(rows_dev), Hd * Wd), "resize_rows")
        if name == "fp32":
            check(lib.w2l_s3fd_pack_rows(s, B, Hd, Wd, ptr(smalls), ptr(y2[name]), 4), "pack_rows")
        else:
            check(lib.w2l_s3fd_pack_rows_bf16(s, B, Hd, Wd, ptr(smalls), ptr(y2[name]), 8), "pack_rows_bf16")

    def timed(fn, name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn(name)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    variants = [(kind, name, fn) for name in ("fp32", "bf16") for kind, fn in (("fused", fused), ("composed", composed))]
    for _, name, fn in variants:
        fn(name)
    torch.cuda.synchronize()
    samples = {"%s_%s" % (kind, name): [] for kind, name, _ in variants}
    for _ in range(max(1, args.alternate)):
        for kind, name, fn in variants:
            samples["%s_%s" % (kind, name)].append(timed(fn, name))
    out = {"what": "reduced-resolution pack: one fused launch vs resize_rows + pack_rows, alternated", "batch": B, "frame": [H, W],
           "detector_frame": [Hd, Wd], "steps_per_sample": args.steps, "device": torch.cuda.get_device_name(0),
           "bytes_read_at_most": B * H * W * 3, "bytes_written": B * Hd * Wd * 16,
           "composed_extra_bytes": 2 * B * Hd * Wd * 3}
    for k, v in samples.items():
        out[k] = _stats(v)
    for name in ("fp32", "bf16"):
        out["equal_%s" % name] = bool(torch.equal(ys[name].view(torch.int16), y2[name].view(torch.int16)))
        out["composed_over_fused_%s" % name] = round(out["composed_" + name]["median"] / out["fused_" + name]["median"], 3)
        ms = out["fused_" + name]["median"]
        out["fused_%s_gb_per_s" % name] = round((out["bytes_read_at_most"] + out["bytes_written"]) / ms / 1e6, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
