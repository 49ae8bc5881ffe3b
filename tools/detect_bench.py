"""Packed face detection against the per-clip loop, alternated in one process: frames/s of `face_detection.detect_many` and of
`for clip: inference.face_detect(frames, detector, ...)` over the same seeded clips.

    python tools/detect_bench.py [--clips 200] [--alternations 5] [--batch 16] [--precision f32] [--seed 0] [--face_track PICK]
                                 [--scene_cuts THRESH] [--all_faces F] [--det_stride N]

The clips are those of tools/filelist_bench.py (160x160 frames, lengths uniform in 30..120, 16 distinct frames cycled), each frame
with the saturated block of synthetic.filelist_frame pasted in so that the seeded S3FD (synthetic.s3fd_state_dict) finds a face;
frames start on the host in both loops, as the commands have them, and both end with every clip's boxes on the host.  Pads
(0, 0, 0, 0), smoothing T = 5: the filelist command's settings.  The per-clip loop is the code path of the commands without
`--packed_face_det`.  Each loop owns a detector, so the graphs it builds are its own.  Pass 0 of each loop is its warm-up and is
reported separately; then the two loops alternate, --alternations pairs.  Prints one JSON line: per loop the frames/s of every pass
with median, min and max, the first-pass seconds, detector graph builds per pass, torch.cuda.max_memory_allocated after the loop's
first pass (the peak since process start for the packed loop, which runs first, and the peak over everything for the per-clip
loop), and how many boxes and clips differ between the two paths.

With `--face_track PICK` (tracked face selection) the two loops are the packed detector without and with
`face_track=PICK` (defaults K = 8, L = 0, min_iou = 0.25) - "packed" and "packed_tracked" - alternated the same way: what the two
small launches per batch in place of one, and the track launch per group, cost.  The seeded clips hold one saturated block each;
how often the seeded detector sees more than one candidate there is reported by `boxes_that_differ`, and says nothing about
selection quality on real footage.

With `--scene_cuts THRESH` (scene-cut detection) the two loops are the packed detector without and with
`scene_cuts=THRESH` - "packed" and "packed_scene" - alternated the same way: what the signature launch over every frame, the cut
launch and the small copy per group cost.  The seeded clips cycle 16 noise frames whose histograms are alike, so at 0.3 no cut
fires on them and `boxes_that_differ` must be 0 (a clip without a cut is the feature switched off); the per-shot tables are built
all the same.  Nothing here says anything about detection quality on real footage.  `--face_track PICK` may be given with it: the
second loop then runs with `scene_cuts=THRESH, face_track=PICK` - every shot tracked alone - against the same plain first loop.

With `--all_faces F` (every face of a shot) the two loops are the packed detector with `track_spans` alone
(bridge 25, min_len 1) and with `all_faces=AllFaces(F)` as well - "packed_spans" and "packed_all_faces" - alternated the same way:
what the candidate launch per batch in place of the rect launch, the walk over F slots and the span and run launches over F
times the rows cost.  `boxes_that_differ` compares the first path's boxes with the boxes of the second path's slot-0 tracks on the
frames both have.  `--track_kernel_ms` instead times the new launch alone over HIP events: one segment of 4096 frames with four
faces that drift, F = 4, K = 8 - the serial walk's worst case - alternated with w2l_face_track_segments over the same arenas.

With `--det_stride N` (key-frame detection) the two loops are the packed detector without and with `det_stride=N` -
"packed" and "packed_stride" - alternated the same way: the detector sees about 1/N of the frames, and the frames between the keys
of a clip are not uploaded; the expand launch per group, the uploads that remain and the finish do not shrink.  The seeded clips
cycle 16 frames whose blocks lie at unrelated places, so the interpolated boxes differ from the per-frame ones on most frames
between keys: `boxes_that_differ` counts them and says nothing about the accuracy cost on real footage, where a face hardly moves
between neighbouring frames.  `--expand_kernel_ms` instead times the new launch alone over HIP events: 64 segments of 4096 frames
at stride N (2 without --det_stride)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filelist_bench import make_clips  # noqa: E402
from wav2lip_amd import face_detection, inference  # noqa: E402
from wav2lip_amd import synthetic as synth  # noqa: E402

PADS = (0, 0, 0, 0)
BUILDS = [0]
_mod = sys.modules["wav2lip_amd.face_detection.s3fd"]        # `face_detection.s3fd` is the class; this is its module
_real_graph = _mod._Graph


def _counting_graph(*a, **k):
    BUILDS[0] += 1
    return _real_graph(*a, **k)


def clips_with_faces(n, seed):
    """[frames] of filelist_bench.make_clips with a seeded saturated block in each of the 16 distinct frames"""
    clips = make_clips(n, seed)
    pool = []
    for j, f in enumerate(clips[0][0][:16]):                 # clip 0 starts with the pool in order
        g = f.copy()
        r = np.random.default_rng([seed, j, 9])
        h, w = r.integers(40, 80, 2)
        y, x = r.integers(0, 160 - h), r.integers(0, 160 - w)
        g[y:y + h, x:x + w] = 255 if j % 2 else 0
        pool.append(g)
    return [[pool[(i + k) % 16] for k in range(len(frames))] for i, (frames, _) in enumerate(clips)]


def detector(dev, precision):
    return face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device=str(dev),
                                        state_dict=synth.s3fd_state_dict(), precision=precision)


def run_packed(det, clips, batch, **kw):
    t0 = time.perf_counter()
    res = [b for _, b, _ in face_detection.detect_many(det, (face_detection.DetectJob(i, f) for i, f in enumerate(clips)), pads=PADS,
                                                       T=5, batch_size=batch, **kw)]
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def run_loop(det, clips, batch):
    t0 = time.perf_counter()
    res = []
    for frames in clips:
        try:
            res.append(np.array([c for _, c in inference.face_detect(frames, detector=det, pads=list(PADS), nosmooth=False, batch_size=batch)]))
        except ValueError:                                  # a frame without a face
            res.append(None)
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0


def span_boxes(result):
    """(boxes per clip, seconds) of a `track_spans` pass: the box arrays, zeros outside kept spans"""
    res, t = result
    return [r.boxes for r in res], t


def slot0(result):
    """(boxes per clip, seconds) of an `all_faces` pass in the shape of a `track_spans` pass: the boxes of the slot-0 tracks"""
    res, t = result
    out = []
    for r in res:
        boxes = np.zeros((len(r), 4), np.int64)
        for tr in r.tracks:
            if tr.slot == 0:
                boxes[tr.a:tr.b] = tr.boxes
        out.append(boxes)
    return out, t


def track_kernel_ms(dev, alternations, n=4096, F=4, K=8, L=25, q=64):
    """milliseconds of w2l_face_tracks_all_segments and of w2l_face_track_segments over one segment of n frames with four drifting
    faces whose order changes from frame to frame, each launch between two HIP events, the two alternated"""
    from wav2lip_amd._lib import BOX_SEGMENT, TRACK_SEGMENT, check, current_stream, load, ptr
    rng = np.random.default_rng(0)
    cands = np.zeros((n, K, 4), np.int32)
    base = np.array([(40 + 200 * j, 50, 140 + 200 * j, 170) for j in range(4)], np.int32)
    for i in range(n):
        d = (i % 7) - 3
        cands[i, :4] = (base + np.array([d, 0, d, 0], np.int32))[rng.permutation(4)]
    c = torch.from_numpy(cands).to(dev)
    nc, cf = torch.full((n,), 4, dtype=torch.int32, device=dev), torch.ones((n,), dtype=torch.int32, device=dev)
    seg = np.zeros(1, BOX_SEGMENT)
    seg[0] = (0, n, 0, 0)
    trk = np.zeros(1, TRACK_SEGMENT)
    trk[0] = (0, n, -1, 0)
    seg, trk = (torch.from_numpy(t.view(np.uint8)).to(dev) for t in (seg, trk))
    rects, flags = torch.empty((F, n, 4), dtype=torch.int32, device=dev), torch.empty((F, n), dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    lib = load()

    def all_faces():
        check(lib.w2l_face_tracks_all_segments(current_stream(), 1, ptr(seg), ptr(c), ptr(nc), ptr(cf), n, K, F, L, q, ptr(rects), ptr(flags),
                                               ptr(status)), "face_tracks_all_segments")

    def one_face():
        check(lib.w2l_face_track_segments(current_stream(), 1, ptr(trk), ptr(c), ptr(nc), ptr(cf), n, K, 0, L, q, None, 0, ptr(rects),
                                          ptr(flags), ptr(status)), "face_track_segments")

    arms = {"all_faces_ms": all_faces, "one_face_ms": one_face}
    ms = {k: [] for k in arms}
    for rep in range(alternations + 1):                     # pass 0: warm-up
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep:
                ms[name].append(e0.elapsed_time(e1))
    all_faces()
    st = status.cpu().tolist()
    out = {"frames": n, "F": F, "K": K, "L": L, "q": q, "status": st, "alternations": alternations}
    for name, v in ms.items():
        out[name] = {"samples": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4), "min": round(min(v), 4),
                     "max": round(max(v), 4)}
    out["us_per_frame_all_faces"] = round(1000 * out["all_faces_ms"]["median"] / n, 3)
    print(json.dumps(out))


def expand_kernel_ms(dev, alternations, N, n=4096, n_seg=64):
    """milliseconds of w2l_face_rects_expand_segments over n_seg segments of n frames each at stride N, every key found, each launch
    between two HIP events"""
    from wav2lip_amd._lib import STRIDE_SEGMENT
    from wav2lip_amd.face_detection.stride import expand_rects, key_frames
    m = len(key_frames(n, N))
    rng = np.random.default_rng(0)
    key_rects = torch.from_numpy(rng.integers(0, 32768, (n_seg * m, 4)).astype(np.int32)).to(dev)
    key_flags = torch.ones((n_seg * m,), dtype=torch.int32, device=dev)
    seg = np.zeros(n_seg, STRIDE_SEGMENT)
    for k in range(n_seg):
        seg[k] = (k * m, k * n, n, 0)
    seg = torch.from_numpy(seg.view(np.uint8)).to(dev)
    rects, flags = torch.empty((n_seg * n, 4), dtype=torch.int32, device=dev), torch.empty((n_seg * n,), dtype=torch.int32, device=dev)
    status = torch.empty(n_seg, dtype=torch.int32, device=dev)
    ms = []
    for rep in range(alternations + 1):                     # pass 0: warm-up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        expand_rects(n_seg, seg, N, key_rects, key_flags, n_seg * m, rects, flags, n_seg * n, status)
        e1.record()
        e1.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    out = {"segments": n_seg, "frames_per_segment": n, "N": N, "key_rows": n_seg * m, "status": sorted(set(status.cpu().tolist())),
           "alternations": alternations,
           "expand_ms": {"samples": [round(x, 4) for x in ms], "median": round(float(np.median(ms)), 4), "min": round(min(ms), 4),
                         "max": round(max(ms), 4)}}
    out["ns_per_frame"] = round(1e6 * out["expand_ms"]["median"] / (n_seg * n), 3)
    print(json.dumps(out))


def stats(v):
    return {"samples": [round(x, 1) for x in v], "median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--clips", type=int, default=200)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--face_track", default=None, choices=["score", "largest", "left", "right"],
                    help="compare the packed detector without and with face_track=PICK instead of packed against per-clip")
    ap.add_argument("--scene_cuts", default=None, type=float, metavar="THRESH",
                    help="compare the packed detector without and with scene_cuts=THRESH instead of packed against per-clip")
    ap.add_argument("--all_faces", default=None, type=int, metavar="F",
                    help="compare the packed detector with track_spans alone and with all_faces=AllFaces(F) as well")
    ap.add_argument("--track_kernel_ms", default=False, action="store_true",
                    help="time w2l_face_tracks_all_segments alone (one segment of 4096 frames, four faces) and print one JSON line")
    ap.add_argument("--det_stride", default=None, type=int, metavar="N",
                    help="compare the packed detector without and with det_stride=N instead of packed against per-clip")
    ap.add_argument("--expand_kernel_ms", default=False, action="store_true",
                    help="time w2l_face_rects_expand_segments alone (64 segments of 4096 frames) and print one JSON line")
    a = ap.parse_args(argv)
    if sum(v is not None for v in (a.face_track if a.scene_cuts is None else None, a.scene_cuts, a.all_faces, a.det_stride)) > 1:
        ap.error("--face_track, --scene_cuts (alone or with --face_track), --all_faces and --det_stride are four comparisons: give one")
    if a.track_kernel_ms:
        return track_kernel_ms(torch.device("cuda", 0), a.alternations)
    if a.expand_kernel_ms:
        return expand_kernel_ms(torch.device("cuda", 0), a.alternations, 2 if a.det_stride is None else a.det_stride)
    dev = torch.device("cuda", 0)
    clips = clips_with_faces(a.clips, a.seed)
    frames = sum(len(c) for c in clips)
    _mod._Graph = _counting_graph
    out = {"clips": a.clips, "frames": frames, "batch": a.batch, "precision": a.precision, "alternations": a.alternations}
    loops = {"packed": (run_packed, detector(dev, a.precision)), "per_clip": (run_loop, detector(dev, a.precision))}
    if a.face_track is not None:
        out["face_track"] = a.face_track
    if a.face_track is not None and a.scene_cuts is None:
        loops["packed_tracked"] = (lambda det, clips, batch: run_packed(det, clips, batch, face_track=a.face_track), loops.pop("per_clip")[1])
    if a.scene_cuts is not None:
        out["scene_cuts"] = a.scene_cuts
        loops["packed_scene"] = (lambda det, clips, batch: run_packed(det, clips, batch, scene_cuts=a.scene_cuts, face_track=a.face_track),
                                 loops.pop("per_clip")[1])
    if a.det_stride is not None:
        out["det_stride"] = a.det_stride
        loops["packed_stride"] = (lambda det, clips, batch: run_packed(det, clips, batch, det_stride=a.det_stride), loops.pop("per_clip")[1])
    if a.all_faces is not None:
        out["all_faces"] = a.all_faces
        spans = face_detection.TrackSpans(25, 1, 0)
        faces = face_detection.AllFaces(a.all_faces)
        loops = {"packed_spans": (lambda det, clips, batch: span_boxes(run_packed(det, clips, batch, track_spans=spans)), loops["packed"][1]),
                 "packed_all_faces": (lambda det, clips, batch: slot0(run_packed(det, clips, batch, track_spans=spans, all_faces=faces)),
                                      loops["per_clip"][1])}
    first, second = list(loops)
    res = {k: {"frames_per_s": [], "graph_builds": []} for k in loops}
    last = {}

    def one_pass(name):
        fn, det = loops[name]
        BUILDS[0] = 0
        last[name], t = fn(det, clips, a.batch)
        print("%s: %d frames, %.2f s, %d graph builds" % (name, frames, t, BUILDS[0]), file=sys.stderr, flush=True)
        return t, BUILDS[0]

    for name in loops:                                      # pass 0: warm-up
        t, b = one_pass(name)
        res[name].update(first_pass_s=round(t, 2), first_pass_graph_builds=b,
                         max_memory_allocated_gb=round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2))
    for _ in range(a.alternations):
        for name in loops:
            t, b = one_pass(name)
            res[name]["frames_per_s"].append(frames / t)
            res[name]["graph_builds"].append(b)
    for name in loops:
        res[name]["frames_per_s"] = stats(res[name]["frames_per_s"])
    out.update(res)
    both = [(p, q) for p, q in zip(last[first], last[second]) if p is not None and q is not None]
    out["clips_with_boxes_in_both"] = len(both)
    out["clips_where_only_one_path_found_faces"] = sum((p is None) != (q is None) for p, q in zip(last[first], last[second]))
    out["boxes_compared"] = int(sum(len(p) for p, _ in both))
    out["boxes_that_differ"] = int(sum((p != q).any(axis=1).sum() for p, q in both))
    out["%s_over_%s_median" % (first, second)] = round(res[first]["frames_per_s"]["median"] / res[second]["frames_per_s"]["median"], 3)
    out["ahead_by_more_than_the_spread"] = bool(res[first]["frames_per_s"]["min"] > res[second]["frames_per_s"]["max"])
    out["behind_by_more_than_the_spread"] = bool(res[first]["frames_per_s"]["max"] < res[second]["frames_per_s"]["min"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
