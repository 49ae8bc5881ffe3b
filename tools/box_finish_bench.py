"""Device time of the two strict box finishes alone, at product sizes: `w2l_face_boxes_segments` on 16 clips of 30..120 frames
and `w2l_face_boxes_stream` on 64 and 256 open streams with one new frame each (50 frames seen), T = 5, every frame detected.

    [W2L_HIP_LIB=other/libw2l_hip.so] python tools/box_finish_bench.py [--launches 200] [--warmup 20] [--seed 0]

Each launch sits between two events of its own; prints one JSON line with the median, min and max microseconds per launch and
the library the figures belong to.  The stream launch's host side (the checks of the segment table) is not in the events; its
wall time per call is reported beside them."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wav2lip_amd import _lib  # noqa: E402
from wav2lip_amd._lib import check, current_stream, ptr  # noqa: E402
from wav2lip_amd.face_detection import live, many  # noqa: E402
from wav2lip_amd.face_detection.s3fd import RECT_FOUND  # noqa: E402

H = W = 160
PADS = (0, 10, 0, 0)
T = 5
SEEN = 50


def timed(launch, warmup, launches):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    us, wall = [], []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        launch()
        wall.append(1e6 * (time.perf_counter() - t0))
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return {"device_us": {"median": round(float(np.median(us)), 2), "min": round(min(us), 2), "max": round(max(us), 2)},
            "host_call_us_median": round(float(np.median(wall)), 2)}


def clips_case(lib, dev, r):
    lengths = r.integers(30, 121, 16)
    rows = int(lengths.sum())
    t = np.zeros(16, many.BOX_SEGMENT)
    row0 = 0
    for k, n in enumerate(lengths):
        t[k] = (row0, int(n), H, W)
        row0 += int(n)
    segs = torch.from_numpy(t.view(np.uint8)).to(dev)
    rects = torch.from_numpy(r.integers(0, 161, (rows, 4)).astype(np.int32)).to(dev)
    flags = torch.full((rows,), RECT_FOUND, dtype=torch.int32, device=dev)
    boxes = torch.zeros((rows, 4), dtype=torch.int32, device=dev)
    status = torch.zeros((16, 2), dtype=torch.int32, device=dev)

    def launch():
        check(lib.w2l_face_boxes_segments(current_stream(), 16, ptr(segs), ptr(rects), ptr(flags), *PADS, T, ptr(boxes), ptr(status)),
              "face_boxes_segments")
    return launch, {"clips": 16, "frames": rows}


def streams_case(lib, dev, r, S):
    t = np.zeros(S, live.BOX_STREAM_SEGMENT)
    for k in range(S):
        t[k] = (k, 1, H, W, k, SEEN, 0, k)                   # one new frame, open: one output row each
    segs = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
    rects = torch.from_numpy(r.integers(0, 161, (S, 4)).astype(np.int32)).to(dev)
    flags = torch.full((S,), RECT_FOUND, dtype=torch.int32, device=dev)
    carry = torch.from_numpy(r.integers(0, 161, (S, 64, 4)).astype(np.int32)).to(dev)
    boxes = torch.zeros((S, 4), dtype=torch.int32, device=dev)
    status = torch.zeros((S, 2), dtype=torch.int32, device=dev)

    def launch():
        check(lib.w2l_face_boxes_stream(current_stream(), S, t.ctypes.data, ptr(segs), ptr(rects), ptr(flags), S, ptr(carry), S, *PADS,
                                        T, ptr(boxes), S, ptr(status)), "face_boxes_stream")
    return launch, {"streams": S, "seen": SEEN, "new_frames_each": 1}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    r = np.random.default_rng(a.seed)
    out = {"lib": os.path.basename(os.environ.get("W2L_HIP_LIB", "")) or "default", "T": T, "launches": a.launches, "cases": []}
    for launch, what in [clips_case(lib, dev, r), streams_case(lib, dev, r, 64), streams_case(lib, dev, r, 256)]:
        what.update(timed(launch, a.warmup, a.launches))
        out["cases"].append(what)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
