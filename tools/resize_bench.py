"""The row-table whole-frame resize against the dense one, alternated in one process: GB/s (bytes read + bytes written) of
`w2l_resize_rows_u8` and of `w2l_resize_u8` over the same stack of frames.

    python tools/resize_bench.py [--frames 32] [--alternations 5] [--iters 20] [--seed 0]

Two cases, the two resizes of `python -m wav2lip_amd.real_videos_inference` at real-video sizes: 1080p -> 720p (the
`--max_frame_res` cap, the bilinear path) and 720p -> 360p (`rescale_frames` by a factor of 2, the 2x2 average path).  Frames are
seeded noise resident on the device; the row table of the row-table kernel is built and uploaded once, outside the timing.  Per
case: one warm-up pass of each kernel, then the two alternate, --alternations pairs; a pass is --iters launches between two
events.  Bytes = frames * (Hs*Ws + Hd*Wd) * 3 per launch: every source byte counted once although neighbouring destination pixels
re-read it from cache.  The outputs are compared byte for byte before anything is timed.  Prints one JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wav2lip_amd import _lib  # noqa: E402
from wav2lip_amd import real_videos_inference as rv  # noqa: E402
from wav2lip_amd._lib import check, current_stream, ptr  # noqa: E402

CASES = [("1080p_to_720p", (1080, 1920), (720, 1280)), ("720p_to_360p", (720, 1280), (360, 640))]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    for name, (Hs, Ws), (Hd, Wd) in CASES:
        g = torch.Generator(device="cpu").manual_seed(a.seed)
        src = torch.randint(0, 256, (a.frames, Hs, Ws, 3), dtype=torch.uint8, generator=g).to(dev)
        dense = torch.empty((a.frames, Hd, Wd, 3), dtype=torch.uint8, device=dev)
        rows = torch.empty_like(dense)
        table = np.zeros(a.frames, rv.RESIZE_ROW)
        for i in range(a.frames):
            table[i] = (src.data_ptr() + i * Hs * Ws * 3, rows.data_ptr() + i * Hd * Wd * 3, Hs, Ws, Hd, Wd)
        table = torch.from_numpy(table.view(np.uint8)).to(dev)

        def run_dense():
            check(lib.w2l_resize_u8(current_stream(), a.frames, ptr(src), Hs, Ws, ptr(dense), Hd, Wd), "resize_u8")

        def run_rows():
            check(lib.w2l_resize_rows_u8(current_stream(), a.frames, ptr(table), Hd * Wd), "resize_rows_u8")

        run_dense()
        run_rows()
        torch.cuda.synchronize()
        equal = bool(torch.equal(dense, rows))
        nbytes = a.frames * (Hs * Ws + Hd * Wd) * 3
        warm = {"resize_u8": timed(run_dense, a.iters), "resize_rows_u8": timed(run_rows, a.iters)}
        passes = {"resize_u8": [], "resize_rows_u8": []}
        for _ in range(a.alternations):
            passes["resize_u8"].append(nbytes / timed(run_dense, a.iters) / 1e9)
            passes["resize_rows_u8"].append(nbytes / timed(run_rows, a.iters) / 1e9)
        out = {"case": name, "frames": a.frames, "src": [Hs, Ws], "dst": [Hd, Wd], "bytes_per_launch": nbytes, "byte_equal": equal,
               "iters": a.iters}
        for k, v in passes.items():
            out[k] = {"GBps": [round(x, 1) for x in v], "median": round(float(np.median(v)), 1), "min": round(min(v), 1),
                      "max": round(max(v), 1), "warmup_GBps": round(nbytes / warm[k] / 1e9, 1)}
        print(json.dumps(out))
        if not equal:
            raise SystemExit("the two kernels differ")


if __name__ == "__main__":
    main()
