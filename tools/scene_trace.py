"""The signature kernel of scene-cut detection against its yardstick, w2l_s3fd_pack_rows on the same batch, in one
kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o stats -- python tools/scene_trace.py run
    python tools/scene_trace.py summarise DIR > profiles/scene_cuts/kernel_trace.json

`run` is the workload: for 8 frames of 720x1280 and 16 frames of 480x640, once with random and once with constant-colour frames,
the packed detector (`face_detection.detect_many(..., scene_cuts=0.3)`, seeded S3FD weights) over the batch twice; then, for the same
four batches in the same order, REPS direct launches of w2l_s3fd_pack_rows (fp32, 4 channels - the detector's) and REPS of
w2l_frame_hist_rows on one address table.  `summarise` reads the trace: the last 4 * REPS dispatches of each of the two kernels are
the direct launches, in case order; the signature dispatches before them are those inside `detect_many`.  Times are the trace's
end - start per dispatch; GB/s counts the frame bytes read (B * H * W * 3), which is all the signature kernel moves and about a
sixth of what the pack moves."""
import csv
import glob
import json
import os
import sys

CASES = [("720x1280 random", 8, 720, 1280, "random"), ("720x1280 constant", 8, 720, 1280, "constant"),
         ("480x640 random", 16, 480, 640, "random"), ("480x640 constant", 16, 480, 640, "constant")]
REPS = 5
HIST, PACK = "frame_hist_rows_kernel", "s3fd_pack_rows_kernel"


def batch(B, H, W, content):
    import numpy as np
    if content == "random":
        return np.random.default_rng(B).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    out = np.empty((B, H, W, 3), np.uint8)
    out[:] = (16, 128, 235)                                  # one colour: every lane of a wave on one counter per channel
    return out


def run():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from wav2lip_amd import face_detection
    from wav2lip_amd import synthetic as synth
    from wav2lip_amd._lib import check, current_stream, load
    from wav2lip_amd.face_detection.scene import frame_signatures
    dev = torch.device("cuda", 0)
    det = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device=str(dev),
                                       state_dict=synth.s3fd_state_dict())
    held = []
    for name, B, H, W, content in CASES:
        frames = torch.from_numpy(batch(B, H, W, content)).to(dev)
        held.append(frames)
        for _ in range(2):
            list(face_detection.detect_many(det, [face_detection.DetectJob(name, frames)], batch_size=B, scene_cuts=0.3))
    torch.cuda.synchronize()
    for (name, B, H, W, content), frames in zip(CASES, held):
        table = torch.from_numpy(frames.data_ptr() + np.arange(B, dtype=np.int64) * (H * W * 3)).to(dev)
        y = torch.empty((B, H, W, 4), dtype=torch.float32, device=dev)
        sig = torch.empty((B, 96), dtype=torch.int32, device=dev)
        for _ in range(REPS):
            check(load().w2l_s3fd_pack_rows(current_stream(), B, H, W, table.data_ptr(), y.data_ptr(), 4), "s3fd_pack_rows")
        for _ in range(REPS):
            frame_signatures(table, sig, 0, rows=(B, H, W))
        torch.cuda.synchronize()
    print("scene_trace: done", flush=True)


def summarise(root):
    import numpy as np
    paths = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    if len(paths) != 1:
        raise SystemExit("expected one *kernel_trace.csv below %s, found %s" % (root, paths))
    rows = {HIST: [], PACK: []}
    with open(paths[0], newline="") as fh:
        for r in csv.DictReader(fh):
            for k in rows:
                if k in r["Kernel_Name"]:
                    rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {"unit": "us", "reps": REPS, "source": "rocprofv3 --kernel-trace --stats, one run; direct launches on one address table",
           "cases": {}, "dispatches": {k: len(v) for k, v in rows.items()}}
    for k in rows:
        rows[k].sort()
        if len(rows[k]) < len(CASES) * REPS:
            raise SystemExit("%s: %d dispatches in the trace, fewer than the %d direct launches" % (k, len(rows[k]), len(CASES) * REPS))
    n_direct = len(CASES) * REPS
    for i, (name, B, H, W, _) in enumerate(CASES):
        case = {}
        for k, label in ((HIST, "w2l_frame_hist_rows"), (PACK, "w2l_s3fd_pack_rows")):
            t = [(e - s) / 1000.0 for s, e in rows[k][len(rows[k]) - n_direct:][i * REPS:(i + 1) * REPS]]
            case[label] = {"samples": [round(v, 2) for v in t], "median": round(float(np.median(t)), 2), "min": round(min(t), 2),
                           "max": round(max(t), 2), "read_GBps_at_median": round(B * H * W * 3 / float(np.median(t)) / 1e3, 1)}
        case["hist_no_longer_than_pack"] = bool(case["w2l_frame_hist_rows"]["median"] <= case["w2l_s3fd_pack_rows"]["median"])
        out["cases"][name] = case
    inside = [(e - s) / 1000.0 for s, e in rows[HIST][:len(rows[HIST]) - n_direct]]
    out["w2l_frame_hist_rows_inside_detect_many"] = [round(v, 2) for v in inside]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "summarise":
        summarise(sys.argv[2])
    else:
        raise SystemExit(__doc__)
