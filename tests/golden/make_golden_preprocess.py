"""Generates the committed preprocessing fixture from the REAL reference: `process_video_file` of the reference's preprocess.py
(its source, executed as written) with the reference's own FaceAlignment (S3FD network, batch_detect, nms, thresholds, int rects)
on CPU fp32.  Runs only in the build container.

    python tests/golden/make_golden_preprocess.py

preprocess.py cannot be imported as a module (it parses sys.argv, checks for s3fd.pth and builds CUDA detectors at import time),
so the function's source is taken from the file and executed in a namespace that holds what the module would have: `fa` (one
CPU FaceAlignment), `np`, `os`, `path` and a `cv2` stub.  The stub's VideoCapture yields the seeded frames of
wav2lip_amd.synthetic.preprocess_clips and its imwrite records (path, crop shape, crc32 of the crop bytes) instead of writing a
JPEG.  Weights are the seeded S3FD state dict (no s3fd.pth offline), handed to the reference's SFDDetector in place of its
download.  The fixture also holds each written frame's float box, and the script checks that every coordinate that lands
inside the frame is at least 0.01 from an integer and every frame's best score at least 0.04 from the 0.5 threshold, so that
fp32 rounding differences cannot move a rect or a detection.
"""
import ast
import os
import sys
import tempfile
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"

from wav2lip_amd import synthetic as synth  # noqa: E402

BATCH_SIZE = 4
PREPROCESSED_ROOT = "preprocessed"


def reference_function(name):
    src = open(os.path.join(REF, "preprocess.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name)
    return ast.get_source_segment(src, fn)


def main():
    writes = []
    clips = synth.preprocess_clips()
    frames_of = {"data/%s/%s.mp4" % (d, n): fr for d, n, fr, _, _ in clips}

    class VideoCapture:
        def __init__(self, vfile):
            self.frames = list(frames_of[vfile])

        def read(self):
            return (True, self.frames.pop(0)) if self.frames else (False, None)

        def release(self):
            pass

    def imwrite(p, img):
        assert img.size > 0
        writes.append((os.path.relpath(p, PREPROCESSED_ROOT), img.shape, zlib.crc32(np.ascontiguousarray(img).tobytes())))
        return True

    cv2 = types.ModuleType("cv2")
    cv2.VideoCapture, cv2.imwrite = VideoCapture, imwrite
    sys.modules["cv2"] = cv2
    sys.path.insert(0, REF)
    import face_detection
    from face_detection.detection.sfd import sfd_detector
    assert face_detection.__file__.startswith(REF)
    sd = synth.s3fd_state_dict()
    sfd_detector.load_url = lambda url: sd              # the reference downloads s3fd.pth when it is missing: hand it the weights
    torch.set_num_threads(8)
    fa = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device="cpu")

    # every frame's rect and best candidate score, for the margin checks (the reference's detector, called per clip)
    from face_detection.detection.sfd.detect import batch_detect
    boxes = {}
    for vfile, fr in frames_of.items():
        det = fa.get_detections_for_batch(np.asarray(fr))
        dense = batch_detect(fa.face_detector.face_detector, fr[..., ::-1].copy(), device="cpu")
        lists = fa.face_detector.detect_from_batch(fr[..., ::-1].copy())
        for k, (r, d) in enumerate(zip(det, lists)):
            best = float(dense[:, k, 4].max())
            assert abs(best - 0.5) >= 0.04, (vfile, k, best)
            if r is None:
                continue
            b = np.asarray(d[0][:4], np.float64)
            H, W = fr.shape[1:3]
            inside = np.array([b[0] < W, b[1] < H, b[2] < W, b[3] < H])
            frac = np.abs(b - np.round(b))[inside]
            assert frac.size == 0 or frac.min() >= 0.01, (vfile, k, b)
            boxes[(vfile, k)] = (r, d[0][:5].astype(np.float32))

    ns = {"fa": [fa], "np": np, "os": os, "path": os.path, "cv2": cv2}
    exec(reference_function("process_video_file"), ns)
    args = types.SimpleNamespace(batch_size=BATCH_SIZE, preprocessed_root=PREPROCESSED_ROOT)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:          # process_video_file creates the clip directories (left empty here)
        os.chdir(tmp)
        try:
            for vfile in frames_of:
                ns["process_video_file"](vfile, args, 0)
        finally:
            os.chdir(cwd)

    paths = [w[0] for w in writes]
    rects, floats = [], []
    for p in paths:
        d, n, f = p.split("/")
        r, b = boxes[("data/%s/%s.mp4" % (d, n), int(f.split(".")[0]))]
        rects.append(r)
        floats.append(b)
    out = {"paths": np.asarray(paths), "shapes": np.asarray([w[1] for w in writes], np.int64),
           "crc32": np.asarray([w[2] for w in writes], np.int64), "rects": np.asarray(rects, np.int64),
           "boxes": np.asarray(floats, np.float32), "batch_size": np.int64(BATCH_SIZE),
           "n_frames": np.asarray([len(fr) for fr in frames_of.values()], np.int64)}
    print("%d crops written of %d frames" % (len(paths), sum(len(fr) for fr in frames_of.values())))
    path = os.path.join(HERE, "golden_preprocess_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
