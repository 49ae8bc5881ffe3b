"""The reference's evaluation/scores_LSE/calculate_scores_LRS.py on the HIP path: every `*.avi` of `--data_root` is scored and
the average LSE-C (confidence) and LSE-D (minimum distance) are printed.

    python -m wav2lip_amd.calculate_scores --data_root results/ --checkpoint_path lipsync_expert.pth

The reference scores one video per call (:41-47).  Here a producer reads a clip, computes its mel and its 96x96 face crops and
hands it to `evaluation.lse_many`, which packs the windows of successive clips into full SyncNet batches and scores a group of
clips in one launch.

Differences, the ones `evaluation.py` and `gen_videos_from_filelist.py` document: the scorer is the in-tree `SyncNet_color`, whose
weights `--checkpoint_path` names in place of `--initial_model` (the published `SyncNetModel.S` is not vendored, so absolute
values are not comparable to the paper's); inputs are the uncompressed AVIs of container.py, and the audio is the clip's own PCM
track, read back with `audio.load_wav(path, 16000)`; `--tmp_dir` and `--reference` are accepted and unused (nothing is unpacked to
disk).  The network sees the lower half of a face crop, so every frame needs a face box: `--box y1 y2 x1 x2` for all frames, or
`inference.face_detect` per clip as the filelist command runs it (no pads, smoothing on).  `--fps` is the frame rate the mel
windows are placed at, `--face_det_precision` the detector's arithmetic, `--face_det_scale K` the size of the frame it sees (1/K), `--precision` SyncNet's (fp32, or the opt-in bf16-storage
plan of DESIGN.md 3o).  `--packed_face_det` (off by default) detects the
faces of successive clips in shared detector batches (`face_detection.detect_many`); scored clips, skipped clips and
their messages stay what they are without it.

One line per scored clip goes to stdout, then the reference's two lines (:49-50), averaged over the scored clips.  A clip that
cannot be decoded, has no audio, has a frame without a face or is too short for one window is named on stderr with the reason.
"""
import argparse
import glob
import os
import sys
import tempfile
import traceback

import numpy as np

from . import container


def build_parser():
    """calculate_scores_LRS.py:14-21: the reference's flags, types and defaults; --checkpoint_path stands in for --initial_model"""
    parser = argparse.ArgumentParser(description="SyncNet")
    parser.add_argument('--checkpoint_path', type=str, required=True, help='SyncNet_color weights (the expert discriminator)')
    parser.add_argument('--batch_size', type=int, default=20, help='')
    parser.add_argument('--vshift', type=int, default=15, help='')
    parser.add_argument('--data_root', type=str, required=True, help='')
    parser.add_argument('--tmp_dir', type=str, default="data/work/pytmp", help='')
    parser.add_argument('--reference', type=str, default="demo", help='')
    return parser


def build_cli_parser():
    """the reference's flags plus what the in-tree scorer needs"""
    p = build_parser()
    p.add_argument('--fps', type=float, default=25., help='Frame rate the mel windows are placed at')
    p.add_argument('--box', nargs=4, type=int, default=None, metavar=('y1', 'y2', 'x1', 'x2'),
                   help='One face box for every frame; without it the face detector runs on every clip')
    p.add_argument('--face_det_precision', default='fp32', choices=['fp32', 'bf16'],
                   help='Face detector arithmetic: fp32 (default, matches the reference) or bf16 storage')
    from .inference import add_det_scale_flag, add_stride_flag
    add_det_scale_flag(p)
    add_stride_flag(p)
    p.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'],
                   help='SyncNet arithmetic: fp32 (default, matches the reference) or bf16 storage')
    p.add_argument('--packed_face_det', default=False, action='store_true',
                   help='Detect faces of successive clips in shared detector batches (face_detection.detect_many)')
    return p


parser = build_parser()
cli_parser = build_cli_parser()
FACE_DET_BATCH_SIZE = 64


def _skip(name, why):
    print("{}: skipped: {}".format(name, why), file=sys.stderr)


def face_crops(frames, boxes, device):
    """uint8 [T,96,96,3] on the device: frame i cropped to boxes[i] and resized (w2l_crop_resize_rows_u8, one launch per clip)"""
    import torch
    from . import _lib, inference, multiclip
    from .evaluation import img_size
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError("face_crops: frames must be uint8 [T,H,W,3], got %s %s" % (frames.dtype, frames.shape))
    boxes = inference.validate_boxes(boxes, frames.shape[1], frames.shape[2])      # the kernel takes the boxes as they are
    if len(boxes) != len(frames):
        raise ValueError("face_crops: %d boxes for %d frames" % (len(boxes), len(frames)))
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(device)
    T, H, W = src.shape[:3]
    table = np.zeros(T, multiclip.FRAME_ROW)
    table["src"] = src.data_ptr() + np.arange(T, dtype=np.int64) * (H * W * 3)
    table["H"], table["W"] = H, W
    b = np.asarray(boxes, dtype=np.int32)
    table["y1"], table["y2"], table["x1"], table["x2"] = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    table_dev = torch.from_numpy(table.view(np.uint8)).to(device)
    out = torch.empty((T, img_size, img_size, 3), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.load().w2l_crop_resize_rows_u8(_lib.current_stream(), T, _lib.ptr(table_dev), img_size, _lib.ptr(out)),
                   "crop_resize_rows")
    return out


def _read_clip(video, name, tmpdir, skip):
    """(wav, frames uint8 [T,H,W,3]) of one clip, or None after `skip(name, why, traceback text or None)`"""
    from .gen_videos_from_filelist import _load_audio
    try:
        wav, _, _ = _load_audio(video, tmpdir)
        frames = container.read_avi(video)["frames"]
    except KeyboardInterrupt:
        raise
    except Exception as e:
        skip(name, "could not be decoded (uncompressed BGR AVI with PCM16 audio only): {}".format(e), traceback.format_exc())
        return None
    if len(frames) == 0:
        skip(name, "no frames", None)
        return None
    return wav, frames


def score_jobs(args, videos, device, detector, skipped):
    """the producer: one evaluation.ScoreJob per readable clip, in `videos` order; `skipped` collects the names it passes over"""
    from . import audio, inference
    from .face_detection.stride import stride_from_args
    from .evaluation import ScoreJob

    def skip(name, why, trace):
        if trace:
            sys.stderr.write(trace)
        _skip(name, why)
        skipped.append(name)

    with tempfile.TemporaryDirectory(prefix="w2l_scores_") as tmpdir:
        for video in videos:
            name = os.path.basename(video)
            try:
                got = _read_clip(video, name, tmpdir, skip)
                if got is None:
                    continue
                wav, frames = got
                if args.box is not None:
                    boxes = inference.validate_boxes([args.box], frames.shape[1], frames.shape[2]) * len(frames)
                else:
                    det = inference.face_detect(list(frames), detector=detector, pads=[0, 0, 0, 0], nosmooth=False,
                                                batch_size=FACE_DET_BATCH_SIZE, **stride_from_args(args))
                    boxes = inference.validate_boxes([c for _, c in det], frames.shape[1], frames.shape[2])
                yield ScoreJob(name, face_crops(frames, boxes, device), audio.melspectrogram_device(wav, device))
            except KeyboardInterrupt:
                raise
            except ValueError as e:                      # no face in a frame, a box outside its frame
                _skip(name, str(e))
                skipped.append(name)


def score_jobs_packed(args, videos, device, detector, skipped):
    """`score_jobs` with detection packed across clips (`--packed_face_det`, no `--box`): clips are read ahead, their frames go
    through `face_detection.detect_many`, and crops + mel are made as each clip's boxes arrive.  What the reading stage has to say
    about a clip it passes over is held back until the scorable clip after it is answered, so stderr and `skipped` read as they do
    from `score_jobs`."""
    from . import audio, face_detection, inference
    from .face_detection.stride import stride_from_args
    from .evaluation import ScoreJob
    held, notes, tail = {}, {}, []       # name -> (wav, frames); name -> [(name, why, trace)] due before it; after the last

    def flush(items):
        for name, why, trace in items:
            if trace:
                sys.stderr.write(trace)
            _skip(name, why)
            skipped.append(name)

    def inputs(tmpdir):
        said = []
        for video in videos:
            name = os.path.basename(video)
            got = _read_clip(video, name, tmpdir, lambda *a: said.append(a))
            if got is None:
                continue
            held[name] = got
            notes[name], said = said, []
            yield face_detection.DetectJob(name, got[1])
        tail.extend(said)

    with tempfile.TemporaryDirectory(prefix="w2l_scores_") as tmpdir:
        for name, boxes, error in face_detection.detect_many(detector, inputs(tmpdir), pads=(0, 0, 0, 0), T=5,
                                                             batch_size=FACE_DET_BATCH_SIZE, **stride_from_args(args)):
            flush(notes.pop(name))
            wav, frames = held.pop(name)
            try:
                if error is not None:
                    raise ValueError(error)
                boxes = inference.validate_boxes(boxes, frames.shape[1], frames.shape[2])
                yield ScoreJob(name, face_crops(frames, boxes, device), audio.melspectrogram_device(wav, device))
            except ValueError as e:                      # no face in a frame, a box outside its frame
                _skip(name, str(e))
                skipped.append(name)
        flush(tail)


def main(argv=None, state_dict=None):
    """calculate_scores_LRS.py:23-50.  `state_dict` (S3FD weights) replaces face_detection/s3fd.pth.  Returns the list of
    `evaluation.lse_many` results of the scored clips, in directory order."""
    import torch
    from . import checkpoint, evaluation, inference
    from .models import SyncNet_color
    args = cli_parser.parse_args(argv)
    device = torch.device("cuda", torch.cuda.current_device())
    model = SyncNet_color()
    model.load_state_dict(checkpoint.strip_module_prefix(checkpoint._load(args.checkpoint_path)["state_dict"]))
    model = model.to(device).eval()
    detector = None
    if args.box is None:
        detector = inference.detector_from_args(args, device, state_dict)
    videos = sorted(glob.glob(os.path.join(args.data_root, "*.avi")))
    scored, skipped = [], []

    def sink(res):
        if res["n"] == 0:
            _skip(res["key"], "too short for one 5-frame / 16-column window")
            skipped.append(res["key"])
            return
        print("{}: offset {}, confidence {:.3f}, minimum distance {:.3f}, windows {}".format(
            res["key"], res["offset"], res["lse_c"], res["lse_d"], res["n"]))
        scored.append(res)

    producer = score_jobs_packed if args.packed_face_det and args.box is None else score_jobs
    evaluation.lse_many(model, producer(args, videos, device, detector, skipped), fps=args.fps, vshift=args.vshift,
                        batch_size=args.batch_size, sink=sink, precision=inference.CLI_PRECISION[args.precision])
    if not scored:
        raise SystemExit("no clip of {} could be scored ({} skipped)".format(args.data_root, len(skipped)))
    print('Average Confidence: {}'.format(sum(r["lse_c"] for r in scored) / len(scored)))
    print('Average Minimum Distance: {}'.format(sum(r["lse_d"] for r in scored) / len(scored)))
    return scored


if __name__ == '__main__':
    main()
