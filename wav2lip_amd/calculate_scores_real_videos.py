"""The reference's evaluation/scores_LSE/calculate_scores_real_videos.py and its .sh on the HIP path: LSE-D / LSE-C of real
videos - ReSyncED, or a user's own results, such as `real_videos_inference` writes - one `dist conf` line per face track.

    python -m wav2lip_amd.calculate_scores_real_videos --videofile result.avi --checkpoint_path lipsync_expert.pth
    python -m wav2lip_amd.calculate_scores_real_videos --data_root results/ --checkpoint_path lipsync_expert.pth \\
        --scores_file all_scores.txt --scene_cuts 0.3 --face_track largest

A real video has cuts, turned heads and frames without a face, so it is not scored as one take (that is `calculate_scores`, the
LRS scorer).  The reference's .sh runs syncnet_python's run_pipeline.py first - not part of the reference tree - which finds shots,
follows faces, bridges short detector misses and drops short tracks, and the .py then scores every face track it left (:32-40).
Here `face_detection.detect_many(track_spans=...)` is that stage: with `--scene_cuts` the video is split into shots,
with `--face_track` one face is followed through each, `w2l_face_spans_segments` turns the detections into face spans
(`--num_failed_det`, `--min_track`, `--min_face_size`), and every kept span (a, b) is one `evaluation.ScoreJob` whose crops are
frames a..b-1 and whose `first` is a, so its windows read the mel columns of its own frames.  All spans of all videos go through
ONE `evaluation.lse_many` call.  With `--all_faces [--max_faces F]` every face in the picture is followed instead of
one per shot - up to F at a time, `--face_track_cands` candidates per frame, `--face_track_iou` overlap, `--num_failed_det` missed
frames tolerated - and every face track is a `ScoreJob` of its own: one line per face track of the video, as the reference's flow
prints them.

Output: stdout gets the reference's line per span (:40), `str(dist) + " " + str(conf)`, in video and span order and nothing else;
`--scores_file PATH` appends the same lines (the .sh's all_scores.txt).  stderr names the videos that cannot be read or have no
kept span, the spans too short for one 5-frame / 16-column window, and with `--all_faces` once per video the candidates that
found no free track slot ("more than F faces: N candidates not followed").

Differences and limits, stated plainly: the scorer is the in-tree `SyncNet_color` whose weights `--checkpoint_path` names in place
of `--initial_model`, so absolute values are not the paper's; without `--all_faces` ONE face per shot is followed where
run_pipeline.py tracks every face in the picture, and with it at most `--max_faces` at a time; the crops are the detector's box with `T = 5` mean smoothing, not run_pipeline.py's padded square with a median
filter; inputs are the AVIs of container.py with their own PCM track; `--data_dir` and `--reference` are accepted and unused
(nothing is unpacked to disk).  The span defaults follow run_pipeline.py's published ones as far as they carry over and are
choices, not measurements; the quality of the spans on real footage is unmeasured, and no throughput is claimed.
"""
import argparse
import glob
import os
import sys
import tempfile

from .calculate_scores import FACE_DET_BATCH_SIZE, _read_clip, _skip, face_crops


def build_parser():
    """calculate_scores_real_videos.py:10-16: the reference's flags, types and defaults; --checkpoint_path stands in for
    --initial_model"""
    parser = argparse.ArgumentParser(description="SyncNet")
    parser.add_argument('--checkpoint_path', type=str, required=True, help='SyncNet_color weights (the expert discriminator)')
    parser.add_argument('--batch_size', type=int, default=20, help='')
    parser.add_argument('--vshift', type=int, default=15, help='')
    parser.add_argument('--data_dir', type=str, default='data/work', help='')
    parser.add_argument('--videofile', type=str, default='', help='')
    parser.add_argument('--reference', type=str, default='', help='')
    return parser


def build_cli_parser():
    """the reference's flags plus the .sh's loop and file, and what the in-tree detector and scorer need"""
    from .face_detection.faces import add_faces_flags
    from .face_detection.spans import add_span_flags
    from .inference import add_det_scale_flag, add_scene_flag, add_stride_flag, add_track_flags
    p = build_parser()
    p.add_argument('--data_root', type=str, default=None, help='Score every *.avi of this directory, in sorted order, instead of --videofile')
    p.add_argument('--scores_file', type=str, default=None, help='Append the printed lines to this file (the reference\'s all_scores.txt)')
    p.add_argument('--fps', type=float, default=25., help='Frame rate the mel windows are placed at')
    p.add_argument('--box', nargs=4, type=int, default=None, metavar=('y1', 'y2', 'x1', 'x2'),
                   help='One face box for every frame: the video is one span and no detector runs')
    p.add_argument('--face_det_precision', default='fp32', choices=['fp32', 'bf16'],
                   help='Face detector arithmetic: fp32 (default, matches the reference) or bf16 storage')
    add_det_scale_flag(p)
    add_stride_flag(p)
    p.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'],
                   help='SyncNet arithmetic: fp32 (default, matches the reference) or bf16 storage')
    add_scene_flag(p)
    add_track_flags(p)
    add_span_flags(p)
    add_faces_flags(p)
    return p


parser = build_parser()
cli_parser = build_cli_parser()


def span_jobs(args, videos, device, detector, skipped):
    """the producer: one evaluation.ScoreJob per kept face span, in `videos` and span order; `skipped` collects the names of the
    videos (and "<name>#<t>" of the spans) it passes over"""
    from . import audio, face_detection
    from .evaluation import ScoreJob
    from .face_detection.faces import faces_from_args, faces_kw
    from .face_detection.scene import scene_from_args, scene_kw
    from .face_detection.spans import spans_from_args
    from .face_detection.stride import stride_from_args
    from .face_detection.track import track_from_args, track_kw
    from .inference import validate_boxes
    spans = spans_from_args(args)
    faces = faces_from_args(args)
    held = {}                            # name -> (wav, frames) of the clips read ahead of their boxes

    def skip(name, why, trace=None):
        if trace:
            sys.stderr.write(trace)
        _skip(name, why)
        skipped.append(name)

    def read(tmpdir):
        for video in videos:
            name = os.path.basename(video)
            got = _read_clip(video, name, tmpdir, skip)
            if got is not None:
                yield name, got

    def span_scores(name, wav, frames, boxes, kept):
        if not kept:
            skip(name, "no face span of at least {} frames".format(spans.min_len))
            return
        mel = audio.melspectrogram_device(wav, device)
        for t, (a, b) in enumerate(kept):
            key = "{}#{}".format(name, t)
            try:
                yield ScoreJob(key, face_crops(frames[a:b], boxes[a:b] if faces is None else boxes[t], device), mel, a)
            except ValueError as e:                      # a box outside its frame
                skip(key, str(e))

    with tempfile.TemporaryDirectory(prefix="w2l_scores_") as tmpdir:
        if args.box is not None:
            for name, (wav, frames) in read(tmpdir):
                try:
                    boxes = validate_boxes([args.box], frames.shape[1], frames.shape[2]) * len(frames)
                except ValueError as e:
                    skip(name, str(e))
                    continue
                yield from span_scores(name, wav, frames, boxes, [(0, len(frames))])
            return

        def inputs():
            for name, got in read(tmpdir):
                held[name] = got
                yield face_detection.DetectJob(name, got[1])

        kw = {**(track_kw(track_from_args(args)) if faces is None else faces_kw(faces)), **scene_kw(scene_from_args(args)),
              **stride_from_args(args)}
        for name, boxes, error in face_detection.detect_many(detector, inputs(), pads=(0, 0, 0, 0), T=5, batch_size=FACE_DET_BATCH_SIZE,
                                                             track_spans=spans, **kw):
            wav, frames = held.pop(name)
            if error is not None:
                skip(name, error)
                continue
            if faces is None:
                yield from span_scores(name, wav, frames, boxes.boxes, boxes.spans)
                continue
            if boxes.dropped:
                sys.stderr.write("{}: more than {} faces: {} candidates not followed\n".format(name, faces.max_faces, boxes.dropped))
            yield from span_scores(name, wav, frames, [t.boxes for t in boxes.tracks], [(t.a, t.b) for t in boxes.tracks])


def main(argv=None, state_dict=None):
    """calculate_scores_real_videos.py:25-40 and the loop of its .sh.  `state_dict` (S3FD weights) replaces face_detection/s3fd.pth.
    Returns the list of `evaluation.lse_many` results of the scored spans, in video and span order (key "<video name>#<t>")."""
    import torch
    from . import checkpoint, evaluation, inference
    from .models import SyncNet_color
    args = cli_parser.parse_args(argv)
    if bool(args.videofile) == (args.data_root is not None):
        cli_parser.error("give one of --videofile FILE and --data_root DIR")
    if args.all_faces and args.face_track is not None:
        cli_parser.error("--all_faces follows every face and --face_track one: give one of them")
    if args.all_faces and args.box is not None:
        cli_parser.error("--box names the one face of every frame: --all_faces does not apply")
    device = torch.device("cuda", torch.cuda.current_device())
    model = SyncNet_color()
    model.load_state_dict(checkpoint.strip_module_prefix(checkpoint._load(args.checkpoint_path)["state_dict"]))
    model = model.to(device).eval()
    detector = None if args.box is not None else inference.detector_from_args(args, device, state_dict)
    videos = [args.videofile] if args.videofile else sorted(glob.glob(os.path.join(args.data_root, "*.avi")))
    scored, skipped = [], []
    scores_file = open(args.scores_file, "a") if args.scores_file else None

    def sink(res):
        if res["n"] == 0:
            _skip(res["key"], "too short for one 5-frame / 16-column window")
            skipped.append(res["key"])
            return
        line = str(res["lse_d"]) + " " + str(res["lse_c"])
        print(line)
        if scores_file is not None:
            scores_file.write(line + "\n")
        scored.append(res)

    try:
        evaluation.lse_many(model, span_jobs(args, videos, device, detector, skipped), fps=args.fps, vshift=args.vshift,
                            batch_size=args.batch_size, sink=sink, precision=inference.CLI_PRECISION[args.precision])
    finally:
        if scores_file is not None:
            scores_file.close()
    return scored


if __name__ == '__main__':
    main()
