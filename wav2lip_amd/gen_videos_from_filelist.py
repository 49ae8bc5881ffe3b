"""The reference's evaluation/gen_videos_from_filelist.py on the HIP path: every line `audio_src video` of `--filelist` drives the
lips of `<data_root>/<video>` with the audio of `<data_root>/<audio_src>` and writes `<results_dir>/<line index>.avi`.  This is how
the benchmark videos for LSE-D / LSE-C are produced.

    python -m wav2lip_amd.gen_videos_from_filelist --filelist test.txt --results_dir out/ --data_root LRS2/main \\
        --checkpoint_path wav2lip.pth
    python -m torch.distributed.run --nproc-per-node 8 -m wav2lip_amd.gen_videos_from_filelist ...

The reference runs one clip at a time (:205-227), every clip a ragged batch of its own.  Here a producer reads a line, computes
its mel and its face boxes and hands the clip to `multiclip.lipsync_many`, which packs the rows of successive clips into full
generator batches; face detection of the next clip runs on the caller's stream while the lanes run earlier batches.

Per line the steps are the reference's `main()` (:158-235).  Differences, all on the file-format side and the same ones
`inference.main` and `preprocess` document: inputs are `<data_root>/<name>.avi`, the uncompressed AVI of container.py (24-bit BGR,
PCM16 audio); the driving audio is the PCM track of `<audio_src>.avi`, written to a temporary WAV (the reference's
`temp/temp.wav`, :167-171) and read back with `audio.load_wav(path, 16000)`, so the mono mix and the resampling are the existing
ones; the result is ONE AVI with that audio muxed in (the reference's `temp/result.avi` + ffmpeg, :229-235).  An input that
cannot be decoded is reported on stderr and skipped.

A line is skipped without output, and the line index still advances, when the mel has NaN (:173), the video has fewer frames
than mel chunks (:195) or a frame has no face (:200-203); every skip names its reason on stderr.  A clip whose audio is too short
for one full 16-column window is skipped too: the reference would fail there on an unbound `out` (:229), no batch having opened
the writer.  Detection is `inference.face_detect` per clip: pads from `--pads`, smoothing always on with T = 5 (:74).

Flags the reference does not have, as in `inference.main`: `--precision`, `--face_det_precision` and `--face_det_scale K` (the
detector sees every frame at 1/K of its size; boxes are mapped back, written frames keep their size).  Another,
`--packed_face_det` (off by default), runs detection through `face_detection.detect_many`: the frames of successive clips share
detector batches of `--face_det_batch_size`, the per-clip finish runs once per group on the device, and lines, skip messages and
written files stay what they are without it.  Under
torch.distributed.run rank r takes the lines i with i % WORLD_SIZE == r and writes its own result files; no collectives.
"""
import argparse
import os
import sys
import tempfile
import traceback
import wave

import numpy as np

from . import container


def build_parser():
    """gen_videos_from_filelist.py:14-33: the reference's flags, names, types and defaults"""
    parser = argparse.ArgumentParser(description='Code to generate results for test filelists')
    parser.add_argument('--filelist', type=str, help='Filepath of filelist file to read', required=True)
    parser.add_argument('--results_dir', type=str, help='Folder to save all results into', required=True)
    parser.add_argument('--data_root', type=str, required=True)
    parser.add_argument('--checkpoint_path', type=str, help='Name of saved checkpoint to load weights from', required=True)
    parser.add_argument('--pads', nargs='+', type=int, default=[0, 0, 0, 0], help='Padding (top, bottom, left, right)')
    parser.add_argument('--face_det_batch_size', type=int, help='Single GPU batch size for face detection', default=64)
    parser.add_argument('--wav2lip_batch_size', type=int, help='Batch size for Wav2Lip', default=128)
    return parser


def build_cli_parser():
    """the reference's flags plus the two additions `inference.main` has, each fp32 by default"""
    p = build_parser()
    p.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'],
                   help='Generator arithmetic: fp32 (default, matches the reference) or bf16 storage')
    p.add_argument('--face_det_precision', default='fp32', choices=['fp32', 'bf16'],
                   help='Face detector arithmetic: fp32 (default, matches the reference) or bf16 storage')
    return p


def build_main_parser():
    """what `main()` parses: `build_cli_parser` plus `--packed_face_det`, which changes how the work is scheduled and nothing of
    what is computed, and `--face_det_scale K`, the size of the frame the detector sees (`inference.add_det_scale_flag`).
    `--blend_feather N` / `--blend_top FRACTION` blend every generated face into its frame (`inference.add_blend_flags`).
    `--color_match {mean,full}` matches every generated face's colours to its crop first (`inference.add_color_match_flag`).
    `--no_face_hold G` generates a line with frames without a face instead of skipping it (`inference.add_hold_flag`).
    `--face_track PICK` follows one face through every line's clip (`inference.add_track_flags`), with and without
    `--packed_face_det`, and so does `--scene_cuts THRESH`, which boxes and tracks every shot of a clip alone
    (`inference.add_scene_flag`), and `--face_det_stride N`, which shows the detector every Nth frame of a clip or
    shot and interpolates the boxes between (`inference.add_stride_flag`).  `cli_parser` stays the reference's surface plus the two precision flags."""
    from .inference import (add_blend_flags, add_color_match_flag, add_det_scale_flag, add_hold_flag, add_scene_flag, add_stride_flag,
                            add_track_flags)
    p = build_cli_parser()
    p.add_argument('--packed_face_det', default=False, action='store_true',
                   help='Detect faces of successive clips in shared detector batches (face_detection.detect_many)')
    add_det_scale_flag(p)
    add_blend_flags(p)
    add_color_match_flag(p)
    add_hold_flag(p)
    add_track_flags(p)
    add_scene_flag(p)
    add_stride_flag(p)
    return p


parser = build_parser()
cli_parser = build_cli_parser()
main_parser = build_main_parser()
fps = 25                  # gen_videos_from_filelist.py:120


def lines_of_rank(lines, ranks):
    """[(line index, line)] this rank runs: line i belongs to rank i % world (the dealing of preprocess.py)"""
    return [(i, line) for i, line in enumerate(lines) if i % ranks.world == ranks.rank]


def _skip_text(idx, line, why):
    return "line {} ({}): skipped: {}\n".format(idx, line.strip(), why)


def _skip(idx, line, why):
    sys.stderr.write(_skip_text(idx, line, why))


def _load_audio(audio_src, tmpdir):
    """:167-171: the audio track of `audio_src` as `temp.wav`, read back with audio.load_wav.  Returns (wav float32 at 16 kHz, the
    track's PCM16 samples, its rate)"""
    from . import audio
    a = container.read_avi(audio_src)
    if a["audio"] is None:
        raise ValueError("%s has no audio track" % audio_src)
    pcm = np.ascontiguousarray(a["audio"], dtype='<i2')
    temp_audio = os.path.join(tmpdir, "temp.wav")
    with wave.open(temp_audio, 'wb') as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(int(a["audio_sr"]))
        w.writeframes(pcm.tobytes())
    return audio.load_wav(temp_audio, 16000), pcm, int(a["audio_sr"])


def _read_line(args, idx, line, ranks, tmpdir, say):
    """everything of one line up to detection: (frames truncated to the chunk count, mel, PCM16 audio, rate), or None after
    `say(text)` has been given the stderr text of the reason"""
    import torch
    from . import audio, multiclip
    audio_src, video = line.strip().split()
    audio_src = os.path.join(args.data_root, audio_src) + '.avi'
    video = os.path.join(args.data_root, video) + '.avi'
    try:
        wav, pcm, sr = _load_audio(audio_src, tmpdir)
        clip = container.read_avi(video)
    except KeyboardInterrupt:
        raise
    except Exception:
        say(traceback.format_exc())
        say(_skip_text(idx, line, "an input could not be decoded (uncompressed BGR AVI with PCM16 audio only)"))
        return None
    mel = audio.melspectrogram_device(wav, ranks.device)
    if bool(torch.isnan(mel).any()):
        say(_skip_text(idx, line, "the mel spectrogram contains NaN"))
        return None
    n_chunks = len(multiclip.filelist_chunk_starts(mel.shape[1]))
    if n_chunks == 0:
        say(_skip_text(idx, line, "the audio is shorter than one 16-column mel window"))
        return None
    full_frames = list(clip["frames"])
    if len(full_frames) < n_chunks:
        say(_skip_text(idx, line, "the video has fewer frames ({}) than mel chunks ({})".format(len(full_frames), n_chunks)))
        return None
    return full_frames[:n_chunks], mel, pcm, sr


def clip_jobs(args, lines, ranks, detector, tracks):
    """the producer: one multiclip.ClipJob per runnable line of this rank, in line order.  `tracks[line index]` receives
    (frame size (w, h), PCM16 audio, rate) for the sink that opens the line's writer."""
    from . import inference, multiclip
    with tempfile.TemporaryDirectory(prefix="w2l_filelist_") as tmpdir:
        for idx, line in lines_of_rank(lines, ranks):
            try:
                got = _read_line(args, idx, line, ranks, tmpdir, sys.stderr.write)
                if got is None:
                    continue
                full_frames, mel, pcm, sr = got
                try:
                    det = inference.face_detect(full_frames, detector=detector, pads=args.pads, nosmooth=False,
                                                batch_size=args.face_det_batch_size, **inference.detect_kw_from_args(args))
                except ValueError as e:
                    _skip(idx, line, str(e))
                    continue
                rows = multiclip.rows_filelist(mel.shape[1], len(full_frames), [c for _, c in det])
                frame_h, frame_w = full_frames[0].shape[:-1]
                tracks[idx] = ((frame_w, frame_h), pcm, sr)
                yield multiclip.ClipJob(idx, full_frames, mel, rows)
            except KeyboardInterrupt:
                raise
            except ValueError as e:                      # a malformed line, a box outside its frame
                traceback.print_exc()
                _skip(idx, line, str(e))


def clip_jobs_packed(args, lines, ranks, detector, tracks):
    """`clip_jobs` with detection packed across lines (`--packed_face_det`), in three stages: `_read_line` for the lines ahead,
    `face_detection.detect_many` over their frames, then rows and the ClipJob as each line's boxes arrive.  detect_many reads a
    group of lines before it answers the first, so what the first stage has to say about a line it passes over is held back
    and written when the runnable line after it is answered: stderr reads as it does from `clip_jobs`."""
    from . import face_detection, inference, multiclip
    held, notes, tail = {}, {}, []       # line index -> (line, frames, mel, pcm, rate); -> stderr text due before it; after the last

    def inputs(tmpdir):
        said = []
        for idx, line in lines_of_rank(lines, ranks):
            try:
                got = _read_line(args, idx, line, ranks, tmpdir, said.append)
            except KeyboardInterrupt:
                raise
            except ValueError as e:                      # a malformed line
                said.append(traceback.format_exc())
                said.append(_skip_text(idx, line, str(e)))
                continue
            if got is None:
                continue
            held[idx] = (line,) + got
            notes[idx], said = "".join(said), []
            yield face_detection.DetectJob(idx, got[0])
        tail.extend(said)

    with tempfile.TemporaryDirectory(prefix="w2l_filelist_") as tmpdir:
        for idx, boxes, error in face_detection.detect_many(detector, inputs(tmpdir), pads=args.pads, T=5,
                                                            batch_size=args.face_det_batch_size,
                                                            **inference.detect_kw_from_args(args)):
            sys.stderr.write(notes.pop(idx))
            line, full_frames, mel, pcm, sr = held.pop(idx)
            try:
                if error is not None:
                    _skip(idx, line, error)
                    continue
                rows = multiclip.rows_filelist(mel.shape[1], len(full_frames), [None if b is None else tuple(b) for b in boxes])
                frame_h, frame_w = full_frames[0].shape[:-1]
                tracks[idx] = ((frame_w, frame_h), pcm, sr)
                yield multiclip.ClipJob(idx, full_frames, mel, rows)
            except KeyboardInterrupt:
                raise
            except ValueError as e:                      # a box outside its frame
                traceback.print_exc()
                _skip(idx, line, str(e))
        sys.stderr.write("".join(tail))


class ResultSink:
    """one AviWriter per open job: `<results_dir>/<line index>.avi` with the driving audio (:211-212, :227-235)"""

    def __init__(self, results_dir, tracks):
        self.results_dir, self.tracks, self.open, self.written = results_dir, tracks, {}, []

    def __call__(self, idx, frame):
        if frame is None:
            w = self.open.pop(idx, None)
            if w is not None:
                w.release()
                self.written.append(idx)
            return
        w = self.open.get(idx)
        if w is None:
            size, pcm, sr = self.tracks.pop(idx)
            w = self.open[idx] = container.AviWriter(os.path.join(self.results_dir, '{}.avi'.format(idx)), fps, size,
                                                     audio=pcm, audio_sr=sr)
        w.write(frame)

    def close(self):
        for w in self.open.values():
            w.release()
        self.open.clear()


def main(argv=None, state_dict=None, backend="nccl"):
    """gen_videos_from_filelist.py:152-235.  `state_dict` (S3FD weights) replaces face_detection/s3fd.pth; `backend` is the
    process group's.  Returns the line indices this rank wrote, in order."""
    from . import inference, multiclip, sharding
    args = main_parser.parse_args(argv)
    args.img_size = 96
    blend_kw = inference._blend_kw(inference.blend_from_args(args))
    color_kw = inference._color_kw(inference.color_match_from_args(args))
    inference.detect_kw_from_args(args)                  # a flag of the track without --face_track: refused before any device work
    ranks = sharding.init_from_env(backend)
    try:
        assert args.data_root is not None
        if not os.path.isdir(args.results_dir):
            os.makedirs(args.results_dir, exist_ok=True)
        with open(args.filelist, 'r') as filelist:
            lines = filelist.readlines()
        print('Using {} for inference.'.format(ranks.device))
        detector = inference.detector_from_args(args, ranks.device, state_dict)
        model = inference.load_model(args.checkpoint_path, ranks.device)
        tracks = {}
        sink = ResultSink(args.results_dir, tracks)
        try:
            producer = clip_jobs_packed if args.packed_face_det else clip_jobs
            multiclip.lipsync_many(model, producer(args, lines, ranks, detector, tracks), batch_size=args.wav2lip_batch_size,
                                   precision=inference.CLI_PRECISION[args.precision], sink=sink, **blend_kw, **color_kw)
        finally:
            sink.close()
        return sink.written
    finally:
        ranks.close()


if __name__ == '__main__':
    main()
