"""The reference's evaluation/real_videos_inference.py on the HIP path: the ReSyncED real-video benchmark in its `random`,
`dubbed` and `tts` modes.  Every line `video audio_src` drives the lips of `<data_root>/<video>` with the audio of
`<data_root>/<audio_src>` and writes `<results_dir>/<line index>.avi` (note the order: the video comes first here, the audio first
in gen_videos_from_filelist.py).

    python -m wav2lip_amd.real_videos_inference --mode random --filelist pairs.txt --results_dir out/ --data_root ReSyncED/ \\
        --checkpoint_path wav2lip.pth
    python -m wav2lip_amd.real_videos_inference --mode dubbed --results_dir out/ --data_root ReSyncED/dubbed --checkpoint_path ...

Per line the steps are the reference's `main()` (:211-301) with the frames resident on the device from the read to the paste:

    mel of the audio (NaN: the reference's ValueError('Mel contains nan!'), :224-225)
    the frames go up ONCE
    frames whose short side exceeds --max_frame_res are resized to it (:239-245)        one w2l_resize_rows_u8 launch
    the frame count is matched to the chunk count (:257-264): truncated; a shortfall in `tts` mode is made up by naming
        frames twice (`increase_frames_index`, :149-167 - a duplicate is a row, not a copy); in the other modes it raises the
        reference's ValueError('#Frames, audio length mismatch'), uncaught there and here
    S3FD on frame 0 (:52-54); no face: the line is skipped (its ValueError is caught at :266-269)
    `rescale_factor` from that face's size (:59-68); factor > 1: every frame // factor     one more w2l_resize_rows_u8 launch
    boxes of all frames on the device frames, pads and T = 5 smoothing (:90-103); a frame without a face skips the line
    a `multiclip.ClipJob` with the device frames and rows (frame index, box, mel start)

and all jobs go lazily through `multiclip.lipsync_many`: rows of successive clips share full generator batches, a clip's frames
are read where they lie (nothing of them is staged per batch) and released after its last row, so device memory is bounded by
the clips in flight.  Skipped lines leave gaps in the numbering, as in the reference.

Differences from the reference, all deliberate:
  * `--face_res`, `--min_frame_res` and `--max_frame_res` are declared `type=int`.  The reference declares no type, so a value
    given on its command line arrives as a string and fails at the first subtraction (:61, :64, :239); its defaults are ints.
  * `--precision`, `--face_det_precision` and `--face_det_scale` are added, as in the sibling commands.
  * `dubbed` mode lists `data_root` SORTED and pairs every file with itself; the reference's `listdir` order (:203) is the
    filesystem's, so its numbering is not reproducible from one machine to the next.
  * file formats are those of gen_videos_from_filelist: a name is `<data_root>/<name>` when that file exists, else
    `<data_root>/<name>.avi`; inputs are the uncompressed AVI of container.py, the driving audio is the PCM track of the audio
    source (through a temporary WAV and audio.load_wav, the reference's `temp/temp.wav`), the result is ONE AVI at the video's
    own frame rate with that audio muxed in.  An input that cannot be decoded is reported on stderr and skipped.
  * an audio shorter than one 16-column window is skipped; the reference fails there with an IndexError on `images[0]` (:52).
Under torch.distributed.run rank r takes the lines i with i % WORLD_SIZE == r; no collectives.
"""
import argparse
import math
import os
import sys
import tempfile
import traceback

import numpy as np

from . import container
from . import gen_videos_from_filelist as gv
from ._lib import RESIZE_ROW
from .staging import Staging

mel_step_size = 16
MAX_ROWS = 65535          # rows of one w2l_resize_rows_u8 launch
MAX_PIXELS = 1 << 29      # its largest destination frame


def build_parser():
    """real_videos_inference.py:14-37: the reference's flags, names and defaults; the three resolutions typed int (module text)"""
    parser = argparse.ArgumentParser(description='Code to generate results on ReSyncED evaluation set')
    parser.add_argument('--mode', type=str, help='random | dubbed | tts', required=True)
    parser.add_argument('--filelist', type=str, help='Filepath of filelist file to read', default=None)
    parser.add_argument('--results_dir', type=str, help='Folder to save all results into', required=True)
    parser.add_argument('--data_root', type=str, required=True)
    parser.add_argument('--checkpoint_path', type=str, help='Name of saved checkpoint to load weights from', required=True)
    parser.add_argument('--pads', nargs='+', type=int, default=[0, 10, 0, 0], help='Padding (top, bottom, left, right)')
    parser.add_argument('--face_det_batch_size', type=int, help='Single GPU batch size for face detection', default=16)
    parser.add_argument('--wav2lip_batch_size', type=int, help='Batch size for Wav2Lip', default=128)
    parser.add_argument('--face_res', type=int, help='Approximate resolution of the face at which to test', default=180)
    parser.add_argument('--min_frame_res', type=int, help='Do not downsample further below this frame resolution', default=480)
    parser.add_argument('--max_frame_res', type=int, help='Downsample to at least this frame resolution', default=720)
    return parser


def build_cli_parser():
    """the reference's flags plus the two additions the sibling commands have, each fp32 by default"""
    p = build_parser()
    p.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'],
                   help='Generator arithmetic: fp32 (default, matches the reference) or bf16 storage')
    p.add_argument('--face_det_precision', default='fp32', choices=['fp32', 'bf16'],
                   help='Face detector arithmetic: fp32 (default, matches the reference) or bf16 storage')
    return p


def build_main_parser():
    """what `main()` parses: `build_cli_parser` plus `--face_det_scale K`, the size of the frame the detector sees
    (`inference.add_det_scale_flag`), `--blend_feather N` / `--blend_top FRACTION`, the blended paste
    (`inference.add_blend_flags`), and `--color_match {mean,full}`, the prediction's colours matched to its crop
    (`inference.add_color_match_flag`), and `--face_det_stride N`, the detector on every Nth frame of a line's frame sequence
    (`inference.add_stride_flag`); `cli_parser` stays the reference's surface plus the two precision flags"""
    from .inference import add_blend_flags, add_color_match_flag, add_det_scale_flag, add_stride_flag
    p = build_cli_parser()
    add_det_scale_flag(p)
    add_stride_flag(p)
    add_blend_flags(p)
    add_color_match_flag(p)
    return p


parser = build_parser()
cli_parser = build_cli_parser()
main_parser = build_main_parser()
MODES = ('random', 'dubbed', 'tts')


# ---------------------------------------------------------------- the host rules, each on its own
def capped_size(h, w, max_frame_res):
    """:239-245: the (w, h) a frame of h x w is resized to at read time, or None when its short side is within `max_frame_res`"""
    if min(h, w) > max_frame_res:
        scale_factor = min(h, w) / float(max_frame_res)
        return int(w / scale_factor), int(h / scale_factor)
    return None


def rescale_factor(face_size, h, w, face_res, min_frame_res):
    """:61-68: the integer factor `rescale_frames` divides every frame of h x w by, for a first-frame face of `face_size` pixels:
    the largest factor that still brings the face closer to `face_res` without taking the frame's short side below
    `min_frame_res`; 1 = no resize (a loop that runs out at 15 leaves 14, as there)"""
    diff = abs(face_size - face_res)
    for factor in range(2, 16):
        downsampled_res = face_size // factor
        if min(h // factor, w // factor) < min_frame_res:
            break
        if abs(downsampled_res - face_res) >= diff:
            break
    factor -= 1
    return int(factor)


def increase_frames_index(n, l):
    """:149-167 `increase_frames(frames, l)` for frames = list(range(n)): the source index of every one of the l output frames,
    frames duplicated evenly (and again, while the list is still short)"""
    frames = list(range(n))
    if n < 1 and l > 0:
        raise ValueError("no frames to duplicate")
    while len(frames) < l:
        dup_every = float(l) / len(frames)
        final_frames = []
        next_duplicate = 0.
        for i, f in enumerate(frames):
            final_frames.append(f)
            if int(math.ceil(next_duplicate)) == i:
                final_frames.append(f)
            next_duplicate += dup_every
        frames = final_frames
    return frames[:l]


def real_chunk_starts(n_mel, fps):
    """:248-255: start column of every FULL 16-column window at the video's own frame rate; no tail window"""
    mel_idx_multiplier = 80. / fps
    starts = []
    i = 0
    while True:
        start_idx = int(i * mel_idx_multiplier)
        if start_idx + mel_step_size > n_mel:
            return starts
        starts.append(start_idx)
        i += 1


def frame_index(n_frames, n_chunks, mode):
    """:257-264: which source frame every chunk runs on.  Enough frames: the first `n_chunks`; too few: duplicated in `tts` mode,
    the reference's ValueError in any other"""
    if n_frames < n_chunks:
        if mode == 'tts':
            return increase_frames_index(n_frames, n_chunks)
        raise ValueError('#Frames, audio length mismatch')
    return list(range(n_chunks))


def lines_of(args):
    """:202-209: `dubbed` pairs every file of data_root with itself (sorted: module text); the other modes read --filelist"""
    if args.mode == 'dubbed':
        return ['{} {}'.format(f, f) for f in sorted(os.listdir(args.data_root))]
    assert args.filelist is not None
    with open(args.filelist, 'r') as filelist:
        return filelist.readlines()


def resolve(data_root, name):
    path = os.path.join(data_root, name)
    return path if os.path.isfile(path) else path + '.avi'


# ---------------------------------------------------------------- the device steps (the seams the host tests stub)
def resize_rows(rows):
    """w2l_resize_rows_u8 on the current stream.  rows: [(src address, dst address, Hs, Ws, Hd, Wd)], device addresses of uint8
    [Hs,Ws,3] / [Hd,Wd,3] frames at any byte alignment.  The sizes are validated here: the kernel cannot (include/w2l_hip.h)."""
    import torch
    from ._lib import check, current_stream, load, ptr
    for _, _, Hs, Ws, Hd, Wd in rows:
        if min(Hs, Ws, Hd, Wd) < 1 or Hd * Wd > MAX_PIXELS or Hs * Ws > MAX_PIXELS:
            raise ValueError("resize %dx%d -> %dx%d: sizes must be at least 1 and at most 2^29 pixels" % (Hs, Ws, Hd, Wd))
    dev = torch.device("cuda", torch.cuda.current_device())
    for lo in range(0, len(rows), MAX_ROWS):
        part = rows[lo:lo + MAX_ROWS]
        st = Staging(dev)
        table = st.table(RESIZE_ROW, len(part))
        st.allocate()
        st.view(table)[:] = [tuple(int(v) for v in r) for r in part]
        st.upload()
        check(load().w2l_resize_rows_u8(current_stream(), len(part), ptr(st.dev), max(r[4] * r[5] for r in part)),
              "resize_rows_u8")


def resize_frames_device(frames, wh):
    """`[cv2.resize(f, (w, h)) for f in frames]` for a contiguous uint8 device tensor [F,Hs,Ws,3], in one launch -> [F,h,w,3]"""
    import torch
    w, h = int(wh[0]), int(wh[1])
    F, Hs, Ws = (int(v) for v in frames.shape[:3])
    with torch.cuda.device(frames.device):
        out = torch.empty((F, h, w, 3), dtype=torch.uint8, device=frames.device)
        resize_rows([(frames.data_ptr() + i * Hs * Ws * 3, out.data_ptr() + i * h * w * 3, Hs, Ws, h, w) for i in range(F)])
    return out


def upload_frames(frames, device):
    """the clip's one trip up: uint8 [F,H,W,3] host frames -> a contiguous device tensor"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(frames)).to(device)


def device_mel(wav, device):
    """:222-225: the spectrogram on the device, with the reference's NaN check"""
    import torch
    from . import audio
    mel = audio.melspectrogram_device(wav, device)
    if bool(torch.isnan(mel).any()):
        raise ValueError('Mel contains nan!')
    return mel


def _device_rects(detector, frames, batch_size):
    """`inference._detect_rects` (:77-88) on device frames: one rect (or None) per frame of the tensor, batches halved on a
    RuntimeError of the detector (`inference.halving`, with this command's final message)"""
    from .inference import halving

    def run(size):
        rects = []
        for lo in range(0, int(frames.shape[0]), size):
            rects += detector.get_detections_for_batch(frames[lo:lo + size])
        return rects

    return halving(run, batch_size, error='Image too big to run face detection on GPU')


def first_rect(detector, frames):
    """:52: the detector's (x1, y1, x2, y2) on frame 0, or None"""
    return detector.get_detections_for_batch(frames[:1])[0]


def clip_boxes(detector, frames, index, pads, batch_size, det_stride=1):
    """:73-103 for the frame sequence frames[index]: int array [len(index), 4] of (y1, y2, x1, x2), padded, clipped and smoothed
    with T = 5 over that sequence; ValueError('Face not detected!...') when a frame has no face.  A sequence without duplicates
    goes through `face_detection.detect_many` on the frames where they lie.  With duplicates (`tts`) every frame is detected
    once, its rect is repeated per row, and the finish is detect_many's host form (`host_boxes`): no frame is copied.
    `det_stride` N > 1 (`--face_det_stride`): the detector sees the key frames of the SEQUENCE only and the rows
    between them are interpolated - `detect_many(det_stride=N)`; with duplicates the distinct key frames are gathered and detected
    once each, and `stride.host_stride_fill` fills the sequence."""
    from . import face_detection
    from .face_detection import many
    from .face_detection.stride import host_stride_fill, key_frames, stride_kw
    n = len(index)
    if list(index) == list(range(n)):
        (_, boxes, error), = face_detection.detect_many(detector, [face_detection.DetectJob(0, frames[:n])], pads=pads, T=5,
                                                        batch_size=batch_size, **stride_kw(det_stride))
        if error is not None:
            raise ValueError(error)
        return boxes
    if det_stride > 1:
        import torch
        keys = [index[k] for k in key_frames(n, det_stride)]
        seen = sorted(set(keys))
        found = dict(zip(seen, _device_rects(detector, frames[torch.tensor(seen, device=frames.device)], batch_size)))
        rects = host_stride_fill([found[i] for i in keys], n, det_stride)
        if any(r is None for r in rects):
            raise ValueError(many.NO_FACE)
        return many.host_boxes(rects, int(frames.shape[1]), int(frames.shape[2]), pads, 5)
    rects = _device_rects(detector, frames, batch_size)
    if any(rects[i] is None for i in index):
        raise ValueError(many.NO_FACE)
    return many.host_boxes([rects[i] for i in index], int(frames.shape[1]), int(frames.shape[2]), pads, 5)


def read_inputs(video, audio_src, tmpdir):
    """(frames uint8 [F,H,W,3], fps, wav float32 at 16 kHz, the audio track's PCM16 samples, its rate).  The frames are read
    onto the current HIP device (the rank's: sharding.init_from_env binds it), where this command keeps each clip anyway: a
    Motion-JPEG clip is decoded there, an uncompressed one uploaded."""
    import torch
    wav, pcm, sr = gv._load_audio(audio_src, tmpdir)
    clip = container.read_avi(video, device=torch.device("cuda", torch.cuda.current_device()))
    return clip["frames"], clip["fps"], wav, pcm, sr


# ---------------------------------------------------------------- the producer
def clip_jobs(args, lines, ranks, detector, tracks, report=None):
    """one multiclip.ClipJob per runnable line of this rank, in line order, its frames a device tensor.  `tracks[line index]`
    receives (fps, frame size (w, h), PCM16 audio, rate) for the sink that opens the line's writer; `report[line index]` (when
    given) what was decided: frame sizes after each resize, the factor, the index list, the boxes."""
    from . import multiclip
    from .face_detection.stride import stride_kw
    with tempfile.TemporaryDirectory(prefix="w2l_real_videos_") as tmpdir:
        for idx, line in gv.lines_of_rank(lines, ranks):
            video, audio_src = line.strip().split()
            try:
                frames, fps, wav, pcm, sr = read_inputs(resolve(args.data_root, video), resolve(args.data_root, audio_src), tmpdir)
            except KeyboardInterrupt:
                raise
            except Exception:
                traceback.print_exc()
                gv._skip(idx, line, "an input could not be decoded (uncompressed or Motion-JPEG AVI with PCM16 audio only)")
                continue
            mel = device_mel(wav, ranks.device)
            starts = real_chunk_starts(int(mel.shape[1]), fps)
            if not starts:
                gv._skip(idx, line, "the audio is shorter than one 16-column mel window")
                continue
            index = frame_index(len(frames), len(starts), args.mode)         # raises in random / dubbed: not caught (:261)
            frames = frames[:len(starts)]
            if not hasattr(frames, "is_cuda"):                               # host frames (a caller's own read_inputs): one trip up
                frames = upload_frames(frames, ranks.device)
            elif frames.device != ranks.device:
                frames = frames.to(ranks.device)
            frames = frames.contiguous()
            note = {"read": tuple(int(v) for v in frames.shape[1:3])}
            cap = capped_size(int(frames.shape[1]), int(frames.shape[2]), args.max_frame_res)
            if cap is not None:
                frames = resize_frames_device(frames, cap)
            note["capped"] = tuple(int(v) for v in frames.shape[1:3])
            if report is not None:
                report[idx] = note
            rect = first_rect(detector, frames)
            if rect is None:
                gv._skip(idx, line, "Face not detected!")
                continue
            h, w = int(frames.shape[1]), int(frames.shape[2])
            x1, y1, x2, y2 = rect
            factor = rescale_factor(max(abs(y1 - y2), abs(x1 - x2)), h, w, args.face_res, args.min_frame_res)
            if factor > 1:
                frames = resize_frames_device(frames, (w // factor, h // factor))
            h, w = int(frames.shape[1]), int(frames.shape[2])
            note.update(factor=factor, rescaled=(h, w), index=list(index))
            try:
                boxes = clip_boxes(detector, frames, index, args.pads, args.face_det_batch_size,
                                   **stride_kw(getattr(args, 'face_det_stride', 1)))
            except ValueError as e:
                gv._skip(idx, line, str(e))
                continue
            note["boxes"] = np.asarray(boxes, np.int64).reshape(-1, 4)
            rows = [(fi, tuple(int(v) for v in box), s) for fi, box, s in zip(index, boxes, starts)]
            tracks[idx] = (fps, (w, h), pcm, sr)
            yield multiclip.ClipJob(idx, frames, mel, rows)
            del frames, mel


class ResultSink(gv.ResultSink):
    """the filelist command's sink at the video's own frame rate (:229, :278): tracks[idx] = (fps, frame size, PCM16 audio, rate)"""

    def __call__(self, idx, frame):
        if frame is not None and idx not in self.open:
            vfps, size, pcm, sr = self.tracks.pop(idx)
            self.open[idx] = container.AviWriter(os.path.join(self.results_dir, '{}.avi'.format(idx)), vfps, size, audio=pcm,
                                                 audio_sr=sr)
        gv.ResultSink.__call__(self, idx, frame)


def run(args, lines, ranks, detector, model, report=None):
    """all lines of this rank through `multiclip.lipsync_many`; returns the line indices written, in order"""
    from . import inference, multiclip
    tracks = {}
    sink = ResultSink(args.results_dir, tracks)
    try:
        multiclip.lipsync_many(model, clip_jobs(args, lines, ranks, detector, tracks, report), batch_size=args.wav2lip_batch_size,
                               precision=inference.CLI_PRECISION[args.precision], sink=sink,
                               **inference._blend_kw(inference.blend_from_args(args)),
                               **inference._color_kw(inference.color_match_from_args(args)))
    finally:
        sink.close()
    return sink.written


def main(argv=None, state_dict=None, backend="nccl", report=None):
    """real_videos_inference.py:199-301.  `state_dict` (S3FD weights) replaces face_detection/s3fd.pth; `backend` is the process
    group's.  Returns the line indices this rank wrote, in order."""
    from . import inference, sharding
    args = main_parser.parse_args(argv)
    inference.blend_from_args(args)              # a bad pair raises here, before the process group and any device work
    if args.mode not in MODES:
        raise ValueError("--mode must be one of random | dubbed | tts")
    args.img_size = 96
    ranks = sharding.init_from_env(backend)
    try:
        if not os.path.isdir(args.results_dir):
            os.makedirs(args.results_dir, exist_ok=True)
        lines = lines_of(args)
        print('Using {} for inference.'.format(ranks.device))
        detector = inference.detector_from_args(args, ranks.device, state_dict)
        model = inference.load_model(args.checkpoint_path, ranks.device)
        return run(args, lines, ranks, detector, model, report)
    finally:
        ranks.close()


if __name__ == '__main__':
    main()
