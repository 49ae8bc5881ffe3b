"""The per-batch inference loop of the reference (inference.py:108-154 `datagen`, :231-240 mel chunking,
:249-272 forward + uint8 frames) on the HIP path, with everything between "uint8 face crops + mel" and
"uint8 generated crops" resident on the device:

    faces u8 [B,96,96,3] --w2l_datagen_pack--> x fp32 NHWC8 --+
    mel [80,T] + starts --w2l_mel_gather----> m fp32 NHWC4 ---+--> generator plan --> w2l_frames_to_u8 --> u8 [B,96,96,3]

With `precision="bf16"` (opt-in; `--precision bf16` on the command line) the same loop runs the bf16-storage generator plan:
w2l_datagen_pack_bf16 / w2l_mel_gather_bf16 fill bf16 NHWC8 inputs and the plan's last launch writes the uint8 frames itself.

Either side of that, also on the device: the face crop + `cv2.resize(face, (96, 96))` of
inference.py:121-126 (w2l_crop_resize_u8) and the `cv2.resize` to the box size + paste-back of :270-271
(w2l_resize_paste_u8), so that full uint8 frames go in and full uint8 frames come out (`Wav2LipRunner.run_frames`).
The output side of the loop (`cv2.VideoWriter` + the ffmpeg mux, inference.py:256-257,272-277) is `write_result` below, on top
of wav2lip_amd/container.py (uncompressed AVI with the PCM16 audio interleaved).  Out of scope: decoding compressed video
(`cv2.VideoCapture` of mp4 input), audio extraction from non-WAV containers (the reference's first ffmpeg call).
"""
import argparse
import copy
import os

import numpy as np
import torch

from . import _lib, audio
from ._lib import check, current_stream, ptr
from .checkpoint import _load, load_model  # noqa: F401  (inference.py:160-179: same names, same behaviour)

mel_step_size = 16   # inference.py:156
img_size = 96
MEL_ROW_BYTES = 16   # sizeof(w2l_mel_row)


# ---------------------------------------------------------------- the command-line surface (inference.py:11-57)
def build_parser():
    """the reference's flags, names, types and defaults (inference.py:11-51); `python -m wav2lip_amd.inference ...` takes the
    command line the reference's `python inference.py ...` takes"""
    parser = argparse.ArgumentParser(description='Inference code to lip-sync videos in the wild using Wav2Lip models')
    parser.add_argument('--checkpoint_path', type=str, help='Name of saved checkpoint to load weights from', required=True)
    parser.add_argument('--face', type=str, help='Filepath of video/image that contains faces to use', required=True)
    parser.add_argument('--audio', type=str, help='Filepath of video/audio file to use as raw audio source', required=True)
    parser.add_argument('--outfile', type=str, help='Video path to save result. See default for an e.g.',
                        default='results/result_voice.mp4')
    parser.add_argument('--static', type=bool, help='If True, then use only first video frame for inference', default=False)
    parser.add_argument('--fps', type=float, help='Can be specified only if input is a static image (default: 25)',
                        default=25., required=False)
    parser.add_argument('--pads', nargs='+', type=int, default=[0, 10, 0, 0],
                        help='Padding (top, bottom, left, right). Please adjust to include chin at least')
    parser.add_argument('--face_det_batch_size', type=int, help='Batch size for face detection', default=16)
    parser.add_argument('--wav2lip_batch_size', type=int, help='Batch size for Wav2Lip model(s)', default=128)
    parser.add_argument('--resize_factor', default=1, type=int,
                        help='Reduce the resolution by this factor. Sometimes, best results are obtained at 480p or 720p')
    parser.add_argument('--crop', nargs='+', type=int, default=[0, -1, 0, -1],
                        help='Crop video to a smaller region (top, bottom, left, right). Applied after resize_factor and rotate arg. '
                             'Useful if multiple face present. -1 implies the value will be auto-inferred based on height, width')
    parser.add_argument('--box', nargs='+', type=int, default=[-1, -1, -1, -1],
                        help='Specify a constant bounding box for the face. Use only as a last resort if the face is not detected.'
                             'Also, might work only if the face is not moving around much. Syntax: (top, bottom, left, right).')
    parser.add_argument('--rotate', default=False, action='store_true',
                        help='Sometimes videos taken from a phone can be flipped 90deg. If true, will flip video right by 90deg.'
                             'Use if you get a flipped result, despite feeding a normal looking video')
    parser.add_argument('--nosmooth', default=False, action='store_true',
                        help='Prevent smoothing face detections over a short temporal window')
    return parser


def det_scale_arg(text):
    """argparse type of `--face_det_scale`: an integer in 1..8 (a parse error otherwise)"""
    import argparse
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not an integer" % (text,))
    if not 1 <= k <= 8:
        raise argparse.ArgumentTypeError("%d is outside 1..8" % k)
    return k


DET_SCALE_HELP = ('Run the face detector on every frame at 1/K of its height and width (K = 1..8; default 1, as the reference). '
                  'The detector then costs about 1/K^2 as much and its boxes are mapped back to the full frame, so output frames '
                  'keep their size (unlike --resize_factor). Boxes move with K: this is not accuracy-neutral')


def add_det_scale_flag(p):
    """`--face_det_scale K` on a command's parser; independent of --resize_factor, --face_det_precision and --packed_face_det"""
    p.add_argument('--face_det_scale', default=1, type=det_scale_arg, metavar='K', help=DET_SCALE_HELP)


# ---------------------------------------------------------------- the feathered, mouth-region paste (opt-in)
BLEND_MAX_FEATHER = 64


def check_blend(blend):
    """the `blend=` of the runners, `lipsync`, `multiclip.lipsync_many` and `streaming.LipsyncStreams`: None (the reference's
    hard-rectangle paste) or a pair (feather, top).  `feather`: an int in 0..64, the width in output-frame pixels of the ramp
    inside the box edge; `top`: a float in [0, 1), the fraction of the box height, from its top, that keeps the original frame
    (0.5: the mouth half alone is pasted).  Returns None when the pair asks for the plain paste (feather 0 and int(top*256) == 0),
    else (feather, top) as (int, float); a ValueError names what is wrong."""
    if blend is None:
        return None
    try:
        feather, top = blend
    except (TypeError, ValueError):
        raise ValueError("blend must be None or a (feather, top) pair, got %r" % (blend,)) from None
    if isinstance(feather, bool) or not isinstance(feather, (int, np.integer)):
        raise ValueError("blend feather must be an integer in 0..%d, got %r" % (BLEND_MAX_FEATHER, feather))
    if not 0 <= feather <= BLEND_MAX_FEATHER:
        raise ValueError("blend feather %d is outside 0..%d" % (feather, BLEND_MAX_FEATHER))
    if isinstance(top, bool) or not isinstance(top, (int, float, np.integer, np.floating)):
        raise ValueError("blend top must be a fraction in [0, 1), got %r" % (top,))
    top = float(top)
    if not 0.0 <= top < 1.0:                # NaN fails both comparisons
        raise ValueError("blend top %r is outside [0, 1)" % (top,))
    if feather == 0 and blend_top_q8(top) == 0:
        return None
    return int(feather), top


def blend_top_q8(top):
    """`top_q8` of the blend kernels for a checked `top` in [0, 1): 0..255"""
    return int(top * 256)


def _blend_kw(blend):
    """the keyword a runner (or what builds one) takes for `blend`, checked first: none for the plain paste, so the default path is
    called with the same arguments as before the option (as `_precision_kw`)"""
    blend = check_blend(blend)
    return {} if blend is None else {"blend": blend}


def blend_feather_arg(text):
    """argparse type of `--blend_feather`: an integer in 0..64 (a parse error otherwise)"""
    try:
        f = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not an integer" % (text,))
    if not 0 <= f <= BLEND_MAX_FEATHER:
        raise argparse.ArgumentTypeError("%d is outside 0..%d" % (f, BLEND_MAX_FEATHER))
    return f


def blend_top_arg(text):
    """argparse type of `--blend_top`: a fraction in [0, 1) (a parse error otherwise)"""
    try:
        t = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not a number" % (text,))
    if not 0.0 <= t < 1.0:
        raise argparse.ArgumentTypeError("%r is outside [0, 1)" % (t,))
    return t


def add_blend_flags(p):
    """`--blend_feather N --blend_top FRACTION` on a command's parser; both 0 by default (the reference's paste) and independent
    of --precision, --out_codec and sharded runs"""
    p.add_argument('--blend_feather', default=0, type=blend_feather_arg, metavar='N',
                   help='Blend the generated face into the frame over a ramp of N pixels (0..64) inside the box edge instead of '
                        'pasting a hard rectangle (default 0, as the reference). Not the reference\'s output')
    p.add_argument('--blend_top', default=0.0, type=blend_top_arg, metavar='FRACTION',
                   help='Keep the original frame in this fraction of the face box, from its top (in [0, 1); default 0.0, as the '
                        'reference). 0.5 pastes the mouth half alone. Not the reference\'s output')


def blend_from_args(a):
    """the `blend=` of a parsed command line (`add_blend_flags`): None when both flags are at their defaults, or when the
    namespace comes from a parser without them"""
    return check_blend((getattr(a, "blend_feather", 0), getattr(a, "blend_top", 0.0)))


# ---------------------------------------------------------------- colour matching of the prediction (opt-in)
COLOR_MATCH_MODES = {"mean": 1, "full": 2}      # the `color_match=` spelling -> the `mode` of w2l_color_match_u8


def check_color_match(value):
    """the `color_match=` of the runners, `lipsync`, `multiclip.lipsync_many` and `streaming.LipsyncStreams`: None (the
    prediction is pasted as the generator gave it, the reference's behaviour), "mean" (every channel's mean over the upper half of
    the prediction is moved onto the crop's) or "full" (mean and spread).  Returns the value; a ValueError names the choices."""
    if value is None:
        return None
    if not isinstance(value, str) or value not in COLOR_MATCH_MODES:
        raise ValueError("color_match must be None, 'mean' or 'full', got %r" % (value,))
    return value


def _color_kw(color_match):
    """the keyword a runner (or what builds one) takes for `color_match`, checked first: none when it is off (as `_blend_kw`)"""
    color_match = check_color_match(color_match)
    return {} if color_match is None else {"color_match": color_match}


def add_color_match_flag(p):
    """`--color_match {mean,full}` on a command's parser; absent by default and independent of --blend_*, --precision,
    --no_face_hold, --face_track, --out_codec and sharded runs"""
    p.add_argument('--color_match', default=None, choices=sorted(COLOR_MATCH_MODES),
                   help='Match the colours of every generated face to the crop it was generated from before it is pasted: the '
                        'per-channel mean (mean) or mean and spread (full) over the upper half of the face, which the generator '
                        'is shown. Off by default, as the reference. Not the reference\'s output')


def color_match_from_args(a):
    """the `color_match=` of a parsed command line (`add_color_match_flag`): None when the flag is absent, or when the namespace
    comes from a parser without it"""
    return check_color_match(getattr(a, "color_match", None))


def build_cli_parser():
    """the command line `main()` parses: the reference's flags (`build_parser`, whose surface stays the reference's) plus
    documented additions that are not among them, each the reference's behaviour by default and independent of the others:
    `--precision {fp32,bf16}`, the generator's arithmetic, `--face_det_precision {fp32,bf16}`, the S3FD detector's,
    `--face_det_scale K`, the detector's frame size (1/K; output frames keep theirs), `--out_codec` / `--out_quality`,
    `--blend_feather N` / `--blend_top FRACTION`, the feathered mouth-region paste, `--color_match {mean,full}`, colour matching
    of the prediction to its crop (absent by default), `--no_face_hold G`, the pass-through for frames without a face (absent by
    default), `--face_track PICK` with its three companions, tracked face selection (`face_detection/track.py`; absent by
    default), `--scene_cuts THRESH`, every shot of the clip boxed and tracked alone (`face_detection/scene.py`; absent by
    default), and `--face_det_stride N`, the detector on every Nth frame and interpolated boxes between
    (`face_detection/stride.py`; 1 by default)"""
    p = build_parser()
    p.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'],
                   help='Generator arithmetic: fp32 (default, matches the reference) or bf16 storage (faster; frames differ by '
                        'about one uint8 level in a few percent of the bytes)')
    p.add_argument('--face_det_precision', default='fp32', choices=['fp32', 'bf16'],
                   help='Face detector arithmetic: fp32 (default, matches the reference) or bf16 storage (faster; boxes move by '
                        'about what bf16 rounding alone moves them)')
    add_det_scale_flag(p)
    p.add_argument('--out_codec', default='raw', choices=['raw', 'mjpg'],
                   help='Video stream of --outfile: raw (default, uncompressed 24-bit BGR) or mjpg (Motion-JPEG, what '
                        "cv2.VideoWriter_fourcc(*'MJPG') writes: every frame is JPEG-encoded on the device and only the files' "
                        'bytes come back; lossy, about a tenth of the size at quality 95)')
    p.add_argument('--out_quality', default=95, type=int, help='JPEG quality of --out_codec mjpg, 1..100 (default 95)')
    add_blend_flags(p)
    add_color_match_flag(p)
    add_hold_flag(p)
    add_track_flags(p)
    add_scene_flag(p)
    add_stride_flag(p)
    return p


def add_scene_flag(p):
    """`--scene_cuts THRESH` on a command's parser (face_detection/scene.py holds the rule): absent by default"""
    from .face_detection.scene import add_scene_flag as add
    add(p)


def add_stride_flag(p):
    """`--face_det_stride N` on a command's parser (face_detection/stride.py holds the rule): 1 by default"""
    from .face_detection.stride import add_stride_flag as add
    add(p)


def add_hold_flag(p):
    """`--no_face_hold G` on a command's parser (face_detection/many.py holds the rule's host side): absent by default"""
    from .face_detection.many import add_hold_flag as add
    add(p)


def add_track_flags(p):
    """`--face_track PICK` and its companions on a command's parser (face_detection/track.py holds the rule): absent by default"""
    from .face_detection.track import add_track_flags as add
    add(p)


def _track_kw(face_track):
    """the keyword `face_detect`, `detect_many` and `LipsyncStreams` take for `face_track`, checked first: none for None (as
    `_hold_kw`)"""
    from .face_detection.track import track_kw
    return track_kw(face_track)


def _hold_kw(no_face_hold):
    """the keyword `face_detect`, `detect_many` and `LipsyncStreams` take for `no_face_hold`, checked first: none for None, so the
    default path is called with the same arguments as before the option (as `_precision_kw`)"""
    from .face_detection.many import check_hold
    hold = check_hold(no_face_hold)
    return {} if hold is None else {"no_face_hold": hold}


CLI_PRECISION = {"fp32": "f32", "bf16": "bf16"}     # --precision / --face_det_precision value -> the `precision=` of the API


parser = build_parser()
cli_parser = build_cli_parser()


def is_image_path(path):
    """inference.py:56 / 185: `path.split('.')[1] in ['jpg', 'png', 'jpeg']`, applied to the file name.  On the whole path the
    test reads past a dot in a directory name (`/tmp/run.v2/face.png` -> 'v2/face'), and an image becomes a video; on the file
    name it is the reference's test, unchanged (`x.png.avi` is an image, a name without a dot raises IndexError)."""
    return os.path.basename(path).split('.')[1] in ['jpg', 'png', 'jpeg']


def parse_args(argv=None):
    """inference.py:53-57: parse (the reference's flags + `--precision` and `--face_det_precision`), then `img_size = 96` and `static = True` for an image
    input"""
    a = cli_parser.parse_args(argv)
    a.img_size = img_size
    if os.path.isfile(a.face) and is_image_path(a.face):
        a.static = True
    return a


# The reference parses sys.argv at import time into a module global that `datagen` / `face_detect` read (inference.py:53).  A
# library cannot do that; `args` holds the defaults until `main()` (or a caller) replaces it.
args = cli_parser.parse_args(['--checkpoint_path', '', '--face', '', '--audio', ''])
args.img_size = img_size
device = 'cuda'      # inference.py:157 (`'cuda' if torch.cuda.is_available() else 'cpu'`): this engine has no CPU path


def mel_chunk_starts(n_mel_frames, fps):
    """inference.py:231-240: start column of each 16-frame window; the tail window is re-anchored at the end.
    Pure host integer arithmetic (double multiply + truncation), bit-exact by construction."""
    mel_idx_multiplier = 80. / fps
    starts = []
    i = 0
    while True:
        start_idx = int(i * mel_idx_multiplier)
        if start_idx + mel_step_size > n_mel_frames:
            starts.append(n_mel_frames - mel_step_size)
            return starts
        starts.append(start_idx)
        i += 1


class Wav2LipRunner:
    """Device-resident replacement of the body of the reference's batch loop for one model and batch size."""

    def __init__(self, model, batch_size=128, lane=0, precision="f32", blend=None, color_match=None):
        from .models.wav2lip import check_precision
        self.model = model
        self.batch_size = batch_size
        self.lane = lane
        self.precision = check_precision(precision)
        self.blend = check_blend(blend)      # None: the reference's paste; (feather, top): `run_frames` / `run_rows` blend
        self.color_match = check_color_match(color_match)   # None, or "mean" / "full": `run_batch` matches its frames to the faces
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("wav2lip_amd.inference: the model must be on a HIP device (no CPU path)")
        self.lib = _lib.load()
        self._out_u8 = {}

    def _graph(self, n):
        return self.model.graph(n, img_size, img_size, self.device, lane=self.lane, precision=self.precision)

    def run_batch(self, faces_u8, mel_windows=None, mel=None, starts=None, out=None, mel_rows=None):
        """faces_u8: torch uint8 [n,96,96,3] on the device.  Audio either as ready windows `mel_windows`
        float32 [n,80,16], or as the full spectrogram `mel` [80,T] plus int32 `starts` [n] (device tensors), or as
        `mel_rows`: a device uint8 tensor holding n w2l_mel_row entries (one spectrogram per row, wav2lip_amd/multiclip.py).
        Returns torch uint8 [n,96,96,3] (BGR order preserved), valid until the next call; `out` (a contiguous uint8
        [n,96,96,3] device tensor, e.g. the send slot of the multi-GPU frame gatherer) receives the frames instead.  With
        `color_match` one more launch matches the frames to `faces_u8` in place (w2l_color_match_u8), whatever consumes them."""
        n = faces_u8.shape[0]
        cap = self.model.MAX_PLAN_BATCH
        if n > cap:     # one NHWC buffer must stay below 2 GiB: run equal chunks and concatenate the uint8 frames
            parts = []
            for lo in range(0, n, cap):
                hi = min(n, lo + cap)
                rows_kw = {} if mel_rows is None else {"mel_rows": mel_rows[lo * MEL_ROW_BYTES:hi * MEL_ROW_BYTES]}
                parts.append(self.run_batch(faces_u8[lo:hi], None if mel_windows is None else mel_windows[lo:hi], mel,
                                            None if starts is None else starts[lo:hi].contiguous(), **rows_kw).clone())
            allf = torch.cat(parts, dim=0)
            if out is not None:
                out.copy_(allf)
                return out
            return allf
        g = self._graph(n)
        faces_u8 = faces_u8.contiguous()
        g.pack_faces(faces_u8)
        g.load_mel(mel, starts, windows=mel_windows, rows=mel_rows)
        g.run()
        if out is not None:
            if out.dtype != torch.uint8 or tuple(out.shape) != (n, img_size, img_size, 3) or not out.is_cuda or not out.is_contiguous():
                raise RuntimeError("run_batch: `out` must be a contiguous uint8 [%d,%d,%d,3] tensor on the HIP device" % (n, img_size, img_size))
        else:
            out = self._out_u8.get(n)
        if out is None:
            out = torch.empty((n, img_size, img_size, 3), dtype=torch.uint8, device=self.device)
            self._out_u8[n] = out
        g.frames_into(out)
        if self.color_match is not None:
            check(self.lib.w2l_color_match_u8(current_stream(), n, ptr(out), ptr(faces_u8), img_size,
                                              COLOR_MATCH_MODES[self.color_match], ptr(out)), "color_match_u8")
        self._last = g
        return out

    def last_pred_nchw(self):
        return self._last.output_nchw()

    def run_rows(self, n, frame_rows, mel_rows, max_frame_pixels):
        """`run_frames` for rows that each name their own frame (wav2lip_amd/multiclip.py): `frame_rows` / `mel_rows` are device
        uint8 tensors holding n w2l_frame_row / w2l_mel_row entries.  Crops and resizes every row's face, runs the batch and
        composes every row's output frame at its `dst` address in one pass (gen_videos_from_filelist.py:85-95, :221-227)."""
        s = current_stream()
        faces = torch.empty((n, img_size, img_size, 3), dtype=torch.uint8, device=self.device)
        check(self.lib.w2l_crop_resize_rows_u8(s, n, ptr(frame_rows), img_size, ptr(faces)), "crop_resize_rows_u8")
        pred = self.run_batch(faces, mel_rows=mel_rows)
        if self.blend is None:
            check(self.lib.w2l_compose_rows_u8(s, n, ptr(pred), img_size, ptr(frame_rows), int(max_frame_pixels)), "compose_rows_u8")
        else:
            check(self.lib.w2l_compose_blend_rows_u8(s, n, ptr(pred), img_size, ptr(frame_rows), int(max_frame_pixels),
                                                     self.blend[0], blend_top_q8(self.blend[1])), "compose_blend_rows_u8")
        return pred

    def run_frames(self, frames, frame_idx, boxes, mel_windows=None, mel=None, starts=None):
        """Full-frame variant of `run_batch` (inference.py:121-126 + :259-271).  frames: torch uint8 [F,H,W,3] on the
        device; frame_idx: n frame numbers; boxes: n (y1, y2, x1, x2) face boxes.  Crops and resizes the faces to 96x96,
        runs the batch, resizes each generated crop to its box and pastes it into a copy of its frame (with `blend`: blends it
        in, w2l_resize_blend_u8).  Returns torch uint8 [n,H,W,3] (a fresh tensor)."""
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_cuda:
            raise RuntimeError("run_frames: frames must be a uint8 [F,H,W,3] tensor on the HIP device")
        frames = frames.contiguous()
        F_, H, W = frames.shape[:3]
        boxes = validate_boxes(boxes, H, W)
        n = len(boxes)
        idx = [int(i) for i in frame_idx]
        if len(idx) != n or any(i < 0 or i >= F_ for i in idx):
            raise ValueError("run_frames: frame_idx must hold one valid frame number per box")
        s = current_stream()
        boxes_dev = torch.tensor(boxes, dtype=torch.int32, device=self.device)
        idx_dev = torch.tensor(idx, dtype=torch.int32, device=self.device)
        faces = torch.empty((n, img_size, img_size, 3), dtype=torch.uint8, device=self.device)
        check(self.lib.w2l_crop_resize_u8(s, n, ptr(frames), H, W, ptr(idx_dev), ptr(boxes_dev), img_size, ptr(faces)),
              "crop_resize_u8")
        pred = self.run_batch(faces, mel_windows=mel_windows, mel=mel, starts=starts)
        out = frames.index_select(0, idx_dev.long())            # frame_batch copies (inference.py:131)
        max_px = max((y2 - y1) * (x2 - x1) for y1, y2, x1, x2 in boxes)
        if self.blend is None:
            check(self.lib.w2l_resize_paste_u8(s, n, ptr(pred), img_size, ptr(boxes_dev), None, ptr(out), H, W, max_px),
                  "resize_paste_u8")
        else:
            check(self.lib.w2l_resize_blend_u8(s, n, ptr(pred), img_size, ptr(boxes_dev), None, ptr(out), H, W, max_px,
                                               self.blend[0], blend_top_q8(self.blend[1])), "resize_blend_u8")
        return out


class PipelinedRunner:
    """`depth` Wav2LipRunner lanes, each with its own generator buffers and HIP stream: successive batches alternate between
    the lanes, so the low-occupancy layers of one batch overlap the chip-filling layers of the others.  This is the loop
    bench.py times (`--pipeline` = depth; `lipsync` / `main` run LIPSYNC_DEPTH).  `submit` enqueues a batch and returns a
    ticket; `result(ticket)` makes the caller's stream wait for that batch and returns its uint8 frames (valid until the lane is
    reused `depth` submits later)."""

    def __init__(self, model, batch_size=128, depth=2, precision="f32", blend=None, color_match=None):
        self.lanes = [Wav2LipRunner(model, batch_size, lane=k, precision=precision, **_blend_kw(blend), **_color_kw(color_match))
                      for k in range(depth)]
        dev = self.lanes[0].device
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(depth)]
        self.depth = depth
        self.n = 0

    def submit(self, faces_u8, mel_windows=None, mel=None, starts=None, frames=None, frame_idx=None, boxes=None, out=None, *,
               rows=None, upload=None, download=None, keep=()):
        """`rows=(n, frame_rows, mel_rows, max_frame_pixels)` runs `Wav2LipRunner.run_rows` on the lane; `upload` / `download`
        are (destination, source) tensor pairs copied on the lane's stream before / after the batch (pinned host memory on the
        host side: the copies overlap the other lanes); `keep` are further device tensors the lane reads."""
        k = self.n % len(self.lanes)
        self.n += 1
        st = self.streams[k]
        st.wait_stream(torch.cuda.current_stream())       # inputs were produced on the caller's stream
        extra = tuple(keep) + tuple(t for pair in (upload, download) if pair is not None for t in pair)
        if rows is not None:
            extra += (rows[1], rows[2])
        for t in (faces_u8, mel_windows, mel, starts, frames) + extra:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(st)                        # the allocator must not recycle them while the lane still reads
        with torch.cuda.stream(st):
            if upload is not None:
                upload[0].copy_(upload[1], non_blocking=True)
            if rows is not None:
                out = self.lanes[k].run_rows(*rows)
            elif frames is not None:
                out = self.lanes[k].run_frames(frames, frame_idx, boxes, mel_windows=mel_windows, mel=mel, starts=starts)
            else:
                out = self.lanes[k].run_batch(faces_u8, mel_windows=mel_windows, mel=mel, starts=starts, out=out)
            if download is not None:
                download[0].copy_(download[1], non_blocking=True)
            done = torch.cuda.Event()
            done.record(st)
        return (out, done)

    @staticmethod
    def result(ticket):
        out, done = ticket
        torch.cuda.current_stream().wait_event(done)
        return out


def validate_boxes(boxes, H, W):
    """(y1, y2, x1, x2) per item, as the reference slices frames (inference.py:87,121): must be non-empty and inside the
    frame — numpy would silently clip an overhanging slice and the later paste would then fail on the shape mismatch"""
    out = []
    for b in boxes:
        y1, y2, x1, x2 = (int(v) for v in b)
        if not (0 <= y1 < y2 <= H and 0 <= x1 < x2 <= W):
            raise ValueError("face box (y1=%d, y2=%d, x1=%d, x2=%d) is empty or outside the %dx%d frame" % (y1, y2, x1, x2, H, W))
        out.append((y1, y2, x1, x2))
    if not out:
        raise ValueError("no face boxes")
    return out


def resize_faces_u8(faces, size=img_size):
    """`cv2.resize(face, (size, size))` of inference.py:126 for a list of uint8 BGR crops of ANY sizes, on the device
    (w2l_crop_resize_u8: OpenCV's fixed-point INTER_LINEAR, csrc/resize.hip).  Returns numpy uint8 [n, size, size, 3]."""
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    out = np.empty((len(faces), size, size, 3), dtype=np.uint8)
    by_shape = {}
    for i, f in enumerate(faces):
        f = np.asarray(f)
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError("face crops must be non-empty uint8 [h, w, 3] arrays, got %s %s" % (f.dtype, f.shape))
        if f.shape[:2] == (size, size):
            out[i] = f
        else:
            by_shape.setdefault(f.shape[:2], []).append(i)
    for (h, w), idxs in by_shape.items():          # one launch per distinct crop size (a video's boxes share few sizes)
        src = torch.from_numpy(np.stack([np.ascontiguousarray(faces[i]) for i in idxs])).to(dev)
        boxes = torch.tensor([[0, h, 0, w]] * len(idxs), dtype=torch.int32, device=dev)
        dst = torch.empty((len(idxs), size, size, 3), dtype=torch.uint8, device=dev)
        check(lib.w2l_crop_resize_u8(current_stream(), len(idxs), ptr(src), h, w, None, ptr(boxes), size, ptr(dst)),
              "crop_resize_u8")
        out[idxs] = dst.cpu().numpy()
    return out


def datagen(frames, mels):
    """The reference's HOST-format batch generator (inference.py:108-154), written from its contract: called as
    `datagen(full_frames.copy(), mel_chunks)` and driven by the module-level `args` (box / static / img_size / wav2lip_batch_size,
    and through `face_detect` pads / nosmooth / face_det_batch_size), it yields per batch of at most `wav2lip_batch_size` chunks

        img_batch     float64 [b, img_size, img_size, 6]   channels 0-2: the resized face with its lower half zeroed, 3-5: the face; / 255.
        mel_batch     float32 [b, 80, 16, 1]
        frame_batch   list of b frame copies               chunk i pairs with frame i % len(frames) (frame 0 when args.static)
        coords_batch  list of b (y1, y2, x1, x2)

    Faces come from `face_detect` (all frames, or the first one when static) or are the `--box` crop of every frame; the
    `cv2.resize(face, (img_size, img_size))` of every face is the device kernel (w2l_crop_resize_u8).  float64 images cannot come out
    of the fp32 device pack, so this generator is for callers that consume the reference's numpy batches; `main()` / `lipsync()` keep
    uint8 crops on the device (`datagen_u8` + `Wav2LipRunner`), which is the measured path."""
    a = args
    if a.box[0] == -1:
        detections = face_detect(frames if not a.static else [frames[0]])
    else:
        print('Using the specified bounding box instead of face detection...')
        y1, y2, x1, x2 = a.box
        detections = [[f[y1: y2, x1:x2], (y1, y2, x1, x2)] for f in frames]
    size, per_batch = a.img_size, a.wav2lip_batch_size
    for lo in range(0, len(mels), per_batch):
        chunk = mels[lo:lo + per_batch]
        which = [0 if a.static else i % len(frames) for i in range(lo, lo + len(chunk))]
        faces = resize_faces_u8([detections[j][0] for j in which], size)          # uint8 [b, size, size, 3]
        masked = faces.copy()
        masked[:, size // 2:] = 0
        mel_batch = np.asarray(chunk)
        yield (np.concatenate((masked, faces), axis=3) / 255., mel_batch.reshape(mel_batch.shape + (1,)),
               [frames[j].copy() for j in which], [detections[j][1] for j in which])


def datagen_u8(frames, mels, batch_size=128, static=False, box=None, first=0):
    """the device-path batching of inference.py:108-154 for faces that are already 96x96: yields (faces_u8 [b,96,96,3],
    mel items [b], frame_batch, coords_batch); the masking / concat / `/255.` happen in w2l_datagen_pack on the device.
    `frames` are HxWx3 uint8 images; with `box=(y1,y2,x1,x2)` the face is the box crop.  Other crop sizes take the
    frames-on-device route of `lipsync` / `Wav2LipRunner.run_frames` (crop + resize + paste-back on the device).
    `first`: the clip position of mels[0] (a rank's shard of the mel chunks starts there; frame i of the clip pairs with
    frames[i % len(frames)] as in the reference)."""
    img_batch, mel_batch, frame_batch, coords_batch = [], [], [], []
    for i, m in enumerate(mels, start=first):
        idx = 0 if static else i % len(frames)
        frame = frames[idx]
        if box is not None:
            y1, y2, x1, x2 = box
        else:
            y1, y2, x1, x2 = 0, frame.shape[0], 0, frame.shape[1]
        face = frame[y1:y2, x1:x2]
        if face.shape[:2] != (img_size, img_size):
            raise ValueError("datagen_u8 batches pre-sized %dx%d faces (got %s): use lipsync() / Wav2LipRunner.run_frames, which "
                             "crop and resize on the device" % (img_size, img_size, face.shape[:2]))
        img_batch.append(face)
        mel_batch.append(m)
        frame_batch.append(frame.copy())
        coords_batch.append((y1, y2, x1, x2))
        if len(img_batch) >= batch_size:
            yield np.asarray(img_batch), np.asarray(mel_batch), frame_batch, coords_batch
            img_batch, mel_batch, frame_batch, coords_batch = [], [], [], []
    if img_batch:
        yield np.asarray(img_batch), np.asarray(mel_batch), frame_batch, coords_batch


LIPSYNC_DEPTH = 4     # batches in flight in lipsync() / main(): the depth bench.py measures (bench.py --pipeline)


def _precision_kw(precision):
    """the keyword a runner, a detector or a SyncNet call takes for `precision`, checked first (engine.check_precision): none for
    "f32", so the default path is called with the same arguments as before the option, and an object that knows nothing of the
    switch keeps working on it"""
    from .engine import check_precision
    return {} if check_precision(precision) == "f32" else {"precision": precision}


def lipsync(model, frames, wav, fps=25., batch_size=128, static=False, box=None, ranks=None, depth=None, precision="f32",
            blend=None, color_match=None):
    """End-to-end body of inference.py:main for in-memory inputs: returns the list of output frames (uint8).
    `precision`: "f32" (default) or "bf16" - the generator's arithmetic (Wav2LipRunner); everything else is the same.
    `blend`: None (default, the reference's paste) or (feather, top), the feathered mouth-region paste (`check_blend`).  It is a
    device paste: frames of one shape and a `box` (a 96x96 one included); anything else raises ValueError before any device work.
    `color_match`: None (default), "mean" or "full" (`check_color_match`): every prediction is matched to its crop on the device
    before either paste, the host one included.

    `ranks` (sharding.init_from_env(), one process per GPU): the mel chunks are cut into contiguous per-rank shards
    (sharding.shard_range), every rank runs ITS chunks through its own runner with the replicated weights, and the generated
    frames are all-gathered in frame order to rank 0 (sharding.gather_shards_to_writer), which alone returns them - every other
    rank returns None (the reference's loop, inference.py:249-272, is single-process)."""
    from .models.wav2lip import check_precision
    check_precision(precision)
    blend = check_blend(blend)
    color_kw = _color_kw(color_match)
    if blend is not None and (box is None or len({tuple(f.shape) for f in frames}) != 1):
        raise ValueError("blend=%r needs the device paste: frames of one shape and a `box`; the host paste of pre-sized faces has "
                         "no blend" % (blend,))
    dev = next(model.parameters()).device
    mel = audio.melspectrogram_device(wav, dev)
    if bool(torch.isnan(mel).any()):
        raise ValueError("Mel contains nan! Using a TTS voice? Add a small epsilon noise to the wav file and try again")
    starts = mel_chunk_starts(mel.shape[1], fps)
    frames = frames[:len(starts)] if not static else frames
    world = 1 if ranks is None or ranks.dist is None else ranks.world
    rank = 0 if world == 1 else ranks.rank
    from . import sharding
    first, last = sharding.shard_range(len(starts), rank, world)
    # later batches are enqueued before batch i is collected; the default precision constructs the runner exactly as before
    runner = PipelinedRunner(model, batch_size, depth=depth or LIPSYNC_DEPTH, **_precision_kw(precision), **_blend_kw(blend),
                             **color_kw)
    out_frames = []
    starts_dev = torch.tensor(starts, dtype=torch.int32, device=dev)
    shapes = {tuple(f.shape) for f in frames}
    if world > 1 and len(shapes) != 1:
        raise ValueError("sharded inference gathers frames of ONE shape (a video); got %d shapes" % len(shapes))
    pending = []
    if len(shapes) == 1 and box is not None and (blend is not None or (box[1] - box[0], box[3] - box[2]) != (img_size, img_size)):
        # faces that need resizing (or blending): keep the frames on the device, crop/resize/paste there (inference.py:121-126, 270-271)
        frames_dev = torch.from_numpy(np.stack(frames)).to(dev)
        for lo in range(first, last, batch_size):
            n = min(batch_size, last - lo)
            idx = [0 if static else (lo + j) % len(frames) for j in range(n)]
            pending.append(runner.submit(None, mel=mel, starts=starts_dev[lo:lo + n].contiguous(), frames=frames_dev, frame_idx=idx,
                                         boxes=[box] * n))
            if len(pending) >= runner.depth:
                out_frames += list(runner.result(pending.pop(0)).cpu().numpy())
        while pending:
            out_frames += list(runner.result(pending.pop(0)).cpu().numpy())
    else:
        def collect(item):
            ticket, frame_batch, coords = item
            u8 = runner.result(ticket).cpu().numpy()
            for p, f, c in zip(u8, frame_batch, coords):
                y1, y2, x1, x2 = c
                f[y1:y2, x1:x2] = p
                out_frames.append(f)

        pos = first
        for faces, _, frame_batch, coords in datagen_u8(frames, starts[first:last], batch_size, static, box, first=first):
            n = len(faces)
            ticket = runner.submit(torch.from_numpy(faces).to(dev), mel=mel, starts=starts_dev[pos:pos + n].contiguous())
            pos += n
            pending.append((ticket, frame_batch, coords))
            if len(pending) >= runner.depth:
                collect(pending.pop(0))
        while pending:
            collect(pending.pop(0))
    if world == 1:
        return out_frames
    local = np.stack(out_frames) if out_frames else None
    allf = sharding.gather_shards_to_writer(ranks.dist, local, len(starts), rank, world, device=dev, chunk=batch_size)
    return list(allf) if allf is not None else None


def write_result(outfile, frames, fps, audio_path=None):
    """inference.py:256-257 (`cv2.VideoWriter('temp/result.avi', DIVX, fps, (w, h))`), :272 (`out.write(f)`), :274 and the mux of
    :276-277 (`ffmpeg -y -i <audio> -i temp/result.avi <outfile>`) in one step: the generated frames and the driving audio go into
    one AVI (lossless BGR video, PCM16 audio).  `audio_path`: the WAV that drove the lips (any rate; stored as it is)."""
    from . import container
    pcm, sr = None, 16000
    if audio_path is not None:
        from scipy.io import wavfile
        sr, pcm = wavfile.read(audio_path)
        if pcm.dtype != np.int16:
            pcm = np.clip(np.round(audio._pcm_to_float32(pcm) * 32768.0), -32768, 32767).astype(np.int16)
    container.write_avi(outfile, frames, fps, audio=pcm, audio_sr=sr)
    return outfile


# ---------------------------------------------------------------- face detection front end (inference.py:59-104)
def get_smoothened_boxes(boxes, T):
    """inference.py:59-66: box i becomes the mean of boxes i .. i+T-1, the last T-1 boxes the mean of the last T; done in
    place and in order on the integer array face_detect builds, so a window sees the boxes already smoothed before it and
    every mean is truncated on assignment (both are the reference's behaviour, kept)."""
    n = len(boxes)
    for i in range(n):
        window = slice(i, i + T) if i + T <= n else slice(n - T, None)      # n < T: a negative start wraps, as there
        boxes[i] = boxes[window].mean(axis=0)
    return boxes


OOM_ERROR = 'Image too big to run face detection on GPU. Please use the --resize_factor argument'      # inference.py:81


def halving(run, batch_size, error=OOM_ERROR):
    """inference.py:75-88: `run(batch_size)`; a RuntimeError of the detector (out of device memory on a large frame) halves the
    batch, prints the reference's message and starts over, down to single frames, where it is the RuntimeError `error`: the
    reference's text, or a command's own"""
    while True:
        try:
            return run(batch_size)
        except RuntimeError:
            if batch_size == 1:
                raise RuntimeError(error)
            batch_size //= 2
            print('Recovering from OOM error; New batch size: {}'.format(batch_size))


def clip_rects(images, detector, batch_size, track=None, scene=None, det_stride=1, ranks=None):
    """inference.py:75-88 and every option in front of the finish: (one rect (x1, y1, x2, y2) or None per frame, the shots [(a, b)]
    of the clip - [(0, n)] without `scene`), in batches under `halving`.

    Plain, the batches go to the detector as numpy arrays.  With `ranks` every rank detects the frames of its contiguous shard and
    the per-frame rects (four numbers each) are all-gathered: the box smoothing that follows needs them all, on every rank, in frame
    order.

    `track` (face_detection/track.py): the candidates of every batch go into device arenas
    (`FaceAlignment.cands_for_batch`), ONE w2l_face_track_segments launch over one segment per shot - a fresh track at every cut -
    follows the face and ONE copy brings rects, flags and status back.  A frame the device does not decide (RECT_HOST) sends the
    whole clip through the host statement of the same rule: `get_candidates_for_batch` (which runs `host_top_rects` on such a frame)
    and `host_track_shots` (for one shot, `host_track`).

    `scene` (face_detection/scene.py): every batch is uploaded ONCE as a device tensor; w2l_frame_hist_rows reads it
    into the clip's signature arena and the detector takes the same tensor.  After the last batch ONE w2l_scene_cuts launch and one
    small copy give the cut flags.

    `det_stride` N > 1 (face_detection/stride.py): the detector sees the key frames of the clip - of every shot, so
    under `scene` the cuts come first, a pass of signatures over every frame - and `host_stride_fill` gives the frames between them
    their rects.  Plain, all shots' keys share batches; under `track` a shot goes at a time: a fresh track each, stepping from key to
    key."""
    n = len(images)
    if det_stride > 1 and n:
        from .face_detection.many import _host_shots
        from .face_detection.stride import host_stride_fill, host_stride_fill_shots, key_frames, shot_key_frames
        shots = [(0, n)] if scene is None else halving(lambda size: _host_shots(detector, images, size, scene), batch_size)
        if track is None:
            key_rects, _ = clip_rects([images[i] for i in shot_key_frames(shots, det_stride)], detector, batch_size)
            return host_stride_fill_shots(key_rects, shots, det_stride), shots
        rects = []
        for a, b in shots:
            key_rects, _ = clip_rects([images[a + i] for i in key_frames(b - a, det_stride)], detector, batch_size, track)
            rects += host_stride_fill(key_rects, b - a, det_stride)
        return rects, shots
    if ranks is not None and ranks.dist is not None and ranks.world > 1:
        from . import sharding
        lo, hi = sharding.shard_range(n, ranks.rank, ranks.world)
        mine = clip_rects(images[lo:hi], detector, batch_size)[0] if hi > lo else []
        parts = [None] * ranks.world
        ranks.dist.all_gather_object(parts, mine)
        return [r for part in parts for r in part], [(0, n)]
    if n == 0:
        return [], [] if scene is not None else [(0, 0)]
    from .face_detection.s3fd import RECT_FOUND, RECT_HOST
    from .face_detection.scene import SIG_WORDS, clip_cuts, frame_signatures, host_track_shots, split_shots
    from .face_detection.track import TRACK_SEGMENT, track_segments

    def run(batch_size):
        rects, shots = [], [(0, n)]
        if track is not None or scene is not None:
            dev = torch.device(detector.device)
        if scene is not None:
            sig = torch.empty((n, SIG_WORDS), dtype=torch.int32, device=dev)
        if track is not None:
            K = track.cands
            cands = torch.empty((n, K, 4), dtype=torch.int32, device=dev)
            ncand = torch.empty((n,), dtype=torch.int32, device=dev)
            cflags = torch.empty((n,), dtype=torch.int32, device=dev)
        for lo in range(0, n, batch_size):
            batch = np.array(images[lo:lo + batch_size])
            if scene is not None:                            # uploaded once: the signatures and the detector read the same tensor
                batch = torch.from_numpy(np.ascontiguousarray(batch)).to(dev)
                frame_signatures(batch, sig, lo)
            if track is None:
                rects += detector.get_detections_for_batch(batch)
            else:
                detector.cands_for_batch(batch, cands, ncand, cflags, lo, K)
        if scene is not None:
            shots = split_shots(n, clip_cuts(sig, *images[0].shape[:2], scene)[0])
        if track is None:
            return rects, shots
        seg = np.zeros(len(shots), dtype=TRACK_SEGMENT)
        for k, (a, b) in enumerate(shots):
            seg[k] = (a, b - a, -1, 0)
        segs = torch.from_numpy(seg.view(np.uint8)).to(dev)
        out = torch.empty(5 * n + len(shots), dtype=torch.int32, device=dev)       # rects [n][4], flags [n], status [shots]: one copy back
        track_segments(segs, len(shots), cands, ncand, cflags, track, out[:4 * n].view(n, 4), out[4 * n:5 * n], out[5 * n:])
        res = out.cpu().numpy()
        rows, flags, status = res[:4 * n].reshape(n, 4), res[4 * n:5 * n], res[5 * n:]
        if status.any():
            raise AssertionError("w2l_face_track_segments did not follow the clip's segment (status %d)" % status[0] if scene is None else
                                 "w2l_face_track_segments did not follow a shot's segment (status %s)" % status.tolist())
        if (flags == RECT_HOST).any():
            per_frame = []
            for lo in range(0, n, batch_size):
                per_frame += detector.get_candidates_for_batch(np.array(images[lo:lo + batch_size]), K)
            return host_track_shots(per_frame, shots, track), shots
        return [tuple(int(v) for v in r) if f == RECT_FOUND else None for r, f in zip(rows, flags)], shots

    return halving(run, batch_size)


def _detect_rects(images, detector, batch_size, ranks=None, det_stride=1):
    """`clip_rects` without a track or a scene: one rect (or None) per frame"""
    return clip_rects(images, detector, batch_size, det_stride=det_stride, ranks=ranks)[0]


def _track_rects(images, detector, batch_size, track, det_stride=1):
    """`clip_rects` under tracked face selection: one rect (or None) per frame"""
    return clip_rects(images, detector, batch_size, track, det_stride=det_stride)[0]


def _shot_rects(images, detector, batch_size, track, scene, det_stride=1):
    """`clip_rects` under scene-cut detection: (one rect or None per frame, the shots [(a, b)] of the clip)"""
    return clip_rects(images, detector, batch_size, track, scene, det_stride)


def _det_scale_kw(det_scale):
    """detector keyword for a reduced detection frame: scale 1 builds the detector with the same arguments as before the option"""
    return {} if det_scale == 1 else {"det_scale": det_scale}


def detector_from_args(args, device, state_dict=None):
    """the FaceAlignment of a parsed command line on `device`: `--face_det_precision` and `--face_det_scale`, each passed on only
    when it is not the default; `state_dict` (S3FD weights) replaces face_detection/s3fd.pth"""
    from . import face_detection
    return face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device=str(device), state_dict=state_dict,
                                        **_precision_kw(CLI_PRECISION[args.face_det_precision]),
                                        **_det_scale_kw(getattr(args, 'face_det_scale', 1)))


def detect_kw_from_args(args):
    """the `no_face_hold=` / `face_track=` keywords of `face_detect`, `detect_many` and `LipsyncStreams` for a parsed command line,
    and the `scene_cuts=` and `det_stride=` of the first two (a parser of the live path has no such flags): none for an absent
    flag (for `--face_det_stride 1`); a lone `--face_track_*` flag is a ValueError"""
    from .face_detection.scene import scene_from_args, scene_kw
    from .face_detection.stride import stride_from_args
    from .face_detection.track import track_from_args
    return {**_hold_kw(getattr(args, 'no_face_hold', None)), **_track_kw(track_from_args(args)), **scene_kw(scene_from_args(args)),
            **stride_from_args(args)}


def face_detect(images, detector=None, pads=None, nosmooth=None, batch_size=None, ranks=None, precision=None, det_scale=None,
                no_face_hold=None, face_track=None, scene_cuts=None, det_stride=None):
    """inference.py:68-104: S3FD boxes per frame (HIP detector), padding, temporal smoothing; returns
    [[face crop, (y1, y2, x1, x2)], ...].  Called as the reference calls it - `face_detect(images)` - pads / nosmooth /
    face_det_batch_size come from the module-level `args` and the detector is built as inference.py:69-70 does
    (`face_detection.FaceAlignment(LandmarksType._2D, flip_input=False, device=device)`, weights `face_detection/s3fd.pth`);
    a ready `wav2lip_amd.face_detection.FaceAlignment` may be passed instead.  `precision` ("f32" or "bf16") selects the
    detector's arithmetic; None means: a passed detector keeps its own, a built one takes the module-level
    `args.face_det_precision` (fp32 when absent).  `det_scale` (1..8) is the detector's frame size, 1/det_scale of the frames'
    (the boxes come back in full-frame coordinates; pads, clipping and smoothing below are on those); None follows the same rule
    with `args.face_det_scale` (1 when absent).

    `no_face_hold`: None (default) raises the reference's ValueError at a frame without a face.  An int G in 0..250 switches the
    pass-through rule on instead (not the reference's behaviour): such a frame keeps the last detected rect for up to
    G frames (no look-ahead), beyond that - and before the first detection - it is a gap frame whose entry is [None, None], and
    every run of boxed frames is padded, clipped and smoothed as a clip of its own (`face_detection.many.host_boxes_runs` states
    the same for one frame shape).  A single frame without a face is still the ValueError.

    `face_track`: None (default) takes the detector's best-scoring box of every frame, as the reference does.  A pick name or a
    `face_detection.track.FaceTrack` follows one face through the clip instead (not the reference's behaviour when
    more than one face is in the picture): the rect of a frame is the candidate that overlaps the tracked face's last rect most, a
    frame on which the track is lost (possible with `reseed` > 0 only) is a frame without a face, and everything after the
    rects - the strict ValueError or `no_face_hold`, pads, smoothing - is as without it.  Not with `ranks` of more than one
    process: the track looks back over the frames of other shards.

    `scene_cuts`: None (default) takes the clip as one continuous take, as the reference does.  A threshold in [1/256, 1) or a
    `face_detection.scene.SceneCuts` splits it into shots where the colour histogram of a frame differs from the previous frame's by
    more than the threshold (not the reference's behaviour), and every shot is handled as a clip of its frames alone:
    a fresh track at its start, a hold that does not look back past it, pads, clipping and smoothing per shot (a shot shorter than
    5 frames takes the wrapped short-clip window).  Without a hold a frame without a face in any shot is still the ValueError.  Not
    with `ranks` of more than one process: a cut compares a frame with the one before it, which may lie in another shard.

    `det_stride`: None or 1 (default) shows every frame to the detector, as the reference does.  An int N in 2..32 shows it the key
    frames 0, N, 2N, ... and the last one of the clip - with `scene_cuts`, of every shot - and interpolates the rects of the frames
    between two detected key frames (face_detection/stride.py; not the reference's behaviour, and not
    accuracy-neutral).  A missed key frame leaves 2N - 1 frames without a face; everything after the rects is as without it.  With
    `face_track` the track steps from key frame to key frame: `reseed` counts key frames, `min_iou` is unchanged.  Not with `ranks`
    of more than one process: a frame is interpolated from key frames of other shards."""
    from .face_detection.many import boxed_runs, check_hold, hold_fill
    from .face_detection.stride import check_stride, stride_kw
    from .face_detection.scene import check_scene
    from .face_detection.track import check_track
    from .face_detection.s3fd import check_det_scale
    from .models.wav2lip import check_precision
    hold = check_hold(no_face_hold)
    track = check_track(face_track)
    if track is not None and ranks is not None and ranks.dist is not None and ranks.world > 1:
        raise ValueError("face_track runs on one GPU: the track looks back over the frames of other shards")
    scene = check_scene(scene_cuts)
    if scene is not None and ranks is not None and ranks.dist is not None and ranks.world > 1:
        raise ValueError("scene_cuts runs on one GPU: a cut compares a frame with the one before it, in another shard")
    skw = stride_kw(check_stride(det_stride))
    if skw and ranks is not None and ranks.dist is not None and ranks.world > 1:
        raise ValueError("det_stride runs on one GPU: a frame is interpolated from key frames of other shards")
    if precision is not None:
        check_precision(precision)
    if det_scale is not None:
        det_scale = check_det_scale(det_scale)
    if detector is None:
        from . import face_detection
        if precision is None:
            precision = check_precision(CLI_PRECISION[getattr(args, "face_det_precision", "fp32")])
        if det_scale is None:
            det_scale = check_det_scale(getattr(args, "face_det_scale", 1))
        detector = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device=device,
                                                **_precision_kw(precision), **_det_scale_kw(det_scale))
    else:
        other_precision = precision is not None and precision != getattr(detector, "precision", "f32")
        other_scale = det_scale is not None and det_scale != getattr(detector, "det_scale", 1)
        if other_precision or other_scale:
            detector = copy.copy(detector)          # same network and graph cache, the other arithmetic / frame size
            if other_precision:
                detector.precision = precision
            if other_scale:
                detector.det_scale = det_scale
    pads = args.pads if pads is None else pads
    nosmooth = args.nosmooth if nosmooth is None else nosmooth
    batch_size = args.face_det_batch_size if batch_size is None else batch_size
    rects, shots = clip_rects(images, detector, batch_size, track, scene, ranks=ranks, **skw)       # no scene: the reference's one take
    if hold is not None:
        rects = [r for a, b in shots for r in hold_fill(rects[a:b], hold)]
    if any(r is None for r in rects) and (hold is None or len(rects) == 1):
        raise ValueError('Face not detected! Ensure the video contains a face in all the frames.')
    top, bottom, left, right = pads
    # (x1, y1, x2, y2) grown by the pads; the near edges are clipped at 0 and the far edges at the frame size ONLY (inference.py:91-98:
    # `max(0, rect[1] - pady1)`, `min(image.shape[0], rect[3] + pady2)`, ...) - a negative pad or a rect beyond the frame is not
    # pulled back from the other side, exactly as there.  A gap frame's row is zeros; the strict array keeps numpy's own dtype
    boxes = np.array([[0, 0, 0, 0] if r is None else
                      [max(0, r[0] - left), max(0, r[1] - top), min(im.shape[1], r[2] + right), min(im.shape[0], r[3] + bottom)]
                      for r, im in zip(rects, images)], dtype=None if hold is None else np.int64).reshape(-1, 4)
    if not nosmooth:
        for lo, hi in shots:
            for a, b in boxed_runs([r is not None for r in rects[lo:hi]]):     # a strict clip: the one run [0, n)
                get_smoothened_boxes(boxes[lo + a:lo + b], T=5)                # a view: in place, as on a clip of the run's frames alone
    return [[None, None] if r is None else [im[y1:y2, x1:x2], (y1, y2, x1, x2)]
            for r, im, (x1, y1, x2, y2) in zip(rects, images, boxes)]


# ---------------------------------------------------------------- main (inference.py:181-277)
def read_image_bgr(path):
    """`cv2.imread(path)`: uint8 [h, w, 3] in BGR order (decoded with PIL; JPEG decoding is a libjpeg matter on both sides)"""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def resize_frames_u8(frames, wh):
    """`cv2.resize(frame, (w, h))` of whole frames on the device (w2l_resize_u8); frames: list of equal-sized uint8 [H,W,3]"""
    w, h = int(wh[0]), int(wh[1])
    if w < 1 or h < 1:
        raise ValueError("resize target %dx%d is empty" % (w, h))
    dev = torch.device("cuda", torch.cuda.current_device())
    src = torch.from_numpy(np.stack(frames)).to(dev)
    dst = torch.empty((len(frames), h, w, 3), dtype=torch.uint8, device=dev)
    check(_lib.load().w2l_resize_u8(current_stream(), len(frames), ptr(src), src.shape[1], src.shape[2], ptr(dst), h, w),
          "resize_u8")
    return list(dst.cpu().numpy())


def read_frames(a):
    """inference.py:185-213: the frames of `--face` and the frame rate.  Images through PIL; video from the AVI container of
    wav2lip_amd/container.py, uncompressed or Motion-JPEG (this loop takes host frames, so MJPG frames are decoded by PIL here;
    `real_videos_inference` decodes them on the device) - inter-frame codecs need cv2.VideoCapture / ffmpeg, which are not here."""
    if not os.path.isfile(a.face):
        raise ValueError('--face argument must be a valid path to video/image file')
    if is_image_path(a.face):
        return [read_image_bgr(a.face)], a.fps
    from . import container
    try:
        clip = container.read_avi(a.face)
        frames, fps = clip["frames"], clip["fps"]
    except Exception as e:      # noqa: BLE001
        raise ValueError("--face %s: only images (jpg/png/jpeg) and AVI video, uncompressed BGR or Motion-JPEG, can be read here "
                         "(no other video codecs in this build): %s" % (a.face, e))
    print('Reading video frames...')
    frames = list(frames)
    if a.resize_factor > 1 and frames:
        h, w = frames[0].shape[:2]
        frames = resize_frames_u8(frames, (w // a.resize_factor, h // a.resize_factor))
    full_frames = []
    for frame in frames:
        if a.rotate:
            frame = np.ascontiguousarray(np.rot90(frame, k=-1))     # cv2.ROTATE_90_CLOCKWISE: pure data movement
        y1, y2, x1, x2 = a.crop
        if x2 == -1:
            x2 = frame.shape[1]
        if y2 == -1:
            y2 = frame.shape[0]
        full_frames.append(frame[y1:y2, x1:x2])
    return full_frames, fps


def main(argv=None, keep_frames=True, backend="nccl"):
    """inference.py:181-277 on the HIP path.  Same flags, same steps, same messages; differences, all on the file-format
    side: video input is the uncompressed AVI of wav2lip_amd/container.py (no codecs here), `--audio` must be a WAV (the
    reference shells out to ffmpeg for anything else), and the result - the reference's `temp/result.avi` + ffmpeg mux - is
    written as ONE AVI (BGR video + the driving audio as PCM16) at `--outfile`.  Flags the reference does not have, each
    the reference's behaviour by default and independent: `--blend_feather N` / `--blend_top FRACTION` blend the generated face
    into the frame instead of pasting a rectangle (every rank of a sharded run pastes its own shard),
    `--color_match {mean,full}` matches the colours of every generated face to its crop before the paste,
    `--precision {fp32,bf16}` selects the generator's arithmetic,
    `--face_det_precision {fp32,bf16}` the S3FD face detector's and `--face_det_scale K` the size of the frame it sees (1/K;
    the output keeps the input's size) - every rank of a sharded run detects its shard with both.

    Like the reference's loop (inference.py:249-274) this one STREAMS: every batch uploads only the frames it pastes into
    (deduplicated, `frame_idx` remapped) and its output frames go to the AVI writer as soon as they are back, so device and host
    memory are bounded by a few batches whatever the clip length.  `keep_frames` (default, what the tests use) additionally
    returns the list of output frames; the command line runs with keep_frames=False.

    Multi-GPU (`python -m torch.distributed.run --nproc-per-node N -m wav2lip_amd.inference ...`): every rank reads
    the inputs, face detection and the mel chunks are cut into contiguous per-rank shards (sharding.shard_range), each rank runs
    its shard on cuda:LOCAL_RANK, the generated frames are all-gathered in frame order in rounds of one batch per rank
    (sharding.gather_shards_to_writer) and rank 0 ALONE writes `--outfile` (and returns the frames; the other ranks return
    None)."""
    global args
    from . import sharding
    args = parse_args(argv)
    blend = blend_from_args(args)
    color_kw = _color_kw(color_match_from_args(args))
    mjpg = args.out_codec == "mjpg"
    if mjpg and not 1 <= args.out_quality <= 100:
        raise ValueError("--out_quality %d is outside [1, 100]" % args.out_quality)
    detect_kw = detect_kw_from_args(args)
    for given, why in ((mjpg, "--out_codec mjpg runs on one GPU: a sharded run gathers raw frames (compressed shards are not gathered yet)"),
                       ("no_face_hold" in detect_kw, "--no_face_hold runs on one GPU: the hold looks back over the frames of other shards"),
                       ("face_track" in detect_kw, "--face_track runs on one GPU: the track looks back over the frames of other shards"),
                       ("scene_cuts" in detect_kw, "--scene_cuts runs on one GPU: a cut compares a frame with the one before it, in another shard"),
                       ("det_stride" in detect_kw, "--face_det_stride runs on one GPU: a frame is interpolated from key frames of other shards")):
        if given and int(os.environ.get("WORLD_SIZE", "1")) > 1:     # before the process group and any device work
            raise ValueError(why)
    ranks = sharding.init_from_env(backend)
    sharded = ranks.dist is not None and ranks.world > 1
    say = print if ranks.writer else (lambda *a, **k: None)
    try:
        full_frames, fps = read_frames(args)
        say("Number of frames available for inference: " + str(len(full_frames)))
        if not args.audio.endswith('.wav'):
            raise ValueError("--audio %s: extracting audio from other containers is the reference's ffmpeg call; pass a .wav" % args.audio)
        wav = audio.load_wav(args.audio, 16000)
        dev = ranks.device
        mel = audio.melspectrogram_device(wav, dev)
        say(tuple(mel.shape))
        if bool(torch.isnan(mel).any()):
            raise ValueError('Mel contains nan! Using a TTS voice? Add a small epsilon noise to the wav file and try again')
        starts = mel_chunk_starts(mel.shape[1], fps)
        say("Length of mel chunks: {}".format(len(starts)))
        full_frames = full_frames[:len(starts)]
        if args.box[0] == -1:
            det = face_detect(full_frames if not args.static else [full_frames[0]], ranks=ranks,
                              precision=CLI_PRECISION[args.face_det_precision], det_scale=args.face_det_scale, **detect_kw)
            coords = [c for _, c in det]
        else:
            say('Using the specified bounding box instead of face detection...')
            coords = [tuple(args.box)] * len(full_frames)
        model = load_model(args.checkpoint_path, dev)
        say("Model loaded")
        n = len(starts)
        idx = [0 if args.static else i % len(full_frames) for i in range(n)]
        # a gap frame (--no_face_hold) has no box: its rows run no generator row and carry the input frame
        boxes = [None if coords[0 if args.static else j] is None else
                 validate_boxes([coords[0 if args.static else j]], *full_frames[j].shape[:2])[0] for j in idx]
        starts_dev = torch.tensor(starts, dtype=torch.int32, device=dev)
        runner = PipelinedRunner(model, args.wav2lip_batch_size, depth=LIPSYNC_DEPTH, **_precision_kw(CLI_PRECISION[args.precision]),
                                 **_blend_kw(blend), **color_kw)
        bs = args.wav2lip_batch_size
        first, last = sharding.shard_range(n, ranks.rank, ranks.world)
        frame_h, frame_w = full_frames[0].shape[:2]
        out_frames, local, pending = [], [], []
        writer = None
        if ranks.writer:
            outdir = os.path.dirname(args.outfile)
            if outdir:
                os.makedirs(outdir, exist_ok=True)
            from . import container
            from scipy.io import wavfile
            sr, pcm = wavfile.read(args.audio)
            if pcm.dtype != np.int16:
                pcm = np.clip(np.round(audio._pcm_to_float32(pcm) * 32768.0), -32768, 32767).astype(np.int16)
            writer = container.AviWriter(args.outfile, fps, (frame_w, frame_h), audio=pcm, audio_sr=sr, codec=args.out_codec,
                                         quality=args.out_quality)
            writer.__enter__()
        try:
            def emit(f):
                writer.write(f)
                if keep_frames:
                    out_frames.append(f)

            def batch_frames(item):
                """the batch's output frames on the device; with gap rows: every row's input frame, the generated ones pasted
                over the rows that ran"""
                ticket, gaps = item
                if gaps is None:
                    return runner.result(ticket)
                frames_dev, which, ran = gaps
                full = frames_dev.index_select(0, torch.tensor(which, dtype=torch.long, device=dev))
                if ticket is not None:
                    full[torch.tensor(ran, dtype=torch.long, device=dev)] = runner.result(ticket)
                return full

            def drain(item):
                if mjpg:
                    # the frames are encoded where they lie and only the files come back; the raw frames follow them to the
                    # host for keep_frames alone (mjpg is never sharded)
                    from . import jpeg
                    res = batch_frames(item)
                    for data in jpeg.encode_frames(res, quality=args.out_quality, restart_rows=writer.restart_rows):
                        writer.write_jpeg(data)
                    if keep_frames:
                        out_frames.extend(res.cpu().numpy())
                    return
                for f in batch_frames(item).cpu().numpy():
                    if sharded:
                        local.append(f)         # this rank's shard, exchanged below
                    else:
                        emit(f)                 # single process: straight to the writer, as the reference's loop does

            for lo in range(first, last, bs):
                hi = min(last, lo + bs)
                uniq = sorted(set(idx[lo:hi]))                              # a static image: one frame per batch
                remap = {j: k for k, j in enumerate(uniq)}
                frames_dev = torch.from_numpy(np.stack([full_frames[j] for j in uniq])).to(dev)
                ran = [k for k in range(lo, hi) if boxes[k] is not None]
                if len(ran) == hi - lo:
                    pending.append((runner.submit(None, mel=mel, starts=starts_dev[lo:hi].contiguous(), frames=frames_dev,
                                                  frame_idx=[remap[j] for j in idx[lo:hi]], boxes=boxes[lo:hi]), None))
                else:                                                       # the rows with a box run; the others pass through
                    ticket = None
                    if ran:
                        ticket = runner.submit(None, mel=mel, starts=starts_dev[torch.tensor(ran, device=dev)].contiguous(),
                                               frames=frames_dev, frame_idx=[remap[idx[k]] for k in ran], boxes=[boxes[k] for k in ran])
                    pending.append((ticket, (frames_dev, [remap[j] for j in idx[lo:hi]], [k - lo for k in ran])))
                if len(pending) >= runner.depth:
                    drain(pending.pop(0))
            while pending:
                drain(pending.pop(0))
            if sharded:
                allf = sharding.gather_shards_to_writer(ranks.dist, np.stack(local) if local else None, n, ranks.rank, ranks.world,
                                                        device=dev, chunk=bs)
                if ranks.writer:
                    for f in allf:
                        emit(f)
        finally:
            if writer is not None:
                writer.__exit__(None, None, None)
        if not ranks.writer:
            return None
        return out_frames if keep_frames else None
    finally:
        ranks.close()


if __name__ == '__main__':
    main(keep_frames=False)
