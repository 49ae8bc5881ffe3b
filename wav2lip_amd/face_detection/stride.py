"""Key-frame face detection (opt-in `det_stride=N`, `--face_det_stride N`): the detector looks at every Nth frame of
a clip and the rects of the frames between are interpolated.  The reference detects on every frame (inference.py:77-78), so this is
not the reference's output; it is off by default (N = 1 is the path without the option, byte for byte).

The rule, integers only - what w2l_face_rects_expand_segments (csrc/detect.hip, include/w2l_hip.h) computes per segment on the
device and `host_stride_fill` states here on the host.  A segment is a clip, or with `scene_cuts` a shot, of n >= 1 frames:

    key frames  0, N, 2N, ... below n, and n - 1: m = (n - 1 + N - 1) // N + 1 of them, key j at pos(j) = min(j * N, n - 1).  Only
                they are shown to S3FD (and, with `face_track` or `all_faces`, to the track, which then steps from key to key).
    key rows    a key frame keeps its own rect, or its own miss
    between     frame i with p = pos(j) < i < q = pos(j + 1): if both keys were detected, every coordinate is
                (r_p * (q - i) + r_q * (i - p)) // (q - p) - the formula of `spans.host_spans`; otherwise the frame has no rect

Everything after it - pads, clipping, smoothing, "no face", `no_face_hold`, `track_spans` - sees ordinary per-frame rects.  A missed
key therefore leaves 2N - 1 frames without a rect: the reference's error in the strict mode, held under `no_face_hold`, bridged
under `track_spans` iff 2N - 1 <= bridge.

The rule looks forward to the next key, so it is for finished clips: the live path (`streaming`, `LipsyncStreams`) has no such
option, and neither has `preprocess`.  How far an interpolated box lies from the box the detector would have found on that frame
depends on the footage and is not measured here: the option is not accuracy-neutral.
"""
import numpy as np

MAX_STRIDE = 32      # w2l_face_rects_expand_segments' largest N


def check_stride(det_stride):
    """the `det_stride=` of `face_detect` and `detect_many`: None (every frame, as 1) or an int in 1..32.  Returns the int; a
    ValueError names what is wrong."""
    if det_stride is None:
        return 1
    if isinstance(det_stride, bool) or not isinstance(det_stride, (int, np.integer)):
        raise ValueError("det_stride must be an integer in 1..%d, got %r" % (MAX_STRIDE, det_stride))
    if not 1 <= det_stride <= MAX_STRIDE:
        raise ValueError("det_stride %d is outside 1..%d" % (det_stride, MAX_STRIDE))
    return int(det_stride)


def stride_arg(text):
    """argparse type of `--face_det_stride`: an integer in 1..32 (a parse error otherwise)"""
    import argparse
    try:
        return check_stride(int(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def add_stride_flag(p):
    """`--face_det_stride N` on a command's parser: 1 by default (the reference's behaviour), independent of every other flag"""
    p.add_argument('--face_det_stride', default=1, type=stride_arg, metavar='N',
                   help='Run the face detector on every Nth frame only (1..%d) - frames 0, N, 2N, ... and the last one of a clip, or '
                        'of a shot with --scene_cuts - and interpolate the boxes of the frames between two detected key frames; a '
                        'missed key frame leaves 2N - 1 frames without a face. With --face_track the track steps from key frame to '
                        'key frame: --face_track_reseed then counts key frames and --face_track_min_iou is unchanged. Ignored with '
                        '--box. Default: 1, every frame as in the reference. Not the reference\'s output, and not accuracy-neutral'
                        % MAX_STRIDE)


def stride_kw(det_stride):
    """the keyword of `face_detect` / `detect_many`: stride 1 calls them with the arguments they had before the option"""
    return {} if det_stride in (None, 1) else {"det_stride": det_stride}


def stride_from_args(a):
    """the `det_stride=` keyword of a parsed command line (`add_stride_flag`)"""
    return stride_kw(check_stride(getattr(a, 'face_det_stride', 1)))


# ---------------------------------------------------------------- the rule on the host
def key_frames(n, N):
    """the key frames of a segment of n frames, in order: 0, N, 2N, ... below n, and n - 1 ([] for n < 1)"""
    if n < 1:
        return []
    return [min(j * N, n - 1) for j in range((n - 1 + N - 1) // N + 1)]


def host_stride_fill(key_rects, n, N):
    """the rule on one clip (or shot): key_rects [(x1, y1, x2, y2) or None per key frame of `key_frames(n, N)`] -> one rect or None
    per frame.  What w2l_face_rects_expand_segments computes for one segment whose key rows are flagged 0 or 1."""
    keys = key_frames(n, N)
    if len(key_rects) != len(keys):
        raise ValueError("%d key rects for the %d key frames of %d frames at stride %d" % (len(key_rects), len(keys), n, N))
    out = [None] * n
    for pos, r in zip(keys, key_rects):
        out[pos] = None if r is None else tuple(int(v) for v in r)
    for p, q in zip(keys, keys[1:]):
        if out[p] is not None and out[q] is not None:
            for i in range(p + 1, q):
                out[i] = tuple((cp * (q - i) + cq * (i - p)) // (q - p) for cp, cq in zip(out[p], out[q]))
    return out


def host_stride_fill_shots(key_rects, shots, N):
    """`host_stride_fill` per shot [a, b) of a clip: key_rects holds the shots' key rects one shot after the other"""
    out, k = [], 0
    for a, b in shots:
        m = len(key_frames(b - a, N))
        out += host_stride_fill(key_rects[k:k + m], b - a, N)
        k += m
    return out


def shot_key_frames(shots, N):
    """the key frames of every shot [a, b), as frames of the clip, one shot after the other"""
    return [a + i for a, b in shots for i in key_frames(b - a, N)]


def faces_reseed(bridge, N):
    """the missed KEY frames a track of `all_faces` tolerates at stride N: max(0, (bridge + 1) // N - 1), so that it tolerates
    exactly the misses the span rule will bridge (L missed keys put two detections (L + 1) * N frames apart, which is bridged iff
    (L + 1) * N <= bridge + 1)"""
    return max(0, (bridge + 1) // N - 1)


# ---------------------------------------------------------------- the device launch
def expand_rects(n_seg, segs, N, key_rects, key_flags, n_key_rows, rects, flags, n_rows, status):
    """w2l_face_rects_expand_segments over a device table of STRIDE_SEGMENT rows: the compact key arenas key_rects int32 [Rk,4] /
    key_flags int32 [Rk] -> the full arenas rects [R,4] / flags [R]; status int32 [n_seg] (flat views will do)"""
    from .._lib import check, current_stream, load, ptr
    check(load().w2l_face_rects_expand_segments(current_stream(), n_seg, ptr(segs), N, ptr(key_rects), ptr(key_flags), n_key_rows,
                                                ptr(rects), ptr(flags), n_rows, ptr(status)), "face_rects_expand_segments")
