"""Face spans of a finished clip (opt-in): the stretches of frames in which the followed face is present, each of
which the real-video scorer scores alone (evaluation/scores_LSE/calculate_scores_real_videos.py:38-40 prints one `dist conf` per
face track; the tracks themselves come from syncnet_python's run_pipeline.py, which is not part of the reference tree).

The rule, integers only - what w2l_face_spans_segments (csrc/detect.hip, include/w2l_hip.h) computes per segment on the device and
`host_spans` states here on the host.  A clip (with `scene_cuts`: a shot) has one rect (x1, y1, x2, y2) or None per frame:

    bridged     for detected frames p < q with no detection between them and 2 <= q - p <= bridge + 1, every frame p < i < q takes
                (r_p * (q - i) + r_q * (i - p)) // (q - p) per coordinate.  Frames before the first detection, after the last one
                or inside a longer miss are gaps: unlike `no_face_hold`, which looks back and holds the last rect AFTER the face
                has gone, a span ends at the last detection.
    spans       a maximal sequence of detected and bridged frames, of length L; kept iff L >= min_len and
                max(sum(x2 - x1), sum(y2 - y1)) >= min_size * L (the mean of the larger side, without a division)
    result      the frames of kept spans keep their detected or bridged rect, every other frame has none

The rule looks forward to the next detection, so it is for finished clips: the live path has no such option.  The defaults
(bridge 25, min_len 100, min_size 0) follow the published defaults of run_pipeline.py (--num_failed_det 25, --min_track 100; its
minimum face size is not carried over, 0 keeps every size) as far as they carry over; that script is not here to pin against,
so they are choices, not measurements.
"""
import collections

import numpy as np

MAX_BRIDGE, MAX_MIN_LEN, MAX_MIN_SIZE = 250, 1 << 30, 32767      # w2l_face_spans_segments' limits

TrackSpans = collections.namedtuple("TrackSpans", "bridge min_len min_size", defaults=(25, 100, 0))
TrackSpans.__doc__ = """face spans: `bridge` B in 0..250 undetected frames between two detections that are interpolated, `min_len` M in
1..2^30 frames a span needs to be kept, `min_size` S in 0..32767 the mean size in pixels (the larger of mean width and mean height)
it needs.  The defaults are choices, not measurements."""


def check_spans(track_spans):
    """the `track_spans=` of `detect_many`: None (a clip is boxed as a whole) or a TrackSpans / (bridge, min_len, min_size) tuple.
    Returns None or a TrackSpans of ints; a ValueError names what is wrong."""
    if track_spans is None:
        return None
    try:
        track_spans = TrackSpans(*track_spans)
    except TypeError:
        raise ValueError("track_spans must be None or a TrackSpans, got %r" % (track_spans,)) from None
    for name, v, lo, hi in (("bridge", track_spans.bridge, 0, MAX_BRIDGE), ("min_len", track_spans.min_len, 1, MAX_MIN_LEN),
                            ("min_size", track_spans.min_size, 0, MAX_MIN_SIZE)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("track_spans %s must be an integer in %d..%d, got %r" % (name, lo, hi, v))
        if not lo <= v <= hi:
            raise ValueError("track_spans %s %d is outside %d..%d" % (name, v, lo, hi))
    return TrackSpans(*(int(v) for v in track_spans))


# ---------------------------------------------------------------- the command line
def add_span_flags(p):
    """`--min_track M --num_failed_det B --min_face_size S` on a command's parser, named as run_pipeline.py names them"""
    from .track import _int_arg
    d = TrackSpans._field_defaults
    p.add_argument('--min_track', default=d["min_len"], type=_int_arg("min_track", 1, MAX_MIN_LEN), metavar='M',
                   help='Frames (1..2^30; default 100) a face span needs to be scored. A choice, not a measured value')
    p.add_argument('--num_failed_det', default=d["bridge"], type=_int_arg("num_failed_det", 0, MAX_BRIDGE), metavar='B',
                   help='Frames without a detection (0..250; default 25) between two detections that are bridged by interpolating '
                        'the two boxes; a longer miss ends the span at the last detection. A choice, not a measured value')
    p.add_argument('--min_face_size', default=d["min_size"], type=_int_arg("min_face_size", 0, MAX_MIN_SIZE), metavar='S',
                   help='Mean size in pixels (0..32767; default 0: every size) of the detected box, the larger of its mean width '
                        'and mean height, a span needs to be scored. A choice, not a measured value')


def spans_from_args(a):
    """the `track_spans=` of a parsed command line (`add_span_flags`)"""
    return check_spans(TrackSpans(a.num_failed_det, a.min_track, a.min_face_size))


# ---------------------------------------------------------------- the rule on the host
def host_spans(rects, bridge, min_len, min_size):
    """the rule on one clip (or shot): rects [(x1, y1, x2, y2) or None per frame] -> (the rects of the frames of kept spans, bridged
    ones filled in, None for every other frame; [(a, b)] the kept spans as frame ranges, in order).  What
    w2l_face_spans_segments computes for one segment."""
    n = len(rects)
    filled = [None if r is None else tuple(int(v) for v in r) for r in rects]
    found = [i for i in range(n) if filled[i] is not None]
    for p, q in zip(found, found[1:]):
        if 2 <= q - p <= bridge + 1:
            for i in range(p + 1, q):
                filled[i] = tuple((cp * (q - i) + cq * (i - p)) // (q - p) for cp, cq in zip(filled[p], filled[q]))
    from .many import boxed_runs
    spans = []
    for a, b in boxed_runs([r is not None for r in filled]):
        sw, sh = sum(r[2] - r[0] for r in filled[a:b]), sum(r[3] - r[1] for r in filled[a:b])
        if b - a >= min_len and max(sw, sh) >= min_size * (b - a):
            spans.append((a, b))
        else:
            filled[a:b] = [None] * (b - a)
    return filled, spans


def host_spans_shots(rects, shots, spans):
    """`host_spans` per shot [a, b) of a clip: (the filled rects of the clip, its kept spans as frame ranges of the clip)"""
    filled, kept = [], []
    for a, b in shots:
        f, s = host_spans(rects[a:b], *spans)
        filled += f
        kept += [(a + lo, a + hi) for lo, hi in s]
    return filled, kept


# ---------------------------------------------------------------- the device launch
def span_segments(n_seg, segs, rects, flags, n_rows, spans, rects_out, flags_out, span_rows, status):
    """w2l_face_spans_segments over a device segment table (BOX_SEGMENT rows): the arenas rects int32 [R,4] / flags int32 [R] ->
    rects_out / flags_out of the same format, span_rows int32 [n_rows,4] and status int32 [n_seg,2] (flat views will do)"""
    from .._lib import check, current_stream, load, ptr
    check(load().w2l_face_spans_segments(current_stream(), n_seg, ptr(segs), ptr(rects), ptr(flags), n_rows, spans.bridge,
                                         spans.min_len, spans.min_size, ptr(rects_out), ptr(flags_out), ptr(span_rows), ptr(status)),
          "face_spans_segments")
