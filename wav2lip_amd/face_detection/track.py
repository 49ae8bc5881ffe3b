"""Tracked face selection (opt-in): follow ONE face through a clip instead of taking the detector's best-scoring
box of every frame (api.py:61-77: `d[0]` after sfd_detector.py:45), which changes hands between two people in the picture.

The rule has two halves, and this file states both on the host, in pure Python on ints - what w2l_s3fd_top_rects and
w2l_face_track_segments (csrc/detect.hip, include/w2l_hip.h) compute on the device, and what the host fallback runs:

    candidates of a frame   `host_top_rects`: the first K rows of the NMS keep list, in its order, whose score is > 0.5, each clipped
                            at 0 and truncated as `get_detections_for_batch` does with its one row
    the track over a clip   `host_track`: frames in order with the state (ref rect, has, missed).  A candidate OVERLAPS when
                            inter > 0 and inter * 256 >= q * union (integers, no + 1).  With a track the overlapping candidate
                            of the largest IoU continues it (ties to the lower index); with none, missed += 1 and the frame has
                            no face while missed <= L, else the track is dropped and the same frame seeds a new one.  Without
                            a track the candidates seed one by `pick`: score (candidate 0), largest (area), left / right (the
                            smallest / largest x1 + x2), ties to the lower index.

Consequences: with L = 0 a frame that has a candidate never comes out without a face, so in the strict mode tracking adds no
"Face not detected"; with L = 0 and pick = score, a clip with at most one candidate per frame - and any clip with K = 1 - gets
exactly the untracked rects.  The defaults (K = 8, L = 0, min_iou = 0.25) are choices, not measurements: there are no real
weights and no footage behind them.
"""
import collections

import numpy as np

from .._lib import TRACK_SEGMENT  # noqa: F401  -- the segment table of w2l_face_track_segments

PICKS = ("score", "largest", "left", "right")            # the index is the kernel's `pick`
MAX_CANDS, MAX_RESEED = 16, 250
FRESH = ((0, 0, 0, 0), 0, 0)                             # the state of a clip's start: (ref rect, has, missed)
STATE_INTS = 8                                           # a slot of the device state: (x1, y1, x2, y2, has, missed, 0, 0)

FaceTrack = collections.namedtuple("FaceTrack", "pick cands reseed min_iou", defaults=(8, 0, 0.25))
FaceTrack.__doc__ = """tracked face selection: `pick` how a track is seeded (one of PICKS; naming it switches the feature on), `cands` K
in 1..16 candidates kept per frame, `reseed` L in 0..250 missed frames tolerated before the track is seeded again, `min_iou` in
(0, 1] the overlap a candidate needs to continue the track (quantised to q/256).  The defaults are choices, not measurements."""


def iou_q8(min_iou):
    """`q` of the track for a `min_iou`: int(min_iou * 256), as `inference.blend_top_q8` quantises"""
    return int(min_iou * 256)


def check_track(track):
    """the `face_track=` of `face_detect`, `detect_many` and `LipsyncStreams`: None (the reference's best-scoring box per frame), a
    pick name, or a FaceTrack / (pick, cands, reseed, min_iou) tuple.  Returns None or a FaceTrack of (str, int, int, float); a
    ValueError names what is wrong."""
    if track is None:
        return None
    if isinstance(track, str):
        track = FaceTrack(track)
    try:
        track = FaceTrack(*track)
    except TypeError:
        raise ValueError("face_track must be None, a pick name or a FaceTrack, got %r" % (track,)) from None
    pick, cands, reseed, min_iou = track
    if pick not in PICKS:
        raise ValueError("face_track pick must be one of %s, got %r" % (", ".join(PICKS), pick))
    for name, v, lo, hi in (("cands", cands, 1, MAX_CANDS), ("reseed", reseed, 0, MAX_RESEED)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("face_track %s must be an integer in %d..%d, got %r" % (name, lo, hi, v))
        if not lo <= v <= hi:
            raise ValueError("face_track %s %d is outside %d..%d" % (name, v, lo, hi))
    if isinstance(min_iou, bool) or not isinstance(min_iou, (int, float, np.integer, np.floating)):
        raise ValueError("face_track min_iou must be a fraction in (0, 1], got %r" % (min_iou,))
    min_iou = float(min_iou)
    if not 0.0 < min_iou <= 1.0 or iou_q8(min_iou) < 1:          # NaN fails the comparisons
        raise ValueError("face_track min_iou %r is outside [1/256, 1]" % (min_iou,))
    return FaceTrack(pick, int(cands), int(reseed), min_iou)


def track_kw(face_track):
    """the keyword `face_detect`, `detect_many` and `LipsyncStreams` take for `face_track`, checked first: none for None, so the
    default path is called with the same arguments as before the option (as `inference._hold_kw`)"""
    track = check_track(face_track)
    return {} if track is None else {"face_track": track}


# ---------------------------------------------------------------- the command line
def _int_arg(name, lo, hi):
    import argparse

    def parse(text):
        try:
            v = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError("%r is not an integer" % (text,))
        if not lo <= v <= hi:
            raise argparse.ArgumentTypeError("%d is outside %d..%d" % (v, lo, hi))
        return v
    parse.__name__ = name
    return parse


def iou_arg(text):
    """argparse type of `--face_track_iou`: a fraction in [1/256, 1] (a parse error otherwise)"""
    import argparse
    try:
        f = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not a number" % (text,))
    if not 0.0 < f <= 1.0 or iou_q8(f) < 1:
        raise argparse.ArgumentTypeError("%r is outside [1/256, 1]" % (f,))
    return f


def add_track_flags(p):
    """`--face_track PICK [--face_track_reseed L] [--face_track_iou F] [--face_track_cands K]` on a command's parser: absent by
    default (the reference's best-scoring box per frame), independent of every other flag"""
    p.add_argument('--face_track', default=None, choices=PICKS, metavar='PICK',
                   help='Follow one face through the clip instead of taking the best-scoring box of every frame: PICK (score, largest, '
                        'left or right) chooses the face the track starts on. Default: absent, as the reference. Not the reference\'s '
                        'output when more than one face is in the picture')
    p.add_argument('--face_track_reseed', default=None, type=_int_arg("reseed", 0, MAX_RESEED), metavar='L',
                   help='Frames (0..250; default 0) the tracked face may be missing before the track starts again on another box; '
                        'such frames count as frames without a face (see --no_face_hold). A choice, not a measured value')
    p.add_argument('--face_track_iou', default=None, type=iou_arg, metavar='F',
                   help='Overlap (intersection over union, in [1/256, 1]; default 0.25) a box needs with the tracked face\'s last box '
                        'to continue the track. A choice, not a measured value')
    p.add_argument('--face_track_cands', default=None, type=_int_arg("cands", 1, MAX_CANDS), metavar='K',
                   help='Boxes kept per frame as candidates (1..16; default 8). A choice, not a measured value')


def track_from_args(a):
    """the `face_track=` of a parsed command line (`add_track_flags`): None without --face_track, or when the namespace comes from
    a parser without the flags.  One of the other three flags without --face_track is a ValueError."""
    pick = getattr(a, "face_track", None)
    rest = {f: getattr(a, "face_track_" + f, None) for f in ("cands", "reseed", "iou")}
    if pick is None:
        given = [f for f, v in rest.items() if v is not None]
        if given:
            raise ValueError("--face_track_%s needs --face_track PICK" % given[0])
        return None
    d = FaceTrack._field_defaults
    return check_track(FaceTrack(pick, d["cands"] if rest["cands"] is None else rest["cands"],
                                 d["reseed"] if rest["reseed"] is None else rest["reseed"],
                                 d["min_iou"] if rest["iou"] is None else rest["iou"]))


# ---------------------------------------------------------------- the rule on the host
def host_top_rects(table_row, keep_row, n, K, scale=None):
    """the candidates of one image on the host: table_row [P,5] float32 and keep_row, n = the image's NMS keep list -> up to K
    rect tuples (x1, y1, x2, y2) of Python ints, the first K rows of keep_row[:n] whose score is > 0.5, each mapped back by
    `scale` = (sx, sy) if given (`s3fd.scale_box`), clipped at 0 and truncated by int() - which raises what it raises on NaN and
    inf, and has no 32767 limit.  Rows after the K-th passing one are not looked at; a keep entry outside the table is an
    IndexError."""
    from .s3fd import scale_box
    table_row = np.asarray(table_row)
    out = []
    for i in range(int(n)):
        if len(out) == K:
            break
        row = int(keep_row[i])
        if not 0 <= row < len(table_row):
            raise IndexError("keep entry %d of the image is row %d, outside the table's %d rows" % (i, row, len(table_row)))
        d = table_row[row]
        if not d[4] > 0.5:
            continue
        box = d[:4] if scale is None else scale_box(d[:4], *scale)
        out.append(tuple(int(v) for v in np.maximum(np.asarray(box), 0)))
    return out


def _area(r):
    return (r[2] - r[0]) * (r[3] - r[1])


def _inter_union(c, ref):
    inter = max(0, min(c[2], ref[2]) - max(c[0], ref[0])) * max(0, min(c[3], ref[3]) - max(c[1], ref[1]))
    return inter, _area(c) + _area(ref) - inter


def _seed(cands, pick):
    """index of the seed among a frame's candidates: ties to the lower index (min / max take the first of equals)"""
    idx = range(len(cands))
    if pick == "largest":
        return max(idx, key=lambda k: _area(cands[k]))
    if pick == "left":
        return min(idx, key=lambda k: cands[k][0] + cands[k][2])
    if pick == "right":
        return max(idx, key=lambda k: cands[k][0] + cands[k][2])
    return 0


def host_track(cands_per_frame, track, state=None):
    """the track over the frames of a clip, or of a piece of one: cands_per_frame = a list of candidate rects per frame
    (`host_top_rects`), `track` a FaceTrack, `state` None for a clip's start or what an earlier call returned for the frames
    before.  Returns (a rect tuple or None per frame, the state after them).  The state is (ref rect, has, missed), with zeros
    for the rect and the count when there is no track (the words of a slot of w2l_face_track_segments' state table)."""
    track = check_track(track)
    q, L = iou_q8(track.min_iou), track.reseed
    ref, has, missed = FRESH if state is None else state
    out = []
    for cands in cands_per_frame:
        cands = [tuple(int(v) for v in c) for c in cands]
        chosen = None
        if has:
            best = None                                     # (inter, union, index) of the best overlapping candidate so far
            for k, c in enumerate(cands):
                inter, union = _inter_union(c, ref)
                if inter > 0 and inter * 256 >= q * union and (best is None or inter * best[1] > best[0] * union):
                    best = (inter, union, k)
            if best is not None:
                chosen = cands[best[2]]
            else:
                missed += 1
                if missed > L:
                    has = 0                                 # dropped: this same frame seeds a new track
        if not has and cands:
            chosen = cands[_seed(cands, track.pick)]
        if chosen is not None:
            ref, has, missed = chosen, 1, 0
        out.append(chosen)
    return out, ((tuple(ref), 1, missed) if has else FRESH)


# ---------------------------------------------------------------- the device launch
def track_segments(segs, n_seg, cands, ncand, cflags, track, rects, flags, status, state=None):
    """w2l_face_track_segments over a device segment table (TRACK_SEGMENT rows, a uint8 or int32 tensor): cands int32 [R,K,4], ncand
    and cflags int32 [R] (`FaceAlignment.cands_for_rows`) -> rects int32 [R,4], flags int32 [R], status int32 [n_seg];
    `state` int32 [slots, 8] for segments that name a slot"""
    import torch
    from .._lib import check, current_stream, load, ptr
    track = check_track(track)
    R, K = int(cands.shape[0]), track.cands
    for name, t, shape in (("cands", cands, (R, K, 4)), ("ncand", ncand, (R,)), ("cflags", cflags, (R,)), ("rects", rects, (R, 4)),
                           ("flags", flags, (R,)), ("status", status, (n_seg,))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("track_segments: %s must be a contiguous int32 tensor of shape %s" % (name, shape))
    if state is not None and (state.dtype != torch.int32 or state.dim() != 2 or state.shape[1] != STATE_INTS or not state.is_contiguous()):
        raise ValueError("track_segments: state must be a contiguous int32 tensor [slots, %d]" % STATE_INTS)
    if segs.numel() * segs.element_size() < n_seg * TRACK_SEGMENT.itemsize:
        raise ValueError("track_segments: the segment table holds fewer than %d segments" % n_seg)
    check(load().w2l_face_track_segments(current_stream(), n_seg, ptr(segs), ptr(cands), ptr(ncand), ptr(cflags), R, K,
                                         PICKS.index(track.pick), track.reseed, iou_q8(track.min_iou), ptr(state),
                                         0 if state is None else int(state.shape[0]), ptr(rects), ptr(flags), ptr(status)),
          "face_track_segments")
