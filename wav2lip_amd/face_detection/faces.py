"""Every face of a shot (opt-in): follow ALL faces in the picture at once, so that the real-video scorer prints one
`dist conf` line per face track as the reference's flow does (syncnet_python's run_pipeline.py tracks every face, then
evaluation/scores_LSE/calculate_scores_real_videos.py:38-40 scores each track), where `face_track=` (track.py) follows one.

The rule, integers only - what w2l_face_tracks_all_segments (csrc/detect.hip, include/w2l_hip.h) computes per segment on the device
and `host_all_tracks` states here on the host.  A segment is a clip, or a shot under `scene_cuts`.  F track slots, each (ref rect,
alive, missed), all free at the segment's start; K candidates per frame (`track.host_top_rects`); q = int(min_iou * 256); L missed
frames tolerated.  A candidate OVERLAPS a slot's ref as in track.py: inter > 0 and inter * 256 >= q * union, no + 1.  Per frame:

    matching   best pair first: of the pairs (alive slot, candidate) that overlap, the one of the largest IoU (cross-multiplied
               integers; ties to the lower slot, then the lower candidate) is matched - the slot's ref becomes the candidate,
               missed = 0 - and both leave the contest; again until no overlapping pair is left
    misses     an alive slot that was not matched does missed += 1 and is freed once missed > L
    seeds      the unclaimed candidates, in index order, each take the lowest free slot (one freed in this frame counts); with
               no free slot the candidate is dropped and counted
    output     a slot has a rect in a frame iff it was matched or seeded there

Consequences: with F = 1 slot 0 is `track.host_track` with pick = score; with at most one candidate per frame and L = 0 slot 0
is the untracked rect sequence and every other slot stays empty; two tracks that use one slot one after the other have at least
L frames without a rect between them - exactly L when the slot is seeded again in the frame that freed it, L + 1 or more
otherwise - so the span rule (spans.py) with bridge < L never joins them.  The product always runs with L = `track_spans.bridge`,
as run_pipeline.py has the single --num_failed_det; there the span rule does bridge the one case of exactly L frames: a face that
takes a slot over in the frame its former face timed out (typically one that was dropped for want of a slot until then)
continues that face's span, with interpolated boxes between the two.  A limit, stated in DESIGN.md 3za.

The defaults (F = 4, K = 8, min_iou = 0.25) are choices, not measurements: there are no real weights and no footage behind them.
"""
import collections

import numpy as np

from .track import MAX_CANDS, MAX_RESEED, _inter_union, iou_q8

MAX_FACES = 16                                           # w2l_face_tracks_all_segments' limit on F

AllFaces = collections.namedtuple("AllFaces", "max_faces cands min_iou", defaults=(4, 8, 0.25))
AllFaces.__doc__ = """every face of a shot: `max_faces` F in 1..16 track slots (faces followed at the same time; candidates beyond them are
dropped and counted), `cands` K in 1..16 candidates kept per frame, `min_iou` in (0, 1] the overlap a candidate needs to continue a
track (quantised to q/256).  The defaults are choices, not measurements."""

FaceSpan = collections.namedtuple("FaceSpan", "slot a b boxes detected", defaults=(None,))
FaceSpan.__doc__ = """one kept face track of a clip: `slot` the track slot it was followed in, frames [a, b) of the clip, `boxes` int [b - a, 4]
of (y1, y2, x1, x2), `detected` the number of its frames the detector found (the others are bridged)"""


class FaceSpans:
    """what `detect_many(..., all_faces=...)` yields for a clip of n frames: `.tracks`, the list of `FaceSpan` sorted by (a, slot),
    and `.dropped`, the number of candidates that found no free slot"""

    def __init__(self, n, tracks, dropped):
        self.n, self.dropped = int(n), int(dropped)
        self.tracks = sorted(tracks, key=lambda t: (t.a, t.slot))

    def __len__(self):
        return self.n


def check_faces(all_faces):
    """the `all_faces=` of `detect_many`: None (one face per shot) or an AllFaces / (max_faces, cands, min_iou) tuple.  Returns
    None or an AllFaces of (int, int, float); a ValueError names what is wrong."""
    if all_faces is None:
        return None
    try:
        all_faces = AllFaces(*all_faces)
    except TypeError:
        raise ValueError("all_faces must be None or an AllFaces, got %r" % (all_faces,)) from None
    max_faces, cands, min_iou = all_faces
    for name, v, lo, hi in (("max_faces", max_faces, 1, MAX_FACES), ("cands", cands, 1, MAX_CANDS)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("all_faces %s must be an integer in %d..%d, got %r" % (name, lo, hi, v))
        if not lo <= v <= hi:
            raise ValueError("all_faces %s %d is outside %d..%d" % (name, v, lo, hi))
    if isinstance(min_iou, bool) or not isinstance(min_iou, (int, float, np.integer, np.floating)):
        raise ValueError("all_faces min_iou must be a fraction in (0, 1], got %r" % (min_iou,))
    min_iou = float(min_iou)
    if not 0.0 < min_iou <= 1.0 or iou_q8(min_iou) < 1:          # NaN fails the comparisons
        raise ValueError("all_faces min_iou %r is outside [1/256, 1]" % (min_iou,))
    return AllFaces(int(max_faces), int(cands), min_iou)


def faces_kw(all_faces):
    """the keyword `detect_many` takes for `all_faces`, checked first: none for None, so the default path is called with the same
    arguments as before the option"""
    faces = check_faces(all_faces)
    return {} if faces is None else {"all_faces": faces}


# ---------------------------------------------------------------- the command line
def add_faces_flags(p):
    """`--all_faces [--max_faces F]` on a command's parser: absent by default (one face per shot).  K and the overlap are the
    command's `--face_track_cands` and `--face_track_iou` where it has them (`track.add_track_flags`)."""
    from .track import _int_arg
    p.add_argument('--all_faces', default=False, action='store_true',
                   help='Follow every face in the picture (up to --max_faces at a time) and score each face track on its own, instead '
                        'of one face per shot. Uses --face_track_cands and --face_track_iou; not together with --face_track. '
                        'Default: absent')
    p.add_argument('--max_faces', default=None, type=_int_arg("max_faces", 1, MAX_FACES), metavar='F',
                   help='Faces followed at the same time with --all_faces (1..16; default 4); boxes beyond them are not followed '
                        'and are counted. A choice, not a measured value')


def faces_from_args(a):
    """the `all_faces=` of a parsed command line (`add_faces_flags`): None without --all_faces, or when the namespace comes from a
    parser without the flags.  --max_faces without --all_faces, and --all_faces with --face_track or --face_track_reseed (the
    missed frames tolerated are --num_failed_det's), are ValueErrors."""
    if not getattr(a, "all_faces", False):
        if getattr(a, "max_faces", None) is not None:
            raise ValueError("--max_faces needs --all_faces")
        return None
    if getattr(a, "face_track", None) is not None:
        raise ValueError("--all_faces follows every face and --face_track one: give one of them")
    if getattr(a, "face_track_reseed", None) is not None:
        raise ValueError("--face_track_reseed does not apply to --all_faces: the missed frames tolerated are --num_failed_det's")
    d = AllFaces._field_defaults
    given = {"max_faces": getattr(a, "max_faces", None), "cands": getattr(a, "face_track_cands", None),
             "min_iou": getattr(a, "face_track_iou", None)}
    return check_faces(AllFaces(**{k: d[k] if v is None else v for k, v in given.items()}))


# ---------------------------------------------------------------- the rule on the host
def host_all_tracks(cands_per_frame, F, q, L, stats=None):
    """the rule over the frames of one segment: cands_per_frame = a list of candidate rects per frame (`track.host_top_rects`, at
    most K of them) -> per slot a list with a rect tuple or None per frame.  `stats`: a dict that receives "started", "dropped"
    and "peak" (the status words of w2l_face_tracks_all_segments)."""
    ref, alive, missed = [None] * F, [False] * F, [0] * F
    out = [[] for _ in range(F)]
    started = dropped = peak = 0
    for cands in cands_per_frame:
        cands = [tuple(int(v) for v in c) for c in cands]
        row = [None] * F
        slots, left = [s for s in range(F) if alive[s]], list(range(len(cands)))
        while True:
            best = None                                     # (inter, union, slot, candidate); slots and candidates ascend
            for s in slots:
                for c in left:
                    inter, union = _inter_union(cands[c], ref[s])
                    if inter > 0 and inter * 256 >= q * union and (best is None or inter * best[1] > best[0] * union):
                        best = (inter, union, s, c)
            if best is None:
                break
            _, _, s, c = best
            ref[s], missed[s], row[s] = cands[c], 0, cands[c]
            slots.remove(s)
            left.remove(c)
        for s in slots:                                     # alive and not matched
            missed[s] += 1
            if missed[s] > L:
                alive[s] = False
        for c in left:
            free = [s for s in range(F) if not alive[s]]
            if not free:
                dropped += 1
                continue
            s = free[0]
            ref[s], alive[s], missed[s], row[s] = cands[c], True, 0, cands[c]
            started += 1
        peak = max(peak, sum(alive))
        for s in range(F):
            out[s].append(row[s])
    if stats is not None:
        stats.update(started=started, dropped=dropped, peak=peak)
    return out


def expand_segments(segments, F, R):
    """the segment table of the span rule and the run finish over the F slot arenas: entry t * n_seg + k = (t * R + row0_k, n_k,
    H_k, W_k) for the (row0, n, H, W) of `segments`, as a list of tuples"""
    return [(t * R + row0, n, H, W) for t in range(F) for row0, n, H, W in segments]


# ---------------------------------------------------------------- the device launch
def faces_segments(n_seg, segs, cands, ncand, cflags, faces, L, rects_out, flags_out, status):
    """w2l_face_tracks_all_segments over a device segment table (BOX_SEGMENT rows, a uint8 or int32 tensor): cands int32 [R,K,4],
    ncand and cflags int32 [R] (`FaceAlignment.cands_for_rows`) -> rects_out int32 [F,R,4], flags_out int32 [F,R] (slot t's arenas
    are the t-th blocks) and status int32 [n_seg,4] = (code, started, dropped, peak); flat views of the outputs will do"""
    import torch
    from .._lib import BOX_SEGMENT, check, current_stream, load, ptr
    faces = check_faces(faces)
    R, K, F = int(cands.shape[0]), faces.cands, faces.max_faces
    for name, t, count in (("cands", cands, R * K * 4), ("ncand", ncand, R), ("cflags", cflags, R), ("rects_out", rects_out, F * R * 4),
                           ("flags_out", flags_out, F * R), ("status", status, n_seg * 4)):
        if t.dtype != torch.int32 or t.numel() != count or not t.is_contiguous():
            raise ValueError("faces_segments: %s must be a contiguous int32 tensor of %d words" % (name, count))
    if tuple(cands.shape) != (R, K, 4):
        raise ValueError("faces_segments: cands must have the shape %s" % ((R, K, 4),))
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 0 <= L <= MAX_RESEED:
        raise ValueError("faces_segments: L must be an integer in 0..%d, got %r" % (MAX_RESEED, L))
    if segs.numel() * segs.element_size() < n_seg * BOX_SEGMENT.itemsize:
        raise ValueError("faces_segments: the segment table holds fewer than %d segments" % n_seg)
    check(load().w2l_face_tracks_all_segments(current_stream(), n_seg, ptr(segs), ptr(cands), ptr(ncand), ptr(cflags), R, K, F, int(L),
                                              iou_q8(faces.min_iou), _ptr(rects_out), _ptr(flags_out), _ptr(status)),
          "face_tracks_all_segments")


def _ptr(view):
    """the device address of a tensor view, also of an empty one (whose own data_ptr() is 0)"""
    import ctypes
    return ctypes.c_void_p(view.untyped_storage().data_ptr() + view.element_size() * view.storage_offset())


# ---------------------------------------------------------------- a look at a video
def main(argv=None, state_dict=None):
    """`python -m wav2lip_amd.face_detection.faces VIDEO.avi [--max_faces F] [--scene_cuts T] [--min_track M] ...`: the kept face
    tracks of an AVI file (`container.read_avi`), one line `slot a b detected` each, in (a, slot) order.  `state_dict` (S3FD
    weights) replaces face_detection/s3fd.pth."""
    import argparse
    import sys
    import torch
    from .. import inference
    from ..container import read_avi
    from .many import DetectJob, detect_many
    from .scene import add_scene_flag, scene_from_args, scene_kw
    from .spans import add_span_flags, spans_from_args
    from .track import _int_arg, iou_arg
    p = argparse.ArgumentParser(description="The face tracks of a video: every face followed, one line `slot a b detected` per kept track")
    p.add_argument("video", help="an AVI file (uncompressed 24-bit or Motion-JPEG)")
    p.add_argument('--max_faces', default=None, type=_int_arg("max_faces", 1, MAX_FACES), metavar='F',
                   help='Faces followed at the same time (1..16; default 4). A choice, not a measured value')
    p.add_argument('--face_track_cands', default=None, type=_int_arg("cands", 1, MAX_CANDS), metavar='K',
                   help='Boxes kept per frame as candidates (1..16; default 8). A choice, not a measured value')
    p.add_argument('--face_track_iou', default=None, type=iou_arg, metavar='F',
                   help='Overlap a box needs with a face\'s last box to continue its track (default 0.25). A choice, not a measured value')
    p.add_argument('--face_det_precision', default='fp32', choices=['fp32', 'bf16'], help='Face detector arithmetic')
    p.add_argument('--face_det_batch_size', default=16, type=int, help='Frames per detector batch')
    inference.add_det_scale_flag(p)
    add_scene_flag(p)
    add_span_flags(p)
    a = p.parse_args(argv)
    a.all_faces = True
    faces = faces_from_args(a)
    detector = inference.detector_from_args(a, torch.device("cuda", torch.cuda.current_device()), state_dict)
    frames = read_avi(a.video)["frames"]
    for _, res, error in detect_many(detector, [DetectJob(a.video, list(frames))], batch_size=a.face_det_batch_size,
                                     track_spans=spans_from_args(a), all_faces=faces, **scene_kw(scene_from_args(a))):
        if error is not None:
            print(error, file=sys.stderr)
            return 1
        for t in res.tracks:
            print("%d %d %d %d" % (t.slot, t.a, t.b, t.detected))
        if res.dropped:
            print("more than %d faces: %d candidates not followed" % (faces.max_faces, res.dropped), file=sys.stderr)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
