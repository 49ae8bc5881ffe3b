"""`inference.face_detect` for many clips in shared detector batches.

The evaluation commands call `face_detect` once per clip (evaluation/gen_videos_from_filelist.py:44-77 is the reference's copy of
inference.py:68-104): every clip uploads its own batches, ends in a ragged batch of its own - another detector graph - and waits for
the device twice per batch.  Frames are independent given the weights, so here the frames of successive clips are the rows of
detector batches of ONE size:

    per group of clips of one frame shape
        one pinned staging buffer  [frame address table][segment table][the frames that were host arrays]  -> one copy to the device
                                   (laid out by wav2lip_amd/staging.py)
        batches of exactly `batch_size` addresses   w2l_s3fd_pack_rows -> S3FD -> gate + NMS -> w2l_s3fd_first_rect
                                                    (rects and flags land in the rows of the group's arenas; no host read)
        one launch                                  w2l_face_boxes_segments: pads, clipping, smoothing, "no face" per clip
        one copy back                               boxes [R,4] + status [clips,2]

The last batch of a group is padded with copies of its last address; those rects fall into scratch rows behind the arena.  A run
over clips of one frame shape therefore builds one detector graph.

With `no_face_hold=G` (opt-in) the one launch is w2l_face_boxes_runs: a frame without a face keeps the last rect for
up to G frames or becomes a gap frame, every run of boxed frames is finished as a clip of its own, and `valid [R]` comes back with
the boxes.  `host_boxes_runs` is that rule on the host.

With `face_track=...` (opt-in) a batch ends in w2l_s3fd_top_rects instead of w2l_s3fd_first_rect - up to K candidate
rects per frame, in arenas of their own - and ONE w2l_face_track_segments launch over the group's clips writes the rects and flags
the finish reads: one face followed through each clip (`face_detection/track.py`).  Still one copy back per group.

With `scene_cuts=...` (opt-in) ONE w2l_frame_hist_rows launch reads the group's frames where they lie and ONE
w2l_scene_cuts launch over the clip table flags the frames that start a shot; the flags come back in a small copy of their own,
queued before the detector batches and waited for after them, and the host then writes one segment per SHOT for the track and the
finish, which run as they are (`face_detection/scene.py`).

With `track_spans=...` (opt-in) ONE w2l_face_spans_segments launch sits between the track and the finish: it bridges
short misses, ends a span at its last detection and drops short or small spans, and w2l_face_boxes_runs with hold 0 finishes what
it leaves.  Its span table rides in the group's one copy back (`face_detection/spans.py`).

With `all_faces=...` (opt-in; needs `track_spans`) the batches leave candidates as for a track and ONE
w2l_face_tracks_all_segments launch follows every face of every segment in F slot arenas; the span launch and the run finish then
run unchanged over a table of F segments per segment, and the one copy back also brings the new status
(`face_detection/faces.py`).

With `det_stride=N` (opt-in) the address table, the batches and the rect or candidate arenas hold the KEY frames of
every clip - of every shot under `scene_cuts` - alone, the track launches step from key to key, and ONE
w2l_face_rects_expand_segments launch - after the track launch, if any - writes the full arenas every finish above then reads as
it always did (`face_detection/stride.py`); under `scene_cuts` the cut flags are then waited for BEFORE the batches.

One routine, `_detect_group`, is all of this: it takes the options as one `_Options` record, `_Tables` lays out and fills every
table of a group - for its clips, for its shots, over full rows or key rows - and one of three finishes (`_finish_plain`,
`_finish_spans`, `_finish_faces`) ends in the one copy back and returns `(boxes, valid, status, kept)`.  A clip the device leaves
to the host goes through `_per_clip`: `inference.clip_rects` and the host statement of the same finish.
"""
import collections

import numpy as np
import torch

from .._lib import BOX_SEGMENT, TRACK_SEGMENT
from ..staging import ADDRESS, Staging
from .scene import host_boxes_shots, split_shots

MAX_T = 64           # w2l_face_boxes_segments' largest smoothing window
NO_FACE = 'Face not detected! Ensure the video contains a face in all the frames.'      # inference.py:89

DetectJob = collections.namedtuple("DetectJob", "key frames")
DetectJob.__doc__ = """one clip to detect faces in: `frames` a sequence of uint8 [H,W,3] BGR host arrays of one shape, or one uint8 device
tensor [T,H,W,3] (read where it lies)"""

_Clip = collections.namedtuple("_Clip", "key frames n H W nbytes")


def host_boxes(rects, H, W, pads, T):
    """the finish of `face_detect` (inference.py:90-104) on the host: rects [(x1, y1, x2, y2)] of one clip of H x W frames ->
    int array [n,4] of (y1, y2, x1, x2).  What w2l_face_boxes_segments computes per segment."""
    from ..inference import get_smoothened_boxes
    top, bottom, left, right = pads
    boxes = np.array([[max(0, r[1] - top), min(H, r[3] + bottom), max(0, r[0] - left), min(W, r[2] + right)] for r in rects],
                     dtype=np.int64).reshape(-1, 4)
    if T:
        boxes = get_smoothened_boxes(boxes, T=T)
    return boxes


MAX_HOLD = 250       # frames a rect is held over undetected frames at the most (w2l_face_boxes_runs' limit)


def check_hold(no_face_hold):
    """the `no_face_hold=` of `face_detect`, `detect_many` and `LipsyncStreams`: None (a frame without a face is the reference's
    ValueError) or an int in 0..250, the number of undetected frames the last rect is held for before frames pass through.  Returns
    None or the int; a ValueError names what is wrong."""
    if no_face_hold is None:
        return None
    if isinstance(no_face_hold, bool) or not isinstance(no_face_hold, (int, np.integer)):
        raise ValueError("no_face_hold must be None or an integer in 0..%d, got %r" % (MAX_HOLD, no_face_hold))
    if not 0 <= no_face_hold <= MAX_HOLD:
        raise ValueError("no_face_hold %d is outside 0..%d" % (no_face_hold, MAX_HOLD))
    return int(no_face_hold)


def hold_arg(text):
    """argparse type of `--no_face_hold`: an integer in 0..250 (a parse error otherwise)"""
    import argparse
    try:
        return check_hold(int(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def add_hold_flag(p):
    """`--no_face_hold G` on a command's parser: absent by default (the reference's behaviour), independent of every other flag"""
    p.add_argument('--no_face_hold', default=None, type=hold_arg, metavar='G',
                   help='Do not stop at a frame without a face: keep the last detected box for up to G such frames (0..250), and '
                        'pass frames beyond that through unchanged. Default: absent, a frame without a face is an error as in the '
                        'reference. Not the reference\'s output')


def hold_fill(rects, hold):
    """the hold of the pass-through rule: rects with None for undetected frames -> the same list with an undetected
    frame i given the rect of the last detected frame p < i while i - p <= hold; what stays None is a gap frame"""
    out, last, at = [], None, 0
    for i, r in enumerate(rects):
        if r is not None:
            last, at = r, i
        out.append(last if last is not None and i - at <= hold else None)
    return out


def boxed_runs(valid):
    """[a, b) of every maximal run of true entries"""
    a, n = 0, len(valid)
    while a < n:
        b = a
        while b < n and valid[b]:
            b += 1
        if b > a:
            yield a, b
        a = b + 1


def host_boxes_runs(rects, H, W, pads, T, hold):
    """`host_boxes` under the pass-through rule, what w2l_face_boxes_runs computes per segment: rects may hold None; after the hold
    every maximal run of boxed frames is finished as `host_boxes` finishes a clip of those frames alone.  Returns (boxes int64
    [n,4] of (y1, y2, x1, x2), zeros on gap rows; valid bool [n])."""
    filled = hold_fill(rects, hold)
    n = len(filled)
    boxes, valid = np.zeros((n, 4), dtype=np.int64), np.array([r is not None for r in filled], dtype=bool).reshape(n)
    for a, b in boxed_runs(valid):
        boxes[a:b] = host_boxes(filled[a:b], H, W, pads, T)
    return boxes, valid


class RunBoxes:
    """what `detect_many(..., no_face_hold=G)` yields for a clip: indexable per frame - `boxes[i]` is the int array (y1, y2, x1, x2)
    or None for a gap frame - with the arrays behind it as `.boxes` (int64 [n,4], zeros on gap rows) and `.valid` (bool [n])"""

    def __init__(self, boxes, valid):
        self.boxes, self.valid = np.asarray(boxes, dtype=np.int64).reshape(-1, 4), np.asarray(valid, dtype=bool).reshape(-1)

    def __len__(self):
        return len(self.valid)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        return self.boxes[i] if self.valid[i] else None

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class SpanBoxes(RunBoxes):
    """what `detect_many(..., track_spans=...)` yields for a clip: a `RunBoxes` whose boxed frames are those of the kept face spans,
    with `.spans` the [(a, b)] frame ranges of the spans, in order (a span never crosses a shot)"""

    def __init__(self, boxes, valid, spans):
        RunBoxes.__init__(self, boxes, valid)
        self.spans = [(int(a), int(b)) for a, b in spans]


def _checked(job):
    """a DetectJob as a _Clip: frames a contiguous uint8 [T,H,W,3] tensor or a list of contiguous uint8 [H,W,3] arrays of one shape;
    a ValueError names the job"""
    frames = job.frames
    try:
        if isinstance(frames, torch.Tensor):
            if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError("a frame tensor must be uint8 [T,H,W,3], got %s %s" % (frames.dtype, tuple(frames.shape)))
            frames = frames.contiguous()
            n, H, W = (int(v) for v in frames.shape[:3])
        else:
            frames = [np.ascontiguousarray(f) for f in frames]
            for f in frames:
                if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape != frames[0].shape:
                    raise ValueError("frames must be uint8 [H,W,3] arrays of one shape, got %s %s" % (f.dtype, f.shape))
            n = len(frames)
            H, W = (int(v) for v in frames[0].shape[:2]) if n else (0, 0)
        if n and (H < 1 or W < 1):
            raise ValueError("empty frames (%d x %d)" % (H, W))
    except ValueError as e:
        raise ValueError("job %r: %s" % (job.key, e)) from None
    return _Clip(job.key, frames, n, H, W, n * H * W * 3)


def _detect_batch(detector, frames, B, H, W, rects, flags, offset):
    """one detector batch: rows [offset, offset + B) of the arenas from the B addresses of `frames`"""
    detector.rects_for_rows(frames, B, H, W, rects, flags, offset)


def _detect_batch_cands(detector, frames, B, H, W, cands, ncand, cflags, offset, K):
    """one detector batch under tracked selection: rows [offset, offset + B) of the candidate arenas"""
    detector.cands_for_rows(frames, B, H, W, cands, ncand, cflags, offset, K)


Arenas = collections.namedtuple("Arenas", "rects flags cands ncand cflags")    # int32 [R,4], [R]; under a track [R,K,4], [R], [R]


def detect_rows(detector, addr_dev, spans, batch_size, n_rows, track=None, K=None):
    """The rect stage of the packed and the live path: arenas of `n_rows` rows, and the batches of exactly `batch_size` addresses
    of the device address table over spans [(H, W, first row, padded end)], one per frame shape.  A batch fills rects / flags, or
    with `track` the candidate arenas (`track_rows` then writes rects / flags) - also without a track when `K`, the candidates per
    frame, is given (`all_faces`).  No host read."""
    K = K if track is None else track.cands
    shapes = [(n_rows, 4), (n_rows,)] + ([] if K is None else [(n_rows, K, 4), (n_rows,), (n_rows,)])
    rects, flags, cands, ncand, cflags = [torch.empty(s, dtype=torch.int32, device=addr_dev.device) for s in shapes] + [None] * (5 - len(shapes))
    for H, W, first, padded in spans:
        for lo in range(first, padded, batch_size):
            frames = addr_dev[lo * 8:(lo + batch_size) * 8]
            if K is None:
                _detect_batch(detector, frames, batch_size, H, W, rects, flags, lo)
            else:
                _detect_batch_cands(detector, frames, batch_size, H, W, cands, ncand, cflags, lo, K)
    return Arenas(rects, flags, cands, ncand, cflags)


def track_rows(n_seg, segs, arenas, track, status, state=None):
    """w2l_face_track_segments, after the batches of `detect_rows`: one face followed through each segment (TRACK_SEGMENT rows) in
    one launch, from the candidates into the arenas' rects and flags; `state`: the live streams' slot table"""
    from .track import track_segments
    track_segments(segs, n_seg, arenas.cands, arenas.ncand, arenas.cflags, track, arenas.rects, arenas.flags, status, state=state)


class BoxOut:
    """the one int32 buffer a finish writes and one copy brings back: boxes [n_boxes][4], with a hold valid [n_boxes], status
    [n_seg][2], with a track its status words [n_seg] - in that order.  `buffer` is the device tensor; `boxes`, `valid` (None
    without a hold), `status` and `track_status` (empty without a track) are flat views of it.  With `spans` (w2l_face_spans_segments'
    outputs ride in the same copy) three more parts follow: up to 3 words that bring the next one to a 16-byte boundary, `span_rows`
    [n_boxes][4] and `span_status` [n_seg][2]; then `extra` more words (`.extra`: w2l_face_tracks_all_segments' status)."""

    def __init__(self, n_boxes, n_seg, hold, track, device, spans=False, extra=0):
        self.sizes = (4 * n_boxes, n_boxes if hold else None, 2 * n_seg, n_seg if track else 0)
        if spans:
            self.sizes += (-sum(n or 0 for n in self.sizes) % 4, 4 * n_boxes, 2 * n_seg)
        if extra:
            self.sizes += (extra,)
        self.buffer = torch.empty(sum(n or 0 for n in self.sizes), dtype=torch.int32, device=device)
        self.boxes, self.valid, self.status, self.track_status = self._parts(self.buffer)[:4]
        self.span_rows, self.span_status = self._parts(self.buffer)[5:7] if spans else (None, None)
        self.extra = self._parts(self.buffer)[-1] if extra else None

    def _parts(self, flat):
        ends = np.cumsum([n or 0 for n in self.sizes]).tolist()
        return [None if n is None else flat[e - n:e] for n, e in zip(self.sizes, ends)]

    def ptr(self, view):
        """the device address of a view, also of an empty one (whose own data_ptr() is 0)"""
        import ctypes
        return ctypes.c_void_p(self.buffer.data_ptr() + 4 * view.storage_offset())

    def split(self, host, of="clip"):
        """the parts of the buffer's host copy (numpy int32): (boxes [n_boxes,4], valid [n_boxes] or None, status [n_seg,2], track
        status [n_seg] or empty); the status words of w2l_face_track_segments are all 0 for a table built here"""
        boxes, valid, status, track_status = self._parts(host)[:4]
        if track_status.any():
            raise AssertionError("w2l_face_track_segments did not follow a %s's segment%s"
                                 % (of, " (status %s)" % track_status.tolist() if of == "clip" else ""))
        return boxes.reshape(-1, 4), valid, status.reshape(-1, 2), track_status

    def split_spans(self, host):
        """the span parts of the buffer's host copy: (span rows [n_boxes,4], span status [n_seg,2])"""
        span_rows, span_status = self._parts(host)[5:7]
        return span_rows.reshape(-1, 4), span_status.reshape(-1, 2)

    def split_extra(self, host):
        """the trailing `extra` words of the buffer's host copy"""
        return self._parts(host)[-1]


def _finish_segments(n_seg, segs, rects, flags, pads, T, boxes, status):
    """w2l_face_boxes_segments: the group's clips in one launch"""
    from .._lib import check, current_stream, load, ptr
    top, bottom, left, right = pads
    check(load().w2l_face_boxes_segments(current_stream(), n_seg, ptr(segs), ptr(rects), ptr(flags), top, bottom, left, right, T,
                                         ptr(boxes), ptr(status)), "face_boxes_segments")


def _finish_runs(n_seg, segs, rects, flags, n_rows, pads, T, hold, boxes, valid, status):
    """w2l_face_boxes_runs: the group's clips in one launch under the pass-through rule"""
    from .._lib import check, current_stream, load, ptr
    top, bottom, left, right = pads
    check(load().w2l_face_boxes_runs(current_stream(), n_seg, ptr(segs), ptr(rects), ptr(flags), n_rows, top, bottom, left, right, T,
                                     hold, ptr(boxes), ptr(valid), ptr(status)), "face_boxes_runs")


def _fold_shot_status(shot_status, shots_of):
    """the per-clip status [clips,2] of the shots' status [shots,2]: across a clip's shots code 2 wins over code 1, and the row is
    the clip's frame that decided it (the first shot with the winning code); shots_of: [(a, b)] per clip, in clip order"""
    out, k = np.zeros((len(shots_of), 2), dtype=shot_status.dtype), 0
    for c, shots in enumerate(shots_of):
        for a, _ in shots:
            code, row = (int(v) for v in shot_status[k])
            if code > out[c][0]:
                out[c] = (code, a + row)
            k += 1
    return out


_Options = collections.namedtuple("_Options", "pads T hold track scene spans faces stride")
_Options.__doc__ = """what `detect_many` was asked for, checked: pads (top, bottom, left, right), the smoothing window T, and per option None
or its checked value - hold (an int), track (a FaceTrack), scene (a SceneCuts), spans (a TrackSpans), faces (an AllFaces); stride is
the int N >= 1"""


class _Tables:
    """The tables of one group, reserved in a Staging, and what the finishes need to know of the group.  `segs`: [(row0, n)] the
    group's segments - clips, or shots - as rows of the FULL arenas of R rows.  The detector's rows are the full rows, or under
    key-frame detection (`det_stride` N > 1) the KEY rows: segment k's key frames (`stride.key_frames`) are the rows
    [key_row0_k, key_row0_k + m_k) of the key arenas, one segment after the other, Rk in all (N = 1: key_row0 = row0, m = n,
    Rk = R).  In reservation order:
        addresses      with `batch_size`: the frame address of every detector row, Rk padded to a batch multiple (`padded`) with
                       copies of the last one                                       (the detector batches)
        segments       BOX_SEGMENT (row0, n, H, W)                                  (the cut launch; the finishes, on full rows)
        stride         N > 1: STRIDE_SEGMENT (t * Rk + key_row0, t * R + row0, n, 0), F * n_seg of them, slot t's after slot t - 1's
        tracks         with `track`: TRACK_SEGMENT (key_row0, m, -1, 0)             (no carried state: a clip, or a shot)
        key_segments   N > 1 with `faces`: BOX_SEGMENT (key_row0, m, H, W) for w2l_face_tracks_all_segments
        wide           with `faces`: the F-slot table of `faces.expand_segments` over the full rows, for the span launch and the
                       run finish
    `_detect_group` adds `lengths` (frames per clip) and, under `scene_cuts`, `shots_of` ([(a, b)] per clip)."""

    def __init__(self, st, segs, shape, R, N=1, batch_size=None, track=None, faces=None):
        from .._lib import STRIDE_SEGMENT
        from .stride import key_frames
        self.st, self.dev, self.segs, self.shape, self.R, self.N = st, st.device, segs, shape, R, N
        self.shots_of = None
        n_seg = self.n_seg = len(segs)
        F = self.F = 1 if faces is None else faces.max_faces
        self.keys = None if N == 1 else [key_frames(n, N) for _, n in segs]
        self.Rk = R if N == 1 else sum(len(k) for k in self.keys)
        self.padded = None if batch_size is None else (self.Rk + batch_size - 1) // batch_size * batch_size
        self.addresses = None if batch_size is None else st.table(ADDRESS, self.padded)
        self.segments = st.table(BOX_SEGMENT, n_seg)
        self.stride = None if N == 1 else st.table(STRIDE_SEGMENT, F * n_seg)
        self.tracks = None if track is None else st.table(TRACK_SEGMENT, n_seg)
        self.key_segments = None if N == 1 or faces is None else st.table(BOX_SEGMENT, n_seg)
        self.wide = None if faces is None else st.table(BOX_SEGMENT, F * n_seg)

    def key_rows(self):
        """the full-arena row of every key row, in key-row order"""
        return np.array([row0 + i for (row0, _), keys in zip(self.segs, self.keys) for i in keys], dtype=np.int64)

    def fill(self, addresses=None):
        """the tables' contents, once the Staging is allocated; addresses: uint64 [Rk], the frame every detector row reads"""
        (H, W), R, Rk, n_seg = self.shape, self.R, self.Rk, self.n_seg
        view = lambda h: None if h is None else self.st.view(h)
        addr, segments, stride, tracks, key_segments = (view(h) for h in (self.addresses, self.segments, self.stride, self.tracks,
                                                                          self.key_segments))
        if addr is not None:
            addr[:Rk] = addresses
            addr[Rk:] = addr[Rk - 1]
        kr = 0
        for k, (row0, n) in enumerate(self.segs):
            m = n if self.keys is None else len(self.keys[k])
            segments[k] = (row0, n, H, W)
            if stride is not None:
                for t in range(self.F):
                    stride[t * n_seg + k] = (t * Rk + kr, t * R + row0, n, 0)
            if tracks is not None:
                tracks[k] = (kr, m, -1, 0)
            if key_segments is not None:
                key_segments[k] = (kr, m, H, W)
            kr += m
        if self.wide is not None:
            from .faces import expand_segments
            view(self.wide)[:] = np.array(expand_segments(segments.tolist(), self.F, R), dtype=BOX_SEGMENT)

    def upload(self):
        """the Staging's one copy; the device tables the launches take"""
        self.st.upload()
        dev = lambda h: None if h is None else self.st.tensor(h)
        self.addr_dev, self.seg_dev, self.stride_dev = dev(self.addresses), dev(self.segments), dev(self.stride)
        self.track_dev, self.key_seg_dev, self.wide_dev = dev(self.tracks), dev(self.key_segments), dev(self.wide)

    def expand(self, key_rects, key_flags, status, out=None):
        """w2l_face_rects_expand_segments: the key arenas (F * Rk rows, or the one slot's arenas with their scratch rows behind) ->
        `Arenas` of the full rects [F * R, 4] and flags [F * R] (`out`, or new ones); status: int32 [F * n_seg] on the device"""
        from .stride import expand_rects
        n_rows = self.F * self.R
        rects, flags = out if out is not None else (torch.empty((n_rows, 4), dtype=torch.int32, device=key_rects.device),
                                                    torch.empty((n_rows,), dtype=torch.int32, device=key_rects.device))
        expand_rects(self.F * self.n_seg, self.stride_dev, self.N, key_rects, key_flags, self.F * self.Rk, rects, flags, n_rows, status)
        return Arenas(rects, flags, None, None, None)

    @staticmethod
    def check(status):
        """the expand launch's status words on the host: all 0 for tables built here"""
        if status.any():
            raise AssertionError("w2l_face_rects_expand_segments did not follow a segment (status %s)" % status.tolist())


def _detect_group(detector, clips, opts, batch_size):
    """One group on the device.  clips: _Clips of one frame shape, each with at least one frame; opts: an `_Options`.  Returns numpy
    (boxes, valid, status, kept) as the option's finish leaves them (`_finish_plain`, `_finish_spans`, `_finish_faces`): status is
    int32 [clips,2] always, a part that does not exist is None.  The skeleton is fixed - stage, upload, batches, (track), (expand),
    finish, ONE copy back - and every option hooks into it at one place:
        `scene`   the signature and the cut launch are queued right after the upload, and the tables the track and the finish read
                  hold one segment per SHOT: they are built once the flags are back - after the batches, which hide the wait;
        `stride`  N > 1: the address table, the batches and the rect or candidate arenas hold KEY rows (`_Tables`), and the expand
                  launch writes the full arenas every finish reads.  Without `scene` the frames between the keys of a clip of host
                  arrays are not even uploaded.  With `scene` every frame goes up - the signatures read them all - and the group
                  WAITS for the flags before the batches: the keys are per shot;
        `track`, `faces`  the batches leave candidates; `hold`, `spans`, `faces` choose the finish."""
    dev = torch.device(detector.device)
    H, W = clips[0].H, clips[0].W
    N, track, scene, faces = opts.stride, opts.track, opts.scene, opts.faces
    lengths = [c.n for c in clips]
    clip_segs = list(zip(np.cumsum([0] + lengths[:-1]).tolist(), lengths))
    R = sum(lengths)
    # ---- one staging buffer: [address table][segment tables][the frames that were host arrays]
    st = Staging(dev)
    if scene is None:
        tabs = _Tables(st, clip_segs, (H, W), R, N, batch_size, track, faces)
    else:                                                    # the clips' table is the cut launch's; the shots' tables follow
        tabs = _Tables(st, clip_segs, (H, W), R, 1, batch_size)
    src = []
    for k, c in enumerate(clips):
        pick = np.arange(c.n, dtype=np.uint64) if tabs.keys is None else np.array(tabs.keys[k], dtype=np.uint64)
        if tabs.keys is None or isinstance(c.frames, torch.Tensor):
            src.append((st.place(c.frames), pick))
        else:                                                # host arrays under key-frame detection: the key frames alone go up
            src.append((st.place([c.frames[i] for i in tabs.keys[k]]), np.arange(len(pick), dtype=np.uint64)))
    st.allocate()
    addresses = np.concatenate([np.uint64(st.address(h)) + pick * np.uint64(H * W * 3) for h, pick in src])
    tabs.fill(addresses)
    tabs.upload()

    def shot_tables():
        shots_of = _wait_cuts(cuts, clip_segs, R)
        shots = _Tables(Staging(dev), [(r + a, b - a) for (r, _), mine in zip(clip_segs, shots_of) for a, b in mine], (H, W), R, N,
                        None if N == 1 else batch_size, track, faces)       # `st` stays: the frames lie in it
        shots.st.allocate()
        shots.fill(None if N == 1 else addresses[shots.key_rows()])
        shots.upload()
        shots.shots_of = shots_of
        return shots

    if scene is not None:                                    # queued before the batches: the flags cross while the detector runs
        cuts = _queue_cuts(tabs.addr_dev, tabs.seg_dev, len(clips), R, H, W, scene, dev)
    if scene is not None and N > 1:                          # the keys are per shot: nothing to detect on before the cuts are known
        tabs = shot_tables()
    arenas = detect_rows(detector, tabs.addr_dev, [(H, W, 0, tabs.padded)], batch_size, tabs.padded, track,      # rows [Rk, padded): scratch
                         None if faces is None else faces.cands)
    if scene is not None and N == 1:                         # the batches hid the wait
        tabs = shot_tables()
    tabs.lengths = lengths
    finish = _finish_faces if faces is not None else _finish_spans if opts.spans is not None else _finish_plain
    return finish(tabs, arenas, opts)


def _queue_cuts(addresses, segments, n_clips, R, H, W, scene, dev):
    """the two scene launches of a group and the copy of their result, all queued on the current stream: signatures of the R frames of
    the address table, cut flags over the clip table -> (the device buffer, its pinned host copy int32 [R + n_clips] = cuts [R] +
    status [n_clips], the event that says the copy has landed)"""
    from .scene import SIG_WORDS, cut_flags, frame_signatures, scene_q8
    sig = torch.empty((R, SIG_WORDS), dtype=torch.int32, device=dev)
    frame_signatures(addresses, sig, 0, rows=(R, H, W))
    buf = torch.empty(R + n_clips, dtype=torch.int32, device=dev)
    cut_flags(segments, n_clips, sig, scene_q8(scene.thresh), buf[:R], buf[R:])
    host = torch.empty(R + n_clips, dtype=torch.int32, pin_memory=True)
    host.copy_(buf, non_blocking=True)
    ready = torch.cuda.Event()
    ready.record()
    return buf, host, ready


def _wait_cuts(cuts, clip_segs, R):
    """what `_queue_cuts` queued, once its copy has landed: the status words checked (all 0 for a table built here) and the shots
    [(a, b)] of every clip [(row0, n)]"""
    _, host, ready = cuts
    ready.synchronize()
    flags = host.numpy()
    if flags[R:].any():
        raise AssertionError("w2l_scene_cuts did not follow a clip's segment (status %s)" % flags[R:].tolist())
    return [split_shots(n, flags[r:r + n]) for r, n in clip_segs]


def _one_rect_rows(tabs, arenas, track, out):
    """between the batches and what reads one rect per frame: with `track` w2l_face_track_segments over the group's segments (of key
    rows under key-frame detection), then under key-frame detection the expand launch, whose status words ride in `out.extra`.
    Returns the `Arenas` whose rects and flags hold the full rows."""
    if track is not None:
        track_rows(tabs.n_seg, tabs.track_dev, arenas, track, out.track_status)
    if tabs.N > 1:
        arenas = tabs.expand(arenas.rects, arenas.flags, out.extra)
    return arenas


def _finish_plain(tabs, arenas, opts):
    """the end of `_detect_group` without `track_spans`: the track launch (if any), the expand launch (under key-frame detection),
    w2l_face_boxes_segments - with `hold` w2l_face_boxes_runs - over the group's segments and the group's one copy back.  Returns
    numpy (boxes int32 [R,4] in (y1, y2, x1, x2) order, rows in clip order; valid int32 [R] with `hold`, else None; status int32
    [clips,2]; None).  The track's status words come back in the same copy and are all 0 (the table is built here); under
    `scene_cuts` the status is folded per clip (`_fold_shot_status`)."""
    n_seg, R, hold = tabs.n_seg, tabs.R, opts.hold
    out = BoxOut(R, n_seg, hold is not None, opts.track is not None, tabs.dev, extra=n_seg if tabs.N > 1 else 0)
    full = _one_rect_rows(tabs, arenas, opts.track, out)
    if hold is None:
        _finish_segments(n_seg, tabs.seg_dev, full.rects, full.flags, opts.pads, opts.T, out.boxes, out.status)
    else:
        _finish_runs(n_seg, tabs.seg_dev, full.rects, full.flags, R, opts.pads, opts.T, hold, out.boxes, out.valid, out.status)
    host = out.buffer.cpu().numpy()                          # the group's one copy back; it also ends the stream's use of the staging buffers
    boxes, valid, status, _ = out.split(host)
    if tabs.N > 1:
        tabs.check(out.split_extra(host))
    if tabs.shots_of is not None:
        status = _fold_shot_status(status, tabs.shots_of)
    return boxes, valid, status, None


def _finish_spans(tabs, arenas, opts):
    """the end of `_detect_group` under `track_spans`: the track launch (if any), the expand launch (under key-frame detection),
    w2l_face_spans_segments over the same segments, w2l_face_boxes_runs with hold 0 on its outputs, and the group's one copy back,
    which also brings the span table.  Returns numpy (boxes [R,4], valid [R], status [clips,2], [the clip's kept spans [(a, b)] per
    clip])."""
    from .spans import span_segments
    n_seg, R, dev = tabs.n_seg, tabs.R, tabs.dev
    out = BoxOut(R, n_seg, True, opts.track is not None, dev, spans=True, extra=n_seg if tabs.N > 1 else 0)
    full = _one_rect_rows(tabs, arenas, opts.track, out)
    rects = torch.empty((R, 4), dtype=torch.int32, device=dev)
    flags = torch.empty((R,), dtype=torch.int32, device=dev)
    span_segments(n_seg, tabs.seg_dev, full.rects, full.flags, R, opts.spans, rects, flags, out.span_rows, out.span_status)
    _finish_runs(n_seg, tabs.seg_dev, rects, flags, R, opts.pads, opts.T, 0, out.boxes, out.valid, out.status)
    host = out.buffer.cpu().numpy()                          # the group's one copy back
    boxes, valid, status, _ = out.split(host)
    span_rows, span_status = out.split_spans(host)
    if tabs.N > 1:
        tabs.check(out.split_extra(host))
    shots_of = tabs.shots_of if tabs.shots_of is not None else [[(0, n)] for n in tabs.lengths]
    if (span_status[:, 0] == 3).any() or (status[:, 0] == 3).any():
        raise AssertionError("w2l_face_spans_segments did not follow a clip's segment (status %s)" % span_status.tolist())
    kept, k, r = [], 0, 0
    for n, shots in zip(tabs.lengths, shots_of):
        mine = []
        for a, _ in shots:                                  # segment k holds the rows from r + a on
            if span_status[k][0] == 0:
                mine += [(a + int(f), a + int(f) + int(L)) for f, L, _, _ in span_rows[r + a:r + a + int(span_status[k][1])]]
            k += 1
        kept.append(mine)
        r += n
    return boxes, valid, _fold_shot_status(status, shots_of), kept


def _finish_faces(tabs, arenas, opts):
    """the end of `_detect_group` under `all_faces`: w2l_face_tracks_all_segments over the group's segments (L = `spans.bridge`) into
    F slot arenas of R rows each, then the unchanged w2l_face_spans_segments and w2l_face_boxes_runs (hold 0) over `tabs.wide_dev`,
    the table of F * n_seg segments on those arenas, and the group's one copy back, which also brings the span table and the new
    status.  Returns (None, None, status [clips,2], [a `faces.FaceSpans` per clip]); a clip with a frame left to the host has code 2.
    Under key-frame detection the candidates are those of key rows: the tracks run over the table of key segments with L =
    `stride.faces_reseed(bridge, N)` into F slot arenas of key rows, and the expand launch over the F-slot wide stride table writes
    the F full slot arenas the span launch reads; its status words ride in the same copy."""
    from .faces import FaceSpan, FaceSpans, faces_segments
    from .spans import span_segments
    from .stride import faces_reseed
    n_seg, R, Rk, dev, spans, keyed = tabs.n_seg, tabs.R, tabs.Rk, tabs.dev, opts.spans, tabs.N > 1
    F = opts.faces.max_faces
    out = BoxOut(F * R, F * n_seg, True, False, dev, spans=True, extra=4 * n_seg + (F * n_seg if keyed else 0))
    slot_rects = torch.empty((2, F * R, 4), dtype=torch.int32, device=dev)          # the tracks, then the spans of them
    slot_flags = torch.empty((2, F * R), dtype=torch.int32, device=dev)
    if keyed:
        key_rects = torch.empty((F * Rk, 4), dtype=torch.int32, device=dev)
        key_flags = torch.empty((F * Rk,), dtype=torch.int32, device=dev)
        faces_segments(n_seg, tabs.key_seg_dev, arenas.cands[:Rk], arenas.ncand[:Rk], arenas.cflags[:Rk], opts.faces,
                       faces_reseed(spans.bridge, tabs.N), key_rects, key_flags, out.extra[:4 * n_seg])
        tabs.expand(key_rects, key_flags, out.extra[4 * n_seg:], out=(slot_rects[0], slot_flags[0]))
    else:
        faces_segments(n_seg, tabs.seg_dev, arenas.cands[:R], arenas.ncand[:R], arenas.cflags[:R], opts.faces, spans.bridge,
                       slot_rects[0], slot_flags[0], out.extra)
    span_segments(F * n_seg, tabs.wide_dev, slot_rects[0], slot_flags[0], F * R, spans, slot_rects[1], slot_flags[1], out.span_rows,
                  out.span_status)
    _finish_runs(F * n_seg, tabs.wide_dev, slot_rects[1], slot_flags[1], F * R, opts.pads, opts.T, 0, out.boxes, out.valid, out.status)
    host = out.buffer.cpu().numpy()                          # the group's one copy back
    boxes, _, status, _ = out.split(host)
    span_rows, span_status = out.split_spans(host)
    faces_status = out.split_extra(host)[:4 * n_seg].reshape(-1, 4)
    if keyed:
        tabs.check(out.split_extra(host)[4 * n_seg:])
    shots_of = tabs.shots_of if tabs.shots_of is not None else [[(0, n)] for n in tabs.lengths]
    if (span_status[:, 0] == 3).any() or (status[:, 0] == 3).any() or faces_status[:, 0].any():
        raise AssertionError("w2l_face_tracks_all_segments did not follow a clip's segment (status %s, %s)"
                             % (faces_status[:, 0].tolist(), span_status.tolist()))
    per_clip, results, k, r = np.zeros((len(tabs.lengths), 2), dtype=status.dtype), [], 0, 0
    for c, (n, shots) in enumerate(zip(tabs.lengths, shots_of)):
        tracks, dropped = [], 0
        for a, _ in shots:                                  # segment k holds the clip's frames from a on, in every slot
            dropped += int(faces_status[k][2])
            for t in range(F):
                code, count = (int(v) for v in span_status[t * n_seg + k])
                if code == 2 and per_clip[c][0] == 0:
                    per_clip[c] = (2, a + count)
                row = t * R + r + a
                for f, L, det, _ in span_rows[row:row + (count if code == 0 else 0)].tolist():
                    tracks.append(FaceSpan(t, a + f, a + f + L, boxes[row + f:row + f + L].astype(np.int64), det))
            k += 1
        results.append(FaceSpans(n, tracks, dropped))
        r += n
    return None, None, per_clip, results


def _host_faces(detector, clip, frames, opts, batch_size):
    """`all_faces` for one clip on the host: the candidates of every frame (`get_candidates_for_batch`, which runs `host_top_rects`
    on a frame the device does not decide), the shots, `faces.host_all_tracks` per shot, then per slot `host_spans_shots` and
    `host_boxes_shots` with hold 0 -> a `faces.FaceSpans`.  With `opts.stride` N > 1 the shots come first, the candidates are those
    of every shot's key frames, the tracks step from key to key with `stride.faces_reseed(bridge, N)` tolerated misses, and every
    slot's key rects go through `stride.host_stride_fill` per shot."""
    from ..inference import halving
    from .faces import FaceSpan, FaceSpans, host_all_tracks
    from .spans import host_spans_shots
    from .stride import faces_reseed, host_stride_fill, key_frames, shot_key_frames
    from .track import iou_q8
    spans, faces, stride = opts.spans, opts.faces, opts.stride
    shots = [(0, clip.n)] if opts.scene is None else _host_shots(detector, frames, batch_size, opts.scene)
    seen = frames if stride == 1 else [frames[i] for i in shot_key_frames(shots, stride)]

    def run(size):
        per_frame = []
        for lo in range(0, len(seen), size):
            per_frame += detector.get_candidates_for_batch(np.array(seen[lo:lo + size]), faces.cands)
        return per_frame

    per_frame = halving(run, batch_size)
    F, dropped = faces.max_faces, 0
    slots = [[] for _ in range(F)]
    k = 0
    for a, b in shots:
        stats = {}
        if stride == 1:
            per_slot = host_all_tracks(per_frame[a:b], F, iou_q8(faces.min_iou), spans.bridge, stats)
        else:
            m = len(key_frames(b - a, stride))
            per_slot = [host_stride_fill(rects, b - a, stride) for rects in
                        host_all_tracks(per_frame[k:k + m], F, iou_q8(faces.min_iou), faces_reseed(spans.bridge, stride), stats)]
            k += m
        for t, rects in enumerate(per_slot):
            slots[t] += rects
        dropped += stats["dropped"]
    tracks = []
    for t, rects in enumerate(slots):
        filled, kept = host_spans_shots(rects, shots, spans)
        boxes, _ = host_boxes_shots(filled, shots, clip.H, clip.W, opts.pads, opts.T, 0)
        tracks += [FaceSpan(t, a, b, boxes[a:b], sum(r is not None for r in rects[a:b])) for a, b in kept]
    return FaceSpans(clip.n, tracks, dropped)


def _host_shots(detector, frames, batch_size, scene):
    """the shots [(a, b)] of one clip of host frames (at least one, of one shape): its signatures batch by batch, one cut launch and
    one small copy"""
    from .scene import SIG_WORDS, clip_cuts, frame_signatures
    dev = torch.device(detector.device)
    n, (H, W) = len(frames), frames[0].shape[:2]
    sig = torch.empty((n, SIG_WORDS), dtype=torch.int32, device=dev)
    for lo in range(0, n, batch_size):
        frame_signatures(torch.from_numpy(np.ascontiguousarray(np.array(frames[lo:lo + batch_size]))).to(dev), sig, lo)
    return split_shots(n, clip_cuts(sig, H, W, scene)[0])


def _per_clip(detector, clip, opts, batch_size):
    """one clip alone on the host path (batch by batch uploads, the host rules): (key, boxes, error).  The strict case with the
    reference's windows goes through `inference.face_detect` as it stands, with the options that are set as its keywords.  Every
    other case takes the clip's rects and shots from `inference.clip_rects` and finishes them with the host statement of its rule:
    `spans.host_spans_shots` and the run finish with hold 0 under `track_spans`, else `scene.host_boxes_shots` with the hold;
    `all_faces` goes through `_host_faces`."""
    from .. import inference
    from .spans import host_spans_shots
    pads, T, hold, track, scene, spans, faces, stride = opts
    frames = list(clip.frames.cpu().numpy()) if isinstance(clip.frames, torch.Tensor) else list(clip.frames)
    try:
        if faces is not None:
            return clip.key, _host_faces(detector, clip, frames, opts, batch_size), None
        if spans is None and hold is None and T in (0, 5):           # face_detect's own finish fits
            kw = {k: v for k, v in (("face_track", track), ("scene_cuts", scene), ("det_stride", stride)) if v not in (None, 1)}
            det = inference.face_detect(frames, detector=detector, pads=list(pads), nosmooth=(T == 0), batch_size=batch_size, **kw)
            return clip.key, np.array([c for _, c in det], dtype=np.int64).reshape(-1, 4), None
        rects, shots = inference.clip_rects(frames, detector, batch_size, track, scene, stride)
        if spans is not None:
            filled, kept = host_spans_shots(rects, shots, spans)
            boxes, valid = host_boxes_shots(filled, shots, clip.H, clip.W, pads, T, 0)
            return clip.key, SpanBoxes(boxes, valid, kept), None
        boxes, valid = host_boxes_shots(rects, shots, clip.H, clip.W, pads, T, hold)
        return clip.key, boxes if hold is None else RunBoxes(boxes, valid), None
    except (ValueError, OverflowError) as e:                         # no face; a coordinate int() refuses
        return clip.key, None, str(e)


def detect_many(detector, jobs, pads=(0, 0, 0, 0), T=5, batch_size=16, group_batches=16, max_group_bytes=1 << 30, no_face_hold=None,
                face_track=None, scene_cuts=None, track_spans=None, all_faces=None, det_stride=None):
    """`inference.face_detect(frames, detector, pads, nosmooth=(T == 0))` for every `DetectJob` of the iterable `jobs`, the frames
    of successive clips packed into detector batches of exactly `batch_size`.  A generator: jobs are consumed lazily and one
    `(key, boxes, error)` comes out per job, in job order - `boxes` the int array [n,4] of (y1, y2, x1, x2) `face_detect` returns
    as coords and `error` None, or `boxes` None and `error` the text of the ValueError `face_detect` raises (a frame without a
    face).  `T` is the smoothing window (`get_smoothened_boxes`; the reference uses 5), 0 for none.

    A group takes consecutive jobs of one frame shape; it closes once it holds `group_batches * batch_size` frames, before a job
    that would take its frames past `max_group_bytes` or has another shape (that one job has been read by then), or when the
    iterator ends, and always holds at least one job.  The group is detected (see the module text), its results are yielded and
    it is released before more jobs are read: the memory alive is one group plus the job that closed it.  A single job larger
    than `max_group_bytes` goes through `inference.face_detect` on its own (batch by batch uploads), and so does a clip with a
    frame the device does not decide (RECT_HOST: a non-finite or huge coordinate, an NMS overflow); that call's result, or the
    text of its ValueError, is the job's.

    A RuntimeError of the detector (out of device memory on a large frame) halves `batch_size` for the rest of the run, prints
    the reference's message and runs the group again; at 1 it raises the reference's error (inference.py:75-88).

    `no_face_hold`: None (default) is all of the above.  An int G in 0..250 switches the pass-through rule on (not
    the reference's behaviour): a frame without a face keeps the last detected rect for up to G frames and is a gap frame beyond
    that, and every run of boxed frames is finished as a clip of its own.  `boxes` is then a `RunBoxes`: `boxes[i]` is frame i's
    (y1, y2, x1, x2) or None for a gap frame (`.boxes` / `.valid` are the arrays); `error` stays for real errors (a coordinate
    int() refuses).

    `face_track`: None (default), or a pick name / `track.FaceTrack`: one face is followed through every clip instead of taking
    the best-scoring box of each frame (not the reference's behaviour), exactly as `face_detect(face_track=...)`
    does for the clip alone.

    `scene_cuts`: None (default), or a threshold in [1/256, 1) / `scene.SceneCuts`: every clip is split into shots where the colour
    histogram of a frame differs from the previous frame's by more than the threshold, and every shot is tracked, held, padded,
    clipped and smoothed as a clip of its own (not the reference's behaviour), exactly as
    `face_detect(scene_cuts=...)` does for the clip alone.  A job still gets one result: in the strict mode a frame without a
    face in any shot is the clip's error.

    `track_spans`: None (default), or a `spans.TrackSpans`: for finished clips that a scorer reads (not the reference's
    code).  Misses of up to `bridge` frames between two detections are interpolated, a longer miss ends the span at the last
    detection, and spans shorter than `min_len` frames or smaller than `min_size` pixels are dropped; every kept span is padded,
    clipped and smoothed as a clip of its own.  `boxes` is then a `SpanBoxes`: a `RunBoxes` over the frames of kept spans with
    `.spans` = [(a, b)], the spans as frame ranges of the clip in order; with `scene_cuts` the rule runs per shot.  Together with
    `no_face_hold` - the other answer to the same question - it is a ValueError.

    `all_faces`: None (default), or a `faces.AllFaces`: every face in the picture is followed, up to `max_faces` at a time
    (not the reference's code), and every face track goes through the span rule on its own; the missed frames a
    track tolerates are `track_spans.bridge`.  It needs `track_spans`; with `face_track` (one face) or `no_face_hold` it is a
    ValueError.  `boxes` is then a `faces.FaceSpans`: `.tracks` is the list of `FaceSpan(slot, a, b, boxes)` - frames [a, b) of the
    clip, `boxes` int [b - a, 4] of (y1, y2, x1, x2) - sorted by (a, slot), and `.dropped` the number of candidates that found no
    free slot.

    `det_stride`: None or 1 (default: every frame is shown to the detector), or an int N in 2..32: key-frame detection (DESIGN.md
    3zb, not the reference's behaviour and not accuracy-neutral).  The detector sees the frames 0, N, 2N, ... and the last one of
    every clip - with `scene_cuts`, of every shot - and one more launch interpolates the rects of the frames between two detected
    key frames (`face_detection/stride.py` states the rule); a missed key frame leaves 2N - 1 frames without a face, which every
    option above then treats as it treats any such frame.  With `face_track` the track steps from key frame to key frame: its
    `reseed` counts key frames and its `min_iou` is unchanged; with `all_faces` a track tolerates `max(0, (bridge + 1) // N - 1)`
    missed key frames, exactly the misses the span rule bridges.  Exactly as `face_detect(det_stride=N)` does for the clip alone."""
    from ..inference import halving
    from .scene import check_scene
    from .faces import FaceSpans, check_faces
    from .spans import check_spans
    from .stride import check_stride
    from .track import check_track
    stride = check_stride(det_stride)
    hold = check_hold(no_face_hold)
    track = check_track(face_track)
    scene = check_scene(scene_cuts)
    spans = check_spans(track_spans)
    if spans is not None and hold is not None:
        raise ValueError("track_spans and no_face_hold are two answers to the same question: give one of them")
    faces = check_faces(all_faces)
    if faces is not None:
        if hold is not None:
            raise ValueError("all_faces and no_face_hold do not go together")
        if track is not None:
            raise ValueError("all_faces follows every face and face_track one: give one of them")
        if spans is None:
            raise ValueError("all_faces needs track_spans: every face track goes through the span rule")
    if batch_size < 1 or group_batches < 1:
        raise ValueError("batch_size and group_batches must be at least 1")
    if not 0 <= int(T) <= MAX_T:
        raise ValueError("T must be in 0..%d" % MAX_T)
    pads = tuple(int(p) for p in pads)
    if len(pads) != 4:
        raise ValueError("pads must be (top, bottom, left, right)")
    opts = _Options(pads, int(T), hold, track, scene, spans, faces, stride)
    it = iter(jobs)
    held, ended = None, False           # the job read but not yet placed
    while not ended or held is not None:
        group, shape, n_frames, n_bytes = [], None, 0, 0
        while True:
            if held is None:
                try:
                    held = _checked(next(it))
                except StopIteration:
                    ended = True
                    break
            c = held
            if c.n == 0:                                   # nothing to detect: answered in its place
                group.append(c)
                held = None
                continue
            if c.nbytes > max_group_bytes:
                if group:
                    break                                  # the jobs before it first
                held = None
                yield _per_clip(detector, c, opts, batch_size)
                del c
                continue
            if shape is not None and ((c.H, c.W) != shape or n_bytes + c.nbytes > max_group_bytes):
                break
            group.append(c)
            held = None
            shape, n_frames, n_bytes = (c.H, c.W), n_frames + c.n, n_bytes + c.nbytes
            del c
            if n_frames >= group_batches * batch_size:
                break
        if not group:
            continue
        clips = [c for c in group if c.n]
        boxes = status = valid = kept = None

        def run_group(size):
            nonlocal batch_size
            batch_size = size                              # a halved batch holds for the rest of the run
            return _detect_group(detector, clips, opts, size)

        if clips:
            boxes, valid, status, kept = halving(run_group, batch_size)
        results, row, k = [], 0, 0
        for c in group:
            if c.n == 0:
                empty = np.zeros((0, 4), np.int64)
                results.append((c.key, FaceSpans(0, [], 0) if faces is not None else SpanBoxes(empty, [], []) if spans is not None
                                else empty if hold is None else RunBoxes(empty, []), None))
                continue
            code = int(status[k][0])                       # status[k][1]: the frame that decided it
            if code == 0 and faces is not None:
                results.append((c.key, kept[k], None))
            elif code == 0 and spans is not None:
                results.append((c.key, SpanBoxes(boxes[row:row + c.n], valid[row:row + c.n] != 0, kept[k]), None))
            elif code == 0 and hold is not None:
                results.append((c.key, RunBoxes(boxes[row:row + c.n], valid[row:row + c.n] != 0), None))
            elif code == 0:
                results.append((c.key, boxes[row:row + c.n].astype(np.int64), None))
            elif code == 1:
                results.append((c.key, None, NO_FACE))
            else:
                results.append(c)                          # the device left a frame to the host: the clip alone, below
            row += c.n
            k += 1
        group = clips = None                               # released before the results go out (a re-run keeps its own clip)
        del c
        while results:
            res = results.pop(0)
            yield _per_clip(detector, res, opts, batch_size) if isinstance(res, _Clip) else res
