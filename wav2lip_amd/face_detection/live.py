"""The finish of `inference.face_detect` for a video that arrives a few frames at a time: what
w2l_face_boxes_stream (csrc/detect.hip) computes per segment, stated on the host.  Pure Python on integers; no device in it.

`get_smoothened_boxes` (inference.py:59-66) looks FORWARD: box i <= n - T is the mean of the padded rects i .. i + T - 1, all still
unsmoothed when it is taken (the loop runs in place and in order), so it is final once T - 1 more frames have been detected,
whatever comes later.  Only the boxes after n - T depend on the end of the video, through the in-place window `boxes[n - T:]`; the
one already-smoothed entry of that window, n - T, has a window that is entirely forward, so it can be computed again from raw
rects.  A stream therefore carries nothing but its last max(T, 1) RAW rects from tick to tick, and its boxes are `face_detect`'s
on the finished video however the video was cut into ticks.

The second half of the file is the same for the opt-in pass-through of frames without a face: what
w2l_face_boxes_stream_runs computes per segment, with twice the carry.
"""
import numpy as np

from .._lib import BOX_STREAM_SEGMENT  # noqa: F401  -- the tick's segment table, filled by streaming.DeviceBoxes

CARRY_ROWS = 64      # rows of a carry slot = w2l_face_boxes_stream's largest smoothing window (many.MAX_T)


def final_range(seen, n_new, closed, T):
    """frames [lo, hi) whose boxes a tick writes: `seen` frames were finished before it, it adds `n_new`, `closed`: the video
    ends with it"""
    n = seen + n_new
    if T == 0:
        return seen, n
    return max(0, seen - T + 1), n if closed else max(0, n - T + 1)


def new_final_count(seen, n_new, closed, T):
    """number of boxes that become final in a tick (rows of the segment in the kernel's output)"""
    lo, hi = final_range(seen, n_new, closed, T)
    return hi - lo


def _mean(values):
    """numpy's float64 mean assigned into an integer array: an exact integer sum, one division, truncation towards zero"""
    return int(sum(values) / float(len(values)))


def stream_boxes_host(state, new_rects, closed, H, W, pads, T):
    """One tick of one stream.  state: None for a new stream, else what the previous call returned; new_rects: the rects
    (x1, y1, x2, y2) of the frames detected in this tick (may be empty); closed: the video ends with this tick.  Returns
    (boxes int64 [new_final_count, 4] of (y1, y2, x1, x2), the next state).  The state is (frames seen, the last
    min(seen, max(T, 1)) raw rects)."""
    seen, carry = (0, []) if state is None else state
    top, bottom, left, right = pads
    keep = max(T, 1)
    assert len(carry) == min(seen, keep)
    held = list(carry) + [tuple(int(v) for v in r) for r in new_rects]
    n = seen + len(new_rects)
    base = n - len(held)                                    # held[h] is frame base + h

    def pad(i):
        r = held[i - base]
        return (max(0, r[1] - top), min(H, r[3] + bottom), max(0, r[0] - left), min(W, r[2] + right))

    lo, hi = final_range(seen, len(new_rects), closed, T)
    out = []
    if T == 0:
        out = [pad(i) for i in range(seen, n)]
    else:
        forward_end = hi if not closed else (n - T if n >= T else 0)
        for i in range(lo, forward_end):
            window = [pad(i + j) for j in range(T)]
            out.append(tuple(_mean([w[c] for w in window]) for c in range(4)))
        if closed and n > 0:
            ws = n - T if n >= T else max(0, 2 * n - T)     # first row of Python's boxes[n - T:]
            window = [list(pad(i)) for i in range(ws, n)]
            for i in range(n - T if n >= T else 0, n):      # in order: the window holds rows already smoothed
                mean = [_mean([w[c] for w in window]) for c in range(4)]
                if i >= ws:
                    window[i - ws] = mean
                if i >= lo:                                 # entry n - T may have gone out in an earlier tick
                    out.append(tuple(mean))
    assert len(out) == hi - lo
    return np.array(out, dtype=np.int64).reshape(-1, 4), (n, held[len(held) - min(n, keep):])


# ---------------------------------------------------------------- the pass-through rule, tick by tick
RUNS_CARRY_ROWS = 2 * CARRY_ROWS                 # rows of a slot of w2l_face_boxes_stream_runs: the last 2 * max(T, 1) frames
RUNS_CARRY_INTS = RUNS_CARRY_ROWS * 5 + 4        # (x1, y1, x2, y2, boxed) per row, then (frames since the last detection, 0, 0, 0)
HOLD_FAR = 251                                   # that count's cap: beyond any hold, and "no detection yet"


def stream_boxes_runs_host(state, new_rects, closed, H, W, pads, T, hold):
    """One tick of one stream under the pass-through rule (`many.host_boxes_runs` on the finished video, however it is cut): what
    w2l_face_boxes_stream_runs computes per segment.  new_rects: a rect (x1, y1, x2, y2) or None per new frame.  Returns (boxes
    int64 [new_final_count, 4], zeros on gap rows; valid bool [new_final_count]; the next state).  The frames written are
    `final_range`'s.  A boxed frame whose next T - 1 frames are boxed takes the forward mean of raw rows; any other boxed frame of
    the range lies in the tail of a run whose end b is known - frame b is a gap, or the video is closed - and takes
    `get_smoothened_boxes`' in-place window over that run.  The tail of a run that ended up to T - 2 frames before this tick reads
    back to b - T, so the state is (frames seen, frames since the last detection capped at HOLD_FAR, the last min(seen,
    2 * max(T, 1)) held-filled rects, None for a gap frame)."""
    seen, dist, carry = (0, HOLD_FAR, []) if state is None else state
    top, bottom, left, right = pads
    Tm = max(T, 1)
    assert len(carry) == min(seen, 2 * Tm)
    held = list(carry)
    last = held[-1] if held else None                       # the rect being held: a gap ends the hold for good
    for r in new_rects:
        if r is not None:
            last, dist = tuple(int(v) for v in r), 0
        else:
            dist = min(dist + 1, HOLD_FAR)
            if dist > hold:
                last = None
        held.append(last)
    n = seen + len(new_rects)
    base = n - len(held)                                    # held[h] is frame base + h

    def boxed(i):
        return base <= i < n and held[i - base] is not None

    def pad(i):
        r = held[i - base]
        return [max(0, r[1] - top), min(H, r[3] + bottom), max(0, r[0] - left), min(W, r[2] + right)]

    tails = {}

    def tail(b):
        """the rows that run in order of the run that ends at b: {frame: box}"""
        if b not in tails:
            a = b
            while b - a < Tm and boxed(a - 1):
                a -= 1
            length = b - a                                  # min(the run's length, T)
            ws = a if length == Tm else a + max(0, 2 * length - Tm)     # a run shorter than T: Python's wrapped boxes[len - T:]
            window, out = [pad(i) for i in range(ws, b)], {}
            for i in range(a, b):
                mean = [_mean([w[c] for w in window]) for c in range(4)]
                if i >= ws:
                    window[i - ws] = mean
                out[i] = mean
            tails[b] = out
        return tails[b]

    lo, hi = final_range(seen, len(new_rects), closed, Tm)
    boxes, valid = np.zeros((hi - lo, 4), dtype=np.int64), np.zeros(hi - lo, dtype=bool)
    for i in range(lo, hi):
        if not boxed(i):
            continue
        valid[i - lo] = True
        if all(boxed(i + j) for j in range(Tm)):
            boxes[i - lo] = [_mean([pad(i + j)[c] for j in range(Tm)]) for c in range(4)]
            continue
        b = i + 1
        while boxed(b):
            b += 1
        assert b < n or closed, "a run's end is known for every frame of the range"
        boxes[i - lo] = tail(b)[i]
    keep = min(n, 2 * Tm)
    return boxes, valid, (n, dist, held[len(held) - keep:])


def runs_carry_words(state):
    """a state of `stream_boxes_runs_host` as the words of its carry slot that are in use: (rows int [k,5], frames since the
    last detection)"""
    _, dist, rows = state
    return np.array([list(r) + [1] if r is not None else [0] * 5 for r in rows], dtype=np.int64).reshape(-1, 5), dist
