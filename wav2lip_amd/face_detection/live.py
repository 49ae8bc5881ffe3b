"""The finish of `inference.face_detect` for a video that arrives a few frames at a time: what
w2l_face_boxes_stream (csrc/detect.hip) computes per segment, stated on the host.  Pure Python on integers; no device in it.

`get_smoothened_boxes` (inference.py:59-66) looks FORWARD: box i <= n - T is the mean of the padded rects i .. i + T - 1, all still
unsmoothed when it is taken (the loop runs in place and in order), so it is final once T - 1 more frames have been detected,
whatever comes later.  Only the boxes after n - T depend on the end of the video, through the in-place window `boxes[n - T:]`; the
one already-smoothed entry of that window, n - T, has a window that is entirely forward, so it can be computed again from raw
rects.  A stream therefore carries nothing but its last max(T, 1) RAW rects from tick to tick, and its boxes are `face_detect`'s
on the finished video however the video was cut into ticks.
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
