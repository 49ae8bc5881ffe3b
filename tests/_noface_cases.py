"""The pass-through rule for frames without a face, stated once more in numpy for the tests, and the clips the
tests run it on.  Written from the rule's text and the reference's inference.py:59-66 / :91-98; nothing of the product is
imported here.

The rule.  A clip has n frames of H x W; the detector gives per frame a rect (x1, y1, x2, y2) or None.
  1. hold: an undetected frame i takes the raw rect of the last detected frame p < i if i - p <= G, else it is a gap frame
     (frames before the first detection are gaps);
  2. runs: each maximal sequence of boxed frames is finished as `face_detect` finishes a clip of those frames alone - pads and
     clipping, then get_smoothened_boxes(T) in place, in order, truncating;
  3. gap frames have no box (zeros here) and valid 0.
The tick form: after a tick that brings a stream to n frames, the frames [max(0, seen - T' + 1), n if closed else
max(0, n - T' + 1)) with T' = max(T, 1) are final, and their boxes are those of the rule on the n frames so far: a frame of that
range is either T' - 1 boxed frames away from the end, so its forward window is complete, or its run has ended before n.
"""
import numpy as np

FH, FW = 40, 50
LENGTHS = (1, 4, 5, 9, 63, 64, 65, 130)
WINDOWS = (0, 1, 2, 5, 64)
HOLDS = (0, 1, 4, 250)
PADS = ((0, 10, 0, 0), (-2, 7, 5, -3))
HOLD_FAR = 251


def smoothened(boxes, T):
    """inference.py:59-66 on an integer array: in place, in order; the assignment truncates the float64 mean"""
    for i in range(len(boxes)):
        if i + T > len(boxes):
            window = boxes[len(boxes) - T:]
        else:
            window = boxes[i:i + T]
        boxes[i] = np.mean(window, axis=0)
    return boxes


def finish(rects, H, W, pads, T):
    """inference.py:91-98 + :100 on the rects of one run, in the (y1, y2, x1, x2) order of `coords`"""
    pady1, pady2, padx1, padx2 = pads
    boxes = np.array([[max(0, r[1] - pady1), min(H, r[3] + pady2), max(0, r[0] - padx1), min(W, r[2] + padx2)] for r in rects],
                     dtype=np.int64).reshape(-1, 4)
    return smoothened(boxes, T) if T else boxes


def filled(rects, G):
    """step 1: ([rect or None per frame], frames since the last detection after the last frame, capped at HOLD_FAR)"""
    out, p = [], None
    for i, r in enumerate(rects):
        if r is not None:
            p = i
        out.append(tuple(int(v) for v in rects[p]) if p is not None and i - p <= G else None)
    return out, HOLD_FAR if p is None else min(len(rects) - 1 - p, HOLD_FAR)


def model(rects, H, W, pads, T, G):
    """(boxes int64 [n,4], valid bool [n]) of a whole clip"""
    held, _ = filled(rects, G)
    n = len(held)
    boxes, valid = np.zeros((n, 4), np.int64), np.array([h is not None for h in held], dtype=bool).reshape(n)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], valid.astype(np.int8), [0]))))
    for a, b in zip(edges[::2], edges[1::2]):
        boxes[a:b] = finish(held[a:b], H, W, pads, T)
    return boxes, valid


def tick_range(seen, n, closed, T):
    Tm = max(T, 1)
    return max(0, seen - Tm + 1), n if closed else max(0, n - Tm + 1)


def model_tick(rects_so_far, seen, closed, H, W, pads, T, G):
    """the tick that brought a stream from `seen` frames to len(rects_so_far): (boxes, valid) of the frames of `tick_range`, and
    the carry the stream holds afterwards: (rows int64 [min(n, 2 T'), 5] of (x1, y1, x2, y2, boxed), frames since the last
    detection)"""
    n = len(rects_so_far)
    lo, hi = tick_range(seen, n, closed, T)
    boxes, valid = model(rects_so_far, H, W, pads, T, G)
    held, dist = filled(rects_so_far, G)
    keep = min(n, 2 * max(T, 1))
    rows = np.array([list(h) + [1] if h is not None else [0] * 5 for h in held[n - keep:]], dtype=np.int64).reshape(-1, 5)
    return boxes[lo:hi], valid[lo:hi], (rows, dist)


# ---------------------------------------------------------------- the clips
def flag_patterns(n, T, G, rng):
    """{name: found bool [n]}: the patterns every length is run with"""
    alt = np.arange(n) % 2 == 0
    out = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first missing": np.arange(n) > 0, "last missing": np.arange(n) < n - 1,
           "alternating": alt, "alternating from a miss": ~alt,
           "sparse": rng.random(n) < 0.25, "dense": rng.random(n) < 0.8}
    block = np.ones(n, bool)                       # misses in blocks of G + 1: the hold runs out on the block's last frame
    block[(np.arange(n) // (G + 1)) % 3 == 1] = False
    out["blocks"] = block
    return out


def special_flags(T, G):
    """found flags of the clips built around the two parameters: a miss of exactly G frames (held throughout) and of G + 1 (one
    gap frame), and runs of T - 1, T and T + 1 boxed frames between gaps"""
    out = {"miss of G": [1, 1] + [0] * G + [1, 1], "miss of G+1": [1, 1] + [0] * (G + 1) + [1, 1]}
    for length in sorted({max(T - 1, 1), max(T, 1), T + 1}):
        if length >= G + 1:
            # a run that a gap follows has held its last rect for G frames: length - G detections, G held frames, one gap frame
            unit = [1] * (length - G) + [0] * (G + 1)
            out["runs of %d" % length] = [0] + unit + unit + [1] * (length - G) + [0] * G
        else:
            # shorter than G + 1: only the clip's last run can be, one detection held to the end
            out["runs of %d" % length] = [1] + [0] * (G + 1) + [1] + [0] * (length - 1)
    return {k: np.array(v, dtype=bool) for k, v in out.items()}


def clip_rects(found, rng):
    """rects for the flags: coordinates in 0..70 reach beyond the 40 x 50 frame; None where nothing was found"""
    coords = rng.integers(0, 71, (len(found), 4)).tolist()
    return [tuple(c) if f else None for c, f in zip(coords, found)]


def all_clips(T, G, seed):
    """[(name, rects)] for one (T, G): every length with every pattern, then the special clips"""
    rng = np.random.default_rng(seed)
    clips = []
    for n in LENGTHS:
        for name, found in flag_patterns(n, T, G, rng).items():
            clips.append(("%d %s" % (n, name), clip_rects(found, rng)))
    for name, found in special_flags(T, G).items():
        clips.append((name, clip_rects(found, rng)))
    return clips


def stream_clips(T, G, seed):
    """a smaller set for the tick form: [(name, rects)]"""
    rng = np.random.default_rng(seed)
    clips = []
    for n, name in ((1, "none"), (4, "first missing"), (5, "alternating"), (9, "sparse"), (63, "dense"), (64, "blocks"),
                    (65, "last missing"), (130, "dense"), (130, "blocks"), (9, "all")):
        clips.append(("%d %s" % (n, name), clip_rects(flag_patterns(n, T, G, rng)[name], rng)))
    for name, found in special_flags(T, G).items():
        clips.append((name, clip_rects(found, rng)))
    return clips


def cuts(kind, n, T, rng):
    """frame counts per tick; the close comes with the last tick"""
    if kind == "whole":
        return [n]
    if kind in ("1", "T-1", "T"):
        step = {"1": 1, "T-1": max(T - 1, 1), "T": max(T, 1)}[kind]
        return [min(step, n - lo) for lo in range(0, n, step)] or [0]
    cut, pos = [0] if rng.integers(2) else [], 0
    while pos < n:
        c = min(int(rng.choice([0, 1, 1, 2, 3, 7, 40])), n - pos)
        cut.append(c)
        pos += c
    return (cut + [0]) if kind == "seeded, closed empty" or not cut else cut
