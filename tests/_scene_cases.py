"""A model of scene-cut detection in plain numpy, written from the rule and importing nothing from the product: what
w2l_frame_hist_rows and w2l_scene_cuts must compute, bit for bit, what the product's host statements must compute too, and the
composed rule - today's models of the hold (tests/_noface_cases.py) and of the track (tests/_track_cases.py) applied per shot.
Shared by tests/test_scene_cpu.py and the two GPU test files, with the clips they run on.

The rule.  thresh in [1/256, 1), q = int(thresh * 256) in 1..255.
  1. signature: a frame is H * W * 3 contiguous bytes, BGR interleaved; byte j belongs to channel j % 3 and bin byte >> 3;
     sig[c * 32 + b] counts them: 96 words, every channel sums to H * W.
  2. distance: D(i) = sum_k |sig_i[k] - sig_{i-1}[k]|.
  3. cut: frame i >= 1 starts a new shot iff D(i) * 256 > q * 6 * H * W; frame 0 never does.
  4. every maximal range [a, b) between cuts is handled exactly as a clip of those frames alone.
"""
import numpy as np

import _noface_cases as nf
import _track_cases as tc

WORDS, BINS = 96, 32
NO_FACE = 'Face not detected! Ensure the video contains a face in all the frames.'


def signature(frame):
    """uint8 [H,W,3] -> int64 [96]: np.bincount per channel"""
    f = np.asarray(frame)
    assert f.dtype == np.uint8 and f.ndim == 3 and f.shape[2] == 3
    return np.concatenate([np.bincount(f[:, :, c].reshape(-1) >> 3, minlength=BINS) for c in range(3)]).astype(np.int64)


def signatures(frames):
    return np.stack([signature(f) for f in frames]).reshape(-1, WORDS) if len(frames) else np.zeros((0, WORDS), np.int64)


def distance_rows(sig):
    """int64 [n]: D per frame, 0 for frame 0 (Python ints underneath: no overflow to think about)"""
    sig = [[int(v) for v in row] for row in np.asarray(sig).reshape(-1, WORDS)]
    return np.array([0] + [sum(abs(a - b) for a, b in zip(sig[i], sig[i - 1])) for i in range(1, len(sig))], dtype=np.int64)[:len(sig)]


def cut_flags(sig, H, W, q):
    """(cuts [n] of 0 / 1, D [n])"""
    d = distance_rows(sig)
    cuts = [1 if i > 0 and int(d[i]) * 256 > q * 6 * H * W else 0 for i in range(len(d))]
    return np.array(cuts, dtype=np.int64), d


def shots(n, cuts):
    out, a = [], 0
    for i in range(1, n):
        if cuts[i]:
            out.append((a, i))
            a = i
    return out + [(a, n)] if n > 0 else []


def q_of(thresh):
    return int(thresh * 256)


# ---------------------------------------------------------------- the composed rule
def finish_clip(rects, H, W, pads, T, hold):
    """today's finish of ONE clip from its rects (None: no face): a list of (y1, y2, x1, x2) tuples, None for a gap frame under a
    hold; in the strict mode the text of the error when a frame has no face"""
    if hold is None:
        if any(r is None for r in rects):
            return NO_FACE
        return [tuple(int(v) for v in b) for b in nf.finish(rects, H, W, pads, T)]
    boxes, valid = nf.model(rects, H, W, pads, T, hold)
    return [tuple(int(v) for v in b) if ok else None for b, ok in zip(boxes, valid)]


def finish_shots(rects, shot_list, H, W, pads, T, hold):
    """the composed rule on the rects of a clip: every shot finished as a clip of its own; in the strict mode a frame without a face
    in any shot is the clip's error"""
    out = []
    for a, b in shot_list:
        part = finish_clip(rects[a:b], H, W, pads, T, hold)
        if isinstance(part, str):
            return part
        out += part
    return out


def track_shots(cands_per_frame, shot_list, pick, L, q):
    """the track's model per shot, a fresh state at every shot's start: frames = [(candidates, flag)] -> a rect tuple or None per
    frame"""
    out = []
    for a, b in shot_list:
        r, f, _, _ = tc.model_track(cands_per_frame[a:b], pick, L, q)
        out += [tuple(int(v) for v in x) if y == tc.FOUND else None for x, y in zip(r, f)]
    return out


# ---------------------------------------------------------------- frames and clips
def flat_frame(H, W, bgr):
    f = np.empty((H, W, 3), np.uint8)
    f[:] = bgr
    return f


CONTENTS = ("zeros", "full", "edges", "ramp", "random", "channels")


def content(kind, H, W, rng):
    """a frame of H x W of one of CONTENTS: all 0; all 255; bytes alternating 7 and 8 (the edge between bins 0 and 1); a byte ramp;
    random bytes; one constant per channel (a wrong channel phase moves whole counts between channels)"""
    n = H * W * 3
    if kind == "zeros":
        flat = np.zeros(n, np.uint8)
    elif kind == "full":
        flat = np.full(n, 255, np.uint8)
    elif kind == "edges":
        flat = np.where(np.arange(n) % 2 == 0, 7, 8).astype(np.uint8)
    elif kind == "ramp":
        flat = (np.arange(n) % 256).astype(np.uint8)
    elif kind == "random":
        flat = rng.integers(0, 256, n, dtype=np.uint8)
    elif kind == "channels":
        flat = np.tile(np.array([10, 100, 200], np.uint8), H * W)
    else:
        raise KeyError(kind)
    return flat.reshape(H, W, 3)


def unused_byte(frame):
    """a byte value from a bin the frame does not use (a poison for the bytes around it), or None when it uses all 32"""
    used = set((np.asarray(frame).reshape(-1) >> 3).tolist())
    free = [b for b in range(BINS) if b not in used]
    return None if not free else free[len(free) // 2] * 8 + 3


def sig_with_distance(H, W, d, base=None):
    """two signatures of H x W frames whose distance is exactly d (even, 0 <= d <= 6 H W): pixels move between bins, channel after
    channel"""
    assert d % 2 == 0 and 0 <= d <= 6 * H * W
    a = np.zeros(WORDS, np.int64)
    for c in range(3):
        a[c * BINS + (3 if base is None else base)] = H * W
    b, left = a.copy(), d // 2
    for c in range(3):
        move = min(left, H * W)
        b[c * BINS + (3 if base is None else base)] -= move
        b[c * BINS + 20] += move
        left -= move
    assert left == 0
    return a, b
