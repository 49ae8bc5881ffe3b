"""A model of tracked face selection in plain Python and numpy, written from the rule and importing nothing from
the product: what w2l_s3fd_top_rects and w2l_face_track_segments must compute, bit for bit, and what the product's
`host_top_rects` / `host_track` must compute too.  Shared by tests/test_track_cpu.py and the two GPU test files.

    model_top_rects   one image's candidates and flag from its box table and NMS keep list
    model_track       the track over a sequence of (candidates, flag) frames, with the state that is carried and, per frame, what
                      happened (for tests that must not pass vacuously)
"""
import numpy as np

NONE, FOUND, HOST = 0, 1, 2
PICKS = ("score", "largest", "left", "right")
FRESH = (0, 0, 0, 0, 0, 0, 0, 0)        # the eight state words: (x1, y1, x2, y2, has, missed, 0, 0)
MAX_COORD = 32767


def model_top_rects(table, keep, n, K, sx=1.0, sy=1.0):
    """table [P,5] float32, keep [P] int32, n the image's count -> (list of up to K (x1, y1, x2, y2) int tuples, flag)"""
    table = np.asarray(table, dtype=np.float32)
    P = len(table)
    if n < 0 or n > P:
        return [], HOST
    scale = np.array([sx, sy, sx, sy], dtype=np.float32)
    out = []
    for i in range(int(n)):
        row = int(keep[i])
        if row < 0 or row >= P:                 # examined: no K-th passing row came before it
            return [], HOST
        if not table[row, 4] > np.float32(0.5):
            continue
        prod = table[row, :4] * scale           # float32 * float32, one rounding
        rect = []
        for v in prod:
            if np.isnan(v):
                return [], HOST
            v = v if v > 0 else np.float32(0)
            if not v < np.float32(2.0 ** 31):
                return [], HOST
            v = int(v)
            if v > MAX_COORD:
                return [], HOST
            rect.append(v)
        out.append(tuple(rect))
        if len(out) == K:
            break                               # rows after the K-th passing row are not looked at
    return out, (FOUND if out else NONE)


def area(r):
    return (r[2] - r[0]) * (r[3] - r[1])


def inter_union(c, ref):
    w = max(0, min(c[2], ref[2]) - max(c[0], ref[0]))
    h = max(0, min(c[3], ref[3]) - max(c[1], ref[1]))
    inter = w * h
    return inter, area(c) + area(ref) - inter


def overlaps(c, ref, q):
    inter, union = inter_union(c, ref)
    return inter > 0 and inter * 256 >= q * union


def seed_index(cands, pick):
    best = 0
    for k in range(1, len(cands)):
        a, b = cands[k], cands[best]
        if pick == "largest" and area(a) > area(b):
            best = k
        elif pick == "left" and a[0] + a[2] < b[0] + b[2]:
            best = k
        elif pick == "right" and a[0] + a[2] > b[0] + b[2]:
            best = k
    return best                                 # "score": candidate 0; every tie stays with the lower index


def seed_tied(cands, pick):
    """does another candidate tie with the seed under `pick`?"""
    key = {"largest": area, "left": lambda r: r[0] + r[2], "right": lambda r: r[0] + r[2]}.get(pick)
    if key is None:
        return False
    s = seed_index(cands, pick)
    return any(k != s and key(c) == key(cands[s]) for k, c in enumerate(cands))


def model_track(frames, pick, L, q, state=None):
    """frames: [(candidates, flag)] in order; state: eight words or None for a clip's start -> (rects int [n,4], flags int [n],
    the eight state words afterwards, events: one set of words per frame out of "host", "continue", "iou_tie", "miss", "lost",
    "reseed", "seed", "seed_tie", "none")"""
    x1, y1, x2, y2, has, missed = (FRESH if state is None else tuple(int(v) for v in state))[:6]
    ref = (x1, y1, x2, y2)
    rects, flags, events = [], [], []
    for cands, flag in frames:
        ev = set()
        if flag not in (NONE, FOUND):
            rects.append((0, 0, 0, 0))
            flags.append(HOST)
            events.append({"host"})
            continue
        cands = list(cands) if flag == FOUND else []
        chosen = None
        if has:
            best = None
            for k, c in enumerate(cands):
                if not overlaps(c, ref, q):
                    continue
                if best is None:
                    best = k
                    continue
                ia, ua = inter_union(c, ref)
                ib, ub = inter_union(cands[best], ref)
                if ia * ub > ib * ua:
                    best = k
                    ev.discard("iou_tie")
                elif ia * ub == ib * ua:
                    ev.add("iou_tie")           # the lower index keeps it
            if best is not None:
                chosen = cands[best]
                ev.add("continue")
            else:
                ev.add("miss")
                missed += 1
                if missed > L:
                    has = 0
                    ev.add("lost")
        if chosen is None and not has:
            if cands:
                chosen = cands[seed_index(cands, pick)]
                ev.add("reseed" if "lost" in ev else "seed")
                if seed_tied(cands, pick):
                    ev.add("seed_tie")
        if chosen is not None:
            ref, has, missed = chosen, 1, 0
            rects.append(chosen)
            flags.append(FOUND)
        else:
            rects.append((0, 0, 0, 0))
            flags.append(NONE)
            ev.add("none")
        events.append(ev)
    words = (ref[0], ref[1], ref[2], ref[3], 1, missed, 0, 0) if has else FRESH
    return np.array(rects, dtype=np.int64).reshape(-1, 4), np.array(flags, dtype=np.int64), words, events


def random_clip(rng, n, K, hi=40, p_host=0.0):
    """n frames of 0..K random candidates with coordinates in 0..hi: overlaps, ties and misses are all frequent"""
    frames = []
    for _ in range(n):
        if rng.random() < p_host:
            frames.append(([], HOST))
            continue
        k = int(rng.integers(0, K + 1))
        cands = []
        for _ in range(k):
            if cands and rng.random() < 0.15:   # an exact copy of an earlier candidate: ties of every kind, resolved by the index
                cands.append(cands[int(rng.integers(0, len(cands)))])
                continue
            xa, xb = (int(v) for v in rng.integers(0, hi + 1, 2))
            ya, yb = (int(v) for v in rng.integers(0, hi + 1, 2))
            if rng.random() < 0.9:              # the rest: rects with a negative side, which the rule must take as they are
                xa, xb, ya, yb = min(xa, xb), max(xa, xb), min(ya, yb), max(ya, yb)
            cands.append((xa, ya, xb, yb))
        frames.append((cands, FOUND if k else NONE))
    return frames


def pack_frames(frames, K):
    """the arenas w2l_s3fd_top_rects would have written for `frames`: (cands int32 [n,K,4], ncand int32 [n], flags int32 [n])"""
    n = len(frames)
    cands, ncand, flags = np.zeros((n, K, 4), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, (c, f) in enumerate(frames):
        flags[i] = f
        if f == FOUND:
            ncand[i] = len(c)
            cands[i, :len(c)] = np.asarray(c, np.int32).reshape(-1, 4)
    return cands, ncand, flags
