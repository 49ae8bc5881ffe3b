"""A model of "every face of a shot"  in plain Python and numpy, written from the rule and importing nothing from the
product: what w2l_face_tracks_all_segments must compute, bit for bit, and what the product's `host_all_tracks` must compute too.
Shared by tests/test_faces_cpu.py and the two GPU test files.

    model_faces    the F track slots over the arenas of one segment (cands [n,K,4], ncand [n], cflags [n]), with the status words
                   and, per frame, what happened (for tests that must not pass vacuously)
    slot_order     the same walk with slot-order matching - NOT the rule; the crossing case must tell the two apart
    CASES          the hand-made cases, one per edge of the rule; random_case() the random ones
"""
from fractions import Fraction

import numpy as np

NONE, FOUND, HOST = 0, 1, 2


def inter_union(c, ref):
    w = max(0, min(c[2], ref[2]) - max(c[0], ref[0]))
    h = max(0, min(c[3], ref[3]) - max(c[1], ref[1]))
    inter = w * h
    return inter, (c[2] - c[0]) * (c[3] - c[1]) + (ref[2] - ref[0]) * (ref[3] - ref[1]) - inter


def overlaps(c, ref, q):
    inter, union = inter_union(c, ref)
    return inter > 0 and inter * 256 >= q * union


def model_faces(cands, ncand, cflags, F, L, q, slot_order=False, seeds=None):
    """-> (rects int64 [F,n,4], flags int64 [F,n], (started, dropped, peak), events: one set of words per frame out of "host",
    "match", "tie_slot", "tie_cand", "miss", "freed", "seed", "reseed", "drop"); a list given as `seeds` receives (slot, frame) of
    every track that starts"""
    cands = np.asarray(cands).astype(np.int64)
    n, K = cands.shape[:2]
    rects, flags = np.zeros((F, n, 4), np.int64), np.zeros((F, n), np.int64)
    ref, alive, missed = [None] * F, [False] * F, [0] * F
    started = dropped = peak = 0
    events = []
    for i in range(n):
        ev = set()
        events.append(ev)
        if int(cflags[i]) not in (NONE, FOUND):
            flags[:, i] = HOST
            ev.add("host")
            continue
        m = min(max(int(ncand[i]), 0), K) if int(cflags[i]) == FOUND else 0
        frame = [tuple(int(v) for v in cands[i, c]) for c in range(m)]
        in_s, in_c = {s for s in range(F) if alive[s]}, set(range(m))
        got = {}
        while True:
            pairs = [(s, c) for s in sorted(in_s) for c in sorted(in_c) if overlaps(frame[c], ref[s], q)]
            if not pairs:
                break
            if slot_order:
                pairs = [p for p in pairs if p[0] == pairs[0][0]]
            iou = {p: Fraction(*inter_union(frame[p[1]], ref[p[0]])) for p in pairs}
            top = max(iou.values())
            tied = [p for p in pairs if iou[p] == top]          # in (slot, candidate) order
            if len({s for s, _ in tied}) > 1:
                ev.add("tie_slot")
            if len([p for p in tied if p[0] == tied[0][0]]) > 1:
                ev.add("tie_cand")
            s, c = tied[0]
            got[s] = frame[c]
            ref[s], missed[s] = frame[c], 0
            in_s.discard(s)
            in_c.discard(c)
            ev.add("match")
        freed = set()
        for s in sorted(in_s):
            missed[s] += 1
            ev.add("miss")
            if missed[s] > L:
                alive[s] = False
                freed.add(s)
                ev.add("freed")
        for c in sorted(in_c):
            free = [s for s in range(F) if not alive[s]]
            if not free:
                dropped += 1
                ev.add("drop")
                continue
            s = free[0]
            ref[s], alive[s], missed[s], got[s] = frame[c], True, 0, frame[c]
            started += 1
            if seeds is not None:
                seeds.append((s, i))
            ev.add("reseed" if s in freed else "seed")
        peak = max(peak, sum(alive))
        for s, r in got.items():
            rects[s, i], flags[s, i] = r, FOUND
    return rects, flags, (started, dropped, peak), events


def pack(frames, K):
    """frames: [(candidates, flag) or (candidates, flag, ncand)] -> the arenas (cands int32 [n,K,4], ncand int32 [n], cflags int32
    [n]); candidates beyond K are not there at all, and a given ncand is written as it stands"""
    n = len(frames)
    cands, ncand, cflags = np.zeros((n, K, 4), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, fr in enumerate(frames):
        c = list(fr[0])[:K]
        cflags[i] = fr[1]
        if c:
            cands[i, :len(c)] = np.asarray(c, np.int32).reshape(-1, 4)
        ncand[i] = fr[2] if len(fr) > 2 else (len(c) if fr[1] == FOUND else 0)
    return cands, ncand, cflags


def found(*cands):
    return (list(cands), FOUND)


NO_FACE = ([], NONE)
HOST_FRAME = ([(1, 2, 3, 4)], HOST, 1)                      # its candidate words must not be looked at
A, B, FAR = (0, 0, 20, 20), (10, 0, 30, 20), (100, 100, 130, 140)
X, Y = (8, 0, 28, 20), (14, 0, 34, 20)                      # X is nearer to B than to A, and nearer to A than Y is
POINT = (15, 15, 15, 15)
BIG, BIG2 = (0, 0, 32767, 32767), (1, 1, 32767, 32767)


def moved(r, d):
    return (r[0] + d, r[1], r[2] + d, r[3])


def spread(k):
    """k rects well apart from each other"""
    return [(40 * j, 0, 40 * j + 20, 20) for j in range(k)]


# name -> (F, K, L, q, frames, events that must occur somewhere, (started, dropped, peak) or None)
CASES = {
    # best pair first: slot 1 takes X (IoU 360/440), then slot 0 takes Y; slot order would give X to slot 0
    "crossing": (2, 4, 0, 32, [found(A, B), found(X, Y)], {"match"}, (2, 0, 2)),
    # one candidate halfway between two refs: inter 200, union 600 towards both -> the lower slot; the other slot misses
    "tie_two_slots": (2, 4, 3, 64, [found((0, 0, 20, 20), (20, 0, 40, 20)), found((10, 0, 30, 20))], {"tie_slot", "miss"}, (2, 0, 2)),
    # two candidates of equal IoU towards one ref -> the lower candidate; the other one seeds slot 1
    "tie_two_cands": (2, 4, 0, 64, [found((20, 20, 40, 40)), found((30, 20, 50, 40), (10, 20, 30, 40))], {"tie_cand", "seed"}, (2, 0, 2)),
    # equal IoU from different (inter, union): 400/800 against 200/400, cross-multiplied
    "tie_cross_multiplied": (1, 4, 0, 64, [found((20, 20, 40, 40)), found((20, 20, 40, 30), (20, 20, 40, 60))], {"tie_cand", "drop"},
                             (1, 1, 1)),
    "more_candidates_than_slots": (2, 8, 0, 64, [found(*spread(5)), found(*spread(5)[::-1])], {"drop", "match"}, (2, 6, 2)),
    "all_sixteen_slots": (16, 16, 0, 64, [found(*spread(16)), found(*spread(16)[::-1]), NO_FACE, found(*spread(3))],
                          {"match", "freed", "seed"}, (19, 0, 16)),
    # L = 2: two missed frames are survived, the third frees the slot and the far candidate seeds it in that same frame
    "freed_after_L_plus_1_and_seeded_again": (1, 4, 2, 64, [found(A), NO_FACE, NO_FACE, found(FAR)], {"freed", "reseed"}, (2, 0, 1)),
    "freed_with_two_slots": (2, 4, 1, 64, [found(A, FAR), found(FAR), found(moved(FAR, 1), (60, 60, 70, 70))], {"freed", "reseed"},
                             (3, 0, 2)),
    "a_miss_of_exactly_L_is_survived": (1, 4, 2, 64, [found(A), NO_FACE, NO_FACE, found(moved(A, 2))], {"miss", "match"}, (1, 0, 1)),
    "L_25_survived": (2, 3, 25, 64, [found(A)] + [NO_FACE] * 25 + [found(moved(A, 1))], {"match"}, (1, 0, 1)),
    "L_25_lost": (2, 3, 25, 64, [found(A)] + [NO_FACE] * 26 + [found(moved(A, 1))], {"freed", "seed"}, (2, 0, 1)),
    "L_250_survived": (2, 3, 250, 64, [found(A)] + [NO_FACE] * 250 + [found(moved(A, 1))], {"match"}, (1, 0, 1)),
    "L_250_lost": (2, 3, 250, 64, [found(A)] + [NO_FACE] * 251 + [found(moved(A, 1))], {"freed"}, (2, 0, 1)),
    # a zero-area candidate seeds a track and never continues it, not even by itself
    "zero_area": (2, 4, 0, 1, [found(POINT), found(POINT), found((12, 10, 12, 20), A)], {"reseed", "seed"}, (4, 0, 2)),
    "zero_area_held": (2, 4, 1, 1, [found(POINT), found(POINT), found(POINT)], {"miss", "freed", "seed"}, (3, 0, 2)),
    "coordinates_at_32767": (2, 4, 0, 255, [found(BIG, (32767, 32767, 32767, 32767)), found(BIG2, (32766, 0, 32767, 32767)),
                                            found((0, 0, 32767, 32766), BIG)], {"match", "seed"}, None),
    # ref 256 x 1 and a candidate q x 1 inside it: inter * 256 == q * union exactly; one pixel less is no overlap
    "q_1_at_the_threshold": (1, 2, 5, 1, [found((0, 0, 256, 1)), found((0, 0, 1, 1))], {"match"}, (1, 0, 1)),
    "q_1_touching": (1, 2, 5, 1, [found((0, 0, 256, 1)), found((256, 0, 300, 1))], {"miss"}, (1, 1, 1)),
    "q_256_same_rect": (1, 2, 5, 256, [found(A), found(moved(A, 1), A)], {"match"}, (1, 1, 1)),
    "q_256_one_pixel_off": (1, 2, 5, 256, [found(A), found(moved(A, 1))], {"miss", "drop"}, (1, 1, 1)),
    "q_128_at_and_below": (2, 2, 0, 128, [found((0, 0, 256, 1)), found((0, 0, 127, 1), (0, 0, 128, 1))], {"match", "seed"}, (2, 0, 2)),
    # L = 1: the host frame is not a miss (started stays 1), and the state is carried across it
    "host_frame_is_not_a_miss": (2, 4, 1, 64, [found(A), HOST_FRAME, NO_FACE, found(moved(A, 1))], {"host", "miss", "match"}, (1, 0, 1)),
    "host_frame_control": (2, 4, 1, 64, [found(A), NO_FACE, NO_FACE, found(moved(A, 1))], {"freed", "seed"}, (2, 0, 1)),
    "host_frames_only": (3, 4, 0, 64, [HOST_FRAME, HOST_FRAME], {"host"}, (0, 0, 0)),
    # ncand beyond K counts as K, a negative one as 0; a frame flagged "none" has no candidates whatever ncand says
    "ncand_beyond_K": (4, 3, 0, 64, [(spread(3), FOUND, 9), (spread(3), FOUND, 1 << 30)], {"seed", "match"}, (3, 0, 3)),
    "ncand_negative": (4, 3, 1, 64, [found(*spread(2)), (spread(3), FOUND, -3), (spread(3), NONE, 3), found(*spread(3))],
                       {"miss", "freed", "seed"}, (5, 0, 3)),
}

LENGTHS = (0, 1, 2, 3, 5, 64, 65, 130)
KS, FS, LS, QS = (1, 3, 16), (1, 2, 4, 16), (0, 1, 25, 250), (1, 64, 256)


def random_case(rng, n, K, hi=40, p_host=0.05, p_none=0.2):
    """n frames of 0..K random candidates with coordinates in 0..hi, some of them copies of the frame before's (tracks that
    continue, ties of every kind), some frames empty, some left to the host"""
    frames, last = [], []
    for _ in range(n):
        u = rng.random()
        if u < p_host:
            frames.append(HOST_FRAME)
            continue
        if u < p_host + p_none:
            frames.append(NO_FACE)
            continue
        k = int(rng.integers(1, K + 1))
        cands = []
        for _ in range(k):
            v = rng.random()
            if last and v < 0.5:                            # a rect of the frame before, moved a little or not at all
                r = last[int(rng.integers(0, len(last)))]
                d = int(rng.integers(0, 3))
                cands.append((r[0] + d, r[1], r[2] + d, r[3]))
            elif cands and v < 0.6:
                cands.append(cands[int(rng.integers(0, len(cands)))])
            else:
                xa, xb = sorted(int(v) for v in rng.integers(0, hi + 1, 2))
                ya, yb = sorted(int(v) for v in rng.integers(0, hi + 1, 2))
                cands.append((xa, ya, xb, yb))
        order = rng.permutation(len(cands))
        cands = [cands[j] for j in order]
        frames.append(found(*cands))
        last = cands
    return frames


def random_cases(seed=0):
    """[(F, K, L, q, [frames per segment: one of every length of LENGTHS])] for every K and F, L and q cycling through their values"""
    out = []
    for j, (K, F) in enumerate((K, F) for K in KS for F in FS):
        rng = np.random.default_rng([seed, K, F])
        out.append((F, K, LS[j % 4], QS[j % 3], [random_case(rng, n, K) for n in LENGTHS]))
    return out
