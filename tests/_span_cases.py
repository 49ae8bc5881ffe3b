"""The span rule for finished clips, stated twice in plain numpy / Python for the tests,
and the cases the tests run it on.  Written from the rule's text; nothing of the product is imported here.

The rule, per segment of n rows with rects (x1, y1, x2, y2) and flags, integers only, with bridge B, min_len M, min_size S:
  - a row whose flag is neither 0 nor 1 leaves the segment to the host: status (2, first such row), rects and flags copied, no
    span row written;
  - a row flagged 1 is detected.  For detected rows p < q with no detected row between them and 2 <= q - p <= B + 1 every row
    p < i < q is bridged with (r_p * (q - i) + r_q * (i - p)) // (q - p) per coordinate.  Every other row is a gap;
  - a span is a maximal sequence of detected and bridged rows, L long; kept iff L >= M and max(sum(x2 - x1), sum(y2 - y1)) >= S * L;
  - rows of kept spans: flag 1 and the rect; every other row: flag 0 and zeros;
  - span row t of the segment: (first row, L, number of detected rows, 0) of the t-th kept span, zeros from the kept count on;
  - status (0, kept count).
"""
import numpy as np

LENGTHS = (1, 2, 63, 64, 65, 128, 129, 300)
BRIDGES = (0, 1, 25, 250)
BIG = 2 ** 31 - 1


def model(rects, flags, B, M, S):
    """(rects_out int64 [n,4], flags_out int64 [n], span rows int64 [n,4] or None when left to the host, status (code, value))"""
    rects, flags = np.asarray(rects, dtype=np.int64).reshape(-1, 4), np.asarray(flags, dtype=np.int64).reshape(-1)
    n = len(flags)
    host = np.flatnonzero((flags != 0) & (flags != 1))
    if len(host):
        return rects.copy(), flags.copy(), None, (2, int(host[0]))
    det, at = flags == 1, np.arange(n)
    p = np.maximum.accumulate(np.where(det, at, -1))                            # the last detected row at or before i
    q = np.minimum.accumulate(np.where(det, at, n)[::-1])[::-1]                 # the first one at or after i
    inside = (p >= 0) & (q < n) & (q - p <= B + 1)
    pc, qc = np.clip(p, 0, n - 1), np.clip(q, 0, n - 1)
    d = np.where(det | ~inside, 1, q - p)
    mix = (rects[pc] * (q - at)[:, None] + rects[qc] * (at - p)[:, None]) // d[:, None]
    out = np.where(inside[:, None], np.where(det[:, None], rects, mix), 0)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], inside.astype(np.int8), [0]))))
    spans, keep = np.zeros((n, 4), np.int64), np.zeros(n, bool)
    t = 0
    for a, b in zip(edges[::2].tolist(), edges[1::2].tolist()):
        L = b - a
        sw, sh = int((out[a:b, 2] - out[a:b, 0]).sum()), int((out[a:b, 3] - out[a:b, 1]).sum())
        if L >= M and max(sw, sh) >= S * L:
            spans[t] = (a, L, int(det[a:b].sum()), 0)
            keep[a:b] = True
            t += 1
    return np.where(keep[:, None], out, 0), keep.astype(np.int64), spans, (0, t)


def brute(rects, flags, B, M, S):
    """the same rule row by row in Python ints: every row looks for its detections itself, spans are collected in one walk"""
    rects = [[int(v) for v in r] for r in np.asarray(rects).reshape(-1, 4).tolist()]
    flags = [int(f) for f in np.asarray(flags).reshape(-1).tolist()]
    n = len(flags)
    for i, f in enumerate(flags):
        if f not in (0, 1):
            return np.array(rects, np.int64).reshape(-1, 4), np.array(flags, np.int64), None, (2, i)
    filled = []
    for i in range(n):
        if flags[i] == 1:
            filled.append(rects[i])
            continue
        p = next((j for j in range(i - 1, max(i - B - 1, -1), -1) if flags[j] == 1), None)
        q = next((j for j in range(i + 1, min(i + B + 1, n)) if flags[j] == 1), None)
        if p is None or q is None or q - p > B + 1:
            filled.append(None)
        else:
            filled.append([(rects[p][c] * (q - i) + rects[q][c] * (i - p)) // (q - p) for c in range(4)])
    rects_out, flags_out, spans = [[0] * 4 for _ in range(n)], [0] * n, []
    i = 0
    while i < n:
        if filled[i] is None:
            i += 1
            continue
        a = i
        while i < n and filled[i] is not None:
            i += 1
        L = i - a
        sw, sh = sum(r[2] - r[0] for r in filled[a:i]), sum(r[3] - r[1] for r in filled[a:i])
        if L >= M and sw >= S * L or L >= M and sh >= S * L:
            spans.append([a, L, sum(flags[a:i]), 0])
            rects_out[a:i], flags_out[a:i] = filled[a:i], [1] * L
    rows = np.zeros((n, 4), np.int64)
    rows[:len(spans)] = np.array(spans, np.int64).reshape(-1, 4)
    return np.array(rects_out, np.int64).reshape(-1, 4), np.array(flags_out, np.int64), rows, (0, len(spans))


def filled_rects(rects_out, flags_out):
    """the model's output as a list of rect tuples with None for the rows outside kept spans"""
    return [tuple(int(v) for v in r) if f else None for r, f in zip(rects_out, flags_out)]


# ---------------------------------------------------------------- the cases
def _rects(n, rng):
    """sizes 0..60 at corners 0..40: the rects reach beyond a 40 x 50 frame"""
    xy = rng.integers(0, 41, (n, 2))
    return np.concatenate([xy, xy + rng.integers(0, 61, (n, 2))], axis=1).astype(np.int64)


def _patterns(n, B, rng):
    alt = np.arange(n) % 2 == 0
    out = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "leading miss": np.arange(n) >= min(3, n - 1),
           "trailing miss": np.arange(n) < max(n - 3, 1), "alternating": alt, "alternating from a miss": ~alt,
           "sparse": rng.random(n) < 0.1, "dense": rng.random(n) < 0.8}
    block = np.ones(n, bool)                       # misses of B and of B + 1 rows in turn
    i, k = 1, 0
    while i < n:
        miss = B + (k % 2)
        block[i:i + miss] = False
        i += miss + 2
        k += 1
    out["blocks"] = block
    return out


def _case(name, found, rng, rects=None):
    found = np.asarray(found, dtype=bool)
    return name, _rects(len(found), rng) if rects is None else np.asarray(rects, np.int64), found.astype(np.int64)


def groups(seed=0):
    """[((B, M, S), [(name, rects int64 [n,4], flags int64 [n])])]: the segments of one launch share its parameters"""
    rng = np.random.default_rng(seed)
    out = []
    for B in BRIDGES:
        plain = []
        for n in LENGTHS:
            for name, found in _patterns(n, B, rng).items():
                plain.append(_case("%d %s" % (n, name), found, rng))
        plain.append(_case("miss of B", [1, 1] + [0] * B + [1, 1], rng))
        plain.append(_case("miss of B+1", [1, 1] + [0] * (B + 1) + [1, 1], rng))
        plain.append(_case("miss across a chunk", [i in (62, 66) for i in range(70)], rng))
        plain.append(_case("detections at 0 and 251", [i in (0, 251) for i in range(252)], rng))
        plain.append(_case("detections at 0 and 252", [i in (0, 252) for i in range(253)], rng))
        big = _rects(252, rng)
        big[0], big[251] = (0, 5, BIG, BIG - 2), (BIG - 7, 0, BIG, BIG)
        plain.append(_case("coordinates up to 2^31 - 1", [i in (0, 251) for i in range(252)], rng, big))
        big = np.full((300, 4), BIG, np.int64)
        big[:, :2] = rng.integers(0, 2, (300, 2))
        plain.append(_case("sizes of 2^31 - 1", rng.random(300) < 0.5, rng, big))
        host = _case("a flag-2 row", rng.random(70) < 0.7, rng)
        host[2][[13, 64]] = 2
        plain.append(host)
        out.append(((B, 1, 0), plain))
        # lengths and sizes that decide: spans around M = 4 rows, sizes around S = 30 (the sizes are uniform in 0..60)
        out.append(((B, 4, 30), [_case("%d %s, M 4, S 30" % (n, name), found, rng) for n in (1, 65, 129, 300)
                                 for name, found in _patterns(n, B, rng).items() if name in ("dense", "sparse", "blocks", "all")]))
    # M equal to a span's length and one above it: spans of 7 (one of them bridged over two rows, B = 2), 8 and 70 rows
    found = [0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0] + [1, 1, 0, 0, 1, 1, 1] + [0] * 3 + [1] * 8 + [0] * 3 + [1] * 70 + [0]
    for M in (7, 8, 9, 70, 71):
        out.append(((2, M, 0), [_case("spans of 7, 7, 8 and 70 rows, M %d" % M, found, rng)]))
    # S at, and one above, a span's exact max(sw, sh) / L: widths 10, 11, 12 (sw = 33, L = 3) over heights of 4: the mean is 11
    r = np.array([[5, 5, 15, 9], [5, 5, 16, 9], [5, 5, 17, 9]], np.int64)
    tall = r[:, [1, 0, 3, 2]]
    # ... and a mean that is no integer: widths 10, 11 (sw = 21, L = 2, mean 10.5): kept at S = 10, dropped at 11
    half = r[:2]
    for S in (10, 11, 12):
        out.append(((0, 1, S), [_case("mean width 11, S %d" % S, [1, 1, 1], rng, r), _case("mean height 11, S %d" % S, [1, 1, 1], rng, tall),
                                _case("mean width 10.5, S %d" % S, [1, 1], rng, half),
                                _case("bridged mean, S %d" % S, [1, 0, 1], rng, r)]))     # B = 0: two spans of one row, 10 and 12 wide
    out.append(((1, 1, 11), [_case("bridged mean 11 with B 1", [1, 0, 1], rng, r)]))
    out.append(((1, 1, 12), [_case("bridged mean 11 with B 1, S 12", [1, 0, 1], rng, r)]))
    out.append(((250, 1 << 30, 32767), [_case("the largest M and S", np.ones(300, bool), rng)]))
    return out
