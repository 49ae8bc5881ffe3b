"""The key-frame rule, stated in plain numpy for the tests, and the cases the tests
run it on.  Written from the rule's text; nothing of the product is imported here.

The rule, per segment of n >= 1 frames at stride N, integers only:
  - the key frames are 0, N, 2N, ... below n, and n - 1: m = (n - 1 + N - 1) // N + 1 of them, key j at pos(j) = min(j * N, n - 1);
    the inputs are the m key rows: rects (x1, y1, x2, y2) and flags (0 none, 1 found, 2 the host must decide);
  - row pos(j) is key row j, rect and flag as they are;
  - a row i with pos(j) = p < i < q = pos(j + 1): if both keys are flagged 1, flag 1 and floor((r_p * (q - i) + r_q * (i - p)) /
    (q - p)) per coordinate; else flag 0 and zeros.
"""
import numpy as np

STRIDES = (2, 3, 5, 32)
TOP = 32767


def lengths(N):
    return sorted({n for n in (1, 2, N - 1, N, N + 1, N + 2, 2 * N, 2 * N + 1, 65, 1100) if n >= 1})


def n_keys(n, N):
    return (n - 1 + N - 1) // N + 1


def key_positions(n, N):
    """the closed form: pos(j) = min(j * N, n - 1) for j < m"""
    return np.minimum(np.arange(n_keys(n, N), dtype=np.int64) * N, n - 1)


def model(key_rects, key_flags, n, N):
    """(rects int64 [n,4], flags int64 [n]) of one segment, all rows at once"""
    kr, kf = np.asarray(key_rects, dtype=np.int64).reshape(-1, 4), np.asarray(key_flags, dtype=np.int64).reshape(-1)
    m = n_keys(n, N)
    assert len(kf) == m and len(kr) == m
    pos, at = key_positions(n, N), np.arange(n, dtype=np.int64)
    is_key = (at % N == 0) | (at == n - 1)
    own = np.where(at == n - 1, m - 1, at // N)
    lo, hi = at // N, np.minimum(at // N + 1, m - 1)
    p, q = pos[lo], pos[hi]
    both = (kf[lo] == 1) & (kf[hi] == 1) & ~is_key
    d = np.where(is_key, 1, q - p)
    mix = (kr[lo] * (q - at)[:, None] + kr[hi] * (at - p)[:, None]) // d[:, None]          # numpy's // is floor
    rects = np.where(is_key[:, None], kr[own], np.where(both[:, None], mix, 0))
    flags = np.where(is_key, kf[own], both.astype(np.int64))
    return rects, flags


def filled_rects(rects, flags):
    """arena rows as a list of rect tuples with None for the rows not flagged 1"""
    return [tuple(int(v) for v in r) if f == 1 else None for r, f in zip(rects, flags)]


def key_list(key_rects, key_flags):
    """the key rows of a case without a flag 2 as `host_stride_fill` takes them"""
    assert not (np.asarray(key_flags) == 2).any()
    return filled_rects(key_rects, key_flags)


# ---------------------------------------------------------------- the cases
def _patterns(m):
    """{name: flags int64 [m]} on the keys"""
    out = {"all found": np.ones(m, np.int64), "every key missing": np.zeros(m, np.int64)}
    for name, idx in (("first key missing", [0]), ("last key missing", [m - 1]), ("a middle key missing", [m // 2]),
                      ("two neighbouring keys missing", [m // 2, min(m // 2 + 1, m - 1)])):
        f = np.ones(m, np.int64)
        f[idx] = 0
        out[name] = f
    host = np.ones(m, np.int64)
    host[m // 2] = 2
    if m > 3:
        host[0] = 0
    out["one key flagged 2"] = host
    return out


def _key_rects(m, rng, kind):
    """coordinates in 0..32767 whose differences are mostly not divisible by the interval; `kind` 1: every coordinate falls from key
    to key, 2: the extremes 0 and 32767 in turn, 3: corners left of and above the frame, down to -200 - the numerator is negative
    there and floor, not truncation, shows"""
    xy = rng.integers(0, TOP + 1, (m, 2))
    r = np.concatenate([xy, np.minimum(xy + rng.integers(0, TOP + 1, (m, 2)), TOP)], axis=1).astype(np.int64)     # x2 >= x1, y2 >= y1
    if kind == 1:
        r = np.sort(r, axis=0)[::-1].copy()            # column by column: the k-th largest x2 is still no less than the k-th largest x1
    elif kind == 2:
        r[::2], r[1::2] = (0, 0, TOP, TOP), (TOP, 1, TOP, TOP - 1)
    elif kind == 3:
        r[:, :2] = rng.integers(-200, 3, (m, 2))
        r[:, 2:] = np.maximum(r[:, 2:], r[:, :2])
    return r


def groups(seed=0):
    """[(N, [(name, n, key_rects int64 [m,4], key_flags int64 [m])])]: the segments of one launch share its stride"""
    rng = np.random.default_rng(seed)
    out = []
    for N in STRIDES:
        group, k = [], 0
        for n in lengths(N):
            for name, flags in _patterns(n_keys(n, N)).items():
                group.append(("N %d, %d frames, %s" % (N, n, name), n, _key_rects(len(flags), rng, k % 4), flags))
                k += 1
        # floor against truncation, by hand: -1 -> 0 and 0 -> -1 over an interval that does not divide them give -1 throughout
        two = np.array([[-1, 0, 3, 0], [0, -1, 10, 7]], np.int64)
        group.append(("N %d, across zero" % N, N + 1, two, np.ones(2, np.int64)))
        out.append((N, group))
    return out


def small_groups(seed=1):
    """the groups without their 1100-frame segments, for the checks that run a per-frame Python model behind the expansion"""
    return [(N, [c for c in group if c[1] <= 130]) for N, group in groups(seed)]
