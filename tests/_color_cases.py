"""The numpy model of colour matching (w2l_color_match_u8, csrc/color_match.hip) and the case list shared by
tests/test_color_cases_cpu.py, tests/test_color_kernels_gpu.py, tests/test_color_product_gpu.py and
tools/color_match_host_check.py.  No fixtures, no tests: numpy and Python integers only.

The rule, for one face: pred, ref uint8 [S,S,3] (BGR), S even, h = S//2, N = h*S.  Per channel c, over rows 0..h-1 only:
    Sp = sum pred, So = sum ref, Qp = sum pred^2, Qo = sum ref^2;  Vp = N*Qp - Sp^2, Vo = N*Qo - So^2
    mean: g = 256;  full: g = 256 if Vp == 0 else clamp(isqrt((Vo << 16) // Vp), 128, 512)
and every pixel x of the channel, in all S rows:
    out = clamp((g*(N*x - Sp) + 256*So + 128*N) // (256*N), 0, 255)             (// floors; the numerator may be negative)

COLOR_BOUND = 1.5 grey levels between the model and the float64 transfer (x - mean_p) * clamp(sigma_o / sigma_p, 0.5, 2) + mean_o
where neither clamps to [0, 255]: g / 256 is the clamped ratio floored to a multiple of 1/256, so it is less than 1/256 below it,
and |x - mean_p| <= 255: less than 255/256 from the gain; the quotient is the transfer with that gain rounded once, half up: at
most 0.5.  The sum stays below 1.5."""
import math

import numpy as np

COLOR_BOUND = 1.5
MODES = {"mean": 1, "full": 2}
G_ONE, G_MIN, G_MAX = 256, 128, 512
PRODUCT_S = 96


def model(pred, ref, mode):
    """(out uint8 [S,S,3], info): info[c] holds the channel's intermediate values - Sp, So, Qp, Qo, Vp, Vo (Python integers),
    `root` (isqrt((Vo << 16) // Vp) before the clamp, None in mean mode and for Vp == 0), `g`, and `quot` (int64 [S,S], the floor
    quotient before the clamp to 0..255) with its numerator `num` and the divisor `den`"""
    assert mode in MODES
    pred, ref = np.asarray(pred), np.asarray(ref)
    S = pred.shape[0]
    assert pred.dtype == ref.dtype == np.uint8 and pred.shape == ref.shape == (S, S, 3) and S % 2 == 0 and 2 <= S <= 256
    h = S // 2
    N = h * S
    out = np.empty_like(pred)
    info = []
    for c in range(3):
        p = [int(v) for v in pred[:h, :, c].reshape(-1)]
        o = [int(v) for v in ref[:h, :, c].reshape(-1)]
        Sp, So, Qp, Qo = sum(p), sum(o), sum(v * v for v in p), sum(v * v for v in o)
        Vp, Vo = N * Qp - Sp * Sp, N * Qo - So * So
        assert Vp >= 0 and Vo >= 0 and max(Qp, Qo) < 1 << 32
        g, root = G_ONE, None
        if mode == "full" and Vp != 0:
            root = math.isqrt((Vo << 16) // Vp)
            g = min(G_MAX, max(G_MIN, root))
        den = 256 * N
        num = g * (N * pred[:, :, c].astype(np.int64) - Sp) + 256 * So + 128 * N        # |.| < 2^33: int64 holds it
        quot = num // den                                                               # numpy's // floors, as Python's
        out[:, :, c] = np.clip(quot, 0, 255).astype(np.uint8)
        info.append(dict(Sp=Sp, So=So, Qp=Qp, Qo=Qo, Vp=Vp, Vo=Vo, root=root, g=g, num=num, den=den, quot=quot))
    return out, info


def model_rows(pred, ref, mode):
    """the model over a batch [B,S,S,3]"""
    return np.stack([model(p, o, mode)[0] for p, o in zip(pred, ref)])


def transfer_f64(pred, ref, mode):
    """float64 [S,S,3]: (x - mean_p) * clamp(sigma_o / sigma_p, 0.5, 2) + mean_o, statistics over the upper half, NOT clamped to
    [0, 255]; the gain is 1 in mean mode and for a flat prediction"""
    S = pred.shape[0]
    h = S // 2
    out = np.empty(pred.shape, dtype=np.float64)
    for c in range(3):
        p, o = pred[:h, :, c].astype(np.float64), ref[:h, :, c].astype(np.float64)
        g = 1.0
        if mode == "full" and p.std() > 0:
            g = min(2.0, max(0.5, o.std() / p.std()))
        out[:, :, c] = (pred[:, :, c].astype(np.float64) - p.mean()) * g + o.mean()
    return out


# ---------------------------------------------------------------- random cases (the float64 comparison)
RANDOM_SIZES = (2, 6, 96)
RANDOM_PER_SIZE = {2: 40, 6: 40, 96: 8}


def random_face(rng, S):
    """a noise image around a per-channel base level with a per-channel spread: most transfers stay inside 0..255, some clamp"""
    base = rng.integers(70, 186, 3).astype(np.float64)
    spread = rng.uniform(2.0, 30.0, 3)
    return np.clip(np.rint(base + spread * rng.standard_normal((S, S, 3))), 0, 255).astype(np.uint8)


def random_cases(seed=5):
    """[(S, pred, ref)], seeded"""
    rng = np.random.default_rng(seed)
    return [(S, random_face(rng, S), random_face(rng, S)) for S in RANDOM_SIZES for _ in range(RANDOM_PER_SIZE[S])]


# ---------------------------------------------------------------- constructed cases (the model's properties; the kernel; the host)
def two_level(rng, S, a, b):
    """the upper half of one channel, uint8 [S//2, S]: half of its pixels at level a, half at b, shuffled - mean (a+b)/2, standard
    deviation |a-b|/2, V = N^2 * (a-b)^2 / 4 exactly"""
    N = (S // 2) * S
    v = np.array([a] * (N // 2) + [b] * (N // 2), dtype=np.uint8)
    return rng.permutation(v).reshape(S // 2, S)


def _face(rng, S, tops, bottom=None):
    """uint8 [S,S,3]: `tops` = three upper halves, the lower half random bytes (or the constant `bottom`)"""
    f = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    if bottom is not None:
        f[:] = bottom
    for c in range(3):
        f[:S // 2, :, c] = tops[c]
    return f


def _const(S, v):
    return np.full((S // 2, S), v, dtype=np.uint8)


def constructed_cases(S, seed=11):
    """{name: (pred, ref)} at size S >= 2 (every level pair is split half and half, which N even allows); what each case is for
    is asserted on the model's intermediate values in tests/test_color_cases_cpu.py"""
    rng = np.random.default_rng(seed + S)
    lv = lambda a, b: two_level(rng, S, a, b)      # noqa: E731
    rnd = lambda lo, hi: rng.integers(lo, hi + 1, (S // 2, S), dtype=np.uint8)     # noqa: E731
    cases = {}
    # a flat prediction (Vp == 0) under a reference with spread: g = 256 in both modes
    cases["flat_pred"] = (_face(rng, S, [_const(S, 90), _const(S, 0), _const(S, 255)]), _face(rng, S, [lv(10, 200), lv(3, 9), lv(0, 255)]))
    # a flat reference (Vo == 0) under a prediction with spread: the root is 0, g clamps to 128
    cases["flat_ref"] = (_face(rng, S, [lv(100, 140), lv(0, 255), lv(7, 8)]), _face(rng, S, [_const(S, 120), _const(S, 0), _const(S, 255)]))
    # a ratio far above 2: g clamps to 512
    cases["ratio_high"] = (_face(rng, S, [lv(100, 102), lv(127, 128), lv(50, 54)]), _face(rng, S, [lv(0, 255), lv(20, 220), lv(90, 190)]))
    # sigma_o / sigma_p = 1/2 exactly: (Vo << 16) // Vp = 128^2, the root IS 128 (no clamp at work)
    cases["ratio_exactly_half"] = (_face(rng, S, [lv(100, 104), lv(0, 254), lv(30, 50)]), _face(rng, S, [lv(50, 52), lv(64, 191), lv(200, 210)]))
    # sigma_o / sigma_p = 2 exactly: the root IS 512
    cases["ratio_exactly_two"] = (_face(rng, S, [lv(100, 101), lv(64, 191), lv(30, 40)]), _face(rng, S, [lv(100, 102), lv(0, 254), lv(200, 220)]))
    # quotients below 0 and above 255 in both modes: a dark reference under a bright prediction, and the reverse; the third channel
    # does both through a gain of 2.  The lower half runs 0, 255, 1, 254, ... (every byte value at S = 96).
    sat = _face(rng, S, [lv(200, 210), lv(5, 15), lv(120, 130)])
    ends = np.stack([np.arange(128), 255 - np.arange(128)], axis=1).reshape(-1).astype(np.uint8)      # 0, 255, 1, 254, ...
    sat[S // 2:] = np.resize(ends.repeat(3), sat[S // 2:].size).reshape(sat[S // 2:].shape)
    cases["saturate"] = (sat, _face(rng, S, [lv(5, 15), lv(200, 210), lv(100, 160)]))
    # three channels, three gains: 192, 256, 384
    cases["three_gains"] = (_face(rng, S, [lv(100, 108), lv(100, 108), lv(100, 108)]), _face(rng, S, [lv(50, 56), lv(60, 68), lv(60, 72)]))
    # equal upper halves, different lower halves: out == pred
    top = [rnd(0, 255) for _ in range(3)]
    cases["identity"] = (_face(rng, S, top), _face(rng, S, top))
    # plain noise of different ranges
    cases["noise"] = (_face(rng, S, [rnd(40, 90), rnd(0, 255), rnd(200, 255)]), _face(rng, S, [rnd(100, 250), rnd(0, 255), rnd(0, 60)]))
    for p, o in cases.values():
        p.setflags(write=False)
        o.setflags(write=False)
    return cases


def largest_sums_cases():
    """S = 256.  `all_255`: the largest sums (N*Qp and Sp^2 are near 2^46; the numerator itself, 256*255*N + 128*N, stays just
    below 2^31).  `wide`: a prediction at 100/101 over a lower half of 255 under a reference at 0/255: the largest Vo << 16, g
    clamps to 512, and the numerator passes 2^31 (512 * N * 154.5) - in mean mode too (256 * (N*154.5 + N*127.5) + 128*N)"""
    S = 256
    rng = np.random.default_rng(256)
    a = np.full((S, S, 3), 255, dtype=np.uint8)
    lv = lambda x, y: two_level(rng, S, x, y)      # noqa: E731
    wide = (_face(rng, S, [lv(100, 101)] * 3, bottom=255), _face(rng, S, [lv(0, 255)] * 3))
    cases = {"all_255": (a, a.copy()), "wide": wide}
    for p, o in cases.values():
        p.setflags(write=False)
        o.setflags(write=False)
    return cases


SMALL_S = 6          # N = 18: the upper half ends inside a group of four pixels


def case_groups():
    """[(S, {name: (pred, ref)})]: every group is one launch per mode, its rows side by side.  S = 96 is the product's size (a lane
    goes round its loops nine times), 6 the smallest with a ragged upper half, 2 the smallest there is, 256 the largest"""
    return [(PRODUCT_S, constructed_cases(PRODUCT_S)), (SMALL_S, constructed_cases(SMALL_S)), (2, constructed_cases(2)),
            (256, largest_sums_cases())]


def stack(group):
    """(pred [B,S,S,3], ref [B,S,S,3]) of a group's cases, in order"""
    return np.stack([p for p, _ in group.values()]), np.stack([o for _, o in group.values()])
