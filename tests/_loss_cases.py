"""Inputs, float64 formulas and error bounds shared by tests/test_train_losses_gpu.py (the HIP kernels) and
tests/test_train_losses_bounds_cpu.py (numpy fp32 restatements of the same arithmetic).  No fixtures, no tests: numpy only.

u = 2^-24 is the unit roundoff of fp32, R = 2^-21 = 8 u the allowance for one short fp32 expression with one transcendental
(tests/test_bf16_train_ops_gpu.py).  A one-wave row reduction over C terms (lane l adds terms l, l + 64, ..., a six-step xor
fold follows) performs ceil(C / 64) + 6 additions per result on once-rounded products: its error is at most
K(C) u sum|terms| with K(C) = ceil(C / 64) + 7.  Everything computed from such sums inherits that through the float64 partial
derivatives of the expression, taken stage by stage with magnitudes (the triangle inequality at every stage, first order in u);
the roundings of each stage's own operations are counted next to it below."""
import numpy as np

U = 2.0 ** -24
R = 2.0 ** -21
SENT = 12352.0
F32 = np.float32
EPS_L2 = float(F32(1e-12))        # F.normalize's eps as the kernels hold it
EPS_COS2 = float(F32(1e-16))      # cosine_similarity's eps^2 (clamp of |a|^2 |v|^2)
BCE_FLOOR = float(F32(1e-12))     # ATen's floor of (1 - p) p in the BCE backward
ADAM_CHUNK = 16384                # kAdamChunk (csrc/train.hip)


def K(C):
    return -(-C // 64) + 7


# ---------------------------------------------------------------- launch rules (transcribed from csrc/w2l_common.h, train.hip)
def grid_cap(work, block, cap):
    return max(1, min(-(-work // block), cap))


def l1_partials(n):
    """workgroups (= fp64 partials) of w2l_l1_mean"""
    return grid_cap(n, 256 * 16, 1024)


def mean_final_walk(nb):
    """mean_final_kernel over nb partials: (trips of lane 0 through the four-way unrolled loop, lanes that take that loop at all,
    partials read by the one-at-a-time tail loop over all lanes)"""
    trips0, lanes, tail = 0, 0, 0
    for lane in range(64):
        i, t = lane, 0
        while i + 192 < nb:
            i, t = i + 256, t + 1
        while i < nb:
            i, tail = i + 64, tail + 1
        lanes += t > 0
        if lane == 0:
            trips0 = t
    return trips0, lanes, tail


# n -> (partials, unrolled trips of lane 0, lanes in the unrolled loop, partials left to the tail loop)
L1_CASES = {
    1: (1, 0, 0, 1),
    255: (1, 0, 0, 1),
    4097: (2, 0, 0, 2),
    192 * 4096 + 1: (193, 1, 1, 189),          # the first n whose lane 0 enters the unrolled loop; its own tail is empty
    260 * 4096 + 5: (261, 1, 64, 5),           # every lane one unrolled trip, then a 5-wide tail
    1024 * 4096 + 4095: (1024, 4, 64, 0),      # the cap: grid-stride with a ragged end, no tail
}


def adam_chunks(sizes):
    return sum(-(-n // ADAM_CHUNK) for n in sizes)


# ---------------------------------------------------------------- L1
def l1_inputs(n, seed):
    """rand images; a tenth of the elements with a == b, a tenth with a - b = +-1 ulp of a"""
    rng = np.random.default_rng(seed)
    a = rng.random(n, dtype=F32)
    b = rng.random(n, dtype=F32)
    kind = rng.random(n)
    eq = kind < 0.1
    b[eq] = a[eq]
    up, dn = (kind >= 0.1) & (kind < 0.15), (kind >= 0.15) & (kind < 0.2)
    b[up] = np.nextafter(a[up], F32(2))
    b[dn] = np.nextafter(a[dn], F32(-1))
    return a, b


def l1_ref(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())


def l1_bound(ref):
    """fp64 accumulation: one fp32 subtraction per term, one final cast"""
    return 2.0 ** -23 * abs(ref)


def l1_bwd_ref(a, b, gout, n):
    """exact: +-fp32(gout * fp32(1 / n)), 0 where a == b"""
    gsc = F32(1.0 if gout is None else gout) * F32(1.0 / n)
    d = a.astype(np.float64) - b.astype(np.float64)
    return np.where(d > 0, gsc, np.where(d < 0, -gsc, F32(0))).astype(F32)


# ---------------------------------------------------------------- L2 normalisation
L2_N, L2_C = (1, 5, 64), (1, 63, 64, 65, 512, 1000)
L2_KINDS = ("scaled", "zero", "below", "above")


def l2_inputs(N, C, rot, seed):
    """x, dy [N, C]; row r is of kind L2_KINDS[(r + rot) % 4]: well scaled, all zero, C copies of 1e-12 / sqrt(C) (1 -+ 2^-10)
    (norm just below / just above the 1e-12 clamp)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, C)) * 1.5).astype(F32)
    dy = rng.standard_normal((N, C)).astype(F32)
    kinds = [L2_KINDS[(r + rot) % 4] for r in range(N)]
    for r, k in enumerate(kinds):
        if k == "zero":
            x[r] = 0
        elif k in ("below", "above"):
            x[r] = F32(1e-12 / np.sqrt(C) * (1 + (2.0 ** -10 if k == "above" else -2.0 ** -10)))
    return x, dy, kinds


def _safe(d):
    return np.where(d == 0, 1.0, d)


def l2_ref(x):
    x = x.astype(np.float64)
    ss = (x * x).sum(1, keepdims=True)
    nrm = np.sqrt(ss)
    return x / np.maximum(nrm, EPS_L2), ss, nrm


def l2_bound(x):
    """y = x / max(sqrt(ss), eps): R |y| for sqrt and the division, plus |dy/dss| K u ss = K u |y| / 2 outside the clamp"""
    y, ss, nrm = l2_ref(x)
    return R * np.abs(y) + np.where(nrm > EPS_L2, 0.5 * K(x.shape[1]) * U * np.abs(y), 0.0)


def l2_bwd_ref(x, dy):
    x, dy = x.astype(np.float64), dy.astype(np.float64)
    _, ss, nrm = l2_ref(x)
    d = np.maximum(nrm, EPS_L2)
    xd = (x * dy).sum(1, keepdims=True)
    k = np.where(nrm > EPS_L2, xd / d ** 3, 0.0)
    return dy / d - x * k


def l2_bwd_bound(x, dy):
    """dx = t1 - t2, t1 = dy / d, t2 = x xd / d^3.  Own roundings: sqrt, d d d (2), xd / d^3, dy / d, x k, the subtraction - at
    most 8 u = R on t2 and 3 u on t1.  Inherited outside the clamp: |d dx/d ss| K u ss <= K u (|t1| / 2 + 3 |t2| / 2) and
    |d dx/d xd| K u sum|x dy| = K u |x| sum|x dy| / d^3; under the clamp the norm is a constant and k = 0"""
    x, dy = x.astype(np.float64), dy.astype(np.float64)
    _, ss, nrm = l2_ref(x)
    d = np.maximum(nrm, EPS_L2)
    free = nrm > EPS_L2
    xd = (x * dy).sum(1, keepdims=True)
    xd_abs = np.abs(x * dy).sum(1, keepdims=True)
    t1 = np.abs(dy) / d
    t2 = np.where(free, np.abs(x * xd) / d ** 3, 0.0)
    ku = K(x.shape[1]) * U
    return R * (t1 + t2) + np.where(free, ku * (0.5 * t1 + 1.5 * t2) + ku * np.abs(x) * xd_abs / d ** 3, 0.0)


# ---------------------------------------------------------------- cosine + BCE
COS_N, COS_C = (1, 6, 7, 130), (7, 64, 512, 1000)


def cosine_inputs(N, C, seed, normalised, labels):
    """non-negative rows a, v = t a + (1 - t) w with t solved (float64 bisection) for cosines spread evenly over
    [0.055, 0.945] (0.5 for N = 1); w lives on the channels where a is small, so that cos(a, w) < 0.05.  labels: "hard"
    (0 / 1 mixed) or "soft" (0.3).  normalised: both rows scaled to unit norm, else by factors in [0.5, 4]"""
    rng = np.random.default_rng(seed)
    half = (C + 1) // 2
    big = np.zeros((N, C))
    big[:, :half] = 1
    a = big * (0.1 + rng.random((N, C))) + 0.01 * rng.random((N, C))
    w = (1 - big) * (0.1 + rng.random((N, C))) + 0.01 * rng.random((N, C))
    w *= np.linalg.norm(a, axis=1, keepdims=True) / np.linalg.norm(w, axis=1, keepdims=True)
    target = np.linspace(0.055, 0.945, N)[:, None] if N > 1 else np.full((1, 1), 0.5)

    def cos_at(t):
        v = t * a + (1 - t) * w
        return (a * v).sum(1, keepdims=True) / (np.linalg.norm(a, axis=1, keepdims=True) * np.linalg.norm(v, axis=1, keepdims=True))
    lo, hi = np.zeros((N, 1)), np.ones((N, 1))
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        below = cos_at(mid) < target
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    t = 0.5 * (lo + hi)
    v = t * a + (1 - t) * w
    if normalised:
        a, v = a / np.linalg.norm(a, axis=1, keepdims=True), v / np.linalg.norm(v, axis=1, keepdims=True)
    else:
        a, v = a * rng.uniform(0.5, 4, (N, 1)), v * rng.uniform(0.5, 4, (N, 1))
    y = np.full(N, 0.3) if labels == "soft" else (np.arange(N) % 2 == 0).astype(np.float64)
    if labels == "hard" and N > 2:
        rng.shuffle(y)
    return a.astype(F32), v.astype(F32), y.astype(F32)


def cosine_edge_inputs(seed=7, C=512):
    """edge rows of cosine + BCE, C = 512: (a, v, y, kind per row).  zero_a / zero_v: a zero row against a unit-norm row;
    disjoint: supports that do not meet (cosine exactly 0); equal: bitwise-equal rows; near: v = a with every fourth element
    moved one ulp (cosines within an ulp or two of 1, on either side).  Every kind under y = 1 and y = 0"""
    rng = np.random.default_rng(seed)
    rows, kinds = [], []

    def unit(x):
        return x / np.linalg.norm(x)
    for y in (1.0, 0.0):
        r = unit(rng.random(C))
        rows.append((np.zeros(C), r, y)); kinds.append("zero_a")
        rows.append((r, np.zeros(C), y)); kinds.append("zero_v")
        a, v = rng.random(C) + 0.1, rng.random(C) + 0.1
        a[C // 2:] = 0
        v[:C // 2] = 0
        rows.append((a, v, y)); kinds.append("disjoint")
        for scale in (1.0, 0.37, 5.0):
            e = (rng.random(C) * scale).astype(F32)
            rows.append((e, e.copy(), y)); kinds.append("equal")
        e = unit(rng.random(C)).astype(F32)
        rows.append((e, e.copy(), y)); kinds.append("equal")
        for j in range(12):
            e = unit(rng.random(C)).astype(F32) if j % 2 else (rng.random(C) * 2).astype(F32)
            f = e.copy()
            f[j % 4::4] = np.nextafter(f[j % 4::4], F32(4) if j % 3 else F32(-1))
            rows.append((e, f, y)); kinds.append("near")
    a = np.stack([np.asarray(r[0], np.float64) for r in rows]).astype(F32)
    v = np.stack([np.asarray(r[1], np.float64) for r in rows]).astype(F32)
    return a, v, np.array([r[2] for r in rows], F32), kinds


def cosine_sums(a, v):
    a, v = a.astype(np.float64), v.astype(np.float64)
    return (a * v).sum(1), (a * a).sum(1), (v * v).sum(1), np.abs(a * v).sum(1)


def cosine_ref(a, v):
    """x.y / sqrt(max(|x|^2 |y|^2, eps^2)), the form of ATen's cosine_similarity that csrc/api.hip cites"""
    dot, na, nv, _ = cosine_sums(a, v)
    return dot / np.sqrt(np.maximum(na * nv, EPS_COS2))


def cosine_bound(a, v):
    """E_cs.  den = sqrt(max(na nv, eps^2)): relative error K u inherited (K u on each of na, nv, halved by the root; none under
    the clamp) + 1.5 u of its own (the product, halved, and the root); cs = dot / den: one more u, and K u sum|a v| / den from dot"""
    dot, na, nv, sabs = cosine_sums(a, v)
    prod = na * nv
    den = np.sqrt(np.maximum(prod, EPS_COS2))
    rel_den = np.where(prod < EPS_COS2, 0.0, K(a.shape[1]) * U) + 1.5 * U
    return np.abs(dot / den) * (rel_den + U) + K(a.shape[1]) * U * sabs / den


def bce_terms(p, y):
    """per-element y lp, (1 - y) lq of ATen's binary_cross_entropy (logs clamped at -100) in float64; where 1 - p <= 0 or
    p <= 0 - outside [0, 1] ATen refuses - lq or lp is -100, what the clamp makes of the kernel's logf of a non-positive number"""
    p, y = p.astype(np.float64), y.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.where(p > 0, np.maximum(np.log(np.where(p > 0, p, 1.0)), -100.0), -100.0)
        q = 1.0 - p
        lq = np.where(q > 0, np.maximum(np.log1p(np.where(q > 0, -p, 0.0)), -100.0), -100.0)    # log1p: exact for tiny p, as ATen
    return y * lp, (1 - y) * lq


def bce_ref(p, y):
    t1, t2 = bce_terms(p, y)
    return float(-(t1 + t2).mean())


def bce_bound(p, y):
    """bce_mean_kernel: fp32 over one workgroup.  Per term R (|y lp| + |(1 - y) lq|) - each logf with its allowance, which also
    covers 1 - y, the two products and their sum - plus (1 - y) u where p < 0.5: the rounding of 1 - p (exact from 0.5 up), which
    the logarithm passes on as an absolute error.  Accumulation: each thread adds ceil(N / 256) terms, 6 + 3 additions follow:
    A u sum|terms| with A = ceil(N / 256) + 9; the final division one more u"""
    N = p.shape[0]
    t1, t2 = bce_terms(p, y)
    mag = float((np.abs(t1) + np.abs(t2)).sum())
    A = -(-N // 256) + 9
    sub = float(((1 - y.astype(np.float64)) * (p.astype(np.float64) < 0.5)).sum())
    return ((R + (A + 1) * U) * mag + U * sub) / N


def bce_bwd_ref(p, y, gout):
    p, y = p.astype(np.float64), y.astype(np.float64)
    return float(F32(1.0 if gout is None else gout)) / p.shape[0] * (p - y) / np.maximum((1 - p) * p, BCE_FLOOR)


def bce_bwd_bound(p, y, gout):
    """R |ref| (g / N, p - y, 1 - p, its product, the scaling, the quotient: 6 u), plus 2^-149 / max((1 - p) p, floor): the
    product g / N (p - y) of a denormal p leaves the fp32 grid, and the quotient scales that step"""
    p64 = p.astype(np.float64)
    return R * np.abs(bce_bwd_ref(p, y, gout)) + 2.0 ** -149 / np.maximum((1 - p64) * p64, BCE_FLOOR)


def _dcos(cs, y, gn):
    """h(cs) = gn (cs - y) / max((1 - cs) cs, floor) and |h'(cs)|"""
    q = (1 - cs) * cs
    fl = q < BCE_FLOOR
    qq = np.where(fl, BCE_FLOOR, q)
    h = gn * (cs - y) / qq
    dh = np.where(fl, gn / BCE_FLOOR, gn * (1 / qq - (cs - y) * (1 - 2 * cs) / qq ** 2))
    return h, np.abs(dh)


def cosine_bce_ref(a, v, y, gout, cs_dev=None):
    """(loss, da, dv) in float64.  cs_dev: evaluate the BCE and its gradient factor at this cosine (the fp32 value the forward
    launch wrote) instead of the float64 cosine"""
    N = a.shape[0]
    dot, na, nv, _ = cosine_sums(a, v)
    prod = na * nv
    clamped = prod < EPS_COS2
    den = np.sqrt(np.maximum(prod, EPS_COS2))
    cs = dot / den if cs_dev is None else cs_dev.astype(np.float64)
    gn = float(F32(1.0 if gout is None else gout)) / N
    dcos, _ = _dcos(cs, y.astype(np.float64), gn)
    k1 = dcos / den
    ka = np.where(clamped, 0.0, dcos * dot * nv / den ** 3)
    kv = np.where(clamped, 0.0, dcos * dot * na / den ** 3)
    a64, v64 = a.astype(np.float64), v.astype(np.float64)
    da = k1[:, None] * v64 - ka[:, None] * a64
    dv = k1[:, None] * a64 - kv[:, None] * v64
    return bce_ref(cs, y), da, dv


def cosine_bce_bounds(a, v, y, gout, cs_dev=None):
    """(bound of the loss, of da, of dv), stage by stage:
    E_cs    as cosine_bound - or 0 with cs_dev, where the reference starts from the device's own cosine;
    E_dcos  = |h'(cs)| E_cs + R |dcos|         (g / N, cs - y, 1 - cs, its product, the quotient, the scaling: 6 u);
    E_k1    = E_dcos / den + |k1| (rel_den + u)                                      k1 = dcos / den;
    E_ka    = E_dcos |dot| nv / den^3 + |dcos| K u sum|a v| nv / den^3 + |ka| (K u + 3 rel_den + 5 u)
                                               ka = dcos dot nv / den^3: K u of nv, two products, den den den, the quotient;
    E_da    = E_k1 |v_c| + E_ka |a_c| + 2 u (|k1 v_c| + |ka a_c|)                    da_c = k1 v_c - ka a_c;
    loss    : bce_bound at the cosine + sum_i |cs_i - y_i| / max(q_i, floor) / N * E_cs_i"""
    N, C = a.shape
    dot, na, nv, sabs = cosine_sums(a, v)
    prod = na * nv
    clamped = prod < EPS_COS2
    den = np.sqrt(np.maximum(prod, EPS_COS2))
    ku = K(C) * U
    rel_den = np.where(clamped, 0.0, ku) + 1.5 * U
    y64 = y.astype(np.float64)
    if cs_dev is None:
        cs, e_cs = dot / den, cosine_bound(a, v)
    else:
        cs, e_cs = cs_dev.astype(np.float64), np.zeros(N)
    gn = float(F32(1.0 if gout is None else gout)) / N
    dcos, dh = _dcos(cs, y64, gn)
    e_dcos = dh * e_cs + R * np.abs(dcos)
    k1 = dcos / den
    e_k1 = e_dcos / den + np.abs(k1) * (rel_den + U)
    a64, v64 = np.abs(a.astype(np.float64)), np.abs(v.astype(np.float64))

    def side(n_other):
        kk = np.where(clamped, 0.0, dcos * dot * n_other / den ** 3)
        e = e_dcos * np.abs(dot) * n_other / den ** 3 + np.abs(dcos) * ku * sabs * n_other / den ** 3 + np.abs(kk) * (ku + 3 * rel_den + 5 * U)
        return np.abs(kk), np.where(clamped, 0.0, e)
    ka, e_ka = side(nv)
    kv, e_kv = side(na)
    k1a, e1 = np.abs(k1)[:, None], e_k1[:, None]
    b_da = e1 * v64 + e_ka[:, None] * a64 + 2 * U * (k1a * v64 + ka[:, None] * a64)
    b_dv = e1 * a64 + e_kv[:, None] * v64 + 2 * U * (k1a * a64 + kv[:, None] * v64)
    q = np.maximum((1 - cs) * cs, BCE_FLOOR)
    b_loss = bce_bound(cs, y) + float((np.abs(cs - y64) / q * e_cs).sum()) / N
    return b_loss, b_da, b_dv


BCE_N = (1, 63, 64, 255, 256, 257, 1000)
BCE_OUTSIDE = (1 + 2.0 ** -23, -2.0 ** -23)        # outside [0, 1], where ATen raises: a cosine an ulp above 1, and its mirror
BCE_SPECIALS = (0.0, 1.0, 2.0 ** -149, 1 - 2.0 ** -24) + BCE_OUTSIDE + (1e-9, 1e-11, 1e-13, 1e-20, 1e-30, 0.5)


def bce_inputs(N, seed, labels):
    """p from rand with BCE_SPECIALS at the head (as many as fit beside one random element): exactly 0 and 1, the smallest
    denormal, the largest value below 1, one ulp above 1 and as far below 0 (BCE_OUTSIDE), values so small that 1 - p rounds to 1 (on either side of the 1e-12 floor of the
    backward).  labels "hard": 0 / 1, "soft": rand"""
    rng = np.random.default_rng(seed)
    p = rng.random(N, dtype=F32)
    k = min(N - 1, len(BCE_SPECIALS))
    p[:k] = np.array(BCE_SPECIALS[:k], F32)
    y = rng.random(N, dtype=F32) if labels == "soft" else (rng.random(N) < 0.5).astype(F32)
    return p, y


# ---------------------------------------------------------------- Adam
ADAM_SIZES = (0, 1, 255, 256, 16383, 16384, 16385, 49153)
ADAM_HYPER = [(1e-4, (0.5, 0.999)), (1e-3, (0.0, 0.9))]     # the reference's (wav2lip_train.py:359), and beta1 = 0
ADAM_WD = (0.0, 0.01)
ADAM_STEPS = (1, 2, 100000)


def adam_inputs(sizes, seed):
    """per tensor (p, g, m, v) fp32.  g: a tenth exact zeros - half of those with zero moments, where the update is exactly 0 -
    and a twentieth 1e-25, whose square underflows in fp32"""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        p = rng.standard_normal(n).astype(F32)
        g = rng.standard_normal(n).astype(F32)
        m = (rng.standard_normal(n) * 0.1).astype(F32)
        v = (rng.random(n) * 0.01).astype(F32)
        kind = rng.random(n)
        g[kind < 0.1] = 0
        m[kind < 0.05] = 0
        v[kind < 0.05] = 0
        g[(kind >= 0.1) & (kind < 0.15)] = F32(1e-25)
        out.append((p, g, m, v))
    return out


def adam_scalars(lr, betas, eps, wd, step):
    """the fp32 scalars adam_kernel receives, as float64: lr, beta1, beta2, eps, wd, bc1, sqrt(bc2).  The host forms the bias
    corrections in double from the fp32 betas and rounds them once"""
    lr, b1, b2, eps, wd = (float(F32(x)) for x in (lr, betas[0], betas[1], eps, wd))
    return lr, b1, b2, eps, wd, float(F32(1.0 - b1 ** step)), float(F32(np.sqrt(1.0 - b2 ** step)))


def adam_ref(p, g, m, v, sc, m_dev=None, v_dev=None):
    """one step in float64 from fp32 state -> (p, m, v).  m_dev / v_dev: form the parameter from these (the fp32 moments the device
    wrote) instead of the float64 ones"""
    lr, b1, b2, eps, wd, bc1, bc2s = sc
    p, g, m, v = (t.astype(np.float64) for t in (p, g, m, v))
    gg = g + wd * p
    m1 = m + (gg - m) * (1 - b1)
    v1 = b2 * v + (1 - b2) * gg * gg
    mm = m1 if m_dev is None else m_dev.astype(np.float64)
    vv = v1 if v_dev is None else v_dev.astype(np.float64)
    return p - lr / bc1 * (mm / (np.sqrt(vv) / bc2s + eps)), m1, v1


def adam_bounds(p, g, m, v, sc, from_device_moments):
    """(bound of p, of m, of v) for one step.  g' = g + wd p carries 2 u (|g| + wd |p|) when wd != 0 (E_g).
    m = m0 + (g' - m0)(1 - beta1): the difference, the product and the sum, each one rounding of a quantity no larger than
    |m0| + |g'|: 2^-22 relative to the magnitudes that enter (|m0| + |g| + wd |p|), E_g included - relative to |m| itself nothing
    holds, m0 and the step may cancel.  The count takes 1.f - beta1 and 1.f - beta2 as exact, which they are for a beta of 0 or in
    [0.5, 1) (asserted below); another beta would add one rounding to each product.
    v = beta2 v0 + (1 - beta2) g'^2, all terms >= 0: four roundings, 2^-22 v, plus (1 - beta2) 2 |g'| E_g, plus 2^-149: the product
    (1 - beta2) g' g' may underflow to the fp32 grid of denormals.
    p = p0 - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps): 2^-24 |p| for the subtraction and R (lr / bc1) |m / denom| for the rest
    (lr / bc1, the root, two quotients, the sum, the product), against the float64 expression AT the moments the device wrote
    (from_device_moments) - or, from the state, plus what the moments' own bounds pass on:
    (lr / bc1) (E_m / denom + |m| E_v / (2 sqrt(v) sqrt(bc2) denom^2))"""
    lr, b1, b2, eps, wd, bc1, bc2s = sc
    assert float(F32(1) - F32(b1)) == 1 - b1 and float(F32(1) - F32(b2)) == 1 - b2
    p64, g64, m64, v64 = (t.astype(np.float64) for t in (p, g, m, v))
    gg = g64 + wd * p64
    e_g = 2 * U * (np.abs(g64) + wd * np.abs(p64)) if wd != 0 else 0.0
    pr, mr, vr = adam_ref(p, g, m, v, sc)
    b_m = 2.0 ** -22 * (np.abs(m64) + np.abs(g64) + wd * np.abs(p64))
    b_v = 2.0 ** -22 * vr + (1 - b2) * 2 * np.abs(gg) * e_g + 2.0 ** -149
    denom = np.sqrt(vr) / bc2s + eps
    b_p = U * np.abs(pr) + R * lr / bc1 * np.abs(mr / denom)
    if not from_device_moments:
        with np.errstate(divide="ignore", invalid="ignore"):
            dv = np.where(vr > 0, b_v / (2 * np.sqrt(_safe(vr)) * bc2s), np.sqrt(b_v) / bc2s)   # sqrt is not smooth at 0
        b_p = b_p + lr / bc1 * (b_m / denom + np.abs(mr) * dv / denom ** 2)
    return b_p, b_m, b_v
