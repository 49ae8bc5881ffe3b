"""Cases, float64 references, error bounds and launch rules shared by tests/test_glue_cases_cpu.py (numpy fp32 restatements of
the kernels' arithmetic) and tests/test_glue_kernels_gpu.py (the detector glue of csrc/detect.hip - w2l_s3fd_decode and, for
fp32 and bf16 storage, w2l_maxpool2x2, w2l_l2norm_scale, w2l_s3fd_pack - and the input packing of csrc/api.hip -
w2l_datagen_pack(_bf16), w2l_frames_to_u8, w2l_nchw_to_nhwc, w2l_nhwc_to_nchw).  No fixtures, no tests: numpy only.

U = 2^-24 is the unit roundoff of fp32, R = 2^-21 = 8 U the allowance for one short fp32 expression with one transcendental
(tests/_loss_cases.py).  Every bound below is derived from fp32 roundoff next to its reference; none is measured from a kernel.
The float64 references follow the operation's definition (oracle/s3fd_ref.py::dense_boxes, ::l2norm), not the kernels; the
`*_f32` functions restate the kernels operation by operation in numpy fp32 (no contraction), and the launch rules (`grid_cap`,
the cap of every launch, the store-path selections) are transcribed from detect.hip, api.hip and w2l_common.h.

The glue kernels are one body for two storages, `kind` "fp32" or "bf16": a thread moves VEC[kind] channels (16 bytes).  The bf16
case tables hold the smallest shapes at which each kernel can still go wrong; inputs are rounded to bf16 first (`to_bf16`), so
the references start from what the kernel reads, and UB = 2^-8 is the unit roundoff of the one rounding on a bf16 store.

`decode_ref` takes `xp`, the array namespace (numpy, or torch for the one case that is generated and compared on the device)."""
import numpy as np

U = 2.0 ** -24
UB = 2.0 ** -8                     # bf16 holds 8 significant bits as fp32 holds 24
R = 2.0 ** -21
F32 = np.float32
SENT = 12352.0                    # sentinel of every destination: exact in fp32 and in bf16
V_XY = float(F32(0.1))            # the variances as fp32 holds them
V_WH = float(F32(0.2))
EPS_NORM = float(F32(1e-10))      # L2Norm's eps as fp32 holds it
BLOCK = 256
VEC = {"fp32": 4, "bf16": 8}      # channels of one 16-byte item
PACK_GRID_CAP = {"fp32": 16384, "bf16": 65536}
POOL_GRID_CAP = 65536


def to_bf16(x):
    """fp32 values rounded to bf16 (nearest, ties to even), returned as fp32; NaN and +-inf stay what they are"""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(F32)
    return np.where(np.isfinite(x), r, x).astype(F32)


# ---------------------------------------------------------------- launch rules
def grid1d(work, block=BLOCK, cap=16384):
    """detect.hip's launches are grid_cap with the cap named at each: 16384 the decode and the fp32 pack, PACK_GRID_CAP["bf16"] the
    bf16 pack, POOL_GRID_CAP both max pools"""
    return max(1, min(-(-work // block), cap))


def grid_cap(work, block, cap):
    """w2l_common.h"""
    return max(1, min(-(-work // block), cap))


def _trips(work, grid, block=BLOCK):
    """trips of thread 0 through `for (i = tid; i < work; i += grid * block)`: the most any thread takes"""
    return -(-work // (grid * block))


def pack_trips(npix, kind="fp32"):
    return _trips(npix, grid1d(npix, BLOCK, PACK_GRID_CAP[kind]))


def decode_trips(B, FH, FW):
    return _trips(B * FH * FW, grid1d(B * FH * FW))


def pool_items(N, H, W, C, kind="fp32"):
    return N * (H // 2) * (W // 2) * (C // VEC[kind])


def pool_trips(N, H, W, C, kind="fp32"):
    return _trips(pool_items(N, H, W, C, kind), grid1d(pool_items(N, H, W, C, kind), BLOCK, POOL_GRID_CAP))


def datagen_trips(N, S):
    return _trips(N * S * S, grid_cap(N * S * S, BLOCK, 8192))


def frames_trips(N, H, W):
    return _trips(N * H * W, grid_cap(N * H * W, BLOCK, 8192))


def l2norm_walk(rows, C, kind="fp32"):
    """l2norm_scale_kernel, one wave per row, four rows per workgroup: (workgroups, waves of the last workgroup that own no row,
    trips of lane 0 - 64 VEC channels each: 256 for fp32, 512 for bf16 -, lanes that take the last of those trips)"""
    v = VEC[kind]
    wg = -(-rows // 4)
    t = -(-C // (64 * v))
    return wg, 4 * wg - rows, t, sum(1 for lane in range(64) if lane * v + 64 * v * (t - 1) < C)


# ---------------------------------------------------------------- w2l_s3fd_decode
# (B, FH, FW, ncls, stride, cls_cs, reg_cs)
DECODE_CASES = [
    (2, 13, 21, 4, 4, 4, 4),          # the first level: max-out over three background channels
    (1, 9, 17, 2, 8, 4, 4),           # the production stride for two classes (channels 2, 3 are padding)
    (2, 5, 7, 2, 16, 2, 4),
    (1, 7, 3, 2, 64, 8, 8),
    (3, 1, 1, 2, 128, 4, 4),
]
DECODE_BIG = (1, 2049, 2048, 2, 4, 4, 4)          # 2049 * 2048 > 16384 * 256: a second grid-stride trip
DECODE_VARIANTS = ("variances_swapped", "no_half_stride", "wx_hy_exchanged", "hy_not_wrapped", "maxout_two_of_three",
                   "bg_as_score", "x2_without_x1")
SAT_GAP = 104.0       # exp(-104) = 6.8e-46 is below half of the smallest fp32 denormal (7.0e-46): the smaller exponential is 0
# (background, foreground) of the saturated rows: |bg - fg| >= 104 up to a difference that overflows fp32
SAT_ROWS = [(52.0, -52.0), (-52.0, 52.0), (75.0, -75.0), (-1e4, 1e4), (3e38, -3e38), (-3e38, 3e38), (104.0, 0.0), (0.0, 104.0)]


def decode_variant_applies(case, variant):
    B, FH, FW, ncls = case[:4]
    if variant == "wx_hy_exchanged":
        return FH > 1 or FW > 1
    if variant == "hy_not_wrapped":
        return B >= 2
    if variant == "maxout_two_of_three":
        return ncls == 4
    return True


def decode_inputs(case, seed):
    """conf [P, cls_cs] ~ N(0, 3), loc [P, reg_cs] ~ N(0, 2), fp32; channels the kernel must not read are NaN.  The last
    min(8, P // 2) positions hold SAT_ROWS (for ncls = 4 the background value moves through the three max-out channels)"""
    B, FH, FW, ncls, stride, cls_cs, reg_cs = case
    P = B * FH * FW
    rng = np.random.default_rng(seed)
    conf = np.full((P, cls_cs), np.nan, F32)
    loc = np.full((P, reg_cs), np.nan, F32)
    conf[:, :ncls] = (rng.standard_normal((P, ncls)) * 3).astype(F32)
    loc[:, :4] = (rng.standard_normal((P, 4)) * 2).astype(F32)
    nsat = min(len(SAT_ROWS), P // 2)
    for k in range(nsat):
        bg, fg = SAT_ROWS[k]
        r = P - nsat + k
        if ncls == 4:
            conf[r, :3] = [bg - 1 - abs(bg) * 0.1, bg - 2 - abs(bg) * 0.12, bg - 3 - abs(bg) * 0.13]
            conf[r, k % 3] = bg
            conf[r, 3] = fg
        else:
            conf[r, :2] = [bg, fg]
    return conf, loc


def decode_bg_fg(conf, ncls):
    c = conf.astype(np.float64)
    return (np.maximum(np.maximum(c[:, 0], c[:, 1]), c[:, 2]), c[:, 3]) if ncls == 4 else (c[:, 0], c[:, 1])


def positions(B, FH, FW, variant=None):
    """(wx, hy) of every row of the [B, FH * FW] table, float64: dense_boxes' meshgrid, once per image"""
    ys, xs = np.meshgrid(np.arange(FH), np.arange(FW), indexing="ij")
    wx, hy = np.tile(xs.ravel(), B), np.tile(ys.ravel(), B)
    if variant == "hy_not_wrapped":
        hy = np.repeat(np.arange(B * FH), FW)
    if variant == "wx_hy_exchanged":
        wx, hy = hy, wx
    return wx.astype(np.float64), hy.astype(np.float64)


def decode_ref(conf, loc, wx, hy, ncls, stride, variant=None, xp=np):
    """(out [P, 5], bound [P, 5]) in float64 from float64 conf [P, >= ncls], loc [P, >= 4] and the positions.
    oracle/s3fd_ref.py::dense_boxes: the max-out of net_s3fd.py:123-126 for ncls = 4, the two-class softmax, priors
    (stride / 2 + i stride, size 4 stride), centre + l_{0,1} 0.1 size, size exp(0.2 l_{2,3}), corner form.

    Coordinates: |err| <= R (M + A).  M is the sum of the magnitudes of the coordinate's terms, |a_c| + 0.1 |l| p + b / 2 for
    x1, y1 and b more for x2, y2: every product, sum and the exponential itself is rounded once or twice relative to a term of
    that sum (at most 8 roundings: R).  A = 0.2 |l_{2,3}| b: the rounding of the exponent's argument 0.2 l, U |0.2 l|, which the
    exponential turns into a relative error of b.
    Score: |err| <= R absolute.  s = e^fg / (e^bg + e^fg) has ds/dd = s (1 - s) in d = fg - bg, so the rounding of the
    argument (U |d|) contributes U |d| s (1 - s): at most 4 U = R / 2 for |d| <= 16 (s (1 - s) <= 1 / 4), and less than U beyond
    (s (1 - s) <= e^-|d|, |d| e^-|d| < 1e-5); the exponential, the sum and the division, each relative to a value <= 1, fit
    in the other half.  So R holds for every finite input, the |d| <= 16 of the drawn rows and the saturated rows alike.
    A `variant` is one named mistake; the bound is that of the right formula either way."""
    v_xy, v_wh = (V_WH, V_XY) if variant == "variances_swapped" else (V_XY, V_WH)
    if ncls == 4:
        bg = xp.maximum(conf[:, 0], conf[:, 1])
        if variant != "maxout_two_of_three":
            bg = xp.maximum(bg, conf[:, 2])
        fg = conf[:, 3]
    else:
        bg, fg = conf[:, 0], conf[:, 1]
    mx = xp.maximum(bg, fg)
    eb, ef = xp.exp(bg - mx), xp.exp(fg - mx)
    score = (eb if variant == "bg_as_score" else ef) / (eb + ef)
    half = 0.0 if variant == "no_half_stride" else stride / 2.0
    p = 4.0 * stride
    ax, ay = half + wx * stride, half + hy * stride
    tx, ty = loc[:, 0] * v_xy * p, loc[:, 1] * v_xy * p
    bw, bh = p * xp.exp(loc[:, 2] * v_wh), p * xp.exp(loc[:, 3] * v_wh)
    x1, y1 = ax + tx - bw / 2, ay + ty - bh / 2
    x2 = bw if variant == "x2_without_x1" else bw + x1
    y2 = bh + y1
    out = xp.stack([x1, y1, x2, y2, score], 1)
    m_x, m_y = xp.abs(ax) + xp.abs(tx) + bw / 2, xp.abs(ay) + xp.abs(ty) + bh / 2
    a_x, a_y = V_WH * xp.abs(loc[:, 2]) * bw, V_WH * xp.abs(loc[:, 3]) * bh
    bound = xp.stack([R * (m_x + a_x), R * (m_y + a_y), R * (m_x + bw + a_x), R * (m_y + bh + a_y), R + 0.0 * score], 1)
    return out, bound


def decode_case_ref(case, conf, loc, variant=None):
    B, FH, FW, ncls, stride = case[:5]
    wx, hy = positions(B, FH, FW, variant)
    return decode_ref(conf.astype(np.float64), loc.astype(np.float64), wx, hy, ncls, stride, variant)


def decode_f32(case, conf, loc):
    """s3fd_decode_kernel operation by operation in numpy fp32"""
    B, FH, FW, ncls, stride = case[:5]
    i = np.arange(B * FH * FW)
    wx, hy = (i % FW).astype(F32), ((i // FW) % FH).astype(F32)
    c, l = conf.astype(F32), loc.astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        if ncls == 4:
            bg, fg = np.maximum(np.maximum(c[:, 0], c[:, 1]), c[:, 2]), c[:, 3]
        else:
            bg, fg = c[:, 0], c[:, 1]
        mx = np.maximum(bg, fg)
        eb, ef = np.exp(bg - mx), np.exp(fg - mx)
        score = ef / (eb + ef)
        s = F32(stride)
        axc, ayc = s / F32(2) + wx * s, s / F32(2) + hy * s
        pw = F32(stride * 4)
        cx, cy = axc + l[:, 0] * F32(0.1) * pw, ayc + l[:, 1] * F32(0.1) * pw
        bw, bh = pw * np.exp(l[:, 2] * F32(0.2)), pw * np.exp(l[:, 3] * F32(0.2))
        cx, cy = cx - bw / F32(2), cy - bh / F32(2)
        out = np.stack([cx, cy, bw + cx, bh + cy, score], 1)
    assert out.dtype == F32
    return out


# ---------------------------------------------------------------- w2l_maxpool2x2
# (N, H, W, C, x_cs, y_cs)
POOL_CASES = [(2, 11, 14, 64, 64, 64), (1, 7, 9, 24, 40, 32), (3, 2, 3, 4, 4, 8), (1, 5, 5, 512, 512, 512), (2, 3, 2, 8, 16, 8)]
POOL_BIG = (1, 2050, 2048, 64, 64, 64)            # 1025 * 1024 * 16 float4 items > 65536 * 256
# bf16: one item; odd H and W (the dropped row and column hold +inf); two groups, two images, a free NaN group in x, y tight;
# channels >= C of y keep the sentinel
POOL_CASES_BF16 = [(1, 2, 2, 8, 8, 8), (1, 3, 5, 8, 8, 8), (2, 4, 6, 16, 24, 16), (1, 4, 4, 8, 8, 16)]
POOL_BIG_BF16 = (1, 2050, 2048, 128, 128, 128)    # the same cap, so the same 1025 * 1024 * 16 items, of 8 bf16 each
POOL_VARIANTS = ("second_row_stride_w_plus_1",)


def pool_inputs(case, seed, kind="fp32"):
    """x [N, H, W, x_cs] fp32 (bf16: rounded to it, which makes no value 0): N(0, 1) with a fiftieth +inf and a fiftieth -inf,
    every third window negative only (a maximum that starts from 0 shows there), the row and the column that an odd H or W drops +inf, channels >= C NaN.  No NaN and no
    zero inside the channels: fmaxf and torch differ on NaN and on windows that mix +0 and -0"""
    N, H, W, C, x_cs, _ = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, H, W, x_cs)).astype(F32)
    x[x == 0] = F32(1)
    what = rng.random((N, H, W, x_cs))
    oy, ox = np.mgrid[0:H, 0:W] // 2
    neg = ((oy + ox) % 3 == 0)[None, :, :, None]
    x = np.where(neg, -np.abs(x), x)
    x[what < 0.02] = np.inf
    x[(what >= 0.02) & (what < 0.04)] = -np.inf
    x = np.where(neg & (x == np.inf), F32(-np.inf), x).astype(F32)
    if H % 2:
        x[:, H - 1] = np.inf
    if W % 2:
        x[:, :, W - 1] = np.inf
    x[..., C:] = np.nan
    return to_bf16(x) if kind == "bf16" else x


def pool_ref(x, C, variant=None):
    """F.max_pool2d(x, 2, 2) of NHWC x: the maximum of the four strided slices.  The variant reads the window's second row one
    pixel further on in memory"""
    N, H, W = x.shape[:3]
    Ho, Wo = H // 2, W // 2
    sl = lambda dy, dx: x[:, dy:2 * Ho:2, dx:2 * Wo:2, :C]
    a, b = sl(0, 0), sl(0, 1)
    if variant is None:
        c, d = sl(1, 0), sl(1, 1)
    else:
        flat = x.reshape(N * H * W, -1)
        n, oy, ox = np.meshgrid(np.arange(N), np.arange(Ho), np.arange(Wo), indexing="ij")
        base = (n * H + 2 * oy) * W + 2 * ox
        last = N * H * W - 1
        c, d = flat[np.minimum(base + W + 1, last)][..., :C], flat[np.minimum(base + W + 2, last)][..., :C]
    return np.maximum(np.maximum(a, b), np.maximum(c, d))


def pool_f32(x, C, y_cs):
    """maxpool2x2_kernel item by item: the index arithmetic of the grid-stride loop over (pixel, float4 group), fmaxf nesting;
    returns y [N, Ho, Wo, y_cs] with SENT where nothing is written"""
    N, H, W, x_cs = x.shape
    Ho, Wo, C4 = H // 2, W // 2, C // 4
    flat = x.reshape(-1)
    y = np.full(N * Ho * Wo * y_cs, SENT, F32)
    i = np.arange(N * Ho * Wo * C4)
    c4, pix = i % C4, i // C4
    ox, pix = pix % Wo, pix // Wo
    oy, n = pix % Ho, pix // Ho
    p = ((n * H + 2 * oy) * W + 2 * ox) * x_cs + c4 * 4
    q = ((n * Ho + oy) * Wo + ox) * y_cs + c4 * 4
    for e in range(4):
        a, b, c, d = flat[p + e], flat[p + x_cs + e], flat[p + W * x_cs + e], flat[p + W * x_cs + x_cs + e]
        y[q + e] = np.maximum(np.maximum(a, b), np.maximum(c, d))
    return y.reshape(N, Ho, Wo, y_cs)


# ---------------------------------------------------------------- w2l_l2norm_scale
L2_SHAPES = [(4, 4, 4), (24, 32, 24), (64, 64, 64), (256, 256, 256), (260, 264, 272), (512, 520, 512), (1024, 1024, 1024)]
L2_ROWS = (1, 5, 70)
L2_KINDS = ("normal", "zero", "tiny", "last")
# bf16: lane 0 alone; exactly one 512-channel trip of all 64 lanes; a second trip that lane 0 takes alone.  Rows 1 and 5: the
# second workgroup of four rows is partial
L2_SHAPES_BF16 = [(8, 8, 8), (512, 512, 520), (520, 528, 520)]
L2_ROWS_BF16 = (1, 5)
L2_VARIANTS = ("eps_dropped", "eps_in_sqrt", "skip_from_256", "weight_mod_256")


def l2norm_cases(kind="fp32"):
    """(C, x_cs, y_cs, rows, rot): row r is of kind L2_KINDS[(r + rot) % 4]; one-row launches take every kind in turn"""
    shapes, nrows = (L2_SHAPES_BF16, L2_ROWS_BF16) if kind == "bf16" else (L2_SHAPES, L2_ROWS)
    return [(C, xc, yc, rows, rot) for C, xc, yc in shapes for rows in nrows for rot in (range(4) if rows == 1 else (0,))]


def l2norm_kinds(rows, rot):
    return [L2_KINDS[(r + rot) % 4] for r in range(rows)]


def l2norm_inputs(C, rows, rot, seed, kind="fp32"):
    """x [rows, C] (bf16: rounded to it), w [C] fp32.  zero: an all-zero row; tiny: N(0, 1) 1e-10, where the eps of the norm is a tenth of it and
    more; last: zero but for the last channel"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, C)) * 2).astype(F32)
    w = (0.5 + rng.random(C) * 10).astype(F32)
    for r, k in enumerate(l2norm_kinds(rows, rot)):
        if k == "zero":
            x[r] = 0
        elif k == "tiny":
            x[r] = (rng.standard_normal(C) * 1e-10).astype(F32)
        elif k == "last":
            x[r] = 0
            x[r, C - 1] = F32(2.5)
    return (to_bf16(x) if kind == "bf16" else x), w


def l2norm_variant_applies(C, kinds, variant):
    if variant == "eps_dropped":
        return "tiny" in kinds or "zero" in kinds
    if variant == "eps_in_sqrt":
        return "tiny" in kinds
    return C > 256 and set(kinds) != {"zero"}


def K2(C, kind="fp32"):
    return VEC[kind] * (-(-C // (64 * VEC[kind]))) + 7


def l2norm_ref(x, w, variant=None):
    """x / (sqrt(sum_c x^2) + 1e-10) w[c] in float64 (oracle/s3fd_ref.py::l2norm, net_s3fd.py:6-19)"""
    x, w = x.astype(np.float64), w.astype(np.float64)
    C = x.shape[1]
    ss = (x * x)[:, :256 if variant == "skip_from_256" else C].sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        if variant == "eps_dropped":
            norm = np.sqrt(ss)
        elif variant == "eps_in_sqrt":
            norm = np.sqrt(ss + EPS_NORM)
        else:
            norm = np.sqrt(ss) + EPS_NORM
        ww = w[np.arange(C) % 256] if variant == "weight_mod_256" else w
        return x / norm * ww[None, :]


def l2norm_bound(ref, C, kind="fp32"):
    """|y - ref| <= (K2(C) / 2 + 4) U |ref|, K2(C) = 4 ceil(C / 256) + 7.  The sum of squares: one rounding per product, four
    additions per lane and 256-channel trip (contracted into FMAs or not), six xor folds - K2 U relative, with no cancellation
    since every term is >= 0.  The root halves that and adds its own rounding; the eps sum, the division and the product by the
    weight one each: K2 / 2 + 4.  Where the reference is 0 the bound is 0: x = 0 gives 0 / norm * w = 0 exactly.
    bf16: the same fp32 arithmetic with eight additions per lane and 512-channel trip, K2 = 8 ceil(C / 512) + 7, gives a value v
    within b32 = (K2 / 2 + 4) U |ref|; the store rounds it once, |y - v| <= UB |v| <= UB (|ref| + b32)"""
    b32 = (K2(C, kind) / 2.0 + 4.0) * U * np.abs(ref)
    return b32 + UB * (np.abs(ref) + b32) if kind == "bf16" else b32


def l2norm_f32(x, w):
    """l2norm_scale_kernel in numpy fp32: lane l sums channels 4 l + 256 t .. + 3 (products added left to right, then to the
    lane's sum), a six-step xor butterfly, sqrtf + 1e-10f, v / norm * w"""
    rows, C = x.shape
    t = -(-C // 256)
    xp_ = np.zeros((rows, t * 256), F32)
    xp_[:, :C] = x
    v = xp_.reshape(rows, t, 64, 4)
    s = np.zeros((rows, 64), F32)
    with np.errstate(under="ignore"):
        for k in range(t):
            q = v[:, k] * v[:, k]
            s = s + (((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3])
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        assert s.dtype == F32 and (s == s[:, :1]).all()
        norm = np.sqrt(s[:, :1]) + F32(1e-10)
        y = x / norm * w[None, :]
    assert y.dtype == F32
    return y


# ---------------------------------------------------------------- w2l_s3fd_pack
PACK_YCS = (3, 4, 5, 8)
PACK_NPIX = (1, 255, 257)
PACK_BIG = 16384 * 256 + 3
PACK_YCS_BF16 = (8, 16)           # at 16 the second 8-channel group must be zeros, not the sentinel
PACK_BIG_BF16 = PACK_GRID_CAP["bf16"] * 256 + 1


def pack_inputs(npix):
    """BGR bytes [npix, 3]; from 256 pixels on every channel takes every byte value"""
    i = np.arange(npix)
    return np.stack([i % 256, (7 * i + 3) % 256, (255 - i) % 256], 1).astype(np.uint8)


def pack_vector_path(y_cs):
    """s3fd_store_px, fp32: one 16-byte store of (c0, c1, c2, 0), else three scalar stores"""
    return y_cs >= 4 and y_cs % 4 == 0


def pack_f32(bgr):
    """s3fd_pixel: RGB order, the mean subtracted in double, one cast"""
    b = bgr.astype(np.float64)
    return np.stack([b[:, 2] - 104.0, b[:, 1] - 117.0, b[:, 0] - 123.0], 1).astype(F32)


def pack_expected(rgb, y_cs, kind="fp32"):
    """the whole destination [npix, y_cs] after the launch on a SENT-filled buffer; bf16 writes every 8-channel group, the pixel
    (integers with |v| <= 152: exact) and zeros"""
    y = np.full((rgb.shape[0], y_cs), F32(0) if kind == "bf16" else SENT, F32)
    y[:, :3] = rgb
    if kind == "fp32" and pack_vector_path(y_cs):
        y[:, 3] = 0
    return y


# ---------------------------------------------------------------- w2l_datagen_pack / w2l_datagen_pack_bf16
DATAGEN_S = (2, 5, 7, 96)
DATAGEN_N = 3
# (y_cs, c_zero_to, elements the base pointer is moved from a 16-byte boundary)
DATAGEN_LAYOUTS = [(8, 8, 0), (6, 6, 0), (8, 7, 0), (12, 8, 0), (10, 8, 0), (8, 0, 0), (8, 8, 1)]
DATAGEN_BIG = (228, 96)                           # 228 * 96 * 96 > 8192 * 256
DATAGEN_VARIANTS = ("mask_row_gt_half",)


def datagen_store_path(elem_bytes, y_cs, c_zero_to, offset_elems):
    """datagen_pack_kernel: "vector" when c_zero_to = 8, the stride is a multiple of 16 bytes' worth of elements (4 fp32,
    8 bf16) and the base is 16-byte aligned; else scalar stores, named by the first condition that fails"""
    czt = max(c_zero_to, 6)
    if czt != 8:
        return "scalar_c_zero_to"
    if y_cs % (16 // elem_bytes) != 0:
        return "scalar_stride"
    if (offset_elems * elem_bytes) % 16 != 0:
        return "scalar_alignment"
    return "vector"


def datagen_inputs(N, S, seed):
    """faces uint8 [N, S, S, 3]: random, the first 256 pixels' first channel running through every byte value where there is
    room, nothing 0 in row S // 2 (where the two mask rules part)"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (N, S, S, 3), dtype=np.uint8)
    flat = f.reshape(-1, 3)
    k = min(256, flat.shape[0])
    flat[:k, 0] = np.arange(k)
    f = flat.reshape(N, S, S, 3)
    f[:, S // 2] = np.maximum(f[:, S // 2], 1)
    return f


def datagen_f32(faces, variant=None):
    """datagen_pack_kernel's six channels [N, S, S, 6] fp32: byte / 255 in double, one cast; rows >= S / 2 of the first three zero"""
    N, S = faces.shape[:2]
    v = (faces.astype(np.float64) / 255.0).astype(F32)
    row = np.arange(S)
    masked = (row > S // 2) if variant == "mask_row_gt_half" else (row >= S // 2)
    m = np.where(masked[None, :, None, None], F32(0), v)
    return np.concatenate([m, v], 3)


def datagen_expected(six, y_cs, c_zero_to):
    """the whole destination [npix, y_cs] (fp32 values) after the launch on a SENT-filled buffer"""
    czt = max(c_zero_to, 6)
    y = np.full((six.reshape(-1, 6).shape[0], y_cs), SENT, F32)
    y[:, :6] = six.reshape(-1, 6)
    y[:, 6:czt] = 0
    return y


# ---------------------------------------------------------------- w2l_frames_to_u8
FRAMES_XCS = (3, 4, 8)
FRAMES_SHAPES = [(1, 24, 32), (3, 16, 16)]        # 768 pixels each
FRAMES_BIG = (1, 1025, 2048)                      # > 8192 * 256 pixels


def frames_values():
    """the 256 values k / 255 in fp32, each with its fp32 neighbour below and above, kept inside [0, 1]: outside it the
    conversion to uint8 is undefined in the reference (numpy's astype) as in the kernel"""
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(F32)
    v = np.concatenate([np.nextafter(k, F32(-1)), k, np.nextafter(k, F32(2))])
    return np.clip(v, F32(0), F32(1)).astype(F32)


def frames_inputs():
    """[768, 3] fp32: every value of frames_values() once per channel, at different pixels"""
    v = frames_values()
    i = np.arange(v.size)
    return np.stack([v[i], v[(i + 256) % v.size], v[(i * 5 + 512) % v.size]], 1)


def frames_f32(x):
    """frames_to_u8_kernel: p * 255.0f, (uint8_t)(int) truncation"""
    return (x.astype(F32) * F32(255.0)).astype(np.int32).astype(np.uint8)


# ---------------------------------------------------------------- w2l_nchw_to_nhwc / w2l_nhwc_to_nchw (fp32)
# N, C, H, W, y_cs, c_zero_to: the shapes of LAYOUT_CASES in tests/test_bf16_train_ops_gpu.py ...
LAYOUT_CASES = {
    "ragged": (3, 37, 5, 9, 48, 40),
    "mel": (2, 1, 80, 16, 8, 8),
    "wide": (2, 70, 13, 11, 88, 72),
    "no_zero": (1, 24, 33, 3, 40, 0),
}
# ... and both sides of the 32 x 32 tile in channels and in pixels
for _C in (1, 32, 33):
    for _HW, (_H, _W) in ((1, (1, 1)), (31, (31, 1)), (33, (3, 11))):
        LAYOUT_CASES["C%d_HW%d" % (_C, _HW)] = (2, _C, _H, _W, _C + 7, _C + 3)


def layout_inputs(N, C, H, W, seed):
    """fp32 NCHW: N(0, 3) with +-0, +-inf, the smallest denormal and the largest finite value at the tail"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(N * C * H * W) * 3).astype(F32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 2.0 ** -149, -3.4028235e38], F32)
    k = min(len(sp), x.size - 1)
    if k > 0:
        x[-k:] = sp[:k]
    return x.reshape(N, C, H, W)


def layout_expected(x, y_cs, c_zero_to):
    N, C, H, W = x.shape
    y = np.full((N, H, W, y_cs), SENT, F32)
    y[..., :C] = x.transpose(0, 2, 3, 1)
    y[..., C:max(C, c_zero_to)] = 0
    return y


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def leaves(got, ref, bound):
    """elements of `got` outside ref +- bound; a NaN is outside"""
    with np.errstate(invalid="ignore"):
        return ~(np.abs(got - ref) <= bound)
