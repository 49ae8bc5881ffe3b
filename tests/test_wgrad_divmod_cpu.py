"""The float-reciprocal index split of the weight-gradient kernels, without a GPU: fast_divmod (csrc/conv_wgrad.hip: pixel ->
image, row, column) and divmod_f (csrc/conv_wino_wgrad.hip: 2x2 tile -> image, tile row, tile column) compute
    q = (int)((float)a * (1.0f / (float)d));  r = a - q * d;  one correction step (q -+ 1)
and claim a / d, a % d exactly for 0 <= a < 2^31 and a quotient below 2^22.  Three things are compared for every (a, d) below: the
true integer quotient and remainder, a numpy float32 restatement of the expression, and the library's own functions evaluated
on the host (w2l_wgrad_divmod_host runs the very functions the kernels inline) - so a change of the kernels' arithmetic fails here.

Why one correction is enough: (float)a, the reciprocal and the product each carry a relative error of at most 2^-24, so the
estimate is off by less than 3 * 2^-24 * q + 1 (truncation) < 2 for q < 2^22: q is off by at most one.  Above that range it is
not: a = 2^27 - 3, d = 1 gives (float)a = 2^27, q = 2^27, r = -3 -> one step back leaves r = -2.

What keeps a launch inside the claim (asserted below through the dry run, so that relaxing a guard fails this file):
  * direct GEMM: numerators are P-grid pixels < N*Hp*Wp < 2^27 (the 2 GiB guard with >= 4 channels of 4 bytes) and rows' remainders
    < Hp*Wp; quotients are the image n < N and the row y < Hp, both refused from 2^22 on;
  * Winograd: numerators are tiles < T < 2^24 (wino_wgrad_ok), quotients n < N and ty < TH <= H with N*H < 2^22 (wino_wgrad_ok)."""
import ctypes as C

import numpy as np

from wav2lip_amd import _lib
from wav2lip_amd._lib import ConvGeom, WgradInfo

A_LIMIT, Q_LIMIT = 1 << 31, 1 << 22


def restated(a, d):
    """numpy float32 restatement of fast_divmod / divmod_f (identical bodies), int64 lanes standing in for the kernels' int32"""
    inv = np.float32(1.0) / d.astype(np.float32)
    q = (a.astype(np.float32) * inv).astype(np.int64)           # v_cvt_f32_i32 rounds to nearest even; (int) truncates
    r = a - q * d
    lo, hi = (r < 0).astype(np.int64), (r >= d).astype(np.int64)
    return q + hi - lo, r + (lo - hi) * d


def library(which, a, d):
    lib = _lib.load()
    a32, d32 = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(d, dtype=np.int32)
    q, r = np.empty_like(a32), np.empty_like(a32)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    _lib.check(lib.w2l_wgrad_divmod_host(which, len(a32), p(a32), p(d32), p(q), p(r)), "divmod_host")
    return q.astype(np.int64), r.astype(np.int64)


def numerators(d, rng):
    """both sides of multiples of d: the lowest, the highest inside the claim (a < 2^31, q < 2^22) and random ones"""
    top = min(A_LIMIT - 1, d * Q_LIMIT - 1)
    mmax = top // d
    ms = np.unique(np.concatenate([np.arange(0, min(mmax, 40) + 1), np.arange(max(mmax - 40, 0), mmax + 1),
                                   rng.integers(0, mmax + 1, 200)]))
    a = (ms[:, None] * d + np.arange(-2, 3)[None, :]).ravel()
    return a[(a >= 0) & (a <= top)]


def divisors():
    """every divisor the launchers can pass is a product Hp*Wp, a width Wp, TH*TW or TW: all small ones, the neighbourhood of every
    power of two up to the largest admitted (2^27 pixels under the 2 GiB guard), and the products of the project's own shapes"""
    ds = set(range(1, 1 << 13))
    for e in range(13, 28):
        ds.update(range((1 << e) - 3, (1 << e) + 4))
    for h, w in ((96, 96), (48, 96), (46, 47), (23, 24), (80, 16), (27, 16), (9, 6), (21, 19), (13, 13), (17, 30), (7, 9)):
        ds.update((h * w, w, ((h + 1) // 2) * ((w + 1) // 2), (w + 1) // 2))
    rng = np.random.default_rng(7)
    ds.update(int(v) for v in rng.integers(1 << 13, 1 << 27, 3000))
    return sorted(v for v in ds if v <= 1 << 27)


def test_one_correction_step_is_exact_inside_the_claimed_range():
    rng = np.random.default_rng(11)
    aa, dd = [], []
    for d in divisors():
        a = numerators(d, rng)
        aa.append(a)
        dd.append(np.full_like(a, d))
    a, d = np.concatenate(aa), np.concatenate(dd)
    assert len(a) > 5_000_000 and int(a.max()) == A_LIMIT - 1 and int((a // d).max()) == Q_LIMIT - 1
    q, r = restated(a, d)
    bad = np.flatnonzero((q != a // d) | (r != a % d))
    assert bad.size == 0, "restated: a=%d d=%d -> q=%d r=%d" % (a[bad[0]], d[bad[0]], q[bad[0]], r[bad[0]])
    for which, name in ((0, "fast_divmod"), (1, "divmod_f")):
        ql, rl = library(which, a, d)
        bad = np.flatnonzero((ql != a // d) | (rl != a % d))
        assert bad.size == 0, "%s: a=%d d=%d -> q=%d r=%d" % (name, a[bad[0]], d[bad[0]], ql[bad[0]], rl[bad[0]])


def test_the_claim_does_not_hold_above_its_range():
    """the guards below are needed: past a quotient of 2^22 a single correction is not enough"""
    a, d = np.array([(1 << 27) - 3]), np.array([1])
    q, r = restated(a, d)
    assert (int(q[0]), int(r[0])) != ((1 << 27) - 3, 0)
    assert tuple(int(v[0]) for v in library(0, a, d)) == (int(q[0]), int(r[0]))     # the library computes what is restated here


def _resolve(g, N, H, W, xcs, dcs):
    info = WgradInfo()
    rc = _lib.load().w2l_conv_wgrad_resolve(C.byref(g), N, H, W, xcs, dcs, _lib.PREC_F32, C.byref(info))
    return rc, info


def test_the_launchers_keep_every_call_inside_the_claimed_range():
    lib = _lib.load()
    k1 = ConvGeom(0, 8, 8, 1, 1, 1, 1, 0, 0, 0, 0, 0)
    # numerators: the 2 GiB guard admits fewer than 2^31 / (8 channels * 4 bytes) = 2^26 pixels here, 2^27 at 4 channels
    assert _resolve(k1, 1, 1, 1 << 26, 8, 8)[0] != 0 and b"2 GiB" in lib.w2l_last_error()
    rc, info = _resolve(k1, 2, 1, (1 << 25) - 1, 8, 8)
    assert rc == 0 and info.family == _lib.WGRAD_DIRECT and info.K == (1 << 26) - 2
    # direct GEMM quotients: image index and row, refused from 2^22 on
    rc, info = _resolve(k1, (1 << 22) - 1, 1, 1, 8, 8)
    assert rc == 0 and info.family == _lib.WGRAD_DIRECT and info.K == (1 << 22) - 1
    assert _resolve(k1, 1 << 22, 1, 1, 8, 8)[0] != 0 and b"2^22" in lib.w2l_last_error()
    assert _resolve(k1, 1, (1 << 22) - 1, 1, 8, 8)[0] == 0
    assert _resolve(k1, 1, 1 << 22, 1, 8, 8)[0] != 0 and b"2^22" in lib.w2l_last_error()
    # Winograd: wino_wgrad_ok wants N*H < 2^22 and T < 2^24.  Its fill-ratio clause admits no layer whose wider side has under 56
    # channels, i.e. under 224 bytes per pixel, and H, W >= 5: the 2 GiB guard then implies both (N*H*W < 2^31 / 224 < 2^24)
    up = lambda v: (v + 63) // 64 * 64
    least = min(max(ci, co) for ci in range(1, 65) for co in range(1, 65) if ci * co * 4 >= up(ci) * up(co) * 3)
    assert least == 56 and (1 << 31) // (least * 4) < 1 << 24 and (1 << 31) // (least * 4) // 5 < 1 << 22
    k3 = lambda ci, co: ConvGeom(0, ci, co, 3, 3, 1, 1, 1, 1, 0, 0, 0)
    assert _resolve(k3(48, 64), 64, 64, 64, 48, 64)[1].family == _lib.WGRAD_WINO
    assert _resolve(k3(47, 64), 64, 64, 64, 48, 64)[1].family == _lib.WGRAD_DIRECT
    N = ((1 << 31) - 1) // (25 * 64 * 4)                     # the largest batch of 5x5 images the byte guard admits
    rc, info = _resolve(k3(48, 64), N, 5, 5, 48, 64)
    assert rc == 0 and info.family == _lib.WGRAD_WINO and info.K == N * 9 < 1 << 24 and N * 5 < 1 << 22
    assert _resolve(k3(48, 64), N + 1, 5, 5, 48, 64)[0] != 0 and b"2 GiB" in lib.w2l_last_error()
