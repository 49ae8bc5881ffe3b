"""Train-mode BatchNorm, activation backward, column sums, row adds (csrc/train_rows.hip: one set of kernels instantiated for
bf16 and fp32 storage) and the bf16 graph-boundary layout changes (csrc/api.hip), through the C ABI, against float64 references computed with torch on
the CPU from the SAME values the device holds: inputs are rounded to the storage type first, then widened; the backward
references take the fp32 mean / rstd / scale / shift vectors the kernel consumed.

Bounds (ref = the float64 result, R = 2^-8 for bf16 storage and 2^-21 for fp32 storage - a few fp32 ulps: the sigmoid's expf,
a fused multiply-add and the residual add; `terms` = the magnitudes that enter the expression):
- exact: add_rows (== storage(float(a) + float(b))); act_bwd with ReLU / no activation and no scale (dz and g_out);
  nchw_to_nhwc_bf16 (== torch's round-to-nearest-even .to(bfloat16)); nhwc_bf16_to_nchw (== the stored bf16 value).
- one rounding to storage: |got - ref| <= R |ref| + 2^-22 sum|terms|: affine_act (terms |z scale|, |shift|, |res|); act_bwd
  with LeakyReLU / sigmoid / a scale and its g_out (terms |ref|).
- BatchNorm backward dz: |got - ref| <= R |ref| + 1e-6 |scale| (|g| + mean|g| + |zhat| mean|g zhat|), per element.
- column sums (dgamma, dbeta, col_sum) accumulate in fp64: |got - ref| <= 1e-7 |ref| + 1e-12 sum|terms|.  The product g * zhat
  is summed with zhat = (z - mean) * rstd formed in fp32 as the kernel forms it (its per-element arithmetic); everything
  above that is float64.
- statistics against float64 statistics of the STORED z: mean <= 2^-24 |ref| + 1e-12 mean|z| (one fp32 rounding),
  rstd <= (2^-24 + 1e-10) ref; scale == fp32(gamma rstd) within 2^-24 |ref|, shift = beta - mean scale within
  2^-23 (|beta| + |mean scale|); running stats after one update: (1 - m) r + m stat (stat = the UNBIASED variance for
  running_var) within 2^-21 ((1 - m) |r| + m |stat|).

Every tensor argument is a channel slice (cs > C, data at a channel offset): the channels outside an input's slice hold NaN (a
stray read poisons the result), those outside an output's slice a sentinel that must survive.  Pad channels [Cvalid, C) of the
per-channel outputs come out exactly 0; the per-channel inputs (gamma, beta, running stats) hold NaN / the sentinel there.

The column reductions are run through every partial regime of their launch rule (launch_rule below, a transcription of
col_reduce_launch): one workgroup, 2-12 workgroups (the finalize's 4-wide walk only), >= 16 workgroups (its
16-wide walk, then the 4-wide tail) and the 512-workgroup cap with a ragged last workgroup."""
import ctypes as C

import numpy as np
import pytest
import torch

from wav2lip_amd import _lib
from wav2lip_amd._lib import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID

pytestmark = pytest.mark.gpu

BF16, FP32 = "bf16", "fp32"
EPS, MOM = 1e-5, 0.1
EPS32, MOM32 = float(np.float32(EPS)), float(np.float32(MOM))   # what the kernels receive
SENT = 12352.0                                                  # exact in bf16 and fp32; no kernel below produces it
NAN = float("nan")
ACTS = {"none": ACT_NONE, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID, "leaky": ACT_LEAKY}

CHANNELS = {BF16: [8, 16, 24, 72, 256, 384, 1000, 1024], FP32: [4, 12, 384, 1020, 1024]}
# channels that exist (bf16 only: the fp32 entries have no Cvalid); the rest of C are pad channels, zero in the tensors
CVALID = {8: 8, 16: 13, 24: 24, 72: 67, 256: 256, 384: 379, 1000: 995, 1024: 1024}
# workgroups of the column reduction in each regime (see regime_rows)
REGIME_BLOCKS = {"one": 1, "few": 8, "many": 23, "cap": 512}


def _dtype(prec):
    return torch.bfloat16 if prec == BF16 else torch.float32


def _width(prec):
    """channels per thread and row (16 bytes)"""
    return 8 if prec == BF16 else 4


def _rel(prec):
    return 2.0 ** -8 if prec == BF16 else 2.0 ** -21


def launch_rule(prec, C_, rows):
    """(workgroups, rows per workgroup, row lanes RPP) of col_reduce_launch: C / width threads per row, RPP = 256 / (C / width)
    rows in flight, at least RPP * 64 / width rows per workgroup (8 bf16, 16 fp32: 64 elements per thread), at most 512"""
    rpp = 256 // (C_ // _width(prec))
    min_rows = rpp * (8 if prec == BF16 else 16)
    per = max(-(-rows // 512), min_rows)
    return -(-rows // per), per, rpp


def regime_rows(prec, C_, regime):
    _, m, rpp = launch_rule(prec, C_, 1)          # m = the minimum rows per workgroup
    return {"one": m - 1,                        # one workgroup; the last row lane gets one row fewer than the others
            "few": 7 * m + rpp // 2 + 1,         # 8 workgroups, the last one with fewer rows than lanes: 4-wide finalize only
            "many": 22 * m + 5,                  # 23 workgroups: the 16-wide finalize walk, then its tail over blocks 16-22
            "cap": 512 * (m + 1) - 1}[regime]    # 512 workgroups (the cap) of m + 1 rows, the last of m: ~8.4 M elements


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _cs(t):
    return 0 if t is None else t.stride(0)


def _slab(host, cs, off, fill, cuda):
    """[rows, C] host tensor -> device buffer [rows, cs] holding it at channel offset `off`, `fill` elsewhere; (buffer, view)"""
    rows, C_ = host.shape
    buf = torch.full((rows, cs), fill, dtype=host.dtype, device=cuda)
    buf[:, off:off + C_] = host.to(cuda)
    return buf, buf[:, off:off + C_]


def _out(rows, C_, cs, off, dtype, cuda):
    buf = torch.full((rows, cs), SENT, dtype=dtype, device=cuda)
    return buf, buf[:, off:off + C_]


def _outside_intact(buf, off, C_, fill):
    rest = torch.cat([buf[:, :off], buf[:, off + C_:]], 1)
    return bool(torch.isnan(rest).all()) if fill != fill else bool((rest == fill).all())


def _pvec(vals, n, fill, cuda):
    """fp32 per-channel vector of n entries: `vals` first, `fill` after"""
    v = torch.full((n,), fill, dtype=torch.float32)
    if vals is not None:
        v[:len(vals)] = vals
    return v.to(cuda)


def _within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)                       # NaN counts as outside
    assert not bool(bad.any()), "%s: %d of %d outside the bound (worst excess %.3e)" % (
        what, int(bad.sum()), bad.numel(), float((err - bound).nan_to_num(float("inf")).max()))


def _d(t):
    return t.double().cpu()


# ---------------------------------------------------------------- the entry points, one signature per operation
def _stats(prec, rows, C_, Cv, z, gamma, beta, rm, rv, out):
    lib, s = _lib.load(), _lib.current_stream()
    if prec == BF16:
        return lib.w2l_bn_train_stats_bf16(s, rows, C_, Cv, _p(z), _cs(z), _p(gamma), _p(beta), EPS, MOM, _p(rm), _p(rv),
                                           *(_p(t) for t in out))
    assert Cv == C_
    return lib.w2l_bn_train_stats(s, rows, C_, _p(z), _cs(z), _p(gamma), _p(beta), EPS, MOM, _p(rm), _p(rv), *(_p(t) for t in out))


def _affine(prec, rows, C_, z, scale, shift, res, act, y):
    fn = _lib.load().w2l_affine_act_bf16 if prec == BF16 else _lib.load().w2l_affine_act
    return fn(_lib.current_stream(), rows, C_, _p(z), _cs(z), _p(scale), _p(shift), _p(res), _cs(res), act, _p(y), _cs(y))


def _bn_bwd(prec, rows, C_, Cv, dy, y, z, act, mean, rstd, scale, shift, dgamma, dbeta, dz, g_out):
    lib, s = _lib.load(), _lib.current_stream()
    if prec == BF16:
        return lib.w2l_bn_train_bwd_bf16(s, rows, C_, Cv, _p(dy), _cs(dy), _p(y), _cs(y), _p(z), _cs(z), act, _p(mean), _p(rstd),
                                         _p(scale), _p(shift), _p(dgamma), _p(dbeta), _p(dz), _cs(dz), _p(g_out), _cs(g_out))
    assert Cv == C_
    return lib.w2l_bn_train_bwd(s, rows, C_, _p(dy), _cs(dy), _p(y), _cs(y), _p(z), _cs(z), act, _p(mean), _p(rstd), _p(scale),
                                _p(dgamma), _p(dbeta), _p(dz), _cs(dz), _p(g_out), _cs(g_out))


def _bn_apply(rows, C_, dy, y, z, act, mean, rstd, scale, shift, dgamma, dbeta, dz, g_out):
    return _lib.load().w2l_bn_train_bwd_apply_bf16(_lib.current_stream(), rows, C_, _p(dy), _cs(dy), _p(y), _cs(y), _p(z), _cs(z),
                                                   act, _p(mean), _p(rstd), _p(scale), _p(shift), _p(dgamma), _p(dbeta), _p(dz),
                                                   _cs(dz), _p(g_out), _cs(g_out))


def _act_bwd(prec, rows, C_, dy, y, act, scale, dz, g_out):
    fn = _lib.load().w2l_act_bwd_bf16 if prec == BF16 else _lib.load().w2l_act_bwd
    return fn(_lib.current_stream(), rows, C_, _p(dy), _cs(dy), _p(y), _cs(y), act, _p(scale), _p(dz), _cs(dz), _p(g_out), _cs(g_out))


def _add_rows(prec, rows, C_, a, b, out):
    fn = _lib.load().w2l_add_rows_bf16 if prec == BF16 else _lib.load().w2l_add_rows
    return fn(_lib.current_stream(), rows, C_, _p(a), _cs(a), _p(b), _cs(b), _p(out), _cs(out))


def _col_sum(prec, rows, C_, x, out):
    fn = _lib.load().w2l_col_sum_bf16 if prec == BF16 else _lib.load().w2l_col_sum
    return fn(_lib.current_stream(), rows, C_, _p(x), _cs(x), _p(out))


# ---------------------------------------------------------------- data
def _make_z(rows, C_, Cv, dtype, gen):
    """z [rows, C]: odd channels N(0.3, 1.7^2); even channels values on a 1/16 grid placed symmetrically about a channel mean
    that is a multiple of 1/2 (exact in bf16 and in the fp64 sums), a quarter of them exactly ON the mean - with beta = 0 there,
    z * scale + shift lands on the ReLU mask boundary (the sign is the rounding error of mean * scale); pad channels zero"""
    z = torch.randn(rows, C_, generator=gen) * 1.7 + 0.3
    h, ne = rows // 2, (Cv + 1) // 2
    d = torch.randint(-40, 41, (h, ne), generator=gen).float() / 16
    d[torch.rand(h, ne, generator=gen) < 0.25] = 0
    m = torch.randint(-3, 4, (1, ne), generator=gen).float() / 2
    ev = m.expand(rows, ne).clone()
    ev[0:2 * h:2] += d
    ev[1:2 * h:2] -= d
    z[:, 0:Cv:2] = ev
    z[:, Cv:] = 0
    return z.to(dtype)


def _randn(rows, C_, Cv, dtype, gen, scale=1.0):
    x = torch.randn(rows, C_, generator=gen) * scale
    x[:, Cv:] = 0
    return x.to(dtype)


# ---------------------------------------------------------------- the column reductions through every regime
CHAIN_CASES = [(p, c, r) for p in (BF16, FP32) for c in CHANNELS[p] for r in REGIME_BLOCKS]


@pytest.mark.parametrize("prec,C_,regime", CHAIN_CASES, ids=["%s-C%d-%s" % c for c in CHAIN_CASES])
def test_batchnorm_chain_through_every_reduction_regime(prec, C_, regime, cuda):
    """stats -> affine_act (ReLU) -> BatchNorm backward -> col_sum over the stored dz, each against float64 of the stored
    operands (bounds in the module docstring), every tensor a NaN-fenced channel slice.  Also: two calls of each reduction are
    bit-identical; bf16: y omitted (the mask recomputed as z * scale + shift), g_out written in place of dy, and the
    apply-only entry (with y, without y, and premasked: dy = g, y = NULL, act = none) all write the dz of the first call bit
    for bit."""
    dt, w, R = _dtype(prec), _width(prec), _rel(prec)
    Cv = CVALID[C_] if prec == BF16 else C_
    rows = regime_rows(prec, C_, regime)
    nb, per, _ = launch_rule(prec, C_, rows)
    assert nb == REGIME_BLOCKS[regime] and (regime != "cap" or rows - (nb - 1) * per < per)
    gen = torch.Generator().manual_seed(C_ * 10 + list(REGIME_BLOCKS).index(regime))
    z = _make_z(rows, C_, Cv, dt, gen)
    gamma = torch.rand(Cv, generator=gen) + 0.5
    beta = torch.randn(Cv, generator=gen) * 0.3
    beta[0::2] = 0
    rm0, rv0 = torch.randn(Cv, generator=gen) * 0.1, torch.rand(Cv, generator=gen) + 0.5
    nv = C_ + w                                                   # per-channel buffers: a sentinel / NaN tail after C
    _, zv = _slab(z, C_ + 3 * w, w, NAN, cuda)
    gam, bet = _pvec(gamma, nv, NAN, cuda), _pvec(beta, nv, NAN, cuda)
    rm, rv = _pvec(rm0, nv, SENT, cuda), _pvec(rv0, nv, SENT, cuda)
    st = [_pvec(None, nv, SENT, cuda) for _ in range(4)]
    _lib.check(_stats(prec, rows, C_, Cv, zv, gam, bet, rm, rv, st), "stats")
    st2 = [_pvec(None, nv, SENT, cuda) for _ in range(4)]
    _lib.check(_stats(prec, rows, C_, Cv, zv, gam, bet, None, None, st2), "stats again")
    torch.cuda.synchronize()
    for a, b in zip(st, st2):
        assert torch.equal(a, b), "statistics are not deterministic"
    mean_d, rstd_d, scale_d, shift_d = st
    # ---- statistics against float64 of the stored z
    zs = z[:, :Cv].double()
    mean64 = zs.mean(0)
    var64 = (zs - mean64).square().mean(0)
    m_, r_, sc_, sh_ = (_d(t) for t in st)
    _within(m_[:Cv], mean64, 2.0 ** -24 * mean64.abs() + 1e-12 * zs.abs().mean(0), "mean")
    rstd64 = 1.0 / torch.sqrt(var64 + EPS32)
    _within(r_[:Cv], rstd64, (2.0 ** -24 + 1e-10) * rstd64, "rstd")
    g64 = gamma.double()
    _within(sc_[:Cv], g64 * r_[:Cv], 2.0 ** -24 * (g64 * r_[:Cv]).abs(), "scale")
    _within(sh_[:Cv], beta.double() - m_[:Cv] * sc_[:Cv], 2.0 ** -23 * (beta.double().abs() + (m_[:Cv] * sc_[:Cv]).abs()), "shift")
    for t, name in ((m_, "mean"), (r_, "rstd"), (sc_, "scale"), (sh_, "shift")):
        assert bool((t[Cv:C_] == 0).all()), "pad channels of %s must be 0" % name
        assert bool((t[C_:] == SENT).all()), "%s written past C" % name
    unb = var64 * rows / (rows - 1)
    rm_ref = (1 - MOM32) * rm0.double() + MOM32 * mean64
    rv_ref = (1 - MOM32) * rv0.double() + MOM32 * unb
    rm_, rv_ = _d(rm), _d(rv)
    _within(rm_[:Cv], rm_ref, 2.0 ** -21 * ((1 - MOM32) * rm0.double().abs() + MOM32 * mean64.abs()), "running_mean")
    _within(rv_[:Cv], rv_ref, 2.0 ** -21 * ((1 - MOM32) * rv0.double() + MOM32 * unb), "running_var (unbiased variance)")
    assert bool((rm_[Cv:] == SENT).all()) and bool((rv_[Cv:] == SENT).all()), "running stats of pad channels touched"

    # ---- forward: y = relu(z * scale + shift)
    ybuf, yv = _out(rows, C_, C_ + 5 * w, 0, dt, cuda)
    _lib.check(_affine(prec, rows, C_, zv, scale_d, shift_d, None, ACT_RELU, yv), "affine_act")
    torch.cuda.synchronize()
    assert _outside_intact(ybuf, 0, C_, SENT), "affine_act wrote outside its slice"
    sc64, sh64 = sc_[:Cv], sh_[:Cv]
    lin = zs * sc64 + sh64
    ys = _d(yv)
    _within(ys[:, :Cv], lin.clamp_min(0), R * lin.abs() + 2.0 ** -22 * ((zs * sc64).abs() + sh64.abs()), "affine_act y")
    assert bool((ys[:, Cv:] == 0).all())
    del lin

    # ---- backward
    dy = _randn(rows, C_, Cv, dt, gen)
    dybuf, dyv = _slab(dy, C_ + 2 * w, w, NAN, cuda)

    def outs():
        dzb, dzv = _out(rows, C_, C_ + 4 * w, 2 * w, dt, cuda)
        return dzb, dzv, _pvec(None, nv, SENT, cuda), _pvec(None, nv, SENT, cuda)
    dzb1, dz1, dg1, db1 = outs()
    _lib.check(_bn_bwd(prec, rows, C_, Cv, dyv, yv, zv, ACT_RELU, mean_d, rstd_d, scale_d, shift_d, dg1, db1, dz1, None), "bn_bwd")
    _, dz1b, dg1b, db1b = outs()
    _lib.check(_bn_bwd(prec, rows, C_, Cv, dyv, yv, zv, ACT_RELU, mean_d, rstd_d, scale_d, shift_d, dg1b, db1b, dz1b, None), "again")
    torch.cuda.synchronize()
    assert torch.equal(dz1, dz1b) and torch.equal(dg1, dg1b) and torch.equal(db1, db1b), "BatchNorm backward is not deterministic"
    assert _outside_intact(dzb1, 2 * w, C_, SENT), "bn_bwd wrote outside its dz slice"
    dys = dy[:, :Cv].double()
    g = dys * (ys[:, :Cv] > 0)
    mu32, rs32 = mean_d[:Cv].cpu(), rstd_d[:Cv].cpu()
    zh32 = ((z[:, :Cv].float() - mu32) * rs32).double()              # the kernel's fp32 zhat
    gz32 = g * zh32
    del zh32
    dg_, db_ = _d(dg1), _d(db1)
    ref_db, ref_dg = g.sum(0), gz32.sum(0)
    _within(db_[:Cv], ref_db, 1e-7 * ref_db.abs() + 1e-12 * g.abs().sum(0), "dbeta")
    _within(dg_[:Cv], ref_dg, 1e-7 * ref_dg.abs() + 1e-12 * gz32.abs().sum(0), "dgamma")
    del gz32
    for t, name in ((dg_, "dgamma"), (db_, "dbeta")):
        assert bool((t[Cv:C_] == 0).all()), "pad channels of %s must be 0" % name
        assert bool((t[C_:] == SENT).all()), "%s written past C" % name
    zh = (zs - m_[:Cv]) * r_[:Cv]
    mg, mgz = g.mean(0), (g * zh).mean(0)
    ref_dz = sc64 * (g - mg - zh * mgz)
    dzs = _d(dz1)
    _within(dzs[:, :Cv], ref_dz, R * ref_dz.abs() + 1e-6 * sc64.abs() * (g.abs() + g.abs().mean(0) + zh.abs() * (g * zh).abs().mean(0)),
            "dz")
    assert bool((dzs[:, Cv:] == 0).all())
    del zh, ref_dz

    # g_out in place of dy (autograd.NodeB with a residual): the same dz, dy overwritten with g = dy * mask
    gbuf, gv = _slab(dy, C_ + 2 * w, w, NAN, cuda)
    dzb3, dz3, dg3, db3 = outs()
    _lib.check(_bn_bwd(prec, rows, C_, Cv, gv, yv, zv, ACT_RELU, mean_d, rstd_d, scale_d, shift_d, dg3, db3, dz3, gv), "bn_bwd g")
    torch.cuda.synchronize()
    assert torch.equal(dz3, dz1) and torch.equal(dg3, dg1) and torch.equal(db3, db1)
    assert torch.equal(_d(gv)[:, :Cv], g), "in-place g_out"
    assert _outside_intact(gbuf, w, C_, NAN)
    if prec == BF16:
        # y omitted: the mask is the forward's own z * scale + shift > 0, also where that sits on the boundary
        dzb2, dz2, dg2, db2 = outs()
        _lib.check(_bn_bwd(prec, rows, C_, Cv, dyv, None, zv, ACT_RELU, mean_d, rstd_d, scale_d, shift_d, dg2, db2, dz2, None),
                   "bn_bwd without y")
        # the elementwise half alone, given the sums: with y, without y, and premasked (dy = g, act none)
        applied = []
        for dyx, yx, act in ((dyv, yv, ACT_RELU), (dyv, None, ACT_RELU), (gv, None, ACT_NONE)):
            dzbx, dzx, _, _ = outs()
            _lib.check(_bn_apply(rows, C_, dyx, yx, zv, act, mean_d, rstd_d, scale_d, shift_d, dg1, db1, dzx, None), "apply")
            applied.append((dzbx, dzx))
        torch.cuda.synchronize()
        assert torch.equal(dz2, dz1) and torch.equal(dg2, dg1) and torch.equal(db2, db1), "y omitted changes the result"
        for i, (dzbx, dzx) in enumerate(applied):
            assert torch.equal(dzx, dz1), "bn_train_bwd_apply_bf16 form %d" % i
            assert _outside_intact(dzbx, 2 * w, C_, SENT)
        assert _outside_intact(dybuf, w, C_, NAN) and torch.equal(_d(dyv), dy.double()), "dy changed without g_out"

    # ---- column sums of the stored dz (a conv bias gradient)
    cs1, cs2 = _pvec(None, nv, SENT, cuda), _pvec(None, nv, SENT, cuda)
    _lib.check(_col_sum(prec, rows, C_, dz1, cs1), "col_sum")
    _lib.check(_col_sum(prec, rows, C_, dz1, cs2), "col_sum again")
    torch.cuda.synchronize()
    assert torch.equal(cs1, cs2), "col_sum is not deterministic"
    c_ = _d(cs1)
    _within(c_[:C_], dzs.sum(0), 1e-7 * dzs.sum(0).abs() + 1e-12 * dzs.abs().sum(0), "col_sum")
    assert bool((c_[C_:] == SENT).all())


@pytest.mark.parametrize("prec", [BF16, FP32])
def test_batchnorm_statistics_defaults_for_null_parameters(prec, cuda):
    """gamma = NULL -> 1, beta = NULL -> 0 (scale == rstd, shift == -(mean * rstd) bit for bit), running stats NULL -> skipped;
    rows = 1: variance 0, rstd = 1 / sqrt(eps), and the running variance takes the (biased = 0) variance, no division by 0"""
    w = _width(prec)
    C_ = 3 * w
    Cv = C_ - 3 if prec == BF16 else C_
    gen = torch.Generator().manual_seed(5)
    for rows in (1, 1000):
        z = _randn(rows, C_, Cv, _dtype(prec), gen, 2.0)
        _, zv = _slab(z, C_ + w, 0, NAN, cuda)
        st = [_pvec(None, C_, SENT, cuda) for _ in range(4)]
        _lib.check(_stats(prec, rows, C_, Cv, zv, None, None, None, None, st), "stats")
        rm, rv = _pvec(torch.zeros(Cv), C_, SENT, cuda), _pvec(torch.ones(Cv), C_, SENT, cuda)
        st2 = [_pvec(None, C_, SENT, cuda) for _ in range(4)]
        _lib.check(_stats(prec, rows, C_, Cv, zv, None, None, rm, rv, st2), "stats with running")
        torch.cuda.synchronize()
        for a, b in zip(st, st2):
            assert torch.equal(a, b)
        mean, rstd, scale, shift = (t.cpu() for t in st)
        assert torch.equal(scale, rstd) and torch.equal(shift[:Cv], -(mean[:Cv] * rstd[:Cv]))
        assert bool((shift[Cv:] == 0).all()) and bool((rstd[Cv:] == 0).all())
        zs = z[:, :Cv].double()
        var = zs.var(0, unbiased=False)
        _within(rstd[:Cv].double(), 1.0 / torch.sqrt(var + EPS32), 1e-7 / torch.sqrt(var + EPS32), "rstd")
        unb = var * rows / (rows - 1) if rows > 1 else var
        _within(rv.cpu()[:Cv].double(), (1 - MOM32) + MOM32 * unb, 2.0 ** -21 * ((1 - MOM32) + MOM32 * unb), "running_var")
        assert bool((rv.cpu()[Cv:] == SENT).all()) and bool((rm.cpu()[Cv:] == SENT).all())


# ---------------------------------------------------------------- elementwise passes
EW_CHANNELS = {BF16: [8, 72, 1000], FP32: [4, 12, 1020]}
EW_CASES = [(p, c) for p in (BF16, FP32) for c in EW_CHANNELS[p]]
EW_ROWS = 3001      # several workgroups of RPP * 4 rows, a ragged last one


def _act_ref(x, act):
    if act == ACT_RELU:
        return x.clamp_min(0)
    if act == ACT_LEAKY:
        return torch.where(x > 0, x, 0.01 * x)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    return x


def _act_grad_ref(y, act):
    if act == ACT_RELU:
        return (y > 0).double()
    if act == ACT_LEAKY:
        return torch.where(y > 0, 1.0, 0.01).double()
    if act == ACT_SIGMOID:
        return y * (1 - y)
    return torch.ones_like(y)


@pytest.mark.parametrize("act", list(ACTS), ids=list(ACTS))
@pytest.mark.parametrize("prec,C_", EW_CASES, ids=["%s-C%d" % c for c in EW_CASES])
def test_affine_act(prec, C_, act, cuda):
    """y = act(z * scale + shift (+ res)): one rounding to storage of the float64 result (terms |z scale|, |shift|, |res|)"""
    dt, w, R = _dtype(prec), _width(prec), _rel(prec)
    rows, a = EW_ROWS, ACTS[act]
    gen = torch.Generator().manual_seed(C_ + a)
    z, res = _randn(rows, C_, C_, dt, gen, 1.5), _randn(rows, C_, C_, dt, gen)
    scale, shift = torch.randn(C_, generator=gen), torch.randn(C_, generator=gen) * 0.5
    _, zv = _slab(z, C_ + w, w, NAN, cuda)
    _, rv = _slab(res, C_ + 3 * w, 2 * w, NAN, cuda)
    sc, sh = _pvec(scale, C_ + w, NAN, cuda), _pvec(shift, C_ + w, NAN, cuda)
    zs, rs, s64, h64 = z.double(), res.double(), scale.double(), shift.double()
    for with_res in (False, True):
        ybuf, yv = _out(rows, C_, C_ + 2 * w, w, dt, cuda)
        _lib.check(_affine(prec, rows, C_, zv, sc, sh, rv if with_res else None, a, yv), "affine_act")
        torch.cuda.synchronize()
        assert _outside_intact(ybuf, w, C_, SENT)
        lin = zs * s64 + h64 + (rs if with_res else 0)
        terms = (zs * s64).abs() + h64.abs() + (rs.abs() if with_res else 0)
        ref = _act_ref(lin, a)
        _within(_d(yv), ref, R * ref.abs() + 2.0 ** -22 * terms, "affine_act %s res=%d" % (act, with_res))


@pytest.mark.parametrize("act", list(ACTS), ids=list(ACTS))
@pytest.mark.parametrize("prec,C_", EW_CASES, ids=["%s-C%d" % c for c in EW_CASES])
def test_act_bwd(prec, C_, act, cuda):
    """dz = dy * act'(y) (* scale), g_out = dy * act'(y): every activation x scale NULL / given x g_out NULL / separate / in
    place of dy.  Exact for ReLU and no activation without a scale, one rounding to storage otherwise"""
    dt, w, R = _dtype(prec), _width(prec), _rel(prec)
    rows, a = EW_ROWS, ACTS[act]
    gen = torch.Generator().manual_seed(100 + C_ + a)
    pre = _randn(rows, C_, C_, torch.float32, gen, 2.0)
    pre[::7] = 0                                                       # y exactly 0 (the mask boundary)
    y = _act_ref(pre.double(), a).to(dt)
    dy = _randn(rows, C_, C_, dt, gen)
    scale = torch.rand(C_, generator=gen) * 2 + 0.25
    _, yv = _slab(y, C_ + 2 * w, w, NAN, cuda)
    ys, dys = y.double(), dy.double()
    g_ref = dys * _act_grad_ref(ys, a)
    for with_scale in (False, True):
        sc = _pvec(scale, C_ + w, NAN, cuda) if with_scale else None
        dz_ref = g_ref * scale.double() if with_scale else g_ref
        exact = a in (ACT_NONE, ACT_RELU) and not with_scale
        for g_mode in ("none", "separate", "in_place"):
            dybuf, dyv = _slab(dy, C_ + 3 * w, 2 * w, NAN, cuda)
            dzbuf, dzv = _out(rows, C_, C_ + w, 0, dt, cuda)
            gbuf, gv = (None, None) if g_mode == "none" else (dybuf, dyv) if g_mode == "in_place" else _out(rows, C_, C_ + 2 * w, w, dt, cuda)
            # act none: y is not read (NULL allowed)
            _lib.check(_act_bwd(prec, rows, C_, dyv, None if a == ACT_NONE else yv, a, sc, dzv, gv), "act_bwd")
            torch.cuda.synchronize()
            what = "act_bwd %s scale=%d g=%s" % (act, with_scale, g_mode)
            assert _outside_intact(dzbuf, 0, C_, SENT), what
            if exact:
                assert torch.equal(_d(dzv), dz_ref), what
            else:
                _within(_d(dzv), dz_ref, R * dz_ref.abs() + 2.0 ** -22 * dz_ref.abs(), what)
            if gv is not None:
                assert _outside_intact(gbuf, 2 * w if g_mode == "in_place" else w, C_, NAN if g_mode == "in_place" else SENT), what
                if a in (ACT_NONE, ACT_RELU):
                    assert torch.equal(_d(gv), g_ref), what + " g_out"
                else:
                    _within(_d(gv), g_ref, R * g_ref.abs() + 2.0 ** -22 * g_ref.abs(), what + " g_out")


@pytest.mark.parametrize("prec,C_", EW_CASES, ids=["%s-C%d" % c for c in EW_CASES])
def test_add_rows(prec, C_, cuda):
    """out = storage(float(a) + float(b)) exactly, into a separate slice and in place of a (autograd.NodeB's residual gradient)"""
    dt, w = _dtype(prec), _width(prec)
    rows = EW_ROWS
    gen = torch.Generator().manual_seed(200 + C_)
    a, b = _randn(rows, C_, C_, dt, gen, 3.0), _randn(rows, C_, C_, dt, gen)
    b[::5] = -a[::5]                                                   # exact cancellations
    ref = (a.float() + b.float()).to(dt)
    abuf, av = _slab(a, C_ + 2 * w, w, NAN, cuda)
    _, bv = _slab(b, C_ + 3 * w, 3 * w, NAN, cuda)
    obuf, ov = _out(rows, C_, C_ + w, 0, dt, cuda)
    _lib.check(_add_rows(prec, rows, C_, av, bv, ov), "add_rows")
    _lib.check(_add_rows(prec, rows, C_, av, bv, av), "add_rows in place")
    torch.cuda.synchronize()
    assert torch.equal(ov.cpu(), ref) and _outside_intact(obuf, 0, C_, SENT)
    assert torch.equal(av.cpu(), ref) and _outside_intact(abuf, w, C_, NAN)


BWD_ACTS = {"relu_res": (ACT_RELU, True), "leaky_res": (ACT_LEAKY, True), "leaky": (ACT_LEAKY, False), "none": (ACT_NONE, False)}


@pytest.mark.parametrize("kind", list(BWD_ACTS), ids=list(BWD_ACTS))
@pytest.mark.parametrize("prec", [BF16, FP32])
def test_batchnorm_backward_activations(prec, kind, cuda):
    """BatchNorm backward with the mask from a stored y = act(z * scale + shift (+ res)) for LeakyReLU, ReLU with a residual and
    no activation; g_out in place of dy when the block has a residual.  dz, dgamma, dbeta, g against float64 (module docstring)"""
    act, with_res = BWD_ACTS[kind]
    dt, w, R = _dtype(prec), _width(prec), _rel(prec)
    C_ = 72 if prec == BF16 else 12
    Cv = 67 if prec == BF16 else C_
    rows = 1501
    gen = torch.Generator().manual_seed(300 + act)
    z = _make_z(rows, C_, Cv, dt, gen)
    _, zv = _slab(z, C_ + w, 0, NAN, cuda)
    gamma = _pvec(torch.rand(Cv, generator=gen) + 0.5, C_, NAN, cuda)
    beta = _pvec(torch.randn(Cv, generator=gen) * 0.3, C_, NAN, cuda)
    st = [_pvec(None, C_, SENT, cuda) for _ in range(4)]
    _lib.check(_stats(prec, rows, C_, Cv, zv, gamma, beta, None, None, st), "stats")
    mean_d, rstd_d, scale_d, shift_d = st
    res = _randn(rows, C_, Cv, dt, gen)
    _, resv = _slab(res, C_ + 2 * w, w, NAN, cuda)
    _, yv = _out(rows, C_, C_ + w, 0, dt, cuda)
    _lib.check(_affine(prec, rows, C_, zv, scale_d, shift_d, resv if with_res else None, act, yv), "affine_act")
    dy = _randn(rows, C_, Cv, dt, gen)
    dybuf, dyv = _slab(dy, C_ + 3 * w, 2 * w, NAN, cuda)
    dzbuf, dzv = _out(rows, C_, C_ + 2 * w, w, dt, cuda)
    dg, db = _pvec(None, C_ + w, SENT, cuda), _pvec(None, C_ + w, SENT, cuda)
    _lib.check(_bn_bwd(prec, rows, C_, Cv, dyv, yv, zv, act, mean_d, rstd_d, scale_d, shift_d, dg, db, dzv,
                       dyv if with_res else None), "bn_bwd")
    torch.cuda.synchronize()
    assert _outside_intact(dzbuf, w, C_, SENT) and _outside_intact(dybuf, 2 * w, C_, NAN)
    ys, dys, zs = _d(yv)[:, :Cv], dy[:, :Cv].double(), z[:, :Cv].double()
    m_, r_, sc_ = (_d(t)[:Cv] for t in (mean_d, rstd_d, scale_d))
    neg = {ACT_RELU: 0.0, ACT_LEAKY: float(np.float32(0.01)), ACT_NONE: 1.0}[act]
    g = dys * torch.where(ys > 0, 1.0, neg).double()
    if act == ACT_LEAKY:
        g = g.float().double()                                         # dy * 0.01f rounded to fp32, as the kernel forms it
    zh32 = ((z[:, :Cv].float() - mean_d[:Cv].cpu()) * rstd_d[:Cv].cpu()).double()
    ref_db, ref_dg = g.sum(0), (g * zh32).sum(0)
    dg_, db_ = _d(dg), _d(db)
    _within(db_[:Cv], ref_db, 1e-7 * ref_db.abs() + 1e-12 * g.abs().sum(0), "dbeta")
    _within(dg_[:Cv], ref_dg, 1e-7 * ref_dg.abs() + 1e-12 * (g * zh32).abs().sum(0), "dgamma")
    assert bool((dg_[Cv:C_] == 0).all()) and bool((db_[Cv:C_] == 0).all()) and bool((dg_[C_:] == SENT).all())
    zh = (zs - m_) * r_
    ref_dz = sc_ * (g - g.mean(0) - zh * (g * zh).mean(0))
    _within(_d(dzv)[:, :Cv], ref_dz, R * ref_dz.abs() + 1e-6 * sc_.abs() * (g.abs() + g.abs().mean(0) + zh.abs() * (g * zh).abs().mean(0)),
            "dz")
    if with_res:
        gd = _d(dyv)[:, :Cv]
        if act == ACT_RELU:
            assert torch.equal(gd, g), "in-place g_out"
        else:
            _within(gd, g, R * g.abs(), "in-place g_out")


# ---------------------------------------------------------------- layout at the graph boundary
LAYOUT_CASES = {  # N, C, H, W, y_cs, c_zero_to
    "ragged": (3, 37, 5, 9, 48, 40),       # C and H*W (45) not multiples of 32, pad channels [37, 40), [40, 48) untouched
    "mel": (2, 1, 80, 16, 8, 8),           # the mel input of bf16 inference: one channel zero-padded to 8
    "wide": (2, 70, 13, 11, 88, 72),       # C > 64: three channel tiles
    "no_zero": (1, 24, 33, 3, 40, 0),      # c_zero_to < C means C
}


@pytest.mark.parametrize("case", list(LAYOUT_CASES))
def test_layout_kernels_bf16(case, cuda):
    """nchw_to_nhwc_bf16 == torch's round-to-nearest-even .to(bfloat16) bit for bit (ties, +-0, +-inf and a value that rounds
    up to inf included), zeros in [C, c_zero_to), channels from c_zero_to to y_cs untouched; nhwc_bf16_to_nchw from a NaN-fenced
    slice with x_cs > C returns the stored bf16 values exactly, and writes nothing past its output"""
    lib, s = _lib.load(), _lib.current_stream()
    N, C_, H, W, y_cs, czt = LAYOUT_CASES[case]
    gen = torch.Generator().manual_seed(len(case))
    x = torch.randn(N, C_, H, W, generator=gen) * 3
    flat = x.view(-1)
    b = flat[: flat.numel() // 2].to(torch.bfloat16).float()
    nxt = (b.view(torch.int32) + (1 << 16)).view(torch.float32)         # the next bf16 value away from zero
    flat[: b.numel() // 2] = ((b + nxt) / 2)[: b.numel() // 2]          # exact ties between neighbouring bf16 values
    specials = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 3.4e38, -3.4e38, 1.00390625, 1.01171875])
    flat[-len(specials):] = specials[: min(len(specials), flat.numel())]
    xd = x.to(cuda)
    y = torch.full((N, H, W, y_cs), SENT, dtype=torch.bfloat16, device=cuda)
    _lib.check(lib.w2l_nchw_to_nhwc_bf16(s, N, C_, H, W, _p(xd), _p(y), y_cs, czt), "nchw_to_nhwc_bf16")
    torch.cuda.synchronize()
    yc = y.cpu()
    ref = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    assert torch.equal(yc[..., :C_].view(torch.int16), ref.view(torch.int16)), "rounding differs from round-to-nearest-even"
    zt = max(czt, C_)
    assert bool((yc[..., C_:zt] == 0).all()) and bool((yc[..., zt:] == SENT).all())
    # back: from a slice at channel offset 8 of a NaN-filled buffer
    x_cs = y_cs + 16
    buf = torch.full((N, H, W, x_cs), NAN, dtype=torch.bfloat16, device=cuda)
    buf[..., 8:8 + C_] = ref.to(cuda)
    out = torch.full((N * C_ * H * W + 64,), SENT, device=cuda)
    _lib.check(lib.w2l_nhwc_bf16_to_nchw(s, N, C_, H, W, C.c_void_p(buf[..., 8:].data_ptr()), x_cs, _p(out)), "nhwc_bf16_to_nchw")
    torch.cuda.synchronize()
    oc = out.cpu()
    assert torch.equal(oc[:-64].view(N, C_, H, W), ref.float().permute(0, 3, 1, 2)) and bool((oc[-64:] == SENT).all())


# ---------------------------------------------------------------- argument errors
def _marker():
    """put a known message into w2l_last_error, so that the next failure is seen to write its own"""
    lib = _lib.load()
    assert lib.w2l_adam_create(0, None, C.byref(C.c_void_p())) != 0
    return lib.w2l_last_error()


def _refused(rc, what):
    msg = _lib.load().w2l_last_error()
    assert rc != 0, "%s: accepted" % what
    assert msg and msg != MARK[0], "%s: no message" % what


MARK = [None]


@pytest.mark.parametrize("prec", [BF16, FP32])
def test_argument_errors_write_nothing(prec, cuda):
    """each entry refuses, with a message and before writing anything: C not a multiple of the vector width, C > 1024, a channel
    stride below C or not a multiple of the width, a pointer off 16-byte alignment, Cvalid > C (bf16), y omitted with a
    non-ReLU activation or together with g_out (bf16 BatchNorm backward)"""
    dt, w = _dtype(prec), _width(prec)
    rows, C0, cs0 = 64, 4 * w, 6 * w
    big = torch.zeros(rows * 2000, dtype=dt, device=cuda)                 # big enough for any of the row views below
    vecs = [torch.full((1100,), SENT, device=cuda) for _ in range(8)]
    outs = [torch.full((rows * 2000,), SENT, dtype=dt, device=cuda) for _ in range(3)]
    mis = lambda t: C.c_void_p(t.data_ptr() + 2 * t.element_size())        # noqa: E731  2 elements off alignment

    class A:                                                              # a row view by pointer and stride
        def __init__(self, t, cs):
            self.t, self.cs = t, cs

        def data_ptr(self):
            return self.t.data_ptr() if isinstance(self.t, torch.Tensor) else self.t.value

        def stride(self, _):
            return self.cs
    MARK[0] = _marker()
    bad = {"C % width": (C0 + w // 2, cs0, None), "C > 1024": (1024 + w, 1024 + w, None), "cs < C": (C0, C0 - w, None),
           "cs % width": (C0, cs0 + 2, None), "misaligned": (C0, cs0, "mis")}
    for name, (C_, cs, how) in bad.items():
        inp = A(mis(big) if how else big, cs)
        o0, o1 = (A(mis(t) if how else t, cs) for t in outs[:2])
        Cv = min(C_, C0)
        calls = {
            "stats": lambda: _stats(prec, rows, C_, Cv if prec == BF16 else C_, inp, vecs[0], vecs[1], vecs[2], vecs[3], vecs[4:8]),
            "affine": lambda: _affine(prec, rows, C_, inp, vecs[0], vecs[1], None, ACT_RELU, o0),
            "bn_bwd": lambda: _bn_bwd(prec, rows, C_, Cv if prec == BF16 else C_, inp, inp, inp, ACT_RELU, vecs[0], vecs[1], vecs[2],
                                      vecs[3], vecs[4], vecs[5], o0, o1),
            "act_bwd": lambda: _act_bwd(prec, rows, C_, inp, inp, ACT_RELU, None, o0, o1),
            "add_rows": lambda: _add_rows(prec, rows, C_, inp, inp, o0),
            "col_sum": lambda: _col_sum(prec, rows, C_, inp, vecs[4]),
        }
        if prec == BF16:
            calls["apply"] = lambda: _bn_apply(rows, C_, inp, inp, inp, ACT_RELU, *vecs[0:6], o0, o1)
        for entry, call in calls.items():
            _refused(call(), "%s %s" % (entry, name))
            MARK[0] = _marker()
        if name in ("C % width", "C > 1024"):
            continue                                                      # properties of the call, not of one tensor
        # well-formed inputs, the bad layout on an output only
        good, dz_ok = A(big, cs0), A(outs[2], cs0)
        for entry, call in {"affine y": lambda: _affine(prec, rows, C0, good, vecs[0], vecs[1], None, ACT_RELU, o0),
                            "bn_bwd dz": lambda: _bn_bwd(prec, rows, C0, C0, good, good, good, ACT_RELU, *vecs[0:6], o0, None),
                            "bn_bwd g": lambda: _bn_bwd(prec, rows, C0, C0, good, good, good, ACT_RELU, *vecs[0:6], dz_ok, o0),
                            "act_bwd dz": lambda: _act_bwd(prec, rows, C0, good, good, ACT_RELU, None, o0, None),
                            "act_bwd g": lambda: _act_bwd(prec, rows, C0, good, good, ACT_RELU, None, dz_ok, o0),
                            "add_rows out": lambda: _add_rows(prec, rows, C0, good, good, o0)}.items():
            _refused(call(), "%s %s" % (entry, name))
            MARK[0] = _marker()
    if prec == BF16:
        good = A(big, cs0)
        o0, o1 = A(outs[0], cs0), A(outs[1], cs0)
        _refused(_stats(prec, rows, C0, C0 + 1, good, None, None, None, None, vecs[4:8]), "stats Cvalid > C")
        MARK[0] = _marker()
        _refused(_bn_bwd(prec, rows, C0, C0 + 1, good, good, good, ACT_RELU, *vecs[0:6], o0, None), "bn_bwd Cvalid > C")
        MARK[0] = _marker()
        for act in (ACT_LEAKY, ACT_SIGMOID, ACT_NONE):
            _refused(_bn_bwd(prec, rows, C0, C0, good, None, good, act, *vecs[0:6], o0, None), "bn_bwd y omitted, act %d" % act)
            MARK[0] = _marker()
        _refused(_bn_bwd(prec, rows, C0, C0, good, None, good, ACT_RELU, *vecs[0:6], o0, o1), "bn_bwd y omitted with g_out")
        MARK[0] = _marker()
        _refused(_bn_bwd(prec, rows, C0, C0, good, None, good, ACT_RELU, *vecs[0:3], None, *vecs[4:6], o0, None),
                 "bn_bwd y omitted without shift")
        MARK[0] = _marker()
        for act in (ACT_LEAKY, ACT_SIGMOID):
            _refused(_bn_apply(rows, C0, good, None, good, act, *vecs[0:6], o0, None), "apply y omitted, act %d" % act)
            MARK[0] = _marker()
        _refused(_bn_apply(rows, C0, good, None, good, ACT_RELU, *vecs[0:6], o0, o1), "apply y omitted with g_out")
        MARK[0] = _marker()
        ly = torch.full((2, 4, 4, 16), SENT, dtype=torch.bfloat16, device=cuda)
        lx = torch.zeros(2, 12, 4, 4, device=cuda)
        lib, s = _lib.load(), _lib.current_stream()
        _refused(lib.w2l_nchw_to_nhwc_bf16(s, 2, 12, 4, 4, _p(lx), _p(ly), 16, 24), "nchw_to_nhwc_bf16 y_cs < c_zero_to")
        MARK[0] = _marker()
        _refused(lib.w2l_nchw_to_nhwc_bf16(s, 2, 12, 4, 4, _p(lx), _p(ly), 8, 0), "nchw_to_nhwc_bf16 y_cs < C")
        MARK[0] = _marker()
        _refused(lib.w2l_nhwc_bf16_to_nchw(s, 2, 12, 4, 4, _p(ly), 8, _p(lx)), "nhwc_bf16_to_nchw x_cs < C")
        torch.cuda.synchronize()
        assert bool((ly == SENT).all()) and bool((lx == 0).all())
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENT).all()), "a refused call wrote its output"
    for v in vecs:
        assert bool((v == SENT).all()), "a refused call wrote a per-channel vector"
