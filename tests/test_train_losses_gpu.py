"""The kernels that close a training step - the loss forward / backward pairs, SyncNet's L2 normalisation and the fused
multi-tensor Adam (csrc/train.hip; l2norm_rows_kernel, cosine_rows_kernel and bce_mean_kernel in csrc/api.hip) - through the C
ABI, against float64 references computed on the CPU from the SAME fp32 values the device holds (constants such as 1e-12 and
Adam's scalars enter the references as their fp32 roundings).  Every tensor with a stride argument is a channel slice: NaN outside
an input's slice, the sentinel outside an output's slice, which must survive; every output has sentinel guard cells behind it.

Bounds (tests/_loss_cases.py holds the formulas, tests/test_train_losses_bounds_cpu.py checks them against fp32 restatements of
the kernels; u = 2^-24, R = 2^-21 as in tests/test_bf16_train_ops_gpu.py, K = ceil(C / 64) + 7):
- a one-wave row reduction over C terms: ceil(C / 64) + 6 additions of once-rounded products, error <= K u sum|terms|;
- l1_mean accumulates in fp64: |got - ref| <= 2^-23 |ref| (one fp32 subtraction per term, one cast); l1_bwd is exact:
  +-fp32(gout fp32(1 / n)) or 0;
- l2norm_rows: R |y| + K u |y| / 2 (nothing inherited under the 1e-12 clamp); a zero row gives exactly 0;
- l2norm_bwd, dx = t1 - t2 with t1 = dy / d, t2 = x <x, dy> / d^3: R (|t1| + |t2|) + K u (|t1| / 2 + 3 |t2| / 2 +
  |x| sum|x dy| / d^3); under the clamp dx == dy / 1e-12f bit for bit;
- the cosine: |cs| (K + 2.5) u + K u sum|a v| / den = E_cs (1.5 u for den = sqrt(na nv), one for the quotient);
- bce_mean: per term R (|y lp| + |(1 - y) lq|) + (1 - y) u [p < 0.5] (the rounding of 1 - p, passed on by the logarithm), then
  (ceil(N / 256) + 9) u sum|terms| for the 256-thread strided sum and its 6 + 3 additions, one u for the division; after the
  cosine additionally sum_i |dL/dcs_i| E_cs_i;
- cosine_bce_bwd: stage by stage from E_cs - E_dcos = |h'(cs)| E_cs + R |dcos|, E_k1, E_ka, E_da as listed at
  _loss_cases.cosine_bce_bounds; the amplification |h'| = 1 / ((1 - cs) cs) + ... is part of the formula, not a factor;
- bce_bwd: R |ref| + 2^-149 / max((1 - p) p, 1e-12) (a denormal p times g / N leaves the fp32 grid);
- Adam, one step from identical fp32 state with the fp32 scalars the kernel receives (bc1 and sqrt(bc2) rounded as the host
  rounds them): exp_avg within 2^-22 (|m0| + |g| + wd |p|) - relative to the magnitudes that enter, since m0 and the step may
  cancel -, exp_avg_sq within 2^-22 v + 2^-149 (+ 4 u (1 - beta2) |g'| (|g| + wd |p|) with weight decay), the parameter within
  2^-24 |p| + R lr / bc1 |m / denom| of the float64 expression at the moments the device wrote; the 5-step trajectory against
  float64 torch.optim.Adam within the sum over its steps of the single-step bound from the state, at the float64 trajectory's
  magnitudes (earlier steps' moment errors are not carried into later parameter steps: tighter than a worst case).

Edge rows of the cosine pair take their reference at the fp32 cosine the forward launch wrote (E_cs = 0): the floors of the BCE
amplify one ulp of the cosine beyond any bound on the inputs, and the same comparison fails if the backward's recomputed cosine
differs from cos_out by a bit.  Outside [0, 1], where ATen raises, the kernels stay finite: lq = -100 where 1 - p <= 0, lp = -100
where p <= 0, the gradient factor (p - y) / 1e-12 where (1 - p) p < 1e-12: the BCE entries get 1 + 2^-23 and
-2^-23 directly, and the edge test asserts that near-equal rows give cosines on both sides of 1 on the device.  On the MI355X bitwise-equal rows give a cosine of exactly
1, rows an ulp apart reach 1 + 2^-23 (3 of the 24 such rows here), and the two kernels' cosines agree on every edge row."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _loss_cases as lc
from _loss_cases import F32, SENT
from wav2lip_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64
ERR_ARG = -1


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _slab(host, cs, off, cuda):
    """[rows, C] fp32 array -> device buffer [rows, cs] holding it at channel offset `off`, NaN elsewhere; (buffer, view)"""
    rows, C_ = host.shape
    buf = torch.full((rows, cs), NAN, dtype=torch.float32, device=cuda)
    buf[:, off:off + C_] = _dev(host, cuda)
    return buf, buf[:, off:off + C_]


def _out(rows, C_, cs, off, cuda):
    """sentinel-filled [rows + 1, cs] buffer (a guard row behind the last), and the [rows, C] view a kernel may write"""
    buf = torch.full((rows + 1, cs), SENT, dtype=torch.float32, device=cuda)
    return buf, buf[:rows, off:off + C_]


def _flat(n, cuda):
    return torch.full((n + GUARD,), SENT, dtype=torch.float32, device=cuda)


def _outside_intact(buf, rows, off, C_):
    b = buf.cpu()
    return bool((b[rows:] == SENT).all()) and bool((b[:rows, :off] == SENT).all()) and bool((b[:rows, off + C_:] == SENT).all())


def _within(got, ref, bound, what):
    got, ref, bound = (np.asarray(t, np.float64) for t in (got, ref, bound))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print("ratio %s %.4f" % (what, float(np.nanmax(ratio)) if ratio.size else 0.0))
    bad = ~(err <= bound)                       # NaN counts as outside
    assert not bad.any(), "%s: %d of %d outside the bound (worst error / bound %.3f)" % (what, int(bad.sum()), bad.size,
                                                                                         float(np.max(np.nan_to_num(ratio, nan=np.inf))))


def _np(t):
    return t.detach().cpu().numpy()


def _gout(g, cuda):
    return None if g is None else torch.tensor([g, SENT], dtype=torch.float32, device=cuda)


def _lib_s():
    return _lib.load(), _lib.current_stream()


# ---------------------------------------------------------------- L1
@pytest.mark.parametrize("n", list(lc.L1_CASES))
def test_l1_mean_and_backward(n, cuda):
    """every regime of the two-stage mean (partials, lane 0's trips through mean_final_kernel's unrolled loop, the lanes in that
    loop, the width of its tail) and the exact backward with a device gout and gout = NULL"""
    lib, s = _lib_s()
    nb, trips0, lanes, tail = lc.L1_CASES[n]
    assert lc.l1_partials(n) == nb and lc.mean_final_walk(nb) == (trips0, lanes, tail)
    a, b = lc.l1_inputs(n, n % 1000)
    assert n < 100 or ((a == b).mean() > 0.05 and (np.abs(a - b) == np.spacing(a)).mean() > 0.02)
    ad, bd = _dev(a, cuda), _dev(b, cuda)
    out = _flat(1, cuda)
    _lib.check(lib.w2l_l1_mean(s, n, _p(ad), _p(bd), _p(out)), "l1_mean")
    torch.cuda.synchronize()
    o = _np(out)
    assert (o[1:] == SENT).all()
    ref = lc.l1_ref(a, b)
    _within(o[0], ref, lc.l1_bound(ref), "l1_mean")
    for g in (None, 0.7, -2.0):
        da = _flat(n, cuda)
        gd = _gout(g, cuda)
        _lib.check(lib.w2l_l1_bwd(s, n, _p(ad), _p(bd), _p(gd), _p(da)), "l1_bwd")
        torch.cuda.synchronize()
        d = _np(da)
        assert (d[n:] == SENT).all(), "l1_bwd wrote past n"
        assert np.array_equal(d[:n], lc.l1_bwd_ref(a, b, g, n)), "l1_bwd is exact (gout %s)" % g
        assert n < 100 or (d[:n] == 0).any()


def test_l1_mean_back_to_back_share_the_scratch(cuda):
    """two means enqueued on one stream without a synchronisation between them use the same per-stream fp64 scratch: 261 partials,
    then 2 partials over the head of the same buffers; both results are right"""
    lib, s = _lib_s()
    n1, n2 = 260 * 4096 + 5, 4097
    a, b = lc.l1_inputs(n1, 5)
    ad, bd = _dev(a, cuda), _dev(b, cuda)
    o1, o2, o3 = _flat(1, cuda), _flat(1, cuda), _flat(1, cuda)
    _lib.check(lib.w2l_l1_mean(s, n1, _p(ad), _p(bd), _p(o1)), "l1_mean")
    _lib.check(lib.w2l_l1_mean(s, n2, _p(ad), _p(bd), _p(o2)), "l1_mean")
    _lib.check(lib.w2l_l1_mean(s, n1, _p(ad), _p(bd), _p(o3)), "l1_mean")
    torch.cuda.synchronize()
    r1, r2 = lc.l1_ref(a, b), lc.l1_ref(a[:n2], b[:n2])
    assert abs(r1 - r2) > 100 * lc.l1_bound(r1)                 # a mix-up of the two would show
    _within(_np(o1)[0], r1, lc.l1_bound(r1), "l1_mean first")
    _within(_np(o2)[0], r2, lc.l1_bound(r2), "l1_mean second")
    assert torch.equal(o1, o3), "l1_mean is not deterministic"


# ---------------------------------------------------------------- L2 normalisation
# (x_cs - C, x offset, dx_cs - C, dx offset): dense; both C + 12 at offset 5; x and dx with different strides and offsets
L2_LAYOUTS = {"dense": (0, 0, 0, 0), "slice": (12, 5, 12, 5), "mixed": (12, 5, 7, 3)}
L2_CASES = [(N, C_, lay) for N in lc.L2_N for C_ in lc.L2_C for lay in L2_LAYOUTS]


@pytest.mark.parametrize("N,C_,layout", L2_CASES, ids=["N%d-C%d-%s" % c for c in L2_CASES])
def test_l2norm_rows_and_backward(N, C_, layout, cuda):
    """F.normalize and its autograd in float64; x and dx dense (stride C), slices of C + 12 channels at offset 5, or x such a slice and dx one of C + 7
    channels at offset 3 (a kernel that took one stride for the other would show); rows well
    scaled, all zero, and with the norm just below / above the 1e-12 clamp (both branches of k), every kind in every row slot"""
    lib, s = _lib_s()
    (xpad, off, dpad, doff), cs, dcs = L2_LAYOUTS[layout], C_ + L2_LAYOUTS[layout][0], C_ + L2_LAYOUTS[layout][2]
    for rot in range(4):
        x, dy, kinds = lc.l2_inputs(N, C_, rot, 1000 * N + C_)
        _, _, nrm = lc.l2_ref(x)
        for r, k in enumerate(kinds):
            assert {"scaled": nrm[r] > 1e-3, "zero": nrm[r] == 0, "below": 0 < nrm[r] < lc.EPS_L2, "above": nrm[r] > lc.EPS_L2}[k]
        xbuf, xv = _slab(x, cs, off, cuda)
        y = _flat(N * C_, cuda)
        _lib.check(lib.w2l_l2norm_rows(s, N, C_, _p(xv), cs, _p(y)), "l2norm_rows")
        dyd = _dev(dy, cuda)
        dxbuf, dxv = _out(N, C_, dcs, doff, cuda)
        _lib.check(lib.w2l_l2norm_bwd(s, N, C_, _p(xv), cs, _p(dyd), _p(dxv), dcs), "l2norm_bwd")
        torch.cuda.synchronize()
        yh = _np(y)
        assert (yh[N * C_:] == SENT).all(), "l2norm_rows wrote behind its last row"
        assert _outside_intact(dxbuf, N, doff, C_), "l2norm_bwd wrote outside its slice"
        x64 = torch.from_numpy(x).double().requires_grad_(True)
        ref = F.normalize(x64, p=2, dim=1, eps=lc.EPS_L2)
        ref.backward(torch.from_numpy(dy).double())
        what = "N%d C%d rot%d" % (N, C_, rot)
        got_y, got_dx = yh[:N * C_].reshape(N, C_), _np(dxv)
        _within(got_y, _np(ref), lc.l2_bound(x), "l2norm_rows " + what)
        _within(got_dx, _np(x64.grad), lc.l2_bwd_bound(x, dy), "l2norm_bwd " + what)
        z = [r for r, k in enumerate(kinds) if k == "zero"]
        assert (got_y[z] == 0).all(), "a zero row normalises to exactly 0"
        c = [r for r, k in enumerate(kinds) if k in ("zero", "below")]
        assert np.array_equal(got_dx[c], dy[c] / F32(1e-12)), "under the clamp dx == dy / 1e-12f"


# ---------------------------------------------------------------- cosine + BCE
COS_CASES = [(N, C_, nm, "hard") for N in lc.COS_N for C_ in lc.COS_C for nm in (True, False)] + [(130, 512, True, "soft")]


def _cosine_launches(a, v, y, gouts, cuda):
    """forward with y = NULL, forward with y, backward per gout -> (cos without y, cos, loss, [(da, dv)]); every sentinel checked"""
    lib, s = _lib_s()
    N, C_ = a.shape
    ad, vd, yd = _dev(a, cuda), _dev(v, cuda), _dev(y, cuda)
    cos0, loss0 = _flat(N, cuda), _flat(1, cuda)
    _lib.check(lib.w2l_cosine_bce(s, N, C_, _p(ad), _p(vd), None, _p(cos0), _p(loss0)), "cosine")
    cos1, loss1 = _flat(N, cuda), _flat(1, cuda)
    _lib.check(lib.w2l_cosine_bce(s, N, C_, _p(ad), _p(vd), _p(yd), _p(cos1), _p(loss1)), "cosine_bce")
    grads = []
    for g in gouts:
        da, dv = _flat(N * C_, cuda), _flat(N * C_, cuda)
        _lib.check(lib.w2l_cosine_bce_bwd(s, N, C_, _p(ad), _p(vd), _p(yd), _p(_gout(g, cuda)), _p(da), _p(dv)), "cosine_bce_bwd")
        grads.append((da, dv))
    torch.cuda.synchronize()
    assert bool((loss0 == SENT).all()), "loss_out touched with y = NULL"
    c0, c1, l1 = _np(cos0), _np(cos1), _np(loss1)
    assert (c0[N:] == SENT).all() and (c1[N:] == SENT).all() and (l1[1:] == SENT).all()
    assert np.array_equal(c0[:N], c1[:N]), "the cosine depends on y"
    res = []
    for da, dv in grads:
        dah, dvh = _np(da), _np(dv)
        assert (dah[N * C_:] == SENT).all() and (dvh[N * C_:] == SENT).all(), "cosine_bce_bwd wrote behind its last row"
        res.append((dah[:N * C_].reshape(N, C_), dvh[:N * C_].reshape(N, C_)))
    return c1[:N], l1[0], res


@pytest.mark.parametrize("N,C_,normalised,labels", COS_CASES,
                         ids=["N%d-C%d-%s-%s" % (n, c, "unit" if nm else "raw", lb) for n, c, nm, lb in COS_CASES])
def test_cosine_bce_and_backward(N, C_, normalised, labels, cuda):
    """cos_out, the loss, da and dv against float64 F.cosine_similarity + F.binary_cross_entropy and their autograd; cosines
    spread over [0.05, 0.95]; y = NULL (cosine only), a device gout and gout = NULL"""
    a, v, y = lc.cosine_inputs(N, C_, 100 * N + C_, normalised, labels)
    cs64 = lc.cosine_ref(a, v)
    assert (cs64 >= 0.05).all() and (cs64 <= 0.95).all() and (N < 6 or (cs64.min() < 0.07 and cs64.max() > 0.93))
    assert (a >= 0).all() and (v >= 0).all() and (labels == "soft" or N == 1 or set(y) == {0.0, 1.0})
    gouts = (0.7, None)
    cos, loss, grads = _cosine_launches(a, v, y, gouts, cuda)
    a64, v64 = torch.from_numpy(a).double().requires_grad_(True), torch.from_numpy(v).double().requires_grad_(True)
    rcos = F.cosine_similarity(a64, v64)
    rloss = F.binary_cross_entropy(rcos, torch.from_numpy(y).double())
    what = "N%d C%d" % (N, C_)
    _within(cos, _np(rcos), lc.cosine_bound(a, v), "cosine " + what)
    _within(loss, lc.bce_ref(cos, y), lc.bce_bound(cos, y), "bce_mean at the device cosine " + what)
    for g, (da, dv) in zip(gouts, grads):
        a64.grad = v64.grad = None
        (rloss * float(F32(1.0 if g is None else g))).backward(retain_graph=True)
        b_loss, b_da, b_dv = lc.cosine_bce_bounds(a, v, y, g)
        _within(loss, rloss.item(), b_loss, "cosine_bce loss " + what)
        _within(da, _np(a64.grad), b_da, "cosine_bce_bwd da " + what)
        _within(dv, _np(v64.grad), b_dv, "cosine_bce_bwd dv " + what)


def test_cosine_bce_edge_rows(cuda):
    """zero rows, disjoint supports, bitwise-equal rows and rows an ulp apart, under y = 1 and y = 0: the cosine is exactly 0
    for the first two kinds and exactly 1 for equal rows (dot == na == nv, and sqrt(fl(s s)) == s); every output is finite, also
    where the cosine leaves [0, 1]; the loss and both gradients equal ATen's formulas evaluated at the fp32 cosine the forward
    wrote - which also holds the backward's recomputed cosine to cos_out bit for bit, since an ulp of the cosine moves the
    gradient factor of these rows by far more than the bound"""
    a, v, y, kinds = lc.cosine_edge_inputs()
    kinds = np.array(kinds)
    N = len(y)
    (cos, loss, ((da, dv), (da1, dv1))) = _cosine_launches(a, v, y, (0.7, None), cuda)
    print("near-equal rows: device cosines - 1 in [%.3e, %.3e], %d above 1" % (
        (cos[kinds == "near"].astype(np.float64) - 1).min(), (cos[kinds == "near"].astype(np.float64) - 1).max(), int((cos > 1).sum())))
    assert np.isfinite(cos).all() and np.isfinite(loss) and all(np.isfinite(t).all() for t in (da, dv, da1, dv1))
    assert (cos[np.isin(kinds, ("zero_a", "zero_v", "disjoint"))] == 0).all()
    assert (cos[kinds == "equal"] == 1).all(), "bitwise-equal rows: the cosine is exactly 1"
    near = cos[kinds == "near"].astype(np.float64)
    assert (np.abs(near - 1) < 1e-6).all()
    assert (near > 1).any() and (near < 1).any(), "the near-equal rows no longer leave [0, 1] on the device: the edge is not reached"
    _within(loss, lc.bce_ref(cos, y), lc.bce_bound(cos, y), "edge rows loss")
    for g, (ga, gv) in ((0.7, (da, dv)), (None, (da1, dv1))):
        _, ra, rv = lc.cosine_bce_ref(a, v, y, g, cs_dev=cos)
        _, b_da, b_dv = lc.cosine_bce_bounds(a, v, y, g, cs_dev=cos)
        _within(ga, ra, b_da, "edge rows da")
        _within(gv, rv, b_dv, "edge rows dv")
    # what the rows are there for
    t1, t2 = lc.bce_terms(cos, y)
    dis1, eq1 = (kinds == "disjoint") & (y == 1), (kinds == "equal") & (y == 1)
    assert (-(t1 + t2)[dis1] == 100).all() and (-(t1 + t2)[(kinds == "equal") & (y == 0)] == 100).all()
    den = np.sqrt((a[dis1].astype(np.float64) ** 2).sum(1) * (v[dis1].astype(np.float64) ** 2).sum(1))
    fac = -float(F32(0.7)) / N / lc.BCE_FLOOR                                      # -1e12 gout / N
    assert np.allclose(da[dis1], fac / den[:, None] * v[dis1], rtol=1e-5, atol=0)
    assert (da[eq1] == 0).all() and (dv[eq1] == 0).all(), "cosine 1 under y = 1: the gradient factor is exactly 0"
    assert (dv[kinds == "zero_a"] == 0).all() and (da[kinds == "zero_v"] == 0).all()      # ka = kv = 0, k1 meets the zero row
    assert (np.abs(da[(kinds == "zero_a") & (y == 1)]).max(1) > 1e15).all()               # k1 = -1e12 gout / N / 1e-8, finite


# ---------------------------------------------------------------- BCE
@pytest.mark.parametrize("labels", ["hard", "soft"])
@pytest.mark.parametrize("N", lc.BCE_N)
def test_bce_mean_and_backward(N, labels, cuda):
    """binary_cross_entropy with the -100 clamp and its backward with the 1e-12 floor; p holds 0, 1, 2^-149, 1 - 2^-24 and
    values whose 1 - p rounds to 1, and 1 + 2^-23 and -2^-23, outside the domain ATen accepts, where the results must be finite and
    as INTEGRATION.md states them; device gout and gout = NULL"""
    lib, s = _lib_s()
    p, y = lc.bce_inputs(N, N, labels)
    assert N < 63 or all(F32(q) in p for q in lc.BCE_SPECIALS)
    pd, yd = _dev(p, cuda), _dev(y, cuda)
    out = _flat(1, cuda)
    _lib.check(lib.w2l_bce_mean(s, N, _p(pd), _p(yd), _p(out)), "bce_mean")
    dps = []
    for g in (-2.0, None):
        dp = _flat(N, cuda)
        _lib.check(lib.w2l_bce_bwd(s, N, _p(pd), _p(yd), _p(_gout(g, cuda)), _p(dp)), "bce_bwd")
        dps.append((g, dp))
    torch.cuda.synchronize()
    o = _np(out)
    assert (o[1:] == SENT).all() and np.isfinite(o[0])
    # ATen's own terms where it accepts p; outside [0, 1] (BCE_OUTSIDE) it raises, and the reference is the pinned behaviour:
    # the logarithm of a non-positive number counts as the clamp value -100, the gradient takes the 1e-12 floor
    inside = (p >= 0) & (p <= 1)
    assert N < 63 or (int((~inside).sum()) == 2 and (p > 1).any() and (p < 0).any())
    t1, t2 = lc.bce_terms(p, y)
    aten = F.binary_cross_entropy(torch.from_numpy(p[inside]).double(), torch.from_numpy(y[inside]).double(), reduction="none")
    assert np.allclose(-(t1 + t2)[inside], _np(aten), rtol=1e-13, atol=0)
    if (~inside).any():
        hi, lo = p > 1, p < 0
        assert (t2[hi] == (1 - y[hi].astype(np.float64)) * -100).all() and (t1[lo] == y[lo].astype(np.float64) * -100).all()
    _within(o[0], lc.bce_ref(p, y), lc.bce_bound(p, y), "bce_mean N%d" % N)
    for g, dp in dps:
        d = _np(dp)
        assert (d[N:] == SENT).all() and np.isfinite(d[:N]).all()
        ref = lc.bce_bwd_ref(p, y, g)
        gn = float(F32(1.0 if g is None else g)) / N
        assert np.array_equal(ref[~inside], gn * (p[~inside].astype(np.float64) - y[~inside]) / lc.BCE_FLOOR)   # (p - y) / 1e-12
        _within(d[:N], ref, lc.bce_bwd_bound(p, y, g), "bce_bwd N%d" % N)


# ---------------------------------------------------------------- Adam
class _Arena:
    """p, g, m, v of a list of tensors as slices of four device arenas, one sentinel cell behind every tensor"""

    def __init__(self, state, cuda):
        self.state, self.sizes = state, [len(t[0]) for t in state]
        self.offs = np.concatenate([[0], np.cumsum([n + 1 for n in self.sizes])]).astype(int)
        self.host = []
        for j in range(4):
            h = np.full(self.offs[-1] + GUARD, SENT, F32)
            for i, t in enumerate(state):
                h[self.offs[i]:self.offs[i] + self.sizes[i]] = t[j]
            self.host.append(h)
        self.dev = [_dev(h, cuda) for h in self.host]
        self.table = (_lib.AdamTensor * len(state))()
        for i, n in enumerate(self.sizes):
            e = self.table[i]
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = (t.data_ptr() + 4 * int(self.offs[i]) for t in self.dev)
            e.n = n
        self.handle = C.c_void_p()
        _lib.check(_lib.load().w2l_adam_create(len(state), (C.c_longlong * len(state))(*self.sizes), C.byref(self.handle)), "adam_create")

    def restore(self):
        for d, h in zip(self.dev, self.host):
            d.copy_(torch.from_numpy(h))

    def step(self, sc_args, step):
        lr, betas, eps, wd = sc_args
        return _lib.load().w2l_adam_step(self.handle, _lib.current_stream(), self.table, lr, betas[0], betas[1], eps, wd, step)

    def read(self):
        """-> per tensor (p, m, v) after a step; asserts sentinels and the gradient arena untouched"""
        torch.cuda.synchronize()
        hp, hg, hm, hv = (_np(t) for t in self.dev)
        assert np.array_equal(hg, self.host[1]), "adam_step wrote the gradients"
        fence = np.ones(len(hp), bool)
        for i, n in enumerate(self.sizes):
            fence[self.offs[i]:self.offs[i] + n] = False
        for h, name in ((hp, "param"), (hm, "exp_avg"), (hv, "exp_avg_sq")):
            assert (h[fence] == SENT).all(), "adam_step wrote %s between or behind the tensors" % name
        return [(hp[o:o + n], hm[o:o + n], hv[o:o + n]) for o, n in zip(self.offs, self.sizes)]

    def close(self):
        _lib.load().w2l_adam_destroy(self.handle)


def _check_adam_step(arena, lr, betas, wd, step):
    sc = lc.adam_scalars(lr, betas, 1e-8, wd, step)
    arena.restore()
    _lib.check(arena.step((lr, betas, 1e-8, wd), step), "adam_step")
    what = "lr%g b%g wd%g step%d" % (lr, betas[0], wd, step)
    for (p, g, m, v), (p1, m1, v1) in zip(arena.state, arena.read()):
        if not len(p):
            continue
        rp, rm, rv = lc.adam_ref(p, g, m, v, sc, m_dev=m1, v_dev=v1)
        bp, bm, bv = lc.adam_bounds(p, g, m, v, sc, True)
        _within(m1, rm, bm, "adam exp_avg " + what)
        _within(v1, rv, bv, "adam exp_avg_sq " + what)
        _within(p1, rp, bp, "adam param " + what)
        if wd == 0:
            still = (g == 0) & (m == 0) & (v == 0)
            assert np.array_equal(p1[still], p[still]) and (m1[still] == 0).all() and (v1[still] == 0).all()
            tiny = (g == F32(1e-25)) & (v == 0)
            assert (v1[tiny] == 0).all()                                  # g^2 underflows, nothing else feeds v


@pytest.mark.parametrize("wd", lc.ADAM_WD)
@pytest.mark.parametrize("hyper", range(len(lc.ADAM_HYPER)), ids=["ref", "beta1_0"])
def test_adam_single_steps(hyper, wd, cuda):
    """one step at a time from identical fp32 state, sizes around the 16 384-element chunk (0, 1, 255, 256, 16383, 16384, 16385,
    49153: 11 chunks, a zero-length tensor in the table), steps 1, 2 and 100 000, with and without weight decay"""
    lr, betas = lc.ADAM_HYPER[hyper]
    assert lc.adam_chunks(lc.ADAM_SIZES) == 11 and [lc.adam_chunks([n]) for n in (16384, 16385, 49153)] == [1, 2, 4]
    state = lc.adam_inputs(lc.ADAM_SIZES, 11)
    assert all(((g == 0) & (m == 0)).any() and (g == F32(1e-25)).any() for p, g, m, v in state if len(p) > 200)
    arena = _Arena(state, cuda)
    try:
        for step in lc.ADAM_STEPS:
            _check_adam_step(arena, lr, betas, wd, step)
    finally:
        arena.close()


def test_adam_table_of_300_small_tensors(cuda):
    """300 tensors of 1 - 40 elements: one chunk each, every chunk must find its own tensor"""
    sizes = [int(n) for n in np.random.default_rng(4).integers(1, 41, 300)]
    assert lc.adam_chunks(sizes) == 300 and min(sizes) == 1 and max(sizes) == 40
    arena = _Arena(lc.adam_inputs(sizes, 12), cuda)
    try:
        lr, betas = lc.ADAM_HYPER[0]
        _check_adam_step(arena, lr, betas, 0.01, 2)
    finally:
        arena.close()


def test_adam_table_of_empty_tensors_writes_nothing(cuda):
    arena = _Arena(lc.adam_inputs([0, 0, 0], 13), cuda)
    try:
        assert lc.adam_chunks(arena.sizes) == 0
        lr, betas = lc.ADAM_HYPER[0]
        assert arena.step((lr, betas, 1e-8, 0.01), 1) == 0
        arena.read()                                                      # every cell of the four arenas is a sentinel cell here
    finally:
        arena.close()


def test_adam_trajectory_against_float64_torch(cuda):
    """five steps of wav2lip_amd.optim.Adam, two parameter groups of different lr and weight decay, against float64
    torch.optim.Adam(foreach=False) on the CPU fed the same (fp32-representable) hyper-parameters.  Bound: the single-step bounds
    from the state, at the float64 trajectory's magnitudes, summed over the five steps (five times their mean).  That is a
    yardstick, not a worst case: a moment's error of an earlier step also enters the later parameter steps, which a worst case
    would count up to three times over; leaving it out makes the bound tighter, never wider"""
    from wav2lip_amd import optim
    f = lambda x: float(F32(x))                                            # noqa: E731
    betas = (0.5, f(0.999))
    groups = [dict(sizes=(16385, 300, 35), lr=f(1e-4), weight_decay=0.0), dict(sizes=(255, 20000), lr=f(1e-3), weight_decay=f(0.01))]
    rng = np.random.default_rng(21)
    ours, refs = [], []
    for g in groups:
        init = [rng.standard_normal(n).astype(F32) for n in g["sizes"]]
        ours.append([torch.nn.Parameter(_dev(x, cuda)) for x in init])
        refs.append([torch.nn.Parameter(torch.from_numpy(x).double()) for x in init])
    mk = lambda ps: [dict(params=p, lr=g["lr"], weight_decay=g["weight_decay"]) for p, g in zip(ps, groups)]   # noqa: E731
    opt = optim.Adam(mk(ours), betas=betas)
    ref = torch.optim.Adam(mk(refs), betas=betas, foreach=False)
    flat_o, flat_r = [p for ps in ours for p in ps], [p for ps in refs for p in ps]
    hyper = [(g["lr"], g["weight_decay"]) for g in groups for _ in g["sizes"]]
    bp, bm, bv = ([np.zeros(p.numel()) for p in flat_r] for _ in range(3))
    for step in range(1, 6):
        for i, (po, pr) in enumerate(zip(flat_o, flat_r)):
            g = rng.standard_normal(pr.numel()).astype(F32)
            g[rng.random(pr.numel()) < 0.1] = 0
            po.grad, pr.grad = _dev(g, cuda), torch.from_numpy(g).double()
            st = ref.state[pr]
            m0 = _np(st["exp_avg"]) if st else np.zeros(pr.numel())
            v0 = _np(st["exp_avg_sq"]) if st else np.zeros(pr.numel())
            lr, wd = hyper[i]
            sc = (lr, betas[0], betas[1], f(1e-8), wd, 1 - betas[0] ** step, np.sqrt(1 - betas[1] ** step))
            b = lc.adam_bounds(_np(pr), g, m0, v0, sc, False)
            for acc, x in zip((bp, bm, bv), b):
                acc[i] += x
        opt.step()
        ref.step()
    torch.cuda.synchronize()
    for i, (po, pr) in enumerate(zip(flat_o, flat_r)):
        _within(_np(po), _np(pr), bp[i], "adam trajectory param %d" % i)
        _within(_np(opt.state[po]["exp_avg"]), _np(ref.state[pr]["exp_avg"]), bm[i], "adam trajectory exp_avg %d" % i)
        _within(_np(opt.state[po]["exp_avg_sq"]), _np(ref.state[pr]["exp_avg_sq"]), bv[i], "adam trajectory exp_avg_sq %d" % i)
        assert int(opt.state[po]["step"]) == 5


# ---------------------------------------------------------------- argument errors
def _marker():
    """put a known message into w2l_last_error, so that the next failure is seen to write its own"""
    lib = _lib.load()
    assert lib.w2l_bn_fold(_lib.current_stream(), 0, None, None, None, None, None, 1e-5, None, None) != 0
    return lib.w2l_last_error()


def test_argument_errors_write_nothing(cuda):
    """each entry refuses with the argument-error code and a message of its own, before writing anything: N or n = 0, C = 0, a
    NULL required pointer, a channel stride below C, y without loss_out, step 0, a negative tensor size"""
    lib, s = _lib_s()
    N, C_ = 6, 40
    src = [torch.rand(N * C_ + GUARD, device=cuda) for _ in range(3)]
    outs = [torch.full((N * C_ + GUARD,), SENT, device=cuda) for _ in range(3)]
    x, y2, y3 = (_p(t) for t in src)
    o0, o1, o2 = (_p(t) for t in outs)
    table = (_lib.AdamTensor * 1)()
    table[0].param, table[0].grad, table[0].exp_avg, table[0].exp_avg_sq = (t.data_ptr() for t in (outs[0], src[0], outs[1], outs[2]))
    table[0].n = N * C_
    h = C.c_void_p()
    _lib.check(lib.w2l_adam_create(1, (C.c_longlong * 1)(N * C_), C.byref(h)), "adam_create")
    h2 = C.c_void_p()
    calls = {
        "l1_mean n=0": lambda: lib.w2l_l1_mean(s, 0, x, y2, o0),
        "l1_mean a": lambda: lib.w2l_l1_mean(s, N, None, y2, o0),
        "l1_mean b": lambda: lib.w2l_l1_mean(s, N, x, None, o0),
        "l1_mean out": lambda: lib.w2l_l1_mean(s, N, x, y2, None),
        "l1_bwd n=0": lambda: lib.w2l_l1_bwd(s, 0, x, y2, None, o0),
        "l1_bwd a": lambda: lib.w2l_l1_bwd(s, N, None, y2, None, o0),
        "l1_bwd b": lambda: lib.w2l_l1_bwd(s, N, x, None, None, o0),
        "l1_bwd da": lambda: lib.w2l_l1_bwd(s, N, x, y2, None, None),
        "l2norm N=0": lambda: lib.w2l_l2norm_rows(s, 0, C_, x, C_, o0),
        "l2norm C=0": lambda: lib.w2l_l2norm_rows(s, N, 0, x, C_, o0),
        "l2norm x": lambda: lib.w2l_l2norm_rows(s, N, C_, None, C_, o0),
        "l2norm y": lambda: lib.w2l_l2norm_rows(s, N, C_, x, C_, None),
        "l2norm x_cs": lambda: lib.w2l_l2norm_rows(s, N, C_, x, C_ - 1, o0),
        "l2norm_bwd N=0": lambda: lib.w2l_l2norm_bwd(s, 0, C_, x, C_, y2, o0, C_),
        "l2norm_bwd C=0": lambda: lib.w2l_l2norm_bwd(s, N, 0, x, C_, y2, o0, C_),
        "l2norm_bwd x": lambda: lib.w2l_l2norm_bwd(s, N, C_, None, C_, y2, o0, C_),
        "l2norm_bwd dy": lambda: lib.w2l_l2norm_bwd(s, N, C_, x, C_, None, o0, C_),
        "l2norm_bwd dx": lambda: lib.w2l_l2norm_bwd(s, N, C_, x, C_, y2, None, C_),
        "l2norm_bwd x_cs": lambda: lib.w2l_l2norm_bwd(s, N, C_, x, C_ - 1, y2, o0, C_),
        "l2norm_bwd dx_cs": lambda: lib.w2l_l2norm_bwd(s, N, C_, x, C_, y2, o0, C_ - 1),
        "cosine_bce N=0": lambda: lib.w2l_cosine_bce(s, 0, C_, x, y2, y3, o0, o1),
        "cosine_bce C=0": lambda: lib.w2l_cosine_bce(s, N, 0, x, y2, y3, o0, o1),
        "cosine_bce a": lambda: lib.w2l_cosine_bce(s, N, C_, None, y2, y3, o0, o1),
        "cosine_bce v": lambda: lib.w2l_cosine_bce(s, N, C_, x, None, y3, o0, o1),
        "cosine_bce cos_out": lambda: lib.w2l_cosine_bce(s, N, C_, x, y2, y3, None, o1),
        "cosine_bce y without loss_out": lambda: lib.w2l_cosine_bce(s, N, C_, x, y2, y3, o0, None),
        "cosine_bce_bwd N=0": lambda: lib.w2l_cosine_bce_bwd(s, 0, C_, x, y2, y3, None, o0, o1),
        "cosine_bce_bwd C=0": lambda: lib.w2l_cosine_bce_bwd(s, N, 0, x, y2, y3, None, o0, o1),
        "cosine_bce_bwd a": lambda: lib.w2l_cosine_bce_bwd(s, N, C_, None, y2, y3, None, o0, o1),
        "cosine_bce_bwd v": lambda: lib.w2l_cosine_bce_bwd(s, N, C_, x, None, y3, None, o0, o1),
        "cosine_bce_bwd y": lambda: lib.w2l_cosine_bce_bwd(s, N, C_, x, y2, None, None, o0, o1),
        "cosine_bce_bwd da": lambda: lib.w2l_cosine_bce_bwd(s, N, C_, x, y2, y3, None, None, o1),
        "cosine_bce_bwd dv": lambda: lib.w2l_cosine_bce_bwd(s, N, C_, x, y2, y3, None, o0, None),
        "bce_mean N=0": lambda: lib.w2l_bce_mean(s, 0, x, y2, o0),
        "bce_mean p": lambda: lib.w2l_bce_mean(s, N, None, y2, o0),
        "bce_mean y": lambda: lib.w2l_bce_mean(s, N, x, None, o0),
        "bce_mean out": lambda: lib.w2l_bce_mean(s, N, x, y2, None),
        "bce_bwd N=0": lambda: lib.w2l_bce_bwd(s, 0, x, y2, None, o0),
        "bce_bwd p": lambda: lib.w2l_bce_bwd(s, N, None, y2, None, o0),
        "bce_bwd y": lambda: lib.w2l_bce_bwd(s, N, x, None, None, o0),
        "bce_bwd dp": lambda: lib.w2l_bce_bwd(s, N, x, y2, None, None),
        "adam_step handle": lambda: lib.w2l_adam_step(None, s, table, 1e-3, 0.5, 0.999, 1e-8, 0.0, 1),
        "adam_step table": lambda: lib.w2l_adam_step(h, s, None, 1e-3, 0.5, 0.999, 1e-8, 0.0, 1),
        "adam_step step=0": lambda: lib.w2l_adam_step(h, s, table, 1e-3, 0.5, 0.999, 1e-8, 0.0, 0),
        "adam_create negative size": lambda: lib.w2l_adam_create(2, (C.c_longlong * 2)(5, -1), C.byref(h2)),
    }
    try:
        for name, call in calls.items():
            mark = _marker()
            rc = call()
            msg = lib.w2l_last_error()
            assert rc == ERR_ARG, "%s: returned %d" % (name, rc)
            assert msg and msg != mark, "%s: no message" % name
        assert h2.value is None, "a refused adam_create returned a handle"
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t == SENT).all()), "a refused call wrote an output"
    finally:
        lib.w2l_adam_destroy(h)
