"""The error bounds of tests/test_train_losses_gpu.py, checked without a GPU: numpy fp32 restatements of the kernels' arithmetic -
the same accumulation order (lane-strided sums, the xor fold, the 256-thread strided sum, the four partial accumulators of
mean_final_kernel) and the same operation order, every operation rounded to fp32 once (no fused multiply-add, numpy's logf) - must
stay inside each bound of tests/_loss_cases.py on the GPU file's own inputs with 4x headroom, the usual spread between a
worst-case bound and one realisation.  A restatement that comes closer says the derivation is wrong, not the kernel.

That spread belongs to bounds that add up many roundings: every bound here that rests on a reduction (the L2 normalisation, the
cosine, the cosine + BCE pair, bce_mean) is held to the 4x.  The elementwise bounds count a handful of roundings per element and
are then taken over thousands of elements, whose worst one comes close to the count itself: the cast that ends w2l_l1_mean alone
reaches half of 2^-23 |ref|, the three to five operations of an Adam moment or of bce_bwd reach 0.3 - 0.6 of 2^-22 and of R on
these inputs.  Those bounds are set by the format, not derived from a sum, so for them (SHORT below) the restatement has to stay
inside the bound, no more; l1_bwd is exact.

Bitwise-equal rows: dot == na == nv bit for bit (the same products in the same order), and in radix 2 with correctly rounded
multiplication and root sqrt(fl(s s)) == s, so the cosine of two bitwise-equal rows is dot / sqrtf(na nv) == 1 exactly under this
accumulation order - it never exceeds 1 (test_cosine_of_equal_rows_is_exactly_one).  Rows that differ by an ulp in some elements
do reach 1 + 2^-23 (test_cosine_edge_rows_stay_finite asserts that the edge inputs hold such a row), which is where the BCE
leaves the domain ATen accepts."""
import numpy as np
import pytest

import _loss_cases as lc
from _loss_cases import F32, U

HEADROOM = 4.0
SHORT = 1.0       # elementwise bounds of a few roundings: see the module docstring
LANES = np.arange(64)


# ---------------------------------------------------------------- the kernels' arithmetic in numpy fp32
def wave_sum(t):
    """one wave per row: lane l adds terms l, l + 64, ...; six xor steps fold the 64 partials"""
    N, C = t.shape
    n = -(-C // 64)
    pad = np.zeros((N, n * 64), F32)
    pad[:, :C] = t
    s = np.zeros((N, 64), F32)
    for j in range(n):
        s = s + pad[:, j * 64:(j + 1) * 64]
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, LANES ^ o]
    return s[:, 0]


def l1_mean_32(a, b):
    """l1_partial_kernel + mean_final_kernel: |a - b| in fp32, everything after it in fp64 in the kernels' order"""
    n = a.shape[0]
    nb = lc.l1_partials(n)
    d = np.abs(a - b).astype(np.float64)
    k = -(-n // (nb * 256))
    pad = np.zeros(k * nb * 256)
    pad[:n] = d
    s = np.zeros((nb, 256))
    for j in range(k):                                   # thread t of block b: elements (j nb + b) 256 + t
        s = s + pad[j * nb * 256:(j + 1) * nb * 256].reshape(nb, 256)
    s = s.reshape(nb, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, LANES ^ o]
    partial = ((s[:, 0, 0] + s[:, 1, 0]) + s[:, 2, 0]) + s[:, 3, 0]
    lane = np.zeros(64)
    for l in range(64):
        t, i = [0.0, 0.0, 0.0, 0.0], l
        while i + 192 < nb:
            for q in range(4):
                t[q] += partial[i + 64 * q]
            i += 256
        while i < nb:
            t[0] += partial[i]
            i += 64
        lane[l] = (t[0] + t[1]) + (t[2] + t[3])
    for o in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[LANES ^ o]
    return F32(lane[0] * (1.0 / n))


def l2norm_32(x):
    d = np.maximum(np.sqrt(wave_sum(x * x)), F32(1e-12))[:, None]
    return x / d


def l2norm_bwd_32(x, dy):
    ss, xd = wave_sum(x * x), wave_sum(x * dy)
    nrm = np.sqrt(ss)
    d = np.maximum(nrm, F32(1e-12))
    with np.errstate(over="ignore"):
        k = np.where(nrm > F32(1e-12), xd / (d * d * d), F32(0))
    return dy / d[:, None] - x * k[:, None]


def cosine_32(a, v):
    dot, na, nv = wave_sum(a * v), wave_sum(a * a), wave_sum(v * v)
    return dot / np.sqrt(np.maximum(na * nv, F32(1e-16))), dot, na, nv


def bce_mean_32(p, y):
    N = p.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.fmax(np.log(p), F32(-100))              # fmax: the operand that is a number, as fmaxf
        lq = np.fmax(np.log(F32(1) - p), F32(-100))
    t = y * lp + (F32(1) - y) * lq
    n = -(-N // 256)
    pad = np.zeros(n * 256, F32)
    pad[:N] = t
    s = np.zeros(256, F32)
    for j in range(n):
        s = s - pad[j * 256:(j + 1) * 256]
    s = s.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, LANES ^ o]
    return (((s[0, 0] + s[1, 0]) + s[2, 0]) + s[3, 0]) / F32(N)


def bce_bwd_32(p, y, gout):
    gsc = F32(1.0 if gout is None else gout) / F32(p.shape[0])
    return gsc * (p - y) / np.maximum((F32(1) - p) * p, F32(1e-12))


def cosine_bce_bwd_32(a, v, y, gout):
    N = a.shape[0]
    _, dot, na, nv = cosine_32(a, v)
    prod = na * nv
    clamped = prod < F32(1e-16)
    den = np.sqrt(np.maximum(prod, F32(1e-16)))
    cs = dot / den
    dcos = F32(1.0 if gout is None else gout) / F32(N) * (cs - y) / np.maximum((F32(1) - cs) * cs, F32(1e-12))
    k1 = dcos / den
    ka = np.where(clamped, F32(0), dcos * dot * nv / (den * den * den))
    kv = np.where(clamped, F32(0), dcos * dot * na / (den * den * den))
    return k1[:, None] * v - ka[:, None] * a, k1[:, None] * a - kv[:, None] * v, cs


def adam_32(p, g, m, v, sc):
    lr, b1, b2, eps, wd, bc1, bc2s = (F32(x) for x in sc)
    if wd != 0:
        g = g + wd * p
    m1 = m + (g - m) * (F32(1) - b1)
    with np.errstate(under="ignore"):
        v1 = b2 * v + (F32(1) - b2) * g * g
    denom = np.sqrt(v1) / bc2s + eps
    return p - (lr / bc1) * (m1 / denom), m1, v1


def _inside(got, ref, bound, what, headroom=HEADROOM):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(err * headroom <= bound)
    assert not bad.any(), "%s: restatement uses more than 1/%g of the bound (worst ratio %.3f)" % (
        what, headroom, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)))))


# ---------------------------------------------------------------- tests
def test_launch_rules_reach_every_regime():
    for n, (nb, trips0, lanes, tail) in lc.L1_CASES.items():
        assert lc.l1_partials(n) == nb and lc.mean_final_walk(nb) == (trips0, lanes, tail), n
    assert lc.l1_partials(1024 * 4096 + 4095) == 1024 < -(-(1024 * 4096 + 4095) // 4096)        # capped
    assert lc.grid_cap(1024 * 4096 + 4095, 256, 16384) == 16384                                  # l1_bwd's cap too
    assert [lc.adam_chunks([n]) for n in lc.ADAM_SIZES] == [0, 1, 1, 1, 1, 1, 2, 4]


@pytest.mark.parametrize("n", list(lc.L1_CASES))
def test_l1_mean_bound(n):
    a, b = lc.l1_inputs(n, n % 1000)
    frac = float((a == b).mean())
    assert n < 100 or 0.05 < frac < 0.15
    ref = lc.l1_ref(a, b)
    _inside(l1_mean_32(a, b), ref, lc.l1_bound(ref), "l1_mean", headroom=SHORT)
    d = a.astype(np.float64) - b
    for gout in (None, 0.7, -2.0):
        r = lc.l1_bwd_ref(a, b, gout, n)
        gsc = F32(1.0 if gout is None else gout) * F32(1.0 / n)
        assert set(np.unique(r)) <= {gsc, -gsc, F32(0)} and np.array_equal(r == 0, d == 0)


@pytest.mark.parametrize("C", lc.L2_C)
@pytest.mark.parametrize("N", lc.L2_N)
def test_l2norm_bounds(N, C):
    for rot in range(4):
        x, dy, kinds = lc.l2_inputs(N, C, rot, 1000 * N + C)
        ref, _, nrm = lc.l2_ref(x)
        for r, k in enumerate(kinds):                         # each row sits in the branch it names
            assert {"scaled": nrm[r] > 1e-3, "zero": nrm[r] == 0, "below": 0 < nrm[r] < lc.EPS_L2, "above": nrm[r] > lc.EPS_L2}[k]
            if k in ("below", "above"):
                assert abs(nrm[r] / lc.EPS_L2 - 1) < 2e-3
        _inside(l2norm_32(x), ref, lc.l2_bound(x), "l2norm N%d C%d" % (N, C))
        _inside(l2norm_bwd_32(x, dy), lc.l2_bwd_ref(x, dy), lc.l2_bwd_bound(x, dy), "l2norm_bwd N%d C%d" % (N, C))
        z = [r for r, k in enumerate(kinds) if k == "zero"]
        assert np.array_equal(l2norm_bwd_32(x, dy)[z], dy[z] / F32(1e-12))


@pytest.mark.parametrize("labels", ["hard", "soft"])
@pytest.mark.parametrize("normalised", [True, False])
@pytest.mark.parametrize("C", lc.COS_C)
@pytest.mark.parametrize("N", lc.COS_N)
def test_cosine_bce_bounds(N, C, normalised, labels):
    a, v, y = lc.cosine_inputs(N, C, 100 * N + C, normalised, labels)
    cs64 = lc.cosine_ref(a, v)
    assert (cs64 >= 0.05).all() and (cs64 <= 0.95).all()
    assert N < 6 or (cs64.min() < 0.07 and cs64.max() > 0.93)
    cs, _, _, _ = cosine_32(a, v)
    _inside(cs, cs64, lc.cosine_bound(a, v), "cosine")
    for gout in (None, 0.7):
        loss, da, dv = lc.cosine_bce_ref(a, v, y, gout)
        b_loss, b_da, b_dv = lc.cosine_bce_bounds(a, v, y, gout)
        _inside(bce_mean_32(cs, y), loss, b_loss, "loss through the cosine")
        ga, gv, _ = cosine_bce_bwd_32(a, v, y, gout)
        _inside(ga, da, b_da, "da")
        _inside(gv, dv, b_dv, "dv")
    _inside(bce_mean_32(cs, y), lc.bce_ref(cs, y), lc.bce_bound(cs, y), "loss at the fp32 cosine")


def test_cosine_of_equal_rows_is_exactly_one():
    rng = np.random.default_rng(3)
    for C in (7, 64, 512, 1000):
        for scale in (1e-3, 1.0, 37.0):
            e = (rng.random((4096, C)) * scale).astype(F32)
            cs, dot, na, nv = cosine_32(e, e.copy())
            assert np.array_equal(dot, na) and np.array_equal(na, nv)
            assert np.array_equal(np.sqrt(na * nv), na) and (cs == 1).all()


def test_cosine_edge_rows_stay_finite():
    a, v, y, kinds = lc.cosine_edge_inputs()
    kinds = np.array(kinds)
    cs, _, _, _ = cosine_32(a, v)
    assert (cs[np.isin(kinds, ("zero_a", "zero_v", "disjoint"))] == 0).all() and (cs[kinds == "equal"] == 1).all()
    near = cs[kinds == "near"]
    assert (near > 1).any() and (near < 1).any() and (np.abs(near - 1) < 1e-6).all()   # the edge inputs leave [0, 1]
    loss = bce_mean_32(cs, y)
    ga, gv, cs_b = cosine_bce_bwd_32(a, v, y, 0.7)
    assert np.isfinite(loss) and np.isfinite(ga).all() and np.isfinite(gv).all()
    ref_loss, da, dv = lc.cosine_bce_ref(a, v, y, 0.7, cs_dev=cs)
    b_loss, b_da, b_dv = lc.cosine_bce_bounds(a, v, y, 0.7, cs_dev=cs)
    _inside(loss, ref_loss, b_loss, "edge loss")
    _inside(ga, da, b_da, "edge da")
    _inside(gv, dv, b_dv, "edge dv")
    N = len(y)
    t1, t2 = lc.bce_terms(cs, y)
    dis1 = (kinds == "disjoint") & (y == 1)
    assert (-(t1 + t2)[dis1] == 100).all()
    k1 = -1e12 * 0.7 / N                                              # the gradient factor at cosine 0 under y = 1
    den = np.sqrt((a[dis1].astype(np.float64) ** 2).sum(1) * (v[dis1].astype(np.float64) ** 2).sum(1))
    assert np.allclose(ga[dis1], float(F32(0.7)) / 0.7 * k1 / den[:, None] * v[dis1], rtol=1e-5)
    for zk, g0 in (("zero_a", gv), ("zero_v", ga)):                  # ka = kv = 0, and the other side's k1 meets a zero row
        assert (g0[kinds == zk] == 0).all()


@pytest.mark.parametrize("labels", ["hard", "soft"])
@pytest.mark.parametrize("N", lc.BCE_N)
def test_bce_bounds(N, labels):
    p, y = lc.bce_inputs(N, N, labels)
    assert N < 63 or all(F32(s) in p for s in lc.BCE_SPECIALS)
    _inside(bce_mean_32(p, y), lc.bce_ref(p, y), lc.bce_bound(p, y), "bce_mean")
    for gout in (None, -2.0):
        ref = lc.bce_bwd_ref(p, y, gout)
        assert np.isfinite(ref).all()
        _inside(bce_bwd_32(p, y, gout), ref, lc.bce_bwd_bound(p, y, gout), "bce_bwd", headroom=SHORT)


@pytest.mark.parametrize("wd", lc.ADAM_WD)
@pytest.mark.parametrize("hyper", range(len(lc.ADAM_HYPER)))
def test_adam_bounds(hyper, wd):
    lr, betas = lc.ADAM_HYPER[hyper]
    state = lc.adam_inputs((255, 16385), 11)
    for step in lc.ADAM_STEPS:
        sc = lc.adam_scalars(lr, betas, 1e-8, wd, step)
        for p, g, m, v in state:
            p1, m1, v1 = adam_32(p, g, m, v, sc)
            rp, rm, rv = lc.adam_ref(p, g, m, v, sc, m_dev=m1, v_dev=v1)
            bp, bm, bv = lc.adam_bounds(p, g, m, v, sc, True)
            _inside(m1, rm, bm, "exp_avg", headroom=SHORT)
            _inside(v1, rv, bv, "exp_avg_sq", headroom=SHORT)
            _inside(p1, rp, bp, "param", headroom=SHORT)
            rp2, _, _ = lc.adam_ref(p, g, m, v, sc)
            bp2, _, _ = lc.adam_bounds(p, g, m, v, sc, False)
            _inside(p1, rp2, bp2, "param from the state", headroom=SHORT)
            still = (g == 0) & (m == 0) & (v == 0)
            assert still.any() and (wd != 0 or np.array_equal(p1[still], p[still]))
            tiny = g == F32(1e-25)
            assert tiny.any() and (wd != 0 or (((F32(1) - F32(sc[2])) * g[tiny]) * g[tiny] == 0).all())
