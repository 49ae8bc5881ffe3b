"""The host side of tests/test_conv_exact_gpu.py, without a GPU: the float64 reference against a plain-loop convolution, every
case's exactness bound, and the selection table (every regime has a case; both conv_wino4 forms, every implicit-GEMM tile with a
ragged M and a ragged cout, split-K with a short last split, an image group running past the batch); and of
tests/test_conv_backward_exact_gpu.py: the float64 reference of every backward case against torch's float64 AUTOGRAD input gradient of
the forward layer, the restated output-padding rule against autograd.dgrad_geom, and ref(w0) != ref(w1) for every update case."""
import numpy as np
import pytest
import torch

import _conv_cases as cc


@pytest.mark.parametrize("tr,cin,cout,k,s,p,op,N,H,W,res", [
    (0, 3, 5, 3, (2, 1), 1, 0, 2, 6, 5, True),           # strided conv with a residual
    (1, 4, 3, 3, 2, 1, 1, 2, 3, 4, False),               # transposed, stride 2, output padding 1
    (0, 2, 4, (5, 5), (1, 2), 2, 0, 1, 7, 6, False),     # 5x5 s(1,2)
])
def test_float64_reference_equals_plain_loops(tr, cin, cout, k, s, p, op, N, H, W, res):
    case = cc.Case("f32", "igemm", tr, cin, cout, k, s, p, op, N, H, W, res=int(res), seed=N + H)
    for make in (cc.int_operands, cc.gauss_operands):
        x, w, scale, shift, r = make(case)
        want = cc.conv_loops(x.numpy(), w.numpy(), tr, case.s, case.p, case.op, scale.numpy(), shift.numpy(),
                             None if r is None else r.numpy(), True)
        got = cc.ref64(case, x, w, scale, shift, r).numpy()
        assert got.shape == want.shape == (N, cout) + case.out_hw()
        if make is cc.int_operands:
            assert np.array_equal(got, want)
        else:
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
        assert np.abs(want).max() > 0


def test_integer_operands_are_what_the_bounds_assume():
    for pool in ("f32 igemm", "wino id 11", "wino id 8"):
        case = cc.exact_cases(pool)[0]
        x, w, scale, shift, _ = cc.int_operands(case)
        assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0} and 0.2 < float((x == 0).double().mean()) < 0.5 or x.numel() < 30
        assert set(scale.abs().unique().tolist()) <= set(abs(s) for s in case.scales()) and float(shift.abs().max()) <= 3
        if case.wmode == "w4":          # one tap of (0..1, 0..1) per pair, a multiple of 576
            assert set(w.unique().tolist()) <= {-576.0, 0.0, 576.0}
            assert int((w != 0).sum(dim=(2, 3)).max()) <= 1 and float(w[:, :, 2, :].abs().max()) == 0 and float(w[:, :, :, 2].abs().max()) == 0
        else:
            assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}


def test_winograd_growth_constants():
    """the row sums the bounds are derived from, recomputed from the transform matrices"""
    G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
    Bt2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]])
    At2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]])
    u, v, a = np.abs(G2).sum(1).max() ** 2, np.abs(Bt2).sum(1).max() ** 2, np.abs(At2).sum(1).max() ** 2
    assert (u, v, a) == (2.25, 4, 9) and cc.WINO2_GROWTH == 4 * a * u * v
    G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])
    Bt4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]])
    At4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]])
    assert np.abs(Bt4).sum(1).max() == 10 and np.abs(At4).sum(1).max() == 19
    umax = 576 * np.abs(G4[:, :2]).max() ** 2                       # taps (0..1, 0..1): columns 0 and 1 of G
    assert umax == 36 and cc.WINO4_GROWTH == 19 * 19 * umax * 100
    for i in range(2):                                               # 576 * G[:, i] G[:, j]^T is integral
        for j in range(2):
            U = 576 * np.outer(G4[:, i], G4[:, j])
            assert np.abs(U - np.round(U)).max() < 1e-9
    assert 361 * 576 * 100 > cc.LIMIT                                # dense taps: the bound fails at cin = 1


@pytest.mark.parametrize("pool", cc.POOLS + ["large"])
def test_every_case_meets_its_exactness_bound(pool):
    cases = cc.exact_cases(pool)
    assert cases, pool
    for c in cases:
        assert c.exact_bound() < cc.LIMIT, (c, c.exact_bound())


def test_every_regime_has_a_case():
    empty = [name for name, _pool, c in cc.select() if c is None]
    assert not empty, empty


def test_selection_reaches_what_the_issue_names():
    sel = {name: c for name, _pool, c in cc.select()}
    forms = {c.wino4_plan()["form"] for n, c in sel.items() if n.startswith("wino4:")}
    assert forms == {0, 1}
    for p in ("f32 igemm", "f32 split", "bf16 igemm"):
        for t in range(6):
            c = sel["%s tile %d: ragged M and ragged cout" % (p, t)]
            bm, bn = c.tile()
            assert c.gemm_rows() % bm and c.gemm_rows() > bm and c.cout % bn and c.cout > bn
            c = sel["%s tile %d: split-K with a short last split" % (p, t)]
            n, per = c.splits()
            assert n >= 2 and n * per > c.ksteps()
    c = sel["wino4: rectangles, several images per block, last group past the batch"]
    assert c.wino4_plan()["ni"] > 1 and c.N % c.wino4_plan()["ni"]
    for fam in ("wino id 8", "wino id 9", "wino id 12", "wino id 19", "tp2", "tp2s", "k3s"):      # every other family that groups images
        c = sel["%s: several images per block, last group past the batch" % fam]
        bh, bw, ni = c.group_plan()
        assert ni > 1 and c.N % ni != 0 and c.family in cc.GROUPED, (fam, c, (bh, bw, ni))
        c = sel["%s: the same with several %s per image" % (fam, "tiles" if fam.startswith("wino") else "pixels")]
        assert c.group_plan()[2] > 1 and c.N % c.group_plan()[2] != 0 and c.H * c.W > 1, (fam, c)
    families = {c.family for c in sel.values()} | {c.family for c in cc.exact_cases("large")}
    assert {"igemm", "split", "wino", "wino2", "wino4", "wino2s", "tp2", "tp2s", "stem7s", "k3s", "stem", "box64", "tp2b", "thin"} <= families
    ids = {c.force for pool in cc.POOLS for c in cc.exact_cases(pool) if c.path == "f32"}
    every = set(range(cc.lib().w2l_conv_num_tiles()))
    assert every - ids == set(), sorted(every - ids)                        # every fp32 configuration id is forced somewhere
    assert {c.force for c in cc.exact_cases("bf16 igemm")} == set(range(cc.lib().w2l_convb_num_tiles()))


def test_tile_tables_list_every_tile_of_the_library():
    assert cc.num_tiles("f32") == len(cc.F32_TILES) == cc.lib().w2l_conv_num_igemm_tiles()
    assert cc.num_tiles("bf16") == len(cc.BF16_TILES) == cc.lib().w2l_convb_num_tiles()
    assert cc.config_id("split", len(cc.F32_TILES) - 1) - cc.config_id("split") == len(cc.F32_TILES) - 1


def test_geometry_list_is_that_of_the_signature_table():
    from test_conv_gpu import SIGS
    assert cc.sigs_geoms(SIGS) == cc.SIGS_GEOMS


def test_block_plan_refuses_families_that_do_not_group_images():
    import ctypes as C
    out = (C.c_int * 3)()
    for cid in (0, 6, 11, cc.config_id("stem7s")):
        assert cc.lib().w2l_conv_block_plan(cid, 3, 5, 4, out) != 0
    for cid in (8, 9, 12, 19, cc.config_id("tp2"), cc.config_id("tp2s"), cc.config_id("k3s")):
        assert cc.lib().w2l_conv_block_plan(cid, 3, 5, 4, out) == 0 and min(out) >= 1


def test_large_cases_lie_between_one_and_two_gib():
    for c in cc.exact_cases("large"):
        for b in c.nbytes():
            assert b == 0 or (1 << 30) < b < (1 << 31), (c, c.nbytes())
    assert len(cc.exact_cases("large")) == len(cc.candidates("large"))


def test_guards_cover_the_largest_block():
    for cs, esz in ((4, 4), (8, 2), (512, 4), (1024, 2)):
        n = cc.guard_elems(cs, esz)
        assert n >= 512 * cs and n * esz >= 64 * 1024 and (n * esz) % 16 == 0


# ---------------------------------------------------------------- the backward pass
def _bwd_candidates():
    return [(pool, c) for pool in cc.BWD_POOLS for c in cc.candidates(pool)]


@pytest.mark.parametrize("pool", cc.BWD_POOLS + ["update"])
def test_every_backward_case_meets_its_exactness_bound(pool):
    cases = cc.exact_cases(pool)
    assert cases, pool
    for c in cases:
        assert c.exact_bound() < cc.LIMIT, (c, c.exact_bound())
        assert sum(c.nbytes()) < (64 << 20) or (c.path == "bf16" and c.N > 16), (c, c.nbytes())      # small, but for the large-N families


def test_in_place_bound_counts_the_prior():
    a = cc.Case("f32", "igemm", 1, 15, 40, 3, 2, 1, 1, 2, 3, 3, force=4, res=3, act=cc.ACT_NONE, bwd=True)
    b = cc.Case("f32", "igemm", 1, 15, 40, 3, 2, 1, 1, 2, 3, 3, force=4, res=1, act=cc.ACT_NONE, bwd=True)
    assert a.exact_bound() - b.exact_bound() == 2 * (3 - 1)
    x, w, scale, shift, prior = cc.int_operands(a)
    assert float(prior.abs().max()) == 3 and bool((prior == prior.round()).all()) and prior.shape == (2, 40, 6, 6)
    assert bool((scale == 1).all()) and bool((shift == 0).all())            # as NodeF builds a data-gradient handle
    assert a.nbytes()[2] == 0 and a.strides()[2:4] == a.strides()[4:6]      # the residual is the output slice, no buffer of its own
    s = cc.Case("f32", "igemm", 1, 15, 40, 3, 2, 1, 1, 2, 3, 3, force=4, res=3, sliced=True, bwd=True)
    assert s.strides()[2:4] == s.strides()[4:6]


def test_every_backward_regime_has_a_case_and_a_name_of_its_own():
    empty = [name for name, _pool, c in cc.select(cc.BWD_REGIMES) if c is None]
    assert not empty, empty
    names = [n for n, _p, _f in cc.REGIMES + cc.BWD_REGIMES]
    assert len(names) == len(set(names))


def test_backward_grid_covers_the_signature_table():
    """every (transposed, k, stride, pad, output padding) row in backward form on each implicit-GEMM path; output padding 0, 1 and 2 on
    an axis and different paddings on the two axes; every Winograd id with transposed = 1; both conv_wino4 forms"""
    assert set(cc.BWD_EXTENTS) == {g[:5] for g in cc.SIGS_GEOMS}
    for pool in ("bwd f32 igemm", "bwd f32 split", "bwd bf16 igemm"):
        cases = cc.exact_cases(pool)
        assert {cc._row(c) for c in cases} == {g[:5] for g in cc.SIGS_GEOMS}, pool
        assert {c.op for c in cases if c.s == (3, 3)} >= {(0, 1), (1, 0), (2, 1), (1, 2), (2, 0)}
        assert {c.op for c in cases if c.s == (3, 1)} == {(0, 0), (1, 0), (2, 0)}
        assert {c.op for c in cases if c.s == (1, 2)} == {(0, 0), (0, 1)}
        base = cc.config_id("split") if pool == "bwd f32 split" else 0
        assert {c.force - base for c in cases if c.res == 3 and not c.ks and c.cout > 16} == set(range(6)), pool                    # every tile in place
        assert {c.force - base for c in cases if c.res == 3 and c.ks == 3} == set(range(6)), pool
        assert {c.N for c in cases} == {2, 3}
    sel = {n: c for n, _p, c in cc.select(cc.BWD_REGIMES)}
    for cid in (6, 7, 8, 9, 12, 11, 19):
        for c in cc.exact_cases("bwd wino id %d" % cid):
            assert c.tr == 1 and c.force == cid and (c.cin, c.cout) == cc.WINO_CH[cid]
    assert sel["wino4 transposed: rectangles, accumulate in place"].wino4_plan()["form"] == 0
    assert sel["wino4 transposed: segments, accumulate in place"].wino4_plan()["form"] == 1
    both = (cc.config_id("tp2"), cc.config_id("tp2s"))
    for c in cc.exact_cases("bwd tp2") + cc.exact_cases("bwd tp2s"):
        if c.declines:      # no residual operand; output padding (1, 1) only
            assert c.declines == both and not c.applicable(both[0]) and not c.applicable(both[1]) and c.family == "igemm", c
            assert c.res == 3 or c.op != (1, 1), c
        else:
            assert c.op == (1, 1) and not c.res and c.applicable(), c
    fams = {c.convb_resolve()[0] for c in cc.exact_cases("bwd bf16 special")}
    assert fams == {"box64", "tp2b"}
    assert {(c.family, c.res) for c in cc.exact_cases("bwd bf16 special")} == {("box64", 0), ("box64", 3), ("tp2b", 0), ("tp2b", 3)}


def test_restated_output_padding_is_that_of_dgrad_geom():
    from wav2lip_amd import autograd
    from wav2lip_amd._lib import ConvGeom
    n = 0
    for _pool, c in _bwd_candidates():
        (tr, cin, cout, k, s, p, op), H, W = c.fwd
        k, s, p, op = (cc._pair(v) for v in (k, s, p, op))
        g = autograd.dgrad_geom(ConvGeom(int(tr), cin, cout, k[0], k[1], s[0], s[1], p[0], p[1], op[0], op[1], cc.ACT_RELU), H, W)
        mine = c.geom()
        for f in ("transposed", "cin", "cout", "kh", "kw", "sh", "sw", "ph", "pw", "oph", "opw", "act"):
            assert getattr(g, f) == getattr(mine, f), (c, f, getattr(g, f), getattr(mine, f))
        assert c.out_hw() == (H, W), c                                    # the gradient has the extent of the forward input
        n += 1
    assert n > 300


def test_backward_reference_is_the_autograd_input_gradient():
    """independence of the reference: the float64 conv_transpose2d / conv2d of the backward Case == torch's float64 autograd gradient
    of the FORWARD layer with respect to its input, bit for bit (same w, same dz; both sides hold integers)"""
    import torch.nn.functional as F
    seen = set()
    for _pool, c in _bwd_candidates():
        key = (c.fwd, c.N if c.N <= 16 else 7, c.seed, c.wmode)
        if key in seen:
            continue
        seen.add(key)
        (tr, cin, cout, k, s, p, op), H, W = c.fwd
        dz, w, scale, shift, _prior = cc.int_operands(c)
        x = torch.zeros(dz.shape[0], cin, H, W, dtype=torch.float64, requires_grad=True)
        z = F.conv_transpose2d(x, w, None, cc._pair(s), cc._pair(p), cc._pair(op)) if tr else F.conv2d(x, w, None, cc._pair(s), cc._pair(p))
        assert z.shape == dz.shape, (c, z.shape, dz.shape)
        z.backward(dz)
        got = cc.ref64(c, dz, w, scale, shift, None)
        assert got.shape == x.grad.shape, (c, got.shape, x.grad.shape)
        assert torch.equal(got, x.grad), (c, float((got - x.grad).abs().max()))
        assert bool((got == got.round()).all()) or c.wmode == "w4"
    assert len(seen) > 100


def test_update_cases_cannot_pass_on_stale_weights():
    cases = cc.exact_cases("update")
    assert len(cases) == len(cc.candidates("update"))
    for c in cases:
        r0, r1, r2 = cc.update_refs(c)
        assert not torch.equal(r0, r1) and not torch.equal(r1, r2), c
        if c.path == "bf16" and not c.head:                                # ... nor after the one rounding to bf16
            assert not torch.equal(r0.float().bfloat16(), r1.float().bfloat16()), c
    ids = {c.force for c in cases if c.path == "f32"}
    assert ids >= {4, 17, 6, 7, 8, 9, 12, 11, 19, cc.config_id("tp2"), cc.config_id("tp2s"), cc.config_id("stem7s"), cc.config_id("k3s")}
    assert {c.tr for c in cases if c.family.startswith("wino")} == {0, 1}
    assert {c.convb_resolve()[0] for c in cases if c.path == "bf16" and not c.head and c.force < 0} == {"stem1", "stem2", "stem3", "box64", "tp2b"}
