"""The yardsticks of tests/test_glue_kernels_gpu.py, checked where no GPU is needed (tests/_glue_cases.py):
  1. the derived bounds hold on the chosen inputs: the numpy fp32 restatement of every kernel stays inside its bound against
     the float64 reference (and equals it where the comparison is bit-exact);
  2. the inputs tell a wrong kernel from a right one: every named wrong variant of a formula leaves the bound on the cases it
     can affect;
  3. the case tables reach the regimes the GPU file claims, computed from the transcribed launch rules.

Restatement / bound, largest over all cases (numpy fp32, no contraction): l2norm 0.30, decode coordinates 0.19, decode score
0.16 - the derivations in _glue_cases.py leave a factor of three and more."""
import numpy as np
import pytest
import torch

import _glue_cases as G
from oracle import datagen_ref, s3fd_ref

F32 = np.float32


def _frac(err, bound):
    """largest err / bound over the elements whose bound is not 0"""
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ---------------------------------------------------------------- decode
@pytest.mark.parametrize("case", G.DECODE_CASES, ids=str)
def test_decode_restatement_stays_inside_the_bounds(case):
    conf, loc = G.decode_inputs(case, seed=sum(case))
    ref, bound = G.decode_case_ref(case, conf, loc)
    got = G.decode_f32(case, conf, loc).astype(np.float64)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    err = np.abs(got - ref)
    fc, fs = _frac(err[:, :4], bound[:, :4]), _frac(err[:, 4:], bound[:, 4:])
    print("decode %s: coordinates %.3f of the bound, score %.3f" % (case, fc, fs))
    assert not G.leaves(got, ref, bound).any(), (case, fc, fs)
    assert fc <= 0.5 and fs <= 0.5, "the restatement comes closer to the bound than its derivation allows for: %.3f %.3f" % (fc, fs)
    bg, fg = G.decode_bg_fg(conf, case[3])
    sat = np.abs(bg - fg) >= G.SAT_GAP
    assert sat.sum() == min(len(G.SAT_ROWS), conf.shape[0] // 2)
    assert np.array_equal(got[sat, 4], (fg[sat] > bg[sat]).astype(np.float64)), "a saturated row is exactly 0.0 or 1.0"
    assert (np.abs(bg - fg)[~sat] <= 16).mean() > 0.99


@pytest.mark.parametrize("case", G.DECODE_CASES, ids=str)
def test_decode_inputs_tell_the_wrong_variants_apart(case):
    conf, loc = G.decode_inputs(case, seed=sum(case))
    ref, bound = G.decode_case_ref(case, conf, loc)
    applied = 0
    for variant in G.DECODE_VARIANTS:
        if not G.decode_variant_applies(case, variant):
            continue
        wrong, _ = G.decode_case_ref(case, conf, loc, variant)
        out = G.leaves(wrong, ref, 2 * bound).any(1)               # twice: a kernel that computes the variant has its own roundoff
        assert out.any(), (case, variant)
        applied += 1
        if variant in ("variances_swapped", "no_half_stride"):
            assert out.mean() >= 0.999, (case, variant, out.mean())
    assert applied >= 5


def test_decode_variants_all_meet_a_case():
    for variant in G.DECODE_VARIANTS:
        assert any(G.decode_variant_applies(c, variant) for c in G.DECODE_CASES), variant
    assert not G.decode_variant_applies((3, 1, 1, 2, 128, 4, 4), "wx_hy_exchanged")


def test_decode_reference_by_hand():
    """one position worked by hand, so that the reference is not itself the unknown: stride 8 at (wx, hy) = (2, 1), l = 0:
    centre (20, 12), size 32 -> (4, -4, 36, 28); conf (0, ln 3) -> 3 / 4"""
    conf = np.array([[0.0, np.log(3.0)]])
    out, bound = G.decode_ref(conf, np.zeros((1, 4)), np.array([2.0]), np.array([1.0]), 2, 8)
    assert np.allclose(out[0], [4, -4, 36, 28, 0.75], atol=1e-12)
    assert np.allclose(bound[0], [G.R * 36, G.R * 28, G.R * 68, G.R * 60, G.R])
    # l = (1, -1, ln 2 / 0.2, 0): centre x + 0.1 * 32, y - 0.1 * 32, width 64 (variances as fp32 holds them: ~1e-8 relative)
    loc = np.array([[1.0, -1.0, np.log(2.0) / 0.2, 0.0]])
    out, _ = G.decode_ref(conf, loc, np.array([2.0]), np.array([1.0]), 2, 8)
    assert np.allclose(out[0, :4], [23.2 - 32, 8.8 - 16, 23.2 + 32, 8.8 + 16], rtol=1e-6)
    # max-out: the largest of the three background channels
    out4, _ = G.decode_ref(np.array([[-5.0, 0.0, -7.0, np.log(3.0)]]), np.zeros((1, 4)), np.array([0.0]), np.array([0.0]), 4, 4)
    assert abs(out4[0, 4] - 0.75) < 1e-12 and np.allclose(out4[0, :4], [-6, -6, 10, 10])


def test_decode_reference_equals_the_oracle():
    """the float64 reference against oracle/s3fd_ref.py::dense_boxes (torch fp32) on the level it is given: within the bounds"""
    case = (2, 5, 7, 2, 4, 2, 4)                                   # level 0 of dense_boxes has stride 4
    conf, loc = G.decode_inputs(case, seed=3)
    B, FH, FW = case[:3]
    nchw = lambda a: torch.from_numpy(a.reshape(B, FH, FW, -1).transpose(0, 3, 1, 2).copy())
    got = s3fd_ref.dense_boxes([nchw(conf), nchw(loc)])[0].reshape(-1, 5).astype(np.float64)
    ref, bound = G.decode_case_ref(case, conf, loc)
    assert not G.leaves(got, ref, bound).any()


# ---------------------------------------------------------------- l2norm
@pytest.mark.parametrize("shape", G.L2_SHAPES, ids=str)
def test_l2norm_restatement_stays_inside_the_bound(shape):
    C = shape[0]
    worst = 0.0
    for _, _, _, rows, rot in [c for c in G.l2norm_cases() if c[0] == C]:
        x, w = G.l2norm_inputs(C, rows, rot, seed=C + rows + rot)
        ref = G.l2norm_ref(x, w)
        bound = G.l2norm_bound(ref, C)
        got = G.l2norm_f32(x, w).astype(np.float64)
        assert not G.leaves(got, ref, bound).any(), (shape, rows, rot)
        assert (got[ref == 0] == 0).all()
        worst = max(worst, _frac(np.abs(got - ref), bound))
    print("l2norm C=%d: %.3f of the bound" % (C, worst))
    assert worst <= 0.5, "the restatement comes closer to the bound than its derivation allows for: %.3f" % worst


def test_l2norm_inputs_tell_the_wrong_variants_apart():
    met = {v: 0 for v in G.L2_VARIANTS}
    for C, _, _, rows, rot in G.l2norm_cases():
        x, w = G.l2norm_inputs(C, rows, rot, seed=C + rows + rot)
        ref = G.l2norm_ref(x, w)
        bound = G.l2norm_bound(ref, C)
        for variant in G.L2_VARIANTS:
            if G.l2norm_variant_applies(C, G.l2norm_kinds(rows, rot), variant):
                assert G.leaves(G.l2norm_ref(x, w, variant), ref, 2 * bound).any(), (C, rows, rot, variant)
                met[variant] += 1
    assert all(n >= 6 for n in met.values()), met


def test_l2norm_reference_equals_the_oracle_and_a_hand_value():
    x, w = np.array([[3.0, 0.0, 4.0, 0.0]], F32), np.array([1.0, 2.0, 10.0, 3.0], F32)
    assert np.allclose(G.l2norm_ref(x, w)[0], [0.6, 0.0, 8.0, 0.0], rtol=1e-10)
    x, w = G.l2norm_inputs(260, 5, 0, seed=1)
    got = s3fd_ref.l2norm(torch.from_numpy(x.T.copy()).view(1, 260, 5, 1).double(), torch.from_numpy(w).double())
    assert np.allclose(got.numpy()[0, :, :, 0].T, G.l2norm_ref(x, w), rtol=1e-7, atol=0)     # the oracle's 1e-10 is a double


# ---------------------------------------------------------------- maxpool
@pytest.mark.parametrize("case", G.POOL_CASES, ids=str)
def test_maxpool_restatement_variant_and_inputs(case):
    N, H, W, C, x_cs, y_cs = case
    x = G.pool_inputs(case, seed=sum(case))
    ref = G.pool_ref(x, C)
    assert ref.shape == (N, H // 2, W // 2, C) and not np.isnan(ref).any()
    got = G.pool_f32(x, C, y_cs)
    assert np.array_equal(got[..., :C], ref) and (got[..., C:] == G.SENT).all()
    want = torch.nn.functional.max_pool2d(torch.from_numpy(x[..., :C].transpose(0, 3, 1, 2).copy()), 2, 2)
    assert np.array_equal(ref, want.numpy().transpose(0, 2, 3, 1))
    assert (ref != G.pool_ref(x, C, G.POOL_VARIANTS[0])).any()
    assert (ref < 0).any(), "a negative-only window"
    if N * H * W * C >= 1000:
        assert np.isposinf(ref).any() and np.isneginf(x[..., :C]).any()
    if H % 2 or W % 2:
        assert np.isposinf(x[:, H - H % 2:, :, :C]).all() and np.isposinf(x[:, :, W - W % 2:, :C]).all()


# ---------------------------------------------------------------- pack
def test_pack_restatement_equals_the_oracle_on_every_byte_value():
    for npix in G.PACK_NPIX:
        bgr = G.pack_inputs(npix)
        want = s3fd_ref.preprocess(bgr.reshape(1, 1, npix, 3)).permute(0, 2, 3, 1).reshape(npix, 3).numpy()
        assert np.array_equal(G.bits(G.pack_f32(bgr)), G.bits(want))
    bgr = G.pack_inputs(max(G.PACK_NPIX))
    for c in range(3):
        assert len(np.unique(bgr[:, c])) == 256
    assert [G.pack_vector_path(c) for c in G.PACK_YCS] == [False, True, False, True]
    e = G.pack_expected(G.pack_f32(bgr), 8)
    assert (e[:, 3] == 0).all() and (e[:, 4:] == G.SENT).all()
    assert (G.pack_expected(G.pack_f32(bgr), 5)[:, 3:] == G.SENT).all()


# ---------------------------------------------------------------- datagen
@pytest.mark.parametrize("S", G.DATAGEN_S)
def test_datagen_restatement_equals_the_oracle_and_the_variant_does_not(S):
    faces = G.datagen_inputs(G.DATAGEN_N, S, seed=S)
    want, _ = datagen_ref.datagen_batch(faces, np.zeros((G.DATAGEN_N, 80, 16), F32), img_size=S)
    got = G.datagen_f32(faces)
    assert np.array_equal(G.bits(got), G.bits(want.astype(F32)))
    assert (got[:, S // 2:, :, :3] == 0).all() and (got[:, :S // 2, :, :3] == got[:, :S // 2, :, 3:]).all()
    assert (got != G.datagen_f32(faces, G.DATAGEN_VARIANTS[0])).any()
    if G.DATAGEN_N * S * S >= 256:
        assert len(np.unique(faces[..., 0])) == 256


# ---------------------------------------------------------------- frames_to_u8
def test_frames_restatement_equals_the_oracle():
    x = G.frames_inputs()
    assert x.shape == (768, 3) and x.min() == 0 and x.max() == 1
    v = G.frames_values()
    for c in range(3):
        assert np.array_equal(np.sort(x[:, c]), np.sort(v))
    for N, H, W in G.FRAMES_SHAPES:
        want = datagen_ref.frames_to_u8(x.reshape(N, H, W, 3).transpose(0, 3, 1, 2))
        assert np.array_equal(G.frames_f32(x).reshape(N, H, W, 3), want)
    got = G.frames_f32(v).astype(np.int32)
    k = np.arange(256)
    assert np.array_equal(got[256:512], k) and np.array_equal(got[512:], k), "fp32(k / 255) * 255 is k again, and so is the value above"
    assert np.array_equal(got[1:256], k[1:] - 1), "the fp32 value below k / 255 truncates to k - 1: rounding instead would show"
    assert set(np.unique(got)) == set(range(256))


# ---------------------------------------------------------------- layouts
def test_layout_cases_straddle_the_tile():
    cs = {c[1] for c in G.LAYOUT_CASES.values()}
    hw = {c[2] * c[3] for c in G.LAYOUT_CASES.values()}
    assert {1, 32, 33, 37, 70} <= cs and {1, 31, 33, 45} <= hw
    for name, (N, C, H, W, y_cs, czt) in G.LAYOUT_CASES.items():
        assert y_cs >= max(C, czt), name
        x = G.layout_inputs(N, C, H, W, seed=1)
        e = G.layout_expected(x, y_cs, czt)
        assert np.array_equal(G.bits(e[..., :C].transpose(0, 3, 1, 2)), G.bits(x))
        assert (e[..., C:max(C, czt)] == 0).all() and (e[..., max(C, czt):] == G.SENT).all()
    assert sum(1 for c in G.LAYOUT_CASES.values() if c[4] > max(c[1], c[5])) >= 10, "room for the sentinel"


# ---------------------------------------------------------------- the regimes, from the launch rules
def test_every_grid_stride_loop_takes_one_trip_and_two():
    assert G.grid1d(1) == 1 and G.grid1d(257) == 2 and G.grid1d(16384 * 256 + 1) == 16384 and G.grid1d(10 ** 9, 256, 65536) == 65536
    assert G.grid_cap(0, 256, 8192) == 1 and G.grid_cap(8192 * 256 + 1, 256, 8192) == 8192
    assert {G.pack_trips(n) for n in G.PACK_NPIX} == {1} and G.pack_trips(G.PACK_BIG) == 2 and G.pack_trips(G.PACK_BIG - 3) == 1
    assert {G.decode_trips(*c[:3]) for c in G.DECODE_CASES} == {1}
    assert G.decode_trips(*G.DECODE_BIG[:3]) == 2 and G.DECODE_BIG[1] * G.DECODE_BIG[2] - 16384 * 256 == 2048
    assert {G.pool_trips(*c[:4]) for c in G.POOL_CASES} == {1}
    assert G.pool_trips(*G.POOL_BIG[:4]) == 2 and G.pool_items(*G.POOL_BIG[:4]) - 65536 * 256 == 16384
    assert {G.datagen_trips(G.DATAGEN_N, S) for S in G.DATAGEN_S} == {1}
    assert G.datagen_trips(*G.DATAGEN_BIG) == 2 and G.datagen_trips(227, 96) == 1
    assert {G.frames_trips(*s) for s in G.FRAMES_SHAPES} == {1} and G.frames_trips(*G.FRAMES_BIG) == 2
    # more than one workgroup below the cap, too
    assert max(G.grid1d(c[0] * c[1] * c[2]) for c in G.DECODE_CASES) >= 2
    assert max(G.grid1d(G.pool_items(*c[:4]), 256, 65536) for c in G.POOL_CASES) >= 2
    assert G.grid1d(max(G.PACK_NPIX)) == 2


def test_datagen_layouts_take_all_three_store_paths_in_both_types():
    for elem in (4, 2):
        paths = {G.datagen_store_path(elem, *lay) for lay in G.DATAGEN_LAYOUTS}
        assert paths == {"vector", "scalar_stride", "scalar_alignment", "scalar_c_zero_to"}, (elem, paths)
    assert G.datagen_store_path(4, 12, 8, 0) == "vector" and G.datagen_store_path(2, 12, 8, 0) == "scalar_stride"
    assert G.datagen_store_path(4, 8, 8, 1) == G.datagen_store_path(2, 8, 8, 1) == "scalar_alignment"
    assert G.datagen_store_path(4, 8, 0, 0) == "scalar_c_zero_to"
    assert any(S % 2 for S in G.DATAGEN_S) and 2 in G.DATAGEN_S


def test_l2norm_cases_reach_both_channel_regimes_and_ragged_rows():
    walks = {(c[0], c[3]): G.l2norm_walk(c[3], c[0]) for c in G.l2norm_cases()}
    trips = {w[2] for w in walks.values()}
    assert trips == {1, 2, 4}
    assert {w[1] for w in walks.values()} == {3, 2}, "waves of the last workgroup without a row"
    assert {c[3] % 4 for c in G.l2norm_cases()} == {1, 2} and max(w[0] for w in walks.values()) == 18
    assert walks[(260, 5)][2:] == (2, 1), "C = 260: lane 0 alone takes the second trip"
    assert walks[(4, 1)][2:] == (1, 1) and walks[(24, 1)][3] == 6 and walks[(512, 70)][2:] == (2, 64)
    kinds = set()
    for c in G.l2norm_cases():
        kinds |= set(G.l2norm_kinds(c[3], c[4]))
        if c[3] >= 4:
            assert set(G.l2norm_kinds(c[3], c[4])) == set(G.L2_KINDS)
    assert kinds == set(G.L2_KINDS)
    assert any(c[1] > c[0] for c in G.l2norm_cases()) and any(c[2] > c[0] for c in G.l2norm_cases())


def test_decode_cases_hold_both_class_counts_and_padded_strides():
    assert {c[3] for c in G.DECODE_CASES} == {2, 4}
    assert any(c[5] > c[3] for c in G.DECODE_CASES) and any(c[5] == c[3] for c in G.DECODE_CASES)
    assert any(c[6] > 4 for c in G.DECODE_CASES)
    assert (1, 9, 17, 2, 8, 4, 4) in G.DECODE_CASES and G.DECODE_BIG[3:] == (2, 4, 4, 4)      # production: cls_cs = 4 for ncls = 2
    assert any(c[0] >= 2 and c[1] > 1 for c in G.DECODE_CASES)
