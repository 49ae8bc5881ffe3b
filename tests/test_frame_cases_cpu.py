"""The yardstick of tests/test_frame_kernels_gpu.py, checked where no GPU is needed: oracle/resize_ref.py (the fixed-point
restatement of cv2.resize that the kernels of csrc/resize.hip must equal byte for byte) against plain float64 bilinear
interpolation written without it (tests/_frame_cases.py), hand-computed pixels at the vertical and horizontal clamps, and the
numpy model of w2l_compose_rows_u8.

Measured (29 size pairs x 3 image kinds): worst |oracle - float64| = 0.7964 grey levels (96x96 -> 300x300, random image); the
bound is 1.0, strict."""
import numpy as np
import pytest

import _frame_cases as FC
from oracle import resize_ref


@pytest.mark.parametrize("case", FC.SIZE_PAIRS + [FC.STRIDE_PAIR], ids=lambda c: c[0])
def test_oracle_stays_within_one_grey_level_of_float64_bilinear(case):
    name, Hs, Ws, Hd, Wd = case
    for kind in FC.IMAGE_KINDS:
        src = FC.image(kind, Hs, Ws, seed=11)
        got = resize_ref.resize_linear_u8(src, (Wd, Hd))
        want = FC.bilinear_f64(src, (Wd, Hd))
        assert got.shape == want.shape == (Hd, Wd, 3) and got.dtype == np.uint8
        d = np.abs(got.astype(np.float64) - want)
        print("%s %s (%s): worst %.4f, above 0.5: %.3f" % (name, kind, FC.expected_path(Hs, Ws, Hd, Wd), d.max(), (d > 0.5).mean()))
        assert d.max() < FC.BOUND, "%s %s: worst %.4f at %s, %d pixels at or above %.1f" % (
            name, kind, d.max(), np.unravel_index(d.argmax(), d.shape), int((d >= FC.BOUND).sum()), FC.BOUND)


def test_the_case_table_takes_every_path():
    paths = [FC.expected_path(*c[1:]) for c in FC.SIZE_PAIRS]
    assert paths.count("copy") >= 2 and paths.count("area") >= 3 and paths.count("general") >= 20
    by_id = {c[0]: FC.expected_path(*c[1:]) for c in FC.SIZE_PAIRS}
    assert by_id["2x_rows_only_190"] == by_id["2x_rows_only"] == by_id["2x_cols_only"] == by_id["4x"] == "general"
    assert FC.STRIDE_PAIR[3] * FC.STRIDE_PAIR[4] > 1024 * 256
    assert 130 * 130 > 64 * 256 and 130 in FC.CROP_S and all(S * S <= 64 * 256 for S in (1, 7, 96))
    assert FC.BIG_BOX[1] * FC.BIG_BOX[3] > 256 * 256
    for S in FC.CROP_S:
        for (H, W), boxes in FC.crop_table(S).items():
            FC.check_rows([(i, H, W, b) for i, b in boxes])
    for H, W in (FC.FRAME_ODD, FC.FRAME_EVEN):
        FC.check_rows([(i, H, W, b) for i, b in FC.paste_boxes(H, W)])
    assert FC.FRAME_ODD[1] % 2 == 1 and FC.FRAME_ODD[1] * 3 == 393


def test_the_compose_tables_cover_what_they_claim():
    sweep, edges, mixed = (FC.check_rows(f()) for f in (FC.compose_sweep, FC.compose_group_edges, FC.compose_mixed_shapes))
    assert {r[2] for r in sweep} >= {1, 2, 3, 4, 5, 131, 150}
    assert {(r[1] * r[2]) % 4 for r in sweep} == {0, 1, 2, 3}
    for W in (1, 3, 5, 131):
        assert {(r[1] * r[2]) % 4 for r in sweep if r[2] == W} == {0, 1, 2, 3}
    modes = {(r[4], r[5]) for r in sweep}
    assert modes >= {(o, o) for o in range(4)} | {(o, None) for o in range(4)} | {(0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)}
    for W in (131, 150):
        px = [r for r in edges if r[2] == W and r[3][1] - r[3][0] == 1 and r[3][3] - r[3][2] == 1 and r[3][0] == 1]
        assert (W * 1) % 4 != 0 and {r[3][2] % 4 for r in px} == {0, 1, 2, 3}             # row 1 starts inside a group
        st = [r for r in edges if r[2] == W and r[3][3] - r[3][2] == 2 and (r[3][0] * W + r[3][2]) % 4 == 3]
        assert len(st) >= 4
    assert len({(r[1], r[2]) for r in mixed}) >= 4


def test_float64_reference_is_plain_bilinear():
    """the reference against values worked by hand, so that it is not itself the unknown"""
    src = np.array([[[0.0], [100.0]], [[50.0], [250.0]]])
    assert np.array_equal(FC.bilinear_f64(src, (2, 2)), src)
    up = FC.bilinear_f64(src, (4, 4))[..., 0]                      # f = -0.25 -> 0, 0.25, 0.75, 1.25 -> 1
    assert np.allclose(up[0], [0, 25, 75, 100], atol=1e-12) and np.allclose(up[:, 0], [0, 12.5, 37.5, 50], atol=1e-12)
    assert abs(up[1, 1] - (0.75 * (0.75 * 0 + 0.25 * 100) + 0.25 * (0.75 * 50 + 0.25 * 250))) < 1e-12
    assert np.allclose(FC.bilinear_f64(src, (1, 1)), 100.0)        # the centre: the mean of the four
    a = FC.image("random", 9, 13, seed=1)
    assert np.array_equal(FC.bilinear_f64(a, (13, 9)), a.astype(np.float64))
    assert np.allclose(FC.bilinear_f64(a[:8, :12], (6, 4)),
                       a[:8, :12].astype(np.float64).reshape(4, 2, 6, 2, 3).mean(axis=(1, 3)), atol=1e-12)


@pytest.mark.parametrize("value", [0, 1, 137, 254, 255])
def test_a_constant_image_stays_constant(value):
    for name, Hs, Ws, Hd, Wd in FC.SIZE_PAIRS:
        out = resize_ref.resize_linear_u8(np.full((Hs, Ws, 3), value, np.uint8), (Wd, Hd))
        assert (out == value).all(), (name, value, np.unique(out).tolist())
        assert (FC.bilinear_f64(np.full((Hs, Ws, 3), value, np.uint8), (Wd, Hd)) == value).all()


def test_a_ramp_resized_along_its_own_axis_is_monotonic():
    for name, Hs, Ws, Hd, Wd in FC.SIZE_PAIRS:
        out = resize_ref.resize_linear_u8(FC.image("ramp", Hs, Ws), (Wd, Hd)).astype(np.int32)
        assert (np.diff(out[..., 0], axis=1) >= 0).all() and (np.diff(out[..., 1], axis=1) <= 0).all(), name
        out = resize_ref.resize_linear_u8(FC.vramp(Hs, Ws), (Wd, Hd)).astype(np.int32)
        assert (np.diff(out, axis=0) >= 0).all(), name
        if Hd >= Hs > 1:                                                     # an up-scale keeps the ends of the ramp
            assert out[0].max() == 0 and out[-1].min() == 255, name


def test_oracle_known_answers_at_the_clamps():
    """fixed-point values worked by hand (coefficients cvRound(f * 2048), horizontal sums, (b * (S >> 4)) >> 16, (+ 2) >> 2)"""
    R = resize_ref.resize_linear_u8

    def col(v):
        return np.array(v, dtype=np.uint8).reshape(-1, 1, 1).repeat(3, axis=2)

    def row(v):
        return np.array(v, dtype=np.uint8).reshape(1, -1, 1).repeat(3, axis=2)

    # 2x1 -> 4x1: fy = -0.25, 0.25, 0.75, 1.25.  dy = 0: sy = -1, fy = 0.75, BOTH rows clip to row 0 (coefficients 512 + 1536:
    # (512 * 25600 >> 16) + (1536 * 25600 >> 16) + 2 >> 2 = (200 + 600 + 2) >> 2 = 200); dy = 3: sy = 1, both rows clip to row 1
    assert R(col([200, 0]), (1, 4))[:, 0, 0].tolist() == [200, 150, 50, 0]
    assert R(col([201, 7]), (1, 4))[:, 0, 0].tolist() == [201, 153, 56, 7]
    # 1x3 -> 1x4: fx = -0.125 (clamped to column 0, coefficient zeroed), 0.625, 1.375, 2.125 (sx = 2 >= W - 1: coefficient zeroed)
    # dx = 1: 10 * 768 + 101 * 1280 = 136960, >> 4 = 8560, * 2048 >> 16 = 267, (267 + 2) >> 2 = 67 (exact value 66.875)
    # dx = 2: 101 * 1280 + 255 * 768 = 325120, >> 4 = 20320, * 2048 >> 16 = 635, (635 + 2) >> 2 = 159 (exact value 158.75)
    assert R(row([10, 101, 255]), (4, 1))[0, :, 0].tolist() == [10, 67, 159, 255]
    # 1x3 -> 1x2: fx = 0.25, 1.75: 10 * 1536 + 101 * 512 -> 33 (32.75), 101 * 512 + 255 * 1536 -> 217 (216.5)
    assert R(row([10, 101, 255]), (2, 1))[0, :, 0].tolist() == [33, 217]
    # 2x2 -> 3x3: f = -1/6, 1/2, 7/6 on both axes.  (0,0): column clamped, rows both 0, coefficients 341 + 1707:
    # (341 * 1280 >> 16) + (1707 * 1280 >> 16) + 2 >> 2 = (6 + 33 + 2) >> 2 = 10.  (0,1): (9 + 50 + 2) >> 2 = 15.
    # (1,1): (1024 * 1920 >> 16) + (1024 * 4544 >> 16) + 2 >> 2 = (30 + 71 + 2) >> 2 = 25.  (2,2): (136 + 27 + 2) >> 2 = 41.
    src = np.array([[10, 20], [30, 41]], dtype=np.uint8)[:, :, None].repeat(3, axis=2)
    out = R(src, (3, 3))[..., 0]
    assert (out[0, 0], out[0, 1], out[1, 1], out[2, 2]) == (10, 15, 25, 41), out.tolist()
    # (2,1): both rows clip to row 1, (1707 * 4544 >> 16) + (341 * 4544 >> 16) + 2 >> 2 = (118 + 23 + 2) >> 2 = 35: the exact value is
    # 35.5, the two truncating shifts take it below the half
    assert out[0].tolist() == [10, 15, 20] and out[2].tolist() == [30, 35, 41] and out[:, 0].tolist() == [10, 20, 30]


def test_compose_model_agrees_with_the_in_place_paste():
    rng = np.random.default_rng(3)
    n = 0
    for rows, S in ((FC.compose_mixed_shapes(), 96), (FC.compose_group_edges()[::7], FC.COMPOSE_SWEEP_S),
                    (FC.compose_sweep()[::11], FC.COMPOSE_SWEEP_S)):
        for name, H, W, box, _, _ in rows:
            src = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            pred = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
            keep = src.copy()
            got = FC.compose_model(src, pred, box)
            assert np.array_equal(src, keep), name                                        # the model leaves its source alone
            assert np.array_equal(got, resize_ref.resize_paste(src.copy(), pred, box)), name
            y1, y2, x1, x2 = box
            mask = np.ones((H, W), bool)
            mask[y1:y2, x1:x2] = False
            assert np.array_equal(got[mask], src[mask]), name
            d = np.abs(got.astype(np.float64) - FC.paste_f64(src, pred, box))
            assert d.max() < FC.BOUND, (name, d.max())
            n += 1
    assert n > 150


def test_face_crops_checks_its_boxes_before_it_touches_the_device():
    """calculate_scores.face_crops hands its boxes to w2l_crop_resize_rows_u8 as they are: empty, inverted and overhanging ones
    must stop on the host (no device is needed to get that far)"""
    from wav2lip_amd import calculate_scores
    frames = np.zeros((2, 40, 60, 3), np.uint8)
    for bad in ([(0, 0, 0, 5)] * 2, [(5, 3, 0, 5)] * 2, [(0, 5, 9, 4)] * 2, [(0, 41, 0, 5)] * 2, [(0, 5, -1, 5)] * 2,
                [(0, 5, 0, 61), (0, 5, 0, 5)], [(0, 5, 0, 5)], []):
        with pytest.raises(ValueError):
            calculate_scores.face_crops(frames, bad, "cuda:0")
    with pytest.raises(ValueError):
        calculate_scores.face_crops(frames.astype(np.float32), [(0, 5, 0, 5)] * 2, "cuda:0")
    with pytest.raises(ValueError):
        calculate_scores.face_crops(frames[0], [(0, 5, 0, 5)] * 2, "cuda:0")
