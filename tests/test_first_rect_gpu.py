"""w2l_s3fd_first_rect (face_detection/s3fd.first_rects) against the per-image Python rule it replaces in
FaceAlignment.get_detections_for_batch (sfd_detector.py:45 + api.py:61-77): hand-made keep lists for the edge cases, random tables
through the device NMS, and the whole detector on the S3FD golden frames in both precisions."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wav2lip_amd import synthetic as synth  # noqa: E402

pytestmark = pytest.mark.gpu


def host_rule(table, keep, n):
    """the per-image rule of the host path: rows of keep[:n] in order, the first with score > 0.5, np.maximum(., 0), int()"""
    d = table[keep[:n]]
    dets = [x for x in d if x[-1] > 0.5]
    if len(dets) == 0:
        return None
    return tuple(int(v) for v in np.maximum(np.asarray(dets[0][:4]), 0))


def device_rects(table, keep, counts, dev):
    from wav2lip_amd.face_detection.s3fd import first_rects
    return first_rects(torch.from_numpy(table).to(dev), torch.from_numpy(keep).to(dev), torch.from_numpy(counts).to(dev), 0.5)


def check_against_host(table, keep, counts, dev):
    from wav2lip_amd.face_detection.s3fd import RECT_FOUND, RECT_HOST, RECT_NONE
    res = device_rects(table, keep, counts, dev)
    assert res.dtype == np.int32 and res.shape == (len(table), 5)
    for b in range(len(table)):
        want = host_rule(table[b], keep[b], counts[b])
        assert res[b, 4] != RECT_HOST, b
        if want is None:
            assert res[b, 4] == RECT_NONE and tuple(res[b, :4]) == (0, 0, 0, 0), b
        else:
            assert res[b, 4] == RECT_FOUND and tuple(int(v) for v in res[b, :4]) == want, (b, res[b], want)
    return res


def one_image(rows, order=None):
    """table [1, P, 5] of `rows` and a keep list over them (default: row order)"""
    t = np.asarray(rows, np.float32).reshape(1, -1, 5)
    k = np.asarray(order if order is not None else range(t.shape[1]), np.int32)
    keep = np.zeros((1, t.shape[1]), np.int32)
    keep[0, :len(k)] = k
    return t, keep, np.asarray([len(k)], np.int32)


def test_zero_survivors_is_no_rect(cuda):
    t, keep, _ = one_image([[1, 2, 3, 4, 0.9]] * 3)
    res = check_against_host(t, keep, np.zeros(1, np.int32), cuda)
    assert res[0, 4] == 0


def test_a_score_of_exactly_one_half_does_not_pass(cuda):
    t, keep, n = one_image([[10, 10, 50, 50, 0.5], [20, 20, 60, 60, 0.5]])
    assert check_against_host(t, keep, n, cuda)[0, 4] == 0
    t, keep, n = one_image([[10, 10, 50, 50, 0.5], [20.5, 21.9, 60.2, 61.7, np.nextafter(np.float32(0.5), np.float32(1))]])
    assert tuple(check_against_host(t, keep, n, cuda)[0, :4]) == (20, 21, 60, 61)


def test_negative_and_fractional_coordinates(cuda):
    t, keep, n = one_image([[-3.7, -0.2, 15.999, 0.9999, 0.97]])
    assert tuple(check_against_host(t, keep, n, cuda)[0, :4]) == (0, 0, 15, 0)
    t, keep, n = one_image([[-0.0, -1e30, 2147483520.0, 7.5, 0.8]])         # the largest float32 below 2^31 still converts
    assert tuple(check_against_host(t, keep, n, cuda)[0, :4]) == (0, 0, 2147483520, 7)


def test_a_later_keep_entry_passes_when_the_first_does_not(cuda):
    rows = [[1, 1, 9, 9, 0.3], [2, 2, 8, 8, 0.45], [3.5, 4.5, 30.5, 40.5, 0.7], [5, 5, 6, 6, 0.99]]
    t, keep, n = one_image(rows, order=[1, 0, 2, 3])
    assert tuple(check_against_host(t, keep, n, cuda)[0, :4]) == (3, 4, 30, 40)
    t, keep, n = one_image(rows, order=[0, 3, 2])                          # keep order decides, not the score
    assert tuple(check_against_host(t, keep, n, cuda)[0, :4]) == (5, 5, 6, 6)


def test_the_first_passing_row_beyond_one_wave(cuda):
    rows = [[0, 0, 1, 1, 0.1]] * 200 + [[11.25, 12.5, 13.75, 14.0, 0.6]] + [[0, 0, 1, 1, 0.9]] * 20
    t, keep, n = one_image(rows)
    assert tuple(check_against_host(t, keep, n, cuda)[0, :4]) == (11, 12, 13, 14)


@pytest.mark.parametrize("bad", [np.inf, np.nan, 2147483648.0, 3e9])
def test_a_coordinate_int_cannot_take_is_left_to_the_host(cuda, bad):
    """the device flags the image; get_detections_for_batch then runs the host rule on it, which returns what Python's int()
    returns (2^31 and above fit a Python int) or raises what it raises (OverflowError on inf, ValueError on NaN)"""
    from wav2lip_amd import face_detection
    from wav2lip_amd.face_detection.s3fd import RECT_FOUND, RECT_HOST
    rows = [[1, 2, 3, 4, 0.2], [1.5, 2.5, bad, 4.5, 0.9], [7, 7, 9, 9, 0.95]]
    t0, keep, n = one_image(rows)
    t1, _, _ = one_image([[1.5, 2.5, -np.inf, 4.5, 0.9]] + rows[2:] + rows[2:])      # -inf clips to 0, as np.maximum does
    t, keep, n = np.concatenate([t0, t1]), np.concatenate([keep, keep]), np.concatenate([n, n])
    res = device_rects(t, keep, n, cuda)
    assert res[0, 4] == RECT_HOST and tuple(res[0, :4]) == (0, 0, 0, 0)
    assert res[1, 4] == RECT_FOUND and tuple(res[1, :4]) == (1, 2, 0, 4) == host_rule(t[1], keep[1], n[1])
    fa = face_detection.FaceAlignment.__new__(face_detection.FaceAlignment)
    fa._candidates = lambda images: tuple(torch.from_numpy(x).to(cuda) for x in (t, keep, n))
    if np.isfinite(bad):
        assert fa.get_detections_for_batch(None) == [host_rule(t[0], keep[0], n[0]), (1, 2, 0, 4)]
        assert fa.get_detections_for_batch(None)[0] == (1, 2, int(np.float32(bad)), 4)
    else:
        with pytest.raises(OverflowError if np.isinf(bad) else ValueError):
            host_rule(t[0], keep[0], n[0])
        with pytest.raises(OverflowError if np.isinf(bad) else ValueError):
            fa.get_detections_for_batch(None)


@pytest.mark.parametrize("B", [1, 64])
def test_random_tables_through_the_device_nms(cuda, B):
    from wav2lip_amd.face_detection.s3fd import nms_batch
    r = np.random.default_rng(B)
    P = 1500
    xy = r.normal(80, 60, (B, P, 2))
    wh = r.uniform(2, 90, (B, P, 2))
    sc = r.uniform(0, 1, (B, P)) * r.uniform(0.3, 1.05, (B, 1))          # some images with no score above 0.5
    t = np.concatenate([xy, xy + wh, sc[..., None]], axis=2).astype(np.float32)
    tab = torch.from_numpy(t).to(cuda)
    keep, counts = nms_batch(tab, 0.05, 0.3)
    keep_h, counts_h = keep.cpu().numpy(), counts.cpu().numpy()
    res = check_against_host(t, keep_h, counts_h, cuda)
    if B == 64:
        assert 0 < (res[:, 4] == 1).sum() < B and (counts_h == 0).sum() == 0


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_get_detections_for_batch_equals_the_per_image_rule_on_the_golden_frames(cuda, precision):
    from wav2lip_amd import face_detection
    fa = face_detection.FaceAlignment(face_detection.LandmarksType._2D, device="cuda", state_dict=synth.s3fd_state_dict(),
                                      precision=precision)
    for img in (synth.s3fd_frames(), synth.preprocess_frames(8, 400)):
        got = fa.get_detections_for_batch(img)
        want = []
        for dets in fa.detect_from_batch(img):                              # the previous path: per-image copies, host rule
            want.append(None if len(dets) == 0 else tuple(int(v) for v in np.maximum(np.asarray(dets[0][:4]), 0)))
        assert got == want
        assert all(r is None or all(type(v) is int for v in r) for r in got)
    if precision == "f32":
        gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_s3fd_v1.npz"))
        got = fa.get_detections_for_batch(synth.s3fd_frames())
        assert [r if r is not None else (-1, -1, -1, -1) for r in got] == [tuple(r) for r in gold["rects"].tolist()]
