"""Reduced-resolution face detection (`det_scale`, `--face_det_scale`) on the device: `w2l_s3fd_pack_rows_scaled[_bf16]` bit for bit
against the two launches it fuses (`w2l_resize_rows_u8`, then `w2l_s3fd_pack_rows[_bf16]`) and against numpy
(oracle.resize_ref + oracle.s3fd_ref.preprocess), `w2l_s3fd_first_rect_scaled` against the numpy statement of its rule, and the
detector end to end: exactly against a plain run on frames resized on the host, and against the CPU oracle within the dense-table
tolerance of tests/test_s3fd_gpu.py."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from oracle import resize_ref, s3fd_ref
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu

DENSE_TOL = 2e-3            # tests/test_s3fd_gpu.py: |dense table - reference| of the fp32 detector
GRID_CAP = 1024             # workgroups per image of the scaled pack (kPackScaledGridCap, csrc/detect.hip), 256 items each
KINDS = {"fp32": ("w2l_s3fd_pack_rows_scaled", "w2l_s3fd_pack_rows", torch.float32, 4),
         "bf16": ("w2l_s3fd_pack_rows_scaled_bf16", "w2l_s3fd_pack_rows_bf16", torch.bfloat16, 8)}
# (Hs, Ws) -> (Hd, Wd): copy | exact 2x average | k = 2 on odd sizes (bilinear) | k = 3 | k = 4 with Wd < 4: ragged items only |
# one full item + a one-pixel tail, 2x vertically but not horizontally
CASES = [((16, 16), (16, 16)), ((18, 22), (9, 11)), ((19, 23), (9, 11)), ((21, 27), (7, 9)), ((17, 13), (4, 3)), ((20, 25), (10, 5))]
ORDER = [3, 0, 4, 1, 2, 0]  # the address table: out of order, frame 0 twice


def _lib3():
    from wav2lip_amd import _lib
    return _lib.load(), _lib.current_stream(), _lib.ptr


def _s3fd_module():
    return importlib.import_module("wav2lip_amd.face_detection.s3fd")         # `face_detection.s3fd` is the class


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _nan_dest(B, Hd, Wd, y_cs, dtype, dev):
    """[B + 2, Hd, Wd, y_cs] of NaN: images 1..B are the destination, 0 and B + 1 the guard bands"""
    y = torch.full((B + 2, Hd, Wd, y_cs), float("nan"), dtype=dtype, device=dev)
    assert y[1].data_ptr() % 16 == 0
    return y


def _frame_buffer(frames, dev):
    """the frames back to back in one device byte buffer that starts 1 byte past a 16-byte aligned address; (buffer, addresses)"""
    n, fb = len(frames), frames[0].size
    buf = torch.zeros(16 + n * fb, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[1:1 + n * fb] = torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).to(dev)
    return buf, buf.data_ptr() + 1 + np.arange(n, dtype=np.int64) * fb


def _table(addrs, dev):
    t = torch.from_numpy(np.asarray(addrs, dtype=np.int64)).to(dev)
    assert t.data_ptr() % 8 == 0
    return t


def _composed(kind, table, B, Hs, Ws, Hd, Wd, dev):
    """w2l_resize_rows_u8 into a scratch batch, then w2l_s3fd_pack_rows[_bf16] on it, into a NaN-filled destination"""
    from wav2lip_amd import real_videos_inference as rv
    lib, s, ptr = _lib3()
    _, plain, dtype, y_cs = KINDS[kind]
    scratch = torch.zeros((B, Hd, Wd, 3), dtype=torch.uint8, device=dev)
    small = scratch.data_ptr() + np.arange(B, dtype=np.int64) * (Hd * Wd * 3)
    rows = np.zeros(B, rv.RESIZE_ROW)
    rows["src"], rows["dst"] = table.cpu().numpy().astype(np.uint64), small.astype(np.uint64)
    rows["Hs"], rows["Ws"], rows["Hd"], rows["Wd"] = Hs, Ws, Hd, Wd
    rows_dev = torch.from_numpy(rows.view(np.uint8)).to(dev)
    assert lib.w2l_resize_rows_u8(s, B, ptr(rows_dev), Hd * Wd) == 0, lib.w2l_last_error()
    y = _nan_dest(B, Hd, Wd, y_cs, dtype, dev)
    small_dev = _table(small, dev)
    assert getattr(lib, plain)(s, B, Hd, Wd, ptr(small_dev), y[1].data_ptr(), y_cs) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    return y


def _scaled(kind, table, B, Hs, Ws, Hd, Wd, dev):
    lib, s, ptr = _lib3()
    fused, _, dtype, y_cs = KINDS[kind]
    y = _nan_dest(B, Hd, Wd, y_cs, dtype, dev)
    assert getattr(lib, fused)(s, B, Hs, Ws, Hd, Wd, ptr(table), y[1].data_ptr(), y_cs) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    return y


# ---------------------------------------------------------------- 1. the scaled pack is the two existing kernels composed
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d" % (c[0] + c[1]))
def test_scaled_pack_equals_resize_then_pack_and_numpy_bit_for_bit(cuda, case, kind):
    (Hs, Ws), (Hd, Wd) = case
    _, _, dtype, y_cs = KINDS[kind]
    frames = np.random.default_rng(Hs * 100 + Ws).integers(0, 256, (5, Hs, Ws, 3), dtype=np.uint8)
    frames[3], frames[4] = 255, 0                        # the clamp of the fixed-point path, both ends
    buf, addrs = _frame_buffer(frames, cuda)
    B = len(ORDER)
    table = _table(addrs[ORDER], cuda)
    got = _scaled(kind, table, B, Hs, Ws, Hd, Wd, cuda)
    want = _composed(kind, table, B, Hs, Ws, Hd, Wd, cuda)
    assert bool(torch.isnan(got[0]).all()) and bool(torch.isnan(got[B + 1]).all()), "a guard band was written"
    assert torch.equal(_bits(got), _bits(want)), "differs from resize_rows + pack_rows at %s" % (
        torch.nonzero(_bits(got) != _bits(want))[0].tolist(),)
    small = np.stack([resize_ref.resize_linear_u8(frames[i], (Wd, Hd)) for i in ORDER])
    ref = torch.zeros((B, Hd, Wd, y_cs), dtype=torch.float32)
    ref[..., :3] = s3fd_ref.preprocess(small).permute(0, 2, 3, 1)            # channels-last, pad channels zero
    ref = ref.to(dtype)
    assert torch.equal(_bits(got[1:B + 1].cpu()), _bits(ref)), "differs from the numpy oracle at %s" % (
        torch.nonzero(_bits(got[1:B + 1].cpu()) != _bits(ref))[0].tolist(),)
    del buf


# ---------------------------------------------------------------- 2. a second grid-stride trip
@pytest.mark.parametrize("kind", list(KINDS))
def test_scaled_pack_second_grid_stride_trip(cuda, kind):
    """513 lines of 512 items (511 full, one of 3 pixels): 512 items more than the 1024 workgroups of 256 hold in one pass;
    k = 2 on odd sizes, so the bilinear path; generated and compared on the device"""
    Hs, Ws, Hd, Wd = 1027, 4095, 513, 2047
    assert Hd * ((Wd + 3) // 4) > GRID_CAP * 256
    gen = torch.Generator(device=cuda).manual_seed(8)
    src = torch.randint(0, 256, (Hs * Ws * 3 + 16,), dtype=torch.uint8, device=cuda, generator=gen)
    table = _table([src.data_ptr() + 3, src.data_ptr() + 3], cuda)
    got = _scaled(kind, table, 2, Hs, Ws, Hd, Wd, cuda)
    want = _composed(kind, table, 2, Hs, Ws, Hd, Wd, cuda)
    nbad = int((_bits(got) != _bits(want)).sum())
    assert nbad == 0, "%d values differ, first at %s" % (nbad, torch.nonzero(_bits(got) != _bits(want))[0].tolist())
    assert not bool(torch.isnan(got[1:3].float()).any()) and bool(torch.isnan(got[0]).all()) and bool(torch.isnan(got[3]).all())
    del src, got, want
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 3. bad arguments
@pytest.mark.parametrize("kind", list(KINDS))
def test_scaled_pack_refuses_bad_arguments_and_writes_nothing(cuda, kind):
    lib, s, ptr = _lib3()
    fused, _, dtype, y_cs = KINDS[kind]
    fn = getattr(lib, fused)
    Hs, Ws, Hd, Wd = 12, 16, 6, 8
    frames = torch.zeros((2, Hs, Ws, 3), dtype=torch.uint8, device=cuda)
    table = _table(frames.data_ptr() + np.arange(3, dtype=np.int64) % 2 * (Hs * Ws * 3), cuda)
    y = _nan_dest(2, Hd, Wd, y_cs, dtype, cuda)
    yp, tp = y[1].data_ptr(), table.data_ptr()
    good = (s, 2, Hs, Ws, Hd, Wd, tp, yp, y_cs)
    bad = {"NULL table": good[:6] + (None,) + good[7:], "NULL y": good[:7] + (None, y_cs),
           "B = 0": (s, 0) + good[2:], "B = 65536": (s, 65536) + good[2:],
           "Hs = 0": (s, 2, 0) + good[3:], "Ws = 0": good[:3] + (0,) + good[4:], "Hd = 0": good[:4] + (0,) + good[5:],
           "Wd = 0": good[:5] + (0,) + good[6:], "table not 8-byte aligned": good[:6] + (tp + 4,) + good[7:],
           "y_cs": good[:8] + ({"fp32": 3, "bf16": 4}[kind],)}
    for what, a in bad.items():
        assert fn(*a) != 0, "%s was accepted" % what
        assert lib.w2l_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()), "a refused call wrote"
    assert fn(*good) == 0, lib.w2l_last_error()                       # the same arguments, unbroken, are taken
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y[1:3].float()).any()) and bool(torch.isnan(y[0]).all()) and bool(torch.isnan(y[3]).all())


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_scaled_first_rect_refuses_a_scale_that_is_not_finite_and_positive(cuda, bad):
    lib, s, ptr = _lib3()
    t = torch.tensor([[[1.0, 2.0, 3.0, 4.0, 0.9]]], device=cuda)
    keep = torch.zeros((1, 1), dtype=torch.int32, device=cuda)
    counts = torch.ones((1,), dtype=torch.int32, device=cuda)
    out = torch.full((5,), -7, dtype=torch.int32, device=cuda)
    for sx, sy in ((bad, 1.0), (1.0, bad)):
        assert lib.w2l_s3fd_first_rect_scaled(s, 1, 1, ptr(t), ptr(keep), ptr(counts), 0.5, sx, sy, ptr(out), ptr(out[4:])) != 0
    assert lib.w2l_s3fd_first_rect_scaled(s, 1, 1, None, ptr(keep), ptr(counts), 0.5, 1.0, 1.0, ptr(out), ptr(out[4:])) != 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-7] * 5
    assert lib.w2l_s3fd_first_rect_scaled(s, 1, 1, ptr(t), ptr(keep), ptr(counts), 0.5, 2.0, 3.0, ptr(out), ptr(out[4:])) == 0
    assert out.cpu().tolist() == [2, 6, 6, 12, 1]


# ---------------------------------------------------------------- 4. the scaled first-rect
def rule3(v, s):
    """one coordinate: the fp32 product, clipped at 0, truncated as int() does"""
    return int(max(np.float32(v) * np.float32(s), 0))


def _numpy_rects(table, keep, counts, sx, sy):
    """(rect, flag) per image by the rule in numpy; only for tables whose passing rows hold finite coordinates below 2^31"""
    out = []
    for b in range(len(table)):
        hit = [r for r in keep[b, :counts[b]] if table[b, r, 4] > 0.5]
        if not hit:
            out.append(((0, 0, 0, 0), 0))
            continue
        d = table[b, hit[0]]
        out.append(((rule3(d[0], sx), rule3(d[1], sy), rule3(d[2], sx), rule3(d[3], sy)), 1))
    return out


def _device_rects(table, keep, counts, scale, dev):
    first_rects = _s3fd_module().first_rects
    return first_rects(torch.from_numpy(table).to(dev), torch.from_numpy(keep).to(dev), torch.from_numpy(counts).to(dev), 0.5, scale)


def test_scaled_first_rect_on_random_tables(cuda):
    r = np.random.default_rng(4)
    B, P = 3, 64
    xy = r.normal(40, 60, (B, P, 2))
    t = np.concatenate([xy, xy + r.uniform(2, 90, (B, P, 2)), r.uniform(0, 1, (B, P, 1))], axis=2).astype(np.float32)
    t[2, :, 4] *= 0.4                                                    # image 2: no row above the threshold
    keep = np.stack([r.permutation(P) for _ in range(B)]).astype(np.int32)
    counts = np.asarray([P, 17, 30], np.int32)
    plain = _device_rects(t, keep, counts, None, cuda)
    ones = _device_rects(t, keep, counts, (np.float32(1), np.float32(1)), cuda)
    assert plain.tobytes() == ones.tobytes()
    assert plain[:, 4].tolist() == [1, 1, 0]
    for sx, sy in ((np.float32(1.5), np.float32(3.0)), (np.float32(23 / 11), np.float32(19 / 9))):
        got = _device_rects(t, keep, counts, (sx, sy), cuda)
        want = _numpy_rects(t, keep, counts, sx, sy)
        assert [(tuple(int(v) for v in g[:4]), int(g[4])) for g in got] == want, (sx, sy)


def test_scaled_first_rect_hand_placed_rows(cuda):
    P = 8

    def image(row, count=1):
        t = np.zeros((P, 5), np.float32)
        t[:, 4] = 0.1
        t[5] = row
        k = np.zeros(P, np.int32)
        k[0] = 5
        return t, k, count

    rows = [image([-3.5, 2.25, 10.5, 1.2e9, 0.9]),               # 0: a negative coordinate clips to 0; 1.2e9 * 2 >= 2^31
            image([1.0, np.nan, 3.0, 4.0, 0.9]),                  # 1: NaN
            image([1.0, 2.0, np.inf, 4.0, 0.9]),                  # 2: +inf
            image([1.0, 2.0, 3.0, 4.0, 0.4]),                     # 3: no row above the threshold
            image([1.0, 2.0, 3.0, 4.0, 0.9], count=-1),           # 4: counts outside [0, P]
            image([1.0, 2.0, 3.0, 4.0, 0.9], count=P + 1),        # 5: the same, above
            image([-np.inf, -0.0, 7.75, 9.99, 0.9])]              # 6: -inf clips to 0
    t = np.stack([r[0] for r in rows])
    keep = np.stack([r[1] for r in rows])
    counts = np.asarray([r[2] for r in rows], np.int32)
    one = _device_rects(t, keep, counts, (np.float32(1), np.float32(1)), cuda)
    two = _device_rects(t, keep, counts, (np.float32(2), np.float32(2)), cuda)
    assert one[:, 4].tolist() == [1, 2, 2, 0, 2, 2, 1]
    assert two[:, 4].tolist() == [2, 2, 2, 0, 2, 2, 1]
    assert tuple(one[0, :4]) == (0, 2, 10, 1200000000) == (rule3(-3.5, 1), rule3(2.25, 1), rule3(10.5, 1), rule3(1.2e9, 1))
    assert tuple(one[6, :4]) == (0, 0, 7, 9) and tuple(two[6, :4]) == (0, 0, 15, 19)
    for res in (one, two):
        for b in (1, 2, 3, 4, 5):
            assert tuple(res[b, :4]) == (0, 0, 0, 0), b
    assert tuple(two[0, :4]) == (0, 0, 0, 0)
    assert _device_rects(t, keep, counts, None, cuda).tobytes() == one.tobytes()


# ---------------------------------------------------------------- 5. end to end, exact
def _frame_sets():
    """128 x 160 frames from a fixed seed (oracle-checked: see test 6) and the first shape's frames of the filelist golden's clips"""
    return {"seeded": synth.s3fd_frames(seed=2, B=2, H=128, W=160), "filelist": synth.filelist_clips()["c0"][0][:6].copy()}


def _detector(precision, det_scale=None):
    from wav2lip_amd import face_detection as fd
    kw = {} if det_scale is None else {"det_scale": det_scale}
    return fd.FaceAlignment(fd.LandmarksType._2D, device="cuda", state_dict=synth.s3fd_state_dict(), precision=precision, **kw)


def _resized(frames, k):
    H, W = frames.shape[1:3]
    return np.stack([resize_ref.resize_linear_u8(f, (W // k, H // k)) for f in frames])


def _best_rows(fa, frames):
    """per image the first kept table row above 0.5 (float32 [5]) or None, of `fa` run as it is"""
    with torch.no_grad():
        table, keep, counts = fa._candidates(frames)
    table, keep, counts = table.cpu().numpy(), keep.cpu().numpy(), counts.cpu().numpy()
    out = []
    for b in range(len(table)):
        hit = [r for r in keep[b, :counts[b]] if table[b, r, 4] > 0.5]
        out.append(table[b, hit[0]].copy() if hit else None)
    return out


def _mapped(row, sx, sy):
    return None if row is None else (rule3(row[0], sx), rule3(row[1], sy), rule3(row[2], sx), rule3(row[3], sy))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("k", [2, 3])
def test_scaled_detector_equals_a_plain_run_on_host_resized_frames(cuda, k, precision):
    """the network sees bit-equal input through the same launches, so the kept rows are the plain run's and the rects are those
    rows through rule 3, exactly; the graph cache is keyed at the reduced size; rects_for_rows gives the same rects and flags"""
    s3fd = _s3fd_module()
    scaled, plain = _detector(precision, k), _detector(precision, 1)
    found = 0
    for name, frames in _frame_sets().items():
        B, H, W = frames.shape[:3]
        Hd, Wd = H // k, W // k
        sx, sy = np.float32(W / Wd), np.float32(H / Hd)
        small = _resized(frames, k)
        got = scaled.get_detections_for_batch(frames)
        assert list(scaled.face_detector._graphs) == [(B, Hd, Wd, "cuda:0", precision)]
        want = [_mapped(r, sx, sy) for r in _best_rows(plain, small)]
        assert list(plain.face_detector._graphs) == [(B, Hd, Wd, "cuda:0", precision)]
        assert got == want, (name, got, want)
        assert [None if r is None else _mapped(r, 1, 1) for r in _best_rows(plain, small)] == plain.get_detections_for_batch(small)
        found += sum(r is not None for r in got)
        # the scaled detector's own table is the plain one's, bit for bit: detector coordinates, not scaled
        a, b = scaled._candidates(frames)[0], plain._candidates(small)[0]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        # detect_from_batch: boxes multiplied the same way, scores untouched
        for ds, dp in zip(scaled.detect_from_batch(frames), plain.detect_from_batch(small)):
            assert len(ds) == len(dp)
            for x, y in zip(ds, dp):
                assert x[4] == y[4] and x[:4].tobytes() == s3fd.scale_box(y[:4], sx, sy).tobytes()
        # rects_for_rows on the frames where they lie
        dev = torch.from_numpy(frames).to(cuda)
        table = torch.arange(B, dtype=torch.int64, device=cuda) * (H * W * 3) + dev.data_ptr()
        rects = torch.full((B + 2, 4), -7, dtype=torch.int32, device=cuda)
        flags = torch.full((B + 2,), -7, dtype=torch.int32, device=cuda)
        scaled.rects_for_rows(table, B, H, W, rects, flags, 1)
        rects, flags = rects.cpu().numpy(), flags.cpu().numpy()
        assert flags.tolist() == [-7] + [0 if r is None else 1 for r in got] + [-7]
        assert [tuple(int(v) for v in r) for r in rects] == [(-7,) * 4] + [r or (0, 0, 0, 0) for r in got] + [(-7,) * 4]
    if k == 2:
        assert found >= 6, "the seeded detector should find its blocks at half size"


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_scale_one_and_no_argument_are_the_same_detector(cuda, precision):
    frames = _frame_sets()["seeded"]
    one, none = _detector(precision, 1), _detector(precision)
    assert one.det_scale == none.det_scale == 1
    assert one.get_detections_for_batch(frames) == none.get_detections_for_batch(frames)
    assert list(one.face_detector._graphs) == list(none.face_detector._graphs) == [(2, 128, 160, "cuda:0", precision)]
    a, b = one._candidates(frames)[0], none._candidates(frames)[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    dev = torch.from_numpy(frames).to(cuda)
    lv = none.face_detector.dense_boxes(dev, precision=precision)
    lv1 = [t.clone() for t in lv]
    lv2 = one.face_detector.dense_boxes(dev, precision=precision, det_scale=1)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(lv1, lv2))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_detect_many_with_a_scaled_detector_equals_face_detect_per_clip(cuda, precision):
    from wav2lip_amd import face_detection as fd
    from wav2lip_amd.inference import face_detect
    pool = _frame_sets()["filelist"]
    clips = [np.stack([pool[i % 6] for i in range(7)]), np.stack([pool[(i + 2) % 6] for i in range(3)])]
    pads = (0, 10, 0, 0)
    det = _detector(precision, 2)
    got = list(fd.detect_many(det, [fd.DetectJob(i, list(c)) for i, c in enumerate(clips)], pads=pads, T=5, batch_size=4))
    assert [g[0] for g in got] == [0, 1]
    for (_, boxes, error), clip in zip(got, clips):
        try:
            want = np.array([c for _, c in face_detect(list(clip), detector=det, pads=list(pads), nosmooth=False, batch_size=4)],
                            dtype=np.int64).reshape(-1, 4)
            want_error = None
        except ValueError as e:
            want, want_error = None, str(e)
        assert error == want_error
        if want is not None:
            assert boxes.dtype == want.dtype and boxes.tobytes() == want.tobytes()
    assert any(g[1] is not None for g in got)
    # an explicit det_scale on a detector of another scale: a copy with that scale, the passed detector keeps its own
    plain = _detector(precision, 1)
    a = face_detect(list(clips[1]), detector=plain, pads=list(pads), nosmooth=False, batch_size=4, det_scale=2)
    b = face_detect(list(clips[1]), detector=det, pads=list(pads), nosmooth=False, batch_size=4)
    assert [c for _, c in a] == [c for _, c in b] and plain.det_scale == 1


def test_a_reduced_frame_of_exactly_the_minimum_runs_and_one_below_is_refused(cuda):
    s3fd = _s3fd_module()
    assert s3fd.MIN_FRAME == 32
    frames = np.random.default_rng(3).integers(0, 256, (2, 64, 70, 3), dtype=np.uint8)
    for precision in ("f32", "bf16"):
        fa = _detector(precision, 2)
        got = fa.get_detections_for_batch(frames)
        assert len(got) == 2 and list(fa.face_detector._graphs) == [(2, 32, 35, "cuda:0", precision)]
        with pytest.raises(ValueError, match="32 x 32"):
            fa.get_detections_for_batch(frames[:, :63])
        assert list(fa.face_detector._graphs) == [(2, 32, 35, "cuda:0", precision)]


# ---------------------------------------------------------------- 6. against the CPU oracle
def test_scaled_fp32_detector_agrees_with_the_cpu_oracle(cuda):
    """oracle chain (preprocess, s3fd_forward, dense_boxes, detections) on the oracle-resized frames: the detector's best box within
    DENSE_TOL of the oracle's in detector coordinates; the integer rect equal to the oracle's through rule 3 wherever the oracle's
    scaled coordinate is farther than DENSE_TOL * scale from an integer, within 1 elsewhere.  The frames were picked so that at
    most one coordinate in four is of the second kind (asserted on the oracle alone first)."""
    sd = synth.s3fd_state_dict()
    total = near_total = 0
    for k in (2, 3):
        fa = _detector("f32", k)
        for name, frames in _frame_sets().items():
            H, W = frames.shape[1:3]
            Hd, Wd = H // k, W // k
            sx, sy = np.float32(W / Wd), np.float32(H / Hd)
            scale = np.array([sx, sy, sx, sy], np.float32)
            with torch.no_grad():
                dets = s3fd_ref.detections(s3fd_ref.dense_boxes(s3fd_ref.s3fd_forward(sd, s3fd_ref.preprocess(_resized(frames, k)))))
            rows = _best_rows(fa, frames)
            rects = fa.get_detections_for_batch(frames)
            for b, d in enumerate(dets):
                assert (len(d) == 0) == (rows[b] is None) == (rects[b] is None), (k, name, b)
                if len(d) == 0:
                    continue
                ref = np.asarray(d[0][:4], np.float32)
                err = np.abs(rows[b][:4].astype(np.float64) - ref.astype(np.float64)).max()
                print("DET_SCALE_ORACLE k=%d %s[%d] best-box L-inf %.3e" % (k, name, b, err))
                assert err <= DENSE_TOL, (k, name, b, err)
                c = ref * scale
                near = np.abs(c.astype(np.float64) - np.rint(c)) <= DENSE_TOL * scale
                total, near_total = total + 4, near_total + int(near.sum())
                want = [int(max(v, 0)) for v in c]
                for j in range(4):
                    assert abs(rects[b][j] - want[j]) <= (1 if near[j] else 0), (k, name, b, j, rects[b], want)
    assert total >= 32 and 4 * near_total <= total, (total, near_total)
