"""The shared pieces of the detection front ends without a device: the layout of the one copy-back buffer (`many.BoxOut`), the one
finish of `inference.face_detect` against the host statements `many.host_boxes` / `host_boxes_runs`, and the halving rule
(`inference.halving`)."""
import numpy as np
import pytest
import torch

from test_noface_cpu import StubDetector

PADS = (3, 10, 5, 7)
SHAPES = ((40, 50), (30, 36))          # rects reach to 70: both shapes clip, each at its own edge


# ---------------------------------------------------------------- the copy-back buffer
@pytest.mark.parametrize("n_seg", [1, 3])
@pytest.mark.parametrize("n_boxes", [0, 1, 5])
@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("hold", [False, True])
def test_box_out_views_tile_the_buffer_in_order_and_split_returns_the_same_parts(hold, track, n_boxes, n_seg):
    from wav2lip_amd.face_detection.many import BoxOut
    out = BoxOut(n_boxes, n_seg, hold, track, "cpu")
    assert out.buffer.dtype == torch.int32 and out.buffer.dim() == 1
    assert (out.valid is None) == (not hold)
    views = [v for v in (out.boxes, out.valid, out.status, out.track_status) if v is not None]
    sizes = [4 * n_boxes] + ([n_boxes] if hold else []) + [2 * n_seg, n_seg if track else 0]
    assert [v.numel() for v in views] == sizes and all(v.dim() == 1 for v in views)
    assert out.boxes.storage_offset() == 0
    at = 0
    for v, n in zip(views, sizes):                     # in order, disjoint, without gaps: each starts where the one before ends
        assert v.storage_offset() == at and out.ptr(v).value == out.buffer.data_ptr() + 4 * at
        at += n
    assert at == out.buffer.numel()                    # and they cover the buffer exactly
    for k, v in enumerate(views):                      # distinct values through the views
        v.copy_(torch.arange(v.numel(), dtype=torch.int32) + 1000 * (k + 1))
    if track:
        out.track_status.zero_()
    boxes, valid, status, track_status = out.split(out.buffer.numpy())
    assert boxes.shape == (n_boxes, 4) and boxes.reshape(-1).tolist() == [1000 + i for i in range(4 * n_boxes)]
    assert (valid is None) == (not hold)
    if hold:
        assert valid.tolist() == [2000 + i for i in range(n_boxes)]
    assert status.shape == (n_seg, 2) and status.reshape(-1).tolist() == [1000 * len(views) - 1000 + i for i in range(2 * n_seg)]
    assert track_status.tolist() == ([0] * n_seg if track else [])
    if track:
        out.track_status[n_seg - 1] = 3
        with pytest.raises(AssertionError, match=r"did not follow a clip's segment \(status \[.*3\]\)"):
            out.split(out.buffer.numpy())
        with pytest.raises(AssertionError, match="did not follow a stream's segment$"):
            out.split(out.buffer.numpy(), of="stream")


# ---------------------------------------------------------------- the one finish of face_detect
def _frame(shape, rect):
    """a frame the StubDetector reads: pixel (0,1) and (0,2) carry the rect, or the "no face" flag for None"""
    f = np.zeros(shape + (3,), np.uint8)
    if rect is None:
        f[0, 2, 1] = 1
    else:
        f[0, 1], f[0, 2, 0] = rect[:3], rect[3]
    f[1:] = np.arange(shape[1] * 3, dtype=np.uint8).reshape(shape[1], 3)       # something to crop
    return f


def _expected(rects, shapes, T, hold):
    """coords per frame (None for a gap frame) from the host statements: one shape -> host_boxes / host_boxes_runs as they
    stand; two shapes -> their padded rows (T = 0) taken per frame shape, then the smoothing of every boxed run"""
    from wav2lip_amd import inference
    from wav2lip_amd.face_detection import many
    if hold is None:
        filled, valid = rects, np.ones(len(rects), bool)
    else:
        filled = many.hold_fill(rects, hold)
        valid = np.array([r is not None for r in filled], bool)
    kinds = sorted(set(shapes))
    if len(kinds) <= 1:
        H, W = kinds[0] if kinds else SHAPES[0]
        if hold is None:
            boxes = many.host_boxes(rects, H, W, PADS, T)
        else:
            boxes, got_valid = many.host_boxes_runs(rects, H, W, PADS, T, hold)
            assert np.array_equal(got_valid, valid)
    else:
        per = {}
        for H, W in kinds:
            per[H, W] = (many.host_boxes(rects, H, W, PADS, 0) if hold is None else many.host_boxes_runs(rects, H, W, PADS, 0, hold)[0])
        boxes = np.array([per[s][i] for i, s in enumerate(shapes)], dtype=np.int64).reshape(-1, 4)
        if T:
            for a, b in many.boxed_runs(valid):
                boxes[a:b] = inference.get_smoothened_boxes(boxes[a:b].copy(), T)
    return [tuple(int(v) for v in b) if ok else None for b, ok in zip(boxes, valid)]


@pytest.mark.parametrize("nosmooth", [False, True])
@pytest.mark.parametrize("hold", [None, 0, 2])
def test_face_detect_is_the_host_statements_for_short_clips_and_two_shapes(hold, nosmooth):
    from wav2lip_amd import inference
    kw = {} if hold is None else {"no_face_hold": hold}
    rng = np.random.default_rng(7 if hold is None else 8 + hold)
    assert inference.face_detect([], detector=StubDetector(), pads=list(PADS), nosmooth=nosmooth, batch_size=3, **kw) == []
    for n in range(1, 7):                                                       # n < 5 takes the wrapped smoothing window
        for mixed in (False, True):
            for trial in range(6):
                rects = [(int(rng.integers(0, 21)), int(rng.integers(0, 16)), int(rng.integers(30, 71)), int(rng.integers(25, 71)))
                         for _ in range(n)]
                if hold is not None:
                    rects = [None if rng.random() < 0.35 else r for r in rects]
                shapes = [SHAPES[int(rng.integers(0, 2))] if mixed else SHAPES[trial % 2] for _ in range(n)]
                frames = [_frame(s, r) for s, r in zip(shapes, rects)]
                batch = 1 if mixed else 3               # a detector batch is one array: frames of two shapes never share one
                if hold is not None and n == 1 and rects[0] is None:            # a single frame without a face stays the error
                    with pytest.raises(ValueError, match="Face not detected"):
                        inference.face_detect(frames, detector=StubDetector(), pads=list(PADS), nosmooth=nosmooth, batch_size=batch, **kw)
                    continue
                det = inference.face_detect(frames, detector=StubDetector(), pads=list(PADS), nosmooth=nosmooth, batch_size=batch, **kw)
                want = _expected(rects, shapes, 0 if nosmooth else 5, hold)
                assert len(det) == n
                for (face, coords), w, f in zip(det, want, frames):
                    if w is None:
                        assert face is None and coords is None
                    else:
                        assert tuple(int(v) for v in coords) == w, (n, rects, shapes)
                        assert np.array_equal(face, f[w[0]:w[1], w[2]:w[3]])
                assert all(np.asarray(c).dtype == np.int64 for _, c in det if c is not None)
    with pytest.raises(ValueError, match="Face not detected! Ensure the video contains a face in all the frames."):
        inference.face_detect([_frame(SHAPES[0], (1, 2, 30, 40)), _frame(SHAPES[0], None)], detector=StubDetector(), pads=list(PADS),
                              nosmooth=nosmooth, batch_size=3)


# ---------------------------------------------------------------- the halving rule
def test_halving_halves_down_to_the_batch_that_runs_and_ends_in_the_references_error(capsys):
    from wav2lip_amd import inference
    tried = []

    def run(batch_size):
        tried.append(batch_size)
        if batch_size > 2:
            raise RuntimeError("out of memory")
        return ("ran", batch_size)

    assert inference.halving(run, 16) == ("ran", 2) and tried == [16, 8, 4, 2]
    assert capsys.readouterr().out.splitlines() == ['Recovering from OOM error; New batch size: %d' % b for b in (8, 4, 2)]

    def never(batch_size):
        tried.append(batch_size)
        raise RuntimeError("out of memory")

    del tried[:]
    with pytest.raises(RuntimeError) as e:
        inference.halving(never, 4)
    assert str(e.value) == 'Image too big to run face detection on GPU. Please use the --resize_factor argument'
    assert tried == [4, 2, 1]
