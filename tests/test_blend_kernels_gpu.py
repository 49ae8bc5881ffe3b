"""The two blend entry points of csrc/resize.hip (w2l_resize_blend_u8, w2l_compose_blend_rows_u8) against the numpy model of
tests/_blend_cases.py, byte for byte.  Frames are carved from larger buffers whose other bytes must come back unchanged, and
whole buffers are compared.  Boxes are non-empty and inside their frames throughout (the callers' precondition, include/w2l_hip.h);
no kernel is handed anything else, and no table here holds an invalid address."""
import functools

import numpy as np
import pytest
import torch

import _blend_cases as BC
import _frame_cases as FC
from oracle import resize_ref

pytestmark = pytest.mark.gpu
GUARD = 16


def _lib3():
    from wav2lip_amd import _lib
    return _lib.load(), _lib.current_stream(), _lib.ptr


def _up(a, cuda):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(cuda)


def _i32(rows, cuda):
    return torch.tensor(rows, dtype=torch.int32, device=cuda)


def _align16(n):
    return (n + 15) & ~15


# ---------------------------------------------------------------- w2l_resize_blend_u8
@functools.lru_cache(maxsize=None)
def _paste_inputs(frame, names, n_frames, seed):
    """frames, predictions and every prediction's oracle resize to its box: computed once, shared by every setting"""
    H, W = frame
    boxes = [(n, b) for n, b in FC.paste_boxes(H, W) + [("big", FC.BIG_BOX), ("general_big", (3, 250, 20, 300))] if n in names]
    assert [n for n, _ in boxes] == list(names)
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8)
    pred = np.stack([FC.image(FC.IMAGE_KINDS[b % 3], FC.PASTE_S, FC.PASTE_S, seed=seed + b) for b in range(len(boxes))])
    resized = [resize_ref.resize_linear_u8(pred[b], (box[3] - box[2], box[1] - box[0])) for b, (_, box) in enumerate(boxes)]
    for a in [frames, pred] + resized:
        a.setflags(write=False)
    return boxes, frames, pred, resized


def _paste_launch(cuda, entry, frames, pred, boxes, idx, max_box_pixels, extra):
    """one launch of `entry` into a guarded copy of `frames`; returns the frames as they come back"""
    lib, s, ptr = _lib3()
    n_frames, H, W = frames.shape[:3]
    host = np.random.default_rng(99).integers(0, 256, GUARD + 3 + frames.size + GUARD, dtype=np.uint8)
    lo, hi = GUARD + 3, GUARD + 3 + frames.size
    host[lo:hi] = frames.reshape(-1)
    dev = _up(host, cuda)
    bd = _i32([b for _, b in boxes], cuda)
    idd = None if idx is None else _i32(idx, cuda)
    pd = _up(pred, cuda)
    rc = getattr(lib, entry)(s, len(boxes), ptr(pd), FC.PASTE_S, ptr(bd), ptr(idd), ptr(dev[lo:hi]), H, W, max_box_pixels, *extra)
    assert rc == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[hi:], host[hi:]), "%s: bytes around the frames changed" % entry
    return got[lo:hi].reshape(frames.shape)


def _paste_case(cuda, frame, names, idx, n_frames, max_box_pixels, F, T, seed):
    boxes, frames, pred, resized = _paste_inputs(frame, tuple(names), n_frames, seed)
    target = list(range(len(boxes))) if idx is None else list(idx)
    assert len(set(target)) == len(boxes)
    got = _paste_launch(cuda, "w2l_resize_blend_u8", frames, pred, boxes, idx, max_box_pixels, (F, T))
    want = frames.copy()
    for b, (name, box) in enumerate(boxes):
        want[target[b]] = BC.blend_resized(frames[target[b]], resized[b], box, F, T)
    for b, (name, box) in enumerate(boxes):
        case = "blend paste %s box %s (%s) frame %dx%d -> frame %d, F=%d T=%d, max_box_pixels %d" % (
            name, box, FC.expected_path(96, 96, box[1] - box[0], box[3] - box[2]), frame[0], frame[1], target[b], F, T, max_box_pixels)
        assert np.array_equal(got[target[b]], want[target[b]]), FC.diff_message(case, got[target[b]], want[target[b]])
    assert np.array_equal(got, want), FC.diff_message("frames nothing names", got, want)


@pytest.mark.parametrize("setting", BC.KERNEL_SETTINGS, ids=lambda s: "F%d_T%d" % s)
@pytest.mark.parametrize("frame", [FC.FRAME_ODD, FC.FRAME_EVEN], ids=lambda f: "%dx%d" % f)
def test_resize_blend_u8_box_table(cuda, frame, setting):
    """all of paste_boxes in one launch: the 1x1 boxes, the one-column and one-row boxes, the copy, area and general paths; the odd
    frame through frame_idx = NULL, the even one scattered"""
    boxes = FC.paste_boxes(*frame)
    paths = {i: FC.expected_path(96, 96, b[1] - b[0], b[3] - b[2]) for i, b in boxes}
    assert (paths["copy_96"], paths["area_48"], paths["general_48x47"]) == ("copy", "area", "general")
    assert {"last_col", "last_row", "last_pixel", "first_pixel"} <= set(paths)
    n = len(boxes)
    largest = max((b[1] - b[0]) * (b[3] - b[2]) for _, b in boxes)
    idx = [int(v) for v in np.random.default_rng(8).permutation(n + 2)[:n]] if frame == FC.FRAME_EVEN else None
    _paste_case(cuda, frame, [i for i, _ in boxes], idx, n + 2, largest, setting[0], setting[1], seed=41)


@pytest.mark.parametrize("setting", BC.COMPOSE_SETTINGS, ids=lambda s: "F%d_T%d" % s)
def test_resize_blend_u8_is_complete_when_max_box_pixels_is_understated(cuda, setting):
    """BIG_BOX holds more pixels than the 256 x 256 threads a launch has at most, and max_box_pixels = 1 gives one workgroup:
    the grid-stride loop goes round again"""
    assert FC.BIG_BOX[1] * FC.BIG_BOX[3] > 65536
    names = ["last_pixel", "area_48", "big", "general_big"]
    for mbp in (FC.BIG_BOX[1] * FC.BIG_BOX[3], 1):
        _paste_case(cuda, FC.FRAME_EVEN, names, [4, 0, 2, 1], 5, mbp, setting[0], setting[1], seed=43)


def test_resize_blend_u8_without_feather_or_top_is_resize_paste_u8(cuda):
    for frame in (FC.FRAME_ODD, FC.FRAME_EVEN):
        names = [i for i, _ in FC.paste_boxes(*frame)]
        boxes, frames, pred, _ = _paste_inputs(frame, tuple(names), len(names) + 2, 41)
        largest = max((b[1] - b[0]) * (b[3] - b[2]) for _, b in boxes)
        plain = _paste_launch(cuda, "w2l_resize_paste_u8", frames, pred, boxes, None, largest, ())
        blend = _paste_launch(cuda, "w2l_resize_blend_u8", frames, pred, boxes, None, largest, (0, 0))
        assert np.array_equal(blend, plain), FC.diff_message("F=0 T=0 on %dx%d" % frame, blend, plain)
        assert not np.array_equal(plain, frames)


def test_resize_blend_u8_reports_argument_errors_and_writes_nothing(cuda):
    lib, s, ptr = _lib3()
    H, W, S = 20, 30, 8
    pred = _up(FC.image("random", S, S), cuda)
    table = _i32([[2, 12, 3, 13], [0, 0, 0, 0]], cuda)
    shifted = torch.zeros(16, dtype=torch.int32, device=cuda)
    shifted[2:6] = _i32([2, 12, 3, 13], cuda)
    host = np.full(GUARD + H * W * 3 + GUARD, FC.SENT, np.uint8)
    frames = _up(host, cuda)
    o, b, p = ptr(frames[GUARD:]), ptr(table), ptr(pred)
    assert shifted[2:].data_ptr() % 16 == 8
    bad = {"no prediction": (1, None, S, b, None, o, H, W, 100, 3, 128), "no boxes": (1, p, S, None, None, o, H, W, 100, 3, 128),
           "no frames": (1, p, S, b, None, None, H, W, 100, 3, 128), "B = 0": (0, p, S, b, None, o, H, W, 100, 3, 128),
           "B = 65536": (65536, p, S, b, None, o, H, W, 100, 3, 128), "S = 0": (1, p, 0, b, None, o, H, W, 100, 3, 128),
           "H = 0": (1, p, S, b, None, o, 0, W, 100, 3, 128), "W = 0": (1, p, S, b, None, o, H, 0, 100, 3, 128),
           "max_box_pixels = 0": (1, p, S, b, None, o, H, W, 0, 3, 128),
           "misaligned boxes": (1, p, S, ptr(shifted[2:]), None, o, H, W, 100, 3, 128),
           "feather = -1": (1, p, S, b, None, o, H, W, 100, -1, 128), "feather = 65": (1, p, S, b, None, o, H, W, 100, 65, 128),
           "top_q8 = -1": (1, p, S, b, None, o, H, W, 100, 3, -1), "top_q8 = 256": (1, p, S, b, None, o, H, W, 100, 3, 256)}
    for name, args in bad.items():
        assert lib.w2l_resize_blend_u8(s, *args) != 0, name
    assert b"top_q8" in lib.w2l_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(frames.cpu().numpy(), host), "w2l_resize_blend_u8 wrote on an argument error"
    assert lib.w2l_resize_blend_u8(s, 1, p, S, b, None, o, H, W, 100, 64, 255) == 0, lib.w2l_last_error()      # the limits themselves
    torch.cuda.synchronize()
    got = frames.cpu().numpy()
    assert (got[:GUARD] == FC.SENT).all() and (got[GUARD + H * W * 3:] == FC.SENT).all()


# ---------------------------------------------------------------- w2l_compose_blend_rows_u8
def _rows_launch(cuda, entry, rows, S, max_frame_pixels, seed, extra):
    """rows (id, H, W, box, source offset, destination offset or None = in place), every frame carved from one byte buffer at its
    offset past a 16-byte boundary with GUARD random bytes either side, destinations filled with the sentinel; one launch of
    `entry` over all rows.  Returns (the buffer as it went in, as it came back, the placements, the predictions)."""
    from wav2lip_amd import multiclip
    lib, s, ptr = _lib3()
    n = len(rows)
    rng = np.random.default_rng(seed)
    place, cur = [], 0
    for name, H, W, box, so, do in rows:
        nb = H * W * 3
        a = _align16(cur) + GUARD + so
        cur = a + nb + GUARD
        d = None
        if do is not None:
            d = _align16(cur) + GUARD + do
            cur = d + nb + GUARD
        place.append((a, d, nb))
    host = rng.integers(0, 256, _align16(cur) + GUARD, dtype=np.uint8)
    for a, d, nb in place:
        if d is not None:
            host[d:d + nb] = FC.SENT
    pred = rng.integers(0, 256, (n, S, S, 3), dtype=np.uint8)
    dev = _up(host, cuda)
    base = dev.data_ptr()
    assert base % 16 == 0
    table = np.zeros(n, multiclip.FRAME_ROW)
    for r, ((name, H, W, (y1, y2, x1, x2), so, do), (a, d, nb)) in enumerate(zip(rows, place)):
        table[r] = (base + a, base + (a if d is None else d), H, W, y1, y2, x1, x2, (0, 0))
        assert (base + a) % 16 == so and (d is None or (base + d) % 16 == do)
    tdev = _up(table.view(np.uint8), cuda)
    assert tdev.data_ptr() % 16 == 0
    pd = _up(pred, cuda)
    assert getattr(lib, entry)(s, n, ptr(pd), S, ptr(tdev), max_frame_pixels, *extra) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    return host, dev.cpu().numpy(), place, pred


def _rows_case(cuda, rows, S, max_frame_pixels, F, T, seed, tag):
    host, got, place, pred = _rows_launch(cuda, "w2l_compose_blend_rows_u8", rows, S, max_frame_pixels, seed, (F, T))
    want = host.copy()
    for r, ((name, H, W, box, so, do), (a, d, nb)) in enumerate(zip(rows, place)):
        o = a if d is None else d
        want[o:o + nb] = BC.blend_model(host[a:a + nb].reshape(H, W, 3), pred[r], box, F, T).reshape(-1)
    for r, ((name, H, W, box, so, do), (a, d, nb)) in enumerate(zip(rows, place)):
        o = a if d is None else d
        case = "%s row %d %s: frame %dx%d box %s, source at +%d, %s, F=%d T=%d, max_frame_pixels %d" % (
            tag, r, name, H, W, box, so, "in place" if d is None else "destination at +%d" % do, F, T, max_frame_pixels)
        assert np.array_equal(got[o:o + nb], want[o:o + nb]), FC.diff_message(case, got[o:o + nb].reshape(H, W, 3), want[o:o + nb].reshape(H, W, 3))
    assert np.array_equal(got, want), FC.diff_message(tag + ": bytes no row owns (guards, sources, gaps)", got, want)


@pytest.mark.parametrize("setting", BC.COMPOSE_SETTINGS, ids=lambda s: "F%d_T%d" % s)
@pytest.mark.parametrize("max_frame_pixels", ["largest", 1])
def test_compose_blend_rows_mixed_shapes(cuda, max_frame_pixels, setting):
    """five frame shapes in one launch at S = 96 (copy, 2x2 area and general boxes), out of place at equal and unequal alignments
    and in place; max_frame_pixels = 1 gives one workgroup, so the grid-stride loop goes round"""
    rows = FC.check_rows(FC.compose_mixed_shapes())
    assert any(r[5] is None for r in rows) and any(r[5] is not None and r[4] != r[5] for r in rows)
    largest = max(r[1] * r[2] for r in rows)
    _rows_case(cuda, rows, 96, largest if max_frame_pixels == "largest" else 1, setting[0], setting[1], seed=53, tag="mixed shapes")


@pytest.mark.parametrize("setting", BC.COMPOSE_SETTINGS, ids=lambda s: "F%d_T%d" % s)
def test_compose_blend_rows_groups_that_wrap_a_row_end(cuda, setting):
    rows = FC.check_rows(FC.compose_group_edges())
    _rows_case(cuda, rows, FC.COMPOSE_SWEEP_S, max(r[1] * r[2] for r in rows), setting[0], setting[1], seed=52, tag="group edges")


@pytest.mark.parametrize("setting", BC.COMPOSE_SETTINGS, ids=lambda s: "F%d_T%d" % s)
def test_compose_blend_rows_width_height_alignment_sweep(cuda, setting):
    """a seventh of compose_sweep(): every width, every alignment mode (in place included) and every box kind stay in"""
    rows = FC.check_rows(BC.thinned_sweep())
    _rows_case(cuda, rows, FC.COMPOSE_SWEEP_S, max(r[1] * r[2] for r in rows), setting[0], setting[1], seed=51, tag="sweep")


def test_compose_blend_rows_without_feather_or_top_is_compose_rows_u8(cuda):
    for rows, S in ((FC.compose_mixed_shapes(), 96), (BC.thinned_sweep(), FC.COMPOSE_SWEEP_S)):
        mfp = max(r[1] * r[2] for r in rows)
        _, plain, _, _ = _rows_launch(cuda, "w2l_compose_rows_u8", rows, S, mfp, 54, ())
        host, blend, _, _ = _rows_launch(cuda, "w2l_compose_blend_rows_u8", rows, S, mfp, 54, (0, 0))
        assert np.array_equal(blend, plain), FC.diff_message("F=0 T=0, S=%d" % S, blend, plain)
        assert not np.array_equal(plain, host)


def test_compose_blend_rows_reports_argument_errors_and_writes_nothing(cuda):
    from wav2lip_amd import multiclip
    lib, s, ptr = _lib3()
    H, W, S = 12, 10, 8
    src = _up(FC.image("random", H, W), cuda)
    host = np.full(GUARD + H * W * 3 + GUARD, FC.SENT, np.uint8)
    dst = _up(host, cuda)
    pred = _up(FC.image("random", S, S), cuda)
    table = np.zeros(2, multiclip.FRAME_ROW)
    table[0] = (src.data_ptr(), dst[GUARD:].data_ptr(), H, W, 2, 9, 1, 8, (0, 0))
    tdev = _up(table.view(np.uint8), cuda)
    shifted = torch.zeros(128, dtype=torch.uint8, device=cuda)
    shifted[8:56] = tdev[:48]
    t, p = ptr(tdev), ptr(pred)
    bad = {"no prediction": (1, None, S, t, 120, 3, 128), "no table": (1, p, S, None, 120, 3, 128), "B = 0": (0, p, S, t, 120, 3, 128),
           "B = 65536": (65536, p, S, t, 120, 3, 128), "S = 0": (1, p, 0, t, 120, 3, 128), "max_frame_pixels = 0": (1, p, S, t, 0, 3, 128),
           "max_frame_pixels > 2^29": (1, p, S, t, (1 << 29) + 1, 3, 128), "misaligned table": (1, p, S, ptr(shifted[8:]), 120, 3, 128),
           "feather = -1": (1, p, S, t, 120, -1, 128), "feather = 65": (1, p, S, t, 120, 65, 128),
           "top_q8 = -1": (1, p, S, t, 120, 3, -1), "top_q8 = 256": (1, p, S, t, 120, 3, 256)}
    for name, args in bad.items():
        assert lib.w2l_compose_blend_rows_u8(s, *args) != 0, name
    assert b"top_q8" in lib.w2l_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), host), "w2l_compose_blend_rows_u8 wrote on an argument error"
    assert lib.w2l_compose_blend_rows_u8(s, 1, p, S, t, 120, 64, 255) == 0, lib.w2l_last_error()               # the limits themselves
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert (got[:GUARD] == FC.SENT).all() and (got[GUARD + H * W * 3:] == FC.SENT).all() and not (got[GUARD:GUARD + H * W * 3] == FC.SENT).all()
