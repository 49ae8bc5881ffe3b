"""The five image kernels of csrc/resize.hip (w2l_resize_u8, w2l_crop_resize_u8, w2l_resize_paste_u8, w2l_crop_resize_rows_u8,
w2l_compose_rows_u8) at their edges.  Every comparison makes two checks: byte equality with oracle/resize_ref.py, and strictly
less than one grey level from the float64 bilinear interpolation of tests/_frame_cases.py, which is written without the oracle
(tests/test_frame_cases_cpu.py holds the oracle itself to that bound).  Destinations are carved from larger buffers whose other
bytes must come back unchanged.  Boxes are non-empty and inside their frames throughout: that is the callers' precondition
(include/w2l_hip.h), and no kernel is handed anything else."""
import functools

import numpy as np
import pytest
import torch

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


class Guarded:
    """a device byte buffer of `nbytes` at `offset` bytes past a 16-byte boundary, GUARD random bytes either side of it"""

    def __init__(self, cuda, nbytes, fill=FC.SENT, offset=0, seed=99):
        self.host = np.random.default_rng(seed).integers(0, 256, GUARD + offset + nbytes + GUARD, dtype=np.uint8)
        self.lo, self.hi = GUARD + offset, GUARD + offset + nbytes
        if fill is not None:
            self.host[self.lo:self.hi] = fill
        self.dev = _up(self.host, cuda)
        assert self.dev.data_ptr() % 16 == 0
        self.body = self.dev[self.lo:self.hi]

    def read(self, case):
        """the body as numpy, after checking that the guards are as they were"""
        got = self.dev.cpu().numpy()
        assert np.array_equal(got[:self.lo], self.host[:self.lo]), "%s: bytes before the destination changed" % (case,)
        assert np.array_equal(got[self.hi:], self.host[self.hi:]), "%s: bytes after the destination changed" % (case,)
        return got[self.lo:self.hi]

    def untouched(self, case):
        assert np.array_equal(self.dev.cpu().numpy(), self.host), "%s: the destination was written" % (case,)


def _check_both(case, got, oracle, f64):
    got = np.asarray(got).reshape(oracle.shape)
    assert np.array_equal(got, oracle), FC.diff_message(case, got, oracle)
    d = np.abs(got.astype(np.float64) - f64)
    assert d.max() < FC.BOUND, "%s: %.4f from float64 bilinear at %s (%d values at or above %.1f)" % (
        case, d.max(), np.unravel_index(d.argmax(), d.shape), int((d >= FC.BOUND).sum()), FC.BOUND)


# ---------------------------------------------------------------- w2l_resize_u8
@functools.lru_cache(maxsize=None)
def _resize_refs(name, Hs, Ws, Hd, Wd):
    """three source images (one of each kind) with their oracle and float64 resizes, computed once per size pair"""
    src = np.stack([FC.image(k, Hs, Ws, seed=17) for k in FC.IMAGE_KINDS])
    src.setflags(write=False)
    return src, np.stack([resize_ref.resize_linear_u8(s, (Wd, Hd)) for s in src]), np.stack([FC.bilinear_f64(s, (Wd, Hd)) for s in src])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", FC.SIZE_PAIRS + [FC.STRIDE_PAIR], ids=lambda c: c[0])
def test_resize_u8_equals_the_oracle_and_float64_bilinear(cuda, case, B):
    lib, s, ptr = _lib3()
    name, Hs, Ws, Hd, Wd = case
    pick = slice(1, 2) if B == 1 else slice(0, 3)           # B = 1: the checkerboard alone (a one-pixel shift inverts it)
    src, want, f64 = (a[pick] for a in _resize_refs(*case))
    dst = Guarded(cuda, B * Hd * Wd * 3, offset=B)          # the destination need not be aligned
    x = _up(src, cuda)
    assert lib.w2l_resize_u8(s, B, ptr(x), Hs, Ws, ptr(dst.body), Hd, Wd) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    _check_both("resize %s %dx%d -> %dx%d (%s) B=%d" % (name, Hs, Ws, Hd, Wd, FC.expected_path(Hs, Ws, Hd, Wd), B),
                dst.read(name), want, f64)


@pytest.mark.parametrize("factor", FC.RESIZE_FACTORS)
def test_resize_frames_u8_is_the_resize_factor_step(cuda, factor):
    from wav2lip_amd import inference
    H, W = FC.RESIZE_FACTOR_FRAME
    frames = [FC.image(k, H, W, seed=23 + factor) for k in FC.IMAGE_KINDS]
    got = inference.resize_frames_u8(frames, (W // factor, H // factor))
    assert len(got) == len(frames)
    for k, (g, f) in enumerate(zip(got, frames)):
        assert g.shape == (H // factor, W // factor, 3) and g.dtype == np.uint8
        _check_both("resize_factor %d frame %d" % (factor, k), g, resize_ref.resize_linear_u8(f, (W // factor, H // factor)),
                    FC.bilinear_f64(f, (W // factor, H // factor)))


def test_resize_frames_u8_refuses_an_empty_target(cuda):
    from wav2lip_amd import inference
    frames = [FC.image("random", 3, 5)]
    for wh in ((0, 4), (4, 0), (5 // 8, 3 // 8), (-1, 2)):
        with pytest.raises(ValueError, match="empty"):
            inference.resize_frames_u8(frames, wh)


def test_resize_u8_reports_argument_errors(cuda):
    lib, s, ptr = _lib3()
    x = _up(FC.image("random", 6, 9), cuda)
    dst = Guarded(cuda, 3 * 4 * 5 * 3)
    o = dst.body
    bad = {"no source": (1, None, 6, 9, ptr(o), 4, 5), "no destination": (1, ptr(x), 6, 9, None, 4, 5),
           "B = 0": (0, ptr(x), 6, 9, ptr(o), 4, 5), "B = -1": (-1, ptr(x), 6, 9, ptr(o), 4, 5),
           "B = 65536": (65536, ptr(x), 6, 9, ptr(o), 4, 5), "Hs = 0": (1, ptr(x), 0, 9, ptr(o), 4, 5),
           "Ws = 0": (1, ptr(x), 6, 0, ptr(o), 4, 5), "Hd = 0": (1, ptr(x), 6, 9, ptr(o), 0, 5),
           "Wd = 0": (1, ptr(x), 6, 9, ptr(o), 4, 0), "Wd < 0": (1, ptr(x), 6, 9, ptr(o), 4, -5),
           "Hd * Wd = 2^31": (1, ptr(x), 6, 9, ptr(o), 1 << 16, 1 << 15)}
    for name, args in bad.items():
        assert lib.w2l_resize_u8(s, *args) != 0, name
        assert lib.w2l_last_error(), name
    torch.cuda.synchronize()
    dst.untouched("w2l_resize_u8 argument errors")
    assert lib.w2l_resize_u8(s, 1, ptr(x), 6, 9, ptr(o), 4, 5) == 0                      # and the good call still runs
    torch.cuda.synchronize()
    assert np.array_equal(dst.read("good")[:60].reshape(4, 5, 3), resize_ref.resize_linear_u8(x.cpu().numpy(), (5, 4)))


# ---------------------------------------------------------------- w2l_crop_resize_u8
N_CROP_FRAMES = 3


@functools.lru_cache(maxsize=None)
def _crop_frames(H, W):
    f = np.stack([FC.image(k, H, W, seed=31) for k in FC.IMAGE_KINDS])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _crop_ref(H, W, fi, box, S):
    face = _crop_frames(H, W)[fi][box[0]:box[1], box[2]:box[3]]
    return resize_ref.crop_resize(_crop_frames(H, W)[fi], box, S), FC.bilinear_f64(face, (S, S))


@pytest.mark.parametrize("frame", [FC.FRAME_ODD, FC.FRAME_EVEN], ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("S", FC.CROP_S)
def test_crop_resize_u8_box_table(cuda, S, frame):
    """every box at every S with frame_idx NULL (box b reads frame b), a permutation, and one frame named by several boxes"""
    lib, s, ptr = _lib3()
    H, W = frame
    boxes = FC.crop_table(S)[frame]
    n = len(boxes)
    rng = np.random.default_rng(S)
    stack = _crop_frames(H, W)
    modes = {"NULL": list(range(n)), "permutation": [int(v) for v in rng.permutation(n)], "shared": [b % 2 for b in range(n)]}
    pics = [j % N_CROP_FRAMES for j in range(n)]          # frame j of the launch is picture pics[j]; NULL needs one frame per box
    frames = _up(stack[pics], cuda)
    for mode, idx in modes.items():
        out = Guarded(cuda, n * S * S * 3, offset=n % 4)
        bd = _i32([b for _, b in boxes], cuda)
        idd = None if mode == "NULL" else _i32(idx, cuda)
        assert lib.w2l_crop_resize_u8(s, n, ptr(frames), H, W, ptr(idd), ptr(bd), S, ptr(out.body)) == 0, lib.w2l_last_error()
        torch.cuda.synchronize()
        got = out.read((mode, S, frame)).reshape(n, S, S, 3)
        for b, (name, box) in enumerate(boxes):
            want, f64 = _crop_ref(H, W, pics[idx[b]], box, S)
            _check_both("crop %s box %s %s S=%d frame %dx%d frame_idx %s" % (name, box, FC.expected_path(
                box[1] - box[0], box[3] - box[2], S, S), S, H, W, mode), got[b], want, f64)


@pytest.mark.parametrize("S", [7, 130])
def test_crop_resize_u8_writes_its_own_output_rows_only(cuda, S):
    lib, s, ptr = _lib3()
    H, W = FC.FRAME_ODD
    frames = _up(_crop_frames(H, W)[:1], cuda)
    for name, box in FC.crop_table(S)[FC.FRAME_ODD][:6]:
        out = Guarded(cuda, 3 * S * S * 3)                                       # B = 1 into the middle slot of three
        mid = out.body[S * S * 3:2 * S * S * 3]
        bd = _i32([box], cuda)
        assert lib.w2l_crop_resize_u8(s, 1, ptr(frames), H, W, None, ptr(bd), S, ptr(mid)) == 0, lib.w2l_last_error()
        torch.cuda.synchronize()
        got = out.read(name).reshape(3, S, S, 3)
        assert (got[0] == FC.SENT).all() and (got[2] == FC.SENT).all(), "%s: a neighbouring output row was written" % name
        _check_both("crop B=1 %s S=%d" % (name, S), got[1], *_crop_ref(H, W, 0, box, S))


def test_crop_resize_u8_reports_argument_errors(cuda):
    lib, s, ptr = _lib3()
    H, W, S = 20, 30, 7
    f = _up(FC.image("random", H, W), cuda)
    table = torch.zeros(16, dtype=torch.int32, device=cuda)
    table[:4] = _i32([0, 10, 0, 10], cuda)
    shifted = torch.zeros(16, dtype=torch.int32, device=cuda)
    shifted[1:5] = _i32([0, 10, 0, 10], cuda)                                    # a valid box 4 bytes past the boundary
    idx = _i32([0], cuda)
    out = Guarded(cuda, 2 * S * S * 3)
    o, b = ptr(out.body), ptr(table)
    assert table.data_ptr() % 16 == 0 and shifted[1:].data_ptr() % 16 == 4
    bad = {"no frames": (1, None, H, W, ptr(idx), b, S, o), "no boxes": (1, ptr(f), H, W, ptr(idx), None, S, o),
           "no output": (1, ptr(f), H, W, ptr(idx), b, S, None), "B = 0": (0, ptr(f), H, W, ptr(idx), b, S, o),
           "B = 65536": (65536, ptr(f), H, W, ptr(idx), b, S, o), "H = 0": (1, ptr(f), 0, W, ptr(idx), b, S, o),
           "W = 0": (1, ptr(f), H, 0, ptr(idx), b, S, o), "S = 0": (1, ptr(f), H, W, ptr(idx), b, 0, o),
           "S < 0": (1, ptr(f), H, W, ptr(idx), b, -7, o), "misaligned boxes": (1, ptr(f), H, W, ptr(idx), ptr(shifted[1:]), S, o)}
    for name, args in bad.items():
        assert lib.w2l_crop_resize_u8(s, *args) != 0, name
    assert b"16-byte" in lib.w2l_last_error()
    torch.cuda.synchronize()
    out.untouched("w2l_crop_resize_u8 argument errors")


# ---------------------------------------------------------------- w2l_resize_paste_u8
def _paste_case(cuda, frame, boxes, idx, n_frames, max_box_pixels, seed, tag):
    """paste b (prediction b resized to box b) goes into frame idx[b] (None: frame b) of n_frames; returns nothing, asserts all"""
    lib, s, ptr = _lib3()
    H, W = frame
    S, n = FC.PASTE_S, len(boxes)
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (n_frames, H, W, 3), dtype=np.uint8)
    pred = np.stack([FC.image(FC.IMAGE_KINDS[b % 3], S, S, seed=seed + b) for b in range(n)])
    buf = Guarded(cuda, frames.size, fill=None, offset=3)
    buf.body.copy_(_up(frames.reshape(-1), cuda))
    buf.host[buf.lo:buf.hi] = frames.reshape(-1)
    bd = _i32([b for _, b in boxes], cuda)
    idd = None if idx is None else _i32(idx, cuda)
    pd = _up(pred, cuda)
    assert lib.w2l_resize_paste_u8(s, n, ptr(pd), S, ptr(bd), ptr(idd), ptr(buf.body), H, W, max_box_pixels) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    got = buf.read(tag).reshape(n_frames, H, W, 3)
    target = list(range(n)) if idx is None else list(idx)
    assert len(set(target)) == n
    for b, (name, box) in enumerate(boxes):
        y1, y2, x1, x2 = box
        case = "paste %s box %s (%s) frame %dx%d -> frame %d, max_box_pixels %d, %s" % (
            name, box, FC.expected_path(S, S, y2 - y1, x2 - x1), H, W, target[b], max_box_pixels, tag)
        g = got[target[b]]
        outside = g.copy()
        outside[y1:y2, x1:x2] = frames[target[b]][y1:y2, x1:x2]
        assert np.array_equal(outside, frames[target[b]]), "%s: %d bytes outside the box changed" % (
            case, int((outside != frames[target[b]]).sum()))
        _check_both(case, g, FC.compose_model(frames[target[b]], pred[b], box), FC.paste_f64(frames[target[b]], pred[b], box))
    for j in set(range(n_frames)) - set(target):
        assert np.array_equal(got[j], frames[j]), "%s: frame %d, which nothing names, changed" % (tag, j)


@pytest.mark.parametrize("frame", [FC.FRAME_ODD, FC.FRAME_EVEN], ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("scatter", [False, True], ids=["frame_idx_NULL", "frame_idx_scatter"])
def test_resize_paste_u8_box_table(cuda, frame, scatter):
    boxes = FC.paste_boxes(*frame)
    paths = {i: FC.expected_path(96, 96, b[1] - b[0], b[3] - b[2]) for i, b in boxes}
    assert (paths["copy_96"], paths["area_48"], paths["general_48x47"]) == ("copy", "area", "general")
    n = len(boxes)
    largest = max((b[1] - b[0]) * (b[3] - b[2]) for _, b in boxes)
    idx = [int(v) for v in np.random.default_rng(8).permutation(n + 2)[:n]] if scatter else None
    assert idx is None or idx != list(range(n))
    _paste_case(cuda, frame, boxes, idx, n + 2, largest, seed=41, tag="box table")


@pytest.mark.parametrize("max_box_pixels", ["largest", 1])
@pytest.mark.parametrize("scatter", [False, True], ids=["frame_idx_NULL", "frame_idx_scatter"])
def test_resize_paste_u8_is_complete_whatever_max_box_pixels_says(cuda, max_box_pixels, scatter):
    """max_box_pixels sizes the launch; the grid-stride loop covers the box whether it is exact, far too small, or capped (a box
    above the 256 x 256 threads the launch has at most)"""
    assert FC.BIG_BOX[1] * FC.BIG_BOX[3] > 65536
    boxes = [("big", FC.BIG_BOX), ("general", (3, 250, 20, 300)), ("area_48", (100, 148, 7, 55)), ("px", (259, 260, 329, 330))]
    largest = max((b[1] - b[0]) * (b[3] - b[2]) for _, b in boxes)
    _paste_case(cuda, FC.FRAME_EVEN, boxes, [4, 0, 2, 1] if scatter else None, 5, largest if max_box_pixels == "largest" else 1,
                seed=43, tag="max_box_pixels")


def test_resize_paste_u8_reports_argument_errors(cuda):
    lib, s, ptr = _lib3()
    H, W, S = 20, 30, 8
    pred = _up(FC.image("random", S, S), cuda)
    table = _i32([[2, 12, 3, 13], [0, 0, 0, 0]], cuda)
    shifted = torch.zeros(16, dtype=torch.int32, device=cuda)
    shifted[2:6] = _i32([2, 12, 3, 13], cuda)
    frames = Guarded(cuda, H * W * 3)
    o, b, p = ptr(frames.body), ptr(table), ptr(pred)
    assert shifted[2:].data_ptr() % 16 == 8
    bad = {"no prediction": (1, None, S, b, None, o, H, W, 100), "no boxes": (1, p, S, None, None, o, H, W, 100),
           "no frames": (1, p, S, b, None, None, H, W, 100), "B = 0": (0, p, S, b, None, o, H, W, 100),
           "B = 65536": (65536, p, S, b, None, o, H, W, 100), "S = 0": (1, p, 0, b, None, o, H, W, 100),
           "H = 0": (1, p, S, b, None, o, 0, W, 100), "W = 0": (1, p, S, b, None, o, H, 0, 100),
           "max_box_pixels = 0": (1, p, S, b, None, o, H, W, 0), "max_box_pixels < 0": (1, p, S, b, None, o, H, W, -4),
           "misaligned boxes": (1, p, S, ptr(shifted[2:]), None, o, H, W, 100)}
    for name, args in bad.items():
        assert lib.w2l_resize_paste_u8(s, *args) != 0, name
    assert b"16-byte" in lib.w2l_last_error()
    torch.cuda.synchronize()
    frames.untouched("w2l_resize_paste_u8 argument errors")


# ---------------------------------------------------------------- w2l_compose_rows_u8 / w2l_crop_resize_rows_u8
def _align16(n):
    return (n + 15) & ~15


def _rows_case(cuda, rows, S, max_frame_pixels, seed, tag):
    """rows (id, H, W, box, source offset, destination offset or None = in place): every frame is carved from one byte buffer at
    its offset past a 16-byte boundary with GUARD random bytes either side; destinations start as the sentinel.  One
    w2l_crop_resize_rows_u8 and one w2l_compose_rows_u8 launch over all rows; the WHOLE buffer is compared with the numpy model,
    so every byte outside the destinations (guards, sources, gaps) must come back as it went in."""
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
    faces = Guarded(cuda, n * S * S * 3, offset=1)
    assert lib.w2l_crop_resize_rows_u8(s, n, ptr(tdev), S, ptr(faces.body)) == 0, lib.w2l_last_error()     # before the paste
    pd = _up(pred, cuda)
    assert lib.w2l_compose_rows_u8(s, n, ptr(pd), S, ptr(tdev), max_frame_pixels) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    got = dev.cpu().numpy()
    got_faces = faces.read(tag).reshape(n, S, S, 3)
    want = host.copy()
    for r, ((name, H, W, box, so, do), (a, d, nb)) in enumerate(zip(rows, place)):
        o = a if d is None else d
        want[o:o + nb] = FC.compose_model(host[a:a + nb].reshape(H, W, 3), pred[r], box).reshape(-1)
    for r, ((name, H, W, box, so, do), (a, d, nb)) in enumerate(zip(rows, place)):
        src = host[a:a + nb].reshape(H, W, 3)
        o = a if d is None else d
        case = "%s row %d %s: frame %dx%d box %s, source at +%d, %s, max_frame_pixels %d" % (
            tag, r, name, H, W, box, so, "in place" if d is None else "destination at +%d" % do, max_frame_pixels)
        assert np.array_equal(got[o - GUARD:o], want[o - GUARD:o]), "%s: the %d bytes before the destination changed" % (case, GUARD)
        assert np.array_equal(got[o + nb:o + nb + GUARD], want[o + nb:o + nb + GUARD]), \
            "%s: the %d bytes after the destination changed" % (case, GUARD)
        _check_both("compose " + case, got[o:o + nb].reshape(H, W, 3), want[o:o + nb].reshape(H, W, 3), FC.paste_f64(src, pred[r], box))
        if d is not None:
            assert np.array_equal(got[a:a + nb], host[a:a + nb]), "%s: the source frame changed" % case
        face = src[box[0]:box[1], box[2]:box[3]]
        _check_both("crop rows " + case, got_faces[r], resize_ref.crop_resize(src, box, S), FC.bilinear_f64(face, (S, S)))
    assert np.array_equal(got, want), FC.diff_message(tag + ": bytes no row owns", got, want)


def test_compose_rows_width_height_alignment_sweep(cuda):
    """widths 1, 2, 3, 4, 5, 8, 131, 150, four heights each (H * W mod 4 = 0, 1, 2, 3), boxes at column 0, ending at column W and
    over the whole frame, every source/destination alignment and in place: the skip, three-dword and per-pixel paths"""
    rows = FC.check_rows(FC.compose_sweep())
    _rows_case(cuda, rows, FC.COMPOSE_SWEEP_S, max(r[1] * r[2] for r in rows), seed=51, tag="sweep")


def test_compose_rows_groups_that_wrap_a_row_end(cuda):
    rows = FC.check_rows(FC.compose_group_edges())
    _rows_case(cuda, rows, FC.COMPOSE_SWEEP_S, max(r[1] * r[2] for r in rows), seed=52, tag="group edges")


@pytest.mark.parametrize("max_frame_pixels", ["largest", 4096, 1])
def test_compose_rows_mixed_shapes_whatever_max_frame_pixels_says(cuda, max_frame_pixels):
    """rows of five frame shapes in one launch at S = 96 (copy, 2x2 area and general boxes).  max_frame_pixels sizes the launch:
    4096 gives 4 workgroups for frames of up to 10 500 groups, 1 gives one workgroup; the grid-stride loop must cover both"""
    rows = FC.check_rows(FC.compose_mixed_shapes())
    largest = max(r[1] * r[2] for r in rows)
    assert largest > 4 * 4096
    _rows_case(cuda, rows, 96, largest if max_frame_pixels == "largest" else max_frame_pixels, seed=53, tag="mixed shapes")


def test_compose_rows_one_row_launches(cuda):
    """B = 1, one launch per row: nothing depends on a neighbour in the table"""
    for k, row in enumerate(FC.compose_mixed_shapes()[:5] + FC.compose_group_edges()[3::97]):
        _rows_case(cuda, [row], 96 if k < 5 else FC.COMPOSE_SWEEP_S, row[1] * row[2], seed=60 + k, tag="B=1")


def test_crop_resize_rows_u8_equals_crop_resize_u8_and_the_oracle(cuda):
    from wav2lip_amd import multiclip
    lib, s, ptr = _lib3()
    for frame in (FC.FRAME_ODD, FC.FRAME_EVEN):
        H, W = frame
        for S in (7, 96, 130):
            boxes = FC.crop_table(S)[frame]
            n = len(boxes)
            pics = [b % N_CROP_FRAMES for b in range(n)]
            frames = _up(_crop_frames(H, W), cuda)
            table = np.zeros(n, multiclip.FRAME_ROW)
            for b, (_, (y1, y2, x1, x2)) in enumerate(boxes):
                table[b] = (frames.data_ptr() + pics[b] * H * W * 3, 0, H, W, y1, y2, x1, x2, (0, 0))
            tdev = _up(table.view(np.uint8), cuda)
            rows_out, one_out = Guarded(cuda, n * S * S * 3, offset=2), Guarded(cuda, n * S * S * 3)
            assert lib.w2l_crop_resize_rows_u8(s, n, ptr(tdev), S, ptr(rows_out.body)) == 0, lib.w2l_last_error()
            idd, bd = _i32(pics, cuda), _i32([b for _, b in boxes], cuda)
            assert lib.w2l_crop_resize_u8(s, n, ptr(frames), H, W, ptr(idd), ptr(bd), S, ptr(one_out.body)) == 0, lib.w2l_last_error()
            torch.cuda.synchronize()
            a, c = rows_out.read("rows").reshape(n, S, S, 3), one_out.read("one video").reshape(n, S, S, 3)
            for b, (name, box) in enumerate(boxes):
                case = "crop rows %s box %s S=%d frame %dx%d" % (name, box, S, H, W)
                assert np.array_equal(a[b], c[b]), FC.diff_message(case + " against w2l_crop_resize_u8", a[b], c[b])
                _check_both(case, a[b], *_crop_ref(H, W, pics[b], box, S))


def test_row_kernels_report_argument_errors_and_write_nothing(cuda):
    from wav2lip_amd import multiclip
    lib, s, ptr = _lib3()
    H, W, S = 12, 10, 8
    src = _up(FC.image("random", H, W), cuda)
    dst = Guarded(cuda, H * W * 3)
    out = Guarded(cuda, S * S * 3)
    pred = _up(FC.image("random", S, S), cuda)
    table = np.zeros(2, multiclip.FRAME_ROW)
    table[0] = (src.data_ptr(), dst.body.data_ptr(), H, W, 2, 9, 1, 8, (0, 0))
    tdev = _up(table.view(np.uint8), cuda)
    shifted = torch.zeros(128, dtype=torch.uint8, device=cuda)
    shifted[8:56] = tdev[:48]
    t, o, p = ptr(tdev), ptr(out.body), ptr(pred)
    for name, args in {"no table": (1, None, S, o), "no output": (1, t, S, None), "B = 0": (0, t, S, o), "B = 65536": (65536, t, S, o),
                       "S = 0": (1, t, 0, o), "misaligned table": (1, ptr(shifted[8:]), S, o)}.items():
        assert lib.w2l_crop_resize_rows_u8(s, *args) != 0, "crop_resize_rows: " + name
    for name, args in {"no prediction": (1, None, S, t, 120), "no table": (1, p, S, None, 120), "B = 0": (0, p, S, t, 120),
                       "B = 65536": (65536, p, S, t, 120), "S = 0": (1, p, 0, t, 120), "max_frame_pixels = 0": (1, p, S, t, 0),
                       "max_frame_pixels > 2^29": (1, p, S, t, (1 << 29) + 1), "misaligned table": (1, p, S, ptr(shifted[8:]), 120)}.items():
        assert lib.w2l_compose_rows_u8(s, *args) != 0, "compose_rows: " + name
    assert b"16-byte" in lib.w2l_last_error()
    torch.cuda.synchronize()
    dst.untouched("w2l_compose_rows_u8 argument errors")
    out.untouched("w2l_crop_resize_rows_u8 argument errors")
