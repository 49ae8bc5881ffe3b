"""Cases and the independent reference shared by tests/test_frame_cases_cpu.py (the oracle against plain bilinear interpolation)
and tests/test_frame_kernels_gpu.py (the five entry points of csrc/resize.hip).  No fixtures, no tests: numpy only.

`bilinear_f64` is bilinear interpolation in float64 with no fixed point in it and nothing taken from oracle/resize_ref.py:
f = (d + 0.5) (ssize / dsize) - 0.5 clamped to [0, ssize - 1], linear along x, then along y, unrounded.

BOUND = 1.0 grey level, strict, between it and the 11-bit fixed-point path of cv::resize that the oracle and the kernels restate.
The fixed-point path leaves the float64 value by: two coefficient roundings per axis (each coefficient is off by at most
0.5 / 2048, and two of them weigh values up to 255: 255 * 2 * 0.5 / 2048 ~ 0.125 per axis), two truncating shifts (>> 4 of the
horizontal sums, >> 16 of the two vertical products: below 2^-2 of a grey level together) and the final (+ 2) >> 2, at most 0.5.
The sum stays below 1.  The exact 2x2 area path is the bilinear value at half positions rounded once: at most 0.5."""
import numpy as np

BOUND = 1.0
SENT = 0xA5          # sentinel byte of every destination and guard


# ---------------------------------------------------------------- the float64 reference
def _axis_f64(ssize, dsize):
    d = np.arange(dsize, dtype=np.float64)
    f = (d + 0.5) * (float(ssize) / float(dsize)) - 0.5
    f = np.minimum(np.maximum(f, 0.0), float(ssize - 1))
    s0 = np.minimum(np.floor(f).astype(np.int64), ssize - 1)
    s1 = np.minimum(s0 + 1, ssize - 1)
    return s0, s1, f - s0


def bilinear_f64(src, dsize_wh):
    """src [H,W,C] -> float64 [h,w,C]; dsize_wh = (width, height), the order cv2.resize takes"""
    src = np.asarray(src, dtype=np.float64)
    H, W = src.shape[:2]
    w, h = int(dsize_wh[0]), int(dsize_wh[1])
    x0, x1, tx = _axis_f64(W, w)
    y0, y1, ty = _axis_f64(H, h)
    rows = src[:, x0] * (1.0 - tx)[None, :, None] + src[:, x1] * tx[None, :, None]              # [H, w, C]
    return rows[y0] * (1.0 - ty)[:, None, None] + rows[y1] * ty[:, None, None]


def paste_f64(frame, pred, box):
    """float64 frame with the float64 resize of `pred` in the box"""
    y1, y2, x1, x2 = box
    out = np.asarray(frame, dtype=np.float64).copy()
    out[y1:y2, x1:x2] = bilinear_f64(pred, (x2 - x1, y2 - y1))
    return out


def compose_model(src, pred, box):
    """numpy model of w2l_compose_rows_u8: a copy of `src` with the oracle resize of `pred` pasted into the box"""
    from oracle import resize_ref
    y1, y2, x1, x2 = box
    out = np.array(src, dtype=np.uint8, copy=True)
    out[y1:y2, x1:x2] = resize_ref.resize_linear_u8(pred, (x2 - x1, y2 - y1))
    return out


# ---------------------------------------------------------------- images
IMAGE_KINDS = ("random", "checker", "ramp")


def image(kind, H, W, seed=0):
    """uint8 [H,W,3].  checker: a 1-pixel checkerboard (a one-pixel shift inverts it); ramp: a horizontal ramp over the full range,
    the channels offset against each other"""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "checker":
        c = ((x + y) & 1) * 255
        return np.stack([c, 255 - c, c], axis=-1).astype(np.uint8)
    if kind == "ramp":
        r = (x * 255) // max(W - 1, 1)
        return np.stack([r, 255 - r, (r + 128 * (y & 1)) % 256], axis=-1).astype(np.uint8)
    raise ValueError(kind)


def vramp(H, W):
    """a vertical ramp (the transpose of `ramp`'s first channel)"""
    y = np.arange(H)[:, None, None]
    return np.broadcast_to((y * 255) // max(H - 1, 1), (H, W, 3)).astype(np.uint8)


# ---------------------------------------------------------------- size pairs (id, Hs, Ws, Hd, Wd)
SIZE_PAIRS = [
    ("identity", 50, 70, 50, 70),
    ("identity_1x1", 1, 1, 1, 1),
    ("area_2x", 192, 192, 96, 96),
    ("area_2x_odd_dst", 100, 142, 50, 71),
    ("area_2x2_to_1x1", 2, 2, 1, 1),
    ("2x_rows_only_190", 192, 190, 96, 96),          # 2x in one axis only: the general path
    ("2x_rows_only", 192, 96, 96, 96),
    ("2x_cols_only", 96, 192, 96, 96),
    ("4x", 96, 96, 24, 24),                          # general path, not area
    ("4x_big", 260, 328, 65, 82),
    ("3x", 96, 96, 32, 32),
    ("3x_floor", 97, 131, 32, 43),                   # h // 3, w // 3
    ("half_floor", 97, 131, 48, 65),                 # h // 2, w // 2 of odd sizes
    ("quarter_floor", 97, 131, 24, 32),
    ("up_by_one", 96, 96, 97, 97),
    ("up_300", 96, 96, 300, 300),
    ("up_2x", 5, 7, 10, 14),
    ("1x1_to_96", 1, 1, 96, 96),
    ("1x1_to_7", 1, 1, 7, 7),
    ("1xN", 1, 37, 96, 96),
    ("Nx1", 37, 1, 96, 96),
    ("2x3_to_96", 2, 3, 96, 96),
    ("2x3_to_7x5", 2, 3, 7, 5),
    ("to_1x1", 97, 131, 1, 1),
    ("to_1xN", 40, 131, 1, 60),
    ("to_Nx1", 97, 50, 60, 1),
    ("strong_down", 250, 3, 96, 96),
    ("down_up_mixed", 130, 20, 33, 77),
]
STRIDE_PAIR = ("stride_520", 130, 130, 520, 520)     # Hd * Wd > 1024 * 256: the grid-stride loop of w2l_resize_u8 goes round again
RESIZE_FACTORS = (2, 3, 4)
RESIZE_FACTOR_FRAME = (97, 131)


def expected_path(Hs, Ws, Hd, Wd):
    """which of resize_px's three paths the pair takes"""
    if (Hs, Ws) == (Hd, Wd):
        return "copy"
    if Hs == 2 * Hd and Ws == 2 * Wd:
        return "area"
    return "general"


# ---------------------------------------------------------------- crop boxes
FRAME_ODD = (260, 131)        # W odd: rows are 393 bytes, no row but the first starts 4-byte aligned
FRAME_EVEN = (260, 330)
CROP_S = (1, 7, 96, 130, 192)     # 130 * 130 > 64 * 256 threads: the grid-stride loop of the crop goes round again (and for 192)


def crop_boxes(H, W, S):
    """[(id, (y1, y2, x1, x2))] on an H x W frame for an S x S result; the sizes that need 2S or S pixels are left out where the
    frame is smaller than that (`crop_table` asserts that each of them appears on one of the two frames where 260 x 330 allows)"""
    bh, bw = min(41, H), min(53, W)
    out = [("top_left", (0, bh, 0, bw)), ("top_right", (0, bh, W - bw, W)), ("bottom_left", (H - bh, H, 0, bw)),
           ("bottom_right", (H - bh, H, W - bw, W)), ("full", (0, H, 0, W)),
           ("last_col", (H // 3, H // 3 + 50, W - 1, W)), ("last_row", (H - 1, H, W // 4, W // 4 + 50)),
           ("last_pixel", (H - 1, H, W - 1, W)), ("first_pixel", (0, 1, 0, 1)), ("inner_general", (7, 50, 3, 61))]
    if S <= H and S <= W:
        out += [("S_top_left", (0, S, 0, S)), ("S_bottom_right", (H - S, H, W - S, W))]
    if 2 * S <= H and 2 * S <= W:
        out += [("2S_top_left", (0, 2 * S, 0, 2 * S)), ("2S_bottom_right", (H - 2 * S, H, W - 2 * S, W))]
    if 2 * S <= H and S <= W:
        out.append(("2S_rows_only", (H - 2 * S, H, W - S, W)))
    if S <= H and 2 * S <= W:
        out.append(("2S_cols_only", (H - S, H, W - 2 * S, W)))
    if S % 2 == 0 and S // 2 <= min(H, W):
        out.append(("half_S", (1, 1 + S // 2, 2, 2 + S // 2)))                # a 2x up-scale: general
    return out


def crop_table(S):
    """{frame shape: boxes}; every size class the frames have room for is present"""
    t = {f: crop_boxes(f[0], f[1], S) for f in (FRAME_ODD, FRAME_EVEN)}
    ids = {i for boxes in t.values() for i, _ in boxes}
    need = {"S_top_left"}
    if 2 * S <= 260:
        need |= {"2S_rows_only", "2S_cols_only", "2S_top_left"}
    assert need <= ids, (S, need - ids)
    return t


# ---------------------------------------------------------------- paste boxes (prediction S = 96 -> box)
PASTE_S = 96


def paste_boxes(H, W):
    """[(id, box)]: the crop table at S = 96 plus the three path selections of the paste direction by name"""
    out = crop_boxes(H, W, PASTE_S)
    out += [("copy_96", (3, 99, 5, 101)), ("area_48", (100, 148, 7, 55)), ("general_48x47", (150, 198, 9, 56))]
    return out


BIG_BOX = (0, 260, 0, 260)        # 67 600 pixels on FRAME_EVEN: above the 256 x 256 threads the paste launches at most


# ---------------------------------------------------------------- compose rows
def _mod4_heights(base):
    """four consecutive heights: H * W mod 4 takes every value the width allows (all four for an odd W)"""
    return [base + k for k in range(4)]


# alignment modes: (source offset, destination offset) from a 16-byte boundary, None = in place at the source offset
ALIGN_MODES = [(0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0), (1, 2), (0, None), (1, None),
               (2, None), (3, None)]
COMPOSE_WIDTHS = (1, 2, 3, 4, 5, 8, 131, 150)


def compose_sweep():
    """rows (id, H, W, box, source offset, destination offset or None) for one launch at S = COMPOSE_SWEEP_S: every width, four
    heights each (H * W mod 4 takes every value the width allows), boxes at column 0, ending at column W and over the full frame,
    every alignment mode"""
    rows = []
    for W in COMPOSE_WIDTHS:
        for H in _mod4_heights(5 if W > 5 else 1):
            boxes = [("col0", (0, max(1, H - 1), 0, max(1, W // 3))), ("to_W", (H // 2, H, W - max(1, W // 3), W)), ("full", (0, H, 0, W))]
            for name, box in boxes:
                for so, do in ALIGN_MODES:
                    rows.append(("W%d_H%d_%s_s%d_d%s" % (W, H, name, so, "ip" if do is None else do), H, W, box, so, do))
    return rows


COMPOSE_SWEEP_S = 16


def compose_group_edges():
    """rows for the group arithmetic: on W = 131 and W = 150 frame row 1 starts inside a group (131 mod 4 = 3, 150 mod 4 = 2), so
    the group that holds the row's first pixels wraps the row end.  A 1x1 box at every x1 mod 4 there and in the last columns, a
    two-column box whose first column is the last pixel of a group and whose last column is the first of the next, the same over
    several rows, boxes that end or start exactly at the wrapping group, on both out-of-place alignments and in place"""
    rows = []
    for W in (131, 150, 8, 5):
        H = 4
        boxes = []
        for y in (1, 2):
            for x in sorted(set(range(0, min(8, W))) | set(range(max(0, W - 5), W))):
                boxes.append(("px_y%d_x%d" % (y, x), (y, y + 1, x, x + 1)))
            xs = [x for x in range(W - 1) if (y * W + x) % 4 == 3]
            for x in sorted({xs[0], xs[len(xs) // 2], xs[-1]}):
                boxes.append(("straddle_y%d_x%d" % (y, x), (y, y + 1, x, x + 2)))
        x = [x for x in range(W - 1) if (W + x) % 4 == 3][0]
        boxes += [("straddle_rows_x%d" % x, (0, H, x, x + 2)), ("row_start", (1, 3, 0, 1)), ("row_end", (0, 3, W - 1, W)),
                  ("one_row_full", (1, 2, 0, W)), ("last_row", (H - 1, H, 0, W)), ("first_row_tail", (0, 1, W - 2, W))]
        for name, box in boxes:
            for so, do in ((0, 0), (1, 3), (0, None), (2, None)):
                rows.append(("W%d_%s_s%d_d%s" % (W, name, so, "ip" if do is None else do), H, W, box, so, do))
    return rows


def compose_mixed_shapes():
    """rows of different frame shapes for one launch at S = 96: the three path selections, all four edges, odd and even widths"""
    shapes = {"a": (120, 150), "b": (97, 131), "c": (200, 210), "d": (3, 2), "e": (1, 7)}
    rows = [("a_general", "a", (10, 100, 20, 130), 0, 0), ("b_full", "b", (0, 97, 0, 131), 1, 2), ("c_area", "c", (4, 196, 10, 202), 0, 3),
            ("a_full", "a", (0, 120, 0, 150), 2, 2), ("b_general", "b", (1, 96, 5, 60), 3, 0), ("a_corner", "a", (24, 120, 54, 150), 0, None),
            ("c_copy", "c", (100, 196, 0, 96), 1, None), ("b_corner", "b", (50, 97, 100, 131), 0, 0), ("a_copy", "a", (0, 96, 0, 96), 0, 1),
            ("c_thin", "c", (0, 200, 0, 1), 0, 0), ("d_full", "d", (0, 3, 0, 2), 0, 0), ("d_px", "d", (1, 2, 1, 2), 3, None),
            ("e_mid", "e", (0, 1, 3, 5), 1, 1), ("a_area_48", "a", (60, 108, 100, 148), 0, None), ("b_48x47", "b", (40, 88, 80, 127), 2, 1)]
    return [(i, shapes[s][0], shapes[s][1], box, so, do) for i, s, box, so, do in rows]


def check_rows(rows):
    """the host precondition of every table here: non-empty boxes inside their frames"""
    for r in rows:
        H, W, (y1, y2, x1, x2) = r[1], r[2], r[3]
        assert 0 <= y1 < y2 <= H and 0 <= x1 < x2 <= W, r
    assert len({r[0] for r in rows}) == len(rows)
    return rows


def diff_message(case, got, want):
    """the failure message of a byte comparison: the case, the number of differing bytes, the first of them"""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want)
    first = tuple(int(v) for v in bad[0]) if len(bad) else None
    return "%s: %d of %d bytes differ, first at %s (got %s, want %s)" % (
        case, len(bad), want.size, first, None if first is None else int(got[first]), None if first is None else int(want[first]))
