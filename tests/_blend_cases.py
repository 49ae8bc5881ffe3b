"""The numpy model of the feathered, mouth-region paste (w2l_resize_blend_u8, w2l_compose_blend_rows_u8 in csrc/resize.hip) and
the case tables shared by tests/test_blend_cases_cpu.py, tests/test_blend_kernels_gpu.py and tests/test_blend_product_gpu.py.
No fixtures, no tests: numpy only.  Images and boxes are those of tests/_frame_cases.py.

The arithmetic, integers only.  For a box of h x w pixels, feather F (0..64), top_q8 T (0..255), box-relative row j, column i:
    t0 = (h*T) >> 8;  hr = h - t0 (>= 1);  Fe = min(F, (min(w, hr) - 1) // 2);  D = (Fe+1)^2
    wy(j) = 0 for j < t0, else min(Fe+1, j-t0+1, h-j);  wx(i) = min(Fe+1, i+1, w-i);  a = wx*wy
    out_c = (a*p_c + (D-a)*o_c + D//2) // D
p = oracle.resize_ref.resize_linear_u8 of the prediction (what the plain paste writes), o = the frame's own pixel.

BLEND_BOUND = 1.5 grey levels, strict, between the model and the float64 blend alpha*bilinear_f64 + (1-alpha)*o, alpha = a/D:
the model is x = alpha*p + (1-alpha)*o rounded once, half up (floor(x + 1/2) for the rational x: at most 0.5 away), and x is
alpha*(p - bilinear_f64) away from the float64 blend, with |p - bilinear_f64| < BOUND = 1.0 (tests/_frame_cases.py) and
alpha <= 1: below 1.0.  The sum stays below 1.5."""
import numpy as np

import _frame_cases as FC

BLEND_BOUND = FC.BOUND + 0.5
MAX_FEATHER = 64
# (feather, top_q8) of the kernel tests; (0, 0) is the plain paste
KERNEL_SETTINGS = [(0, 0), (1, 0), (3, 128), (8, 255), (64, 0), (64, 200)]
COMPOSE_SETTINGS = [(3, 128), (64, 0)]
# the model's own cases on the CPU
MODEL_FEATHERS = (1, 3, 8, 64)
MODEL_TOPS = (0, 128, 255)


def effective_feather(h, w, F, T):
    """(t0, Fe) of a box of h x w pixels"""
    t0 = (h * T) >> 8
    hr = h - t0
    assert hr >= 1
    return t0, min(F, (min(w, hr) - 1) // 2)


def weights(h, w, F, T):
    """(a int64 [h, w], D)"""
    t0, Fe = effective_feather(h, w, F, T)
    j, i = np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64)
    wy = np.where(j < t0, 0, np.minimum(Fe + 1, np.minimum(j - t0 + 1, h - j)))
    wx = np.minimum(Fe + 1, np.minimum(i + 1, w - i))
    return wy[:, None] * wx[None, :], (Fe + 1) ** 2


def blend_resized(src, p, box, F, T):
    """a copy of `src` with `p` (uint8 [h, w, 3], the prediction already resized to the box) blended into the box"""
    y1, y2, x1, x2 = box
    a, D = weights(y2 - y1, x2 - x1, F, T)
    out = np.array(src, dtype=np.uint8, copy=True)
    o = out[y1:y2, x1:x2].astype(np.int64)
    num = a[:, :, None] * np.asarray(p, dtype=np.int64) + (D - a)[:, :, None] * o + D // 2
    assert num.max() <= MAX_NUMERATOR
    out[y1:y2, x1:x2] = (num // D).astype(np.uint8)
    return out


def blend_model(src, pred, box, F, T):
    """numpy model of both blend entry points: `src` with the oracle resize of `pred` blended into the box"""
    from oracle import resize_ref
    y1, y2, x1, x2 = box
    return blend_resized(src, resize_ref.resize_linear_u8(pred, (x2 - x1, y2 - y1)), box, F, T)


def blend_f64(src, pred, box, F, T):
    """float64 frame: alpha * bilinear_f64(pred) + (1 - alpha) * o in the box, alpha = a / D"""
    y1, y2, x1, x2 = box
    a, D = weights(y2 - y1, x2 - x1, F, T)
    alpha = (a.astype(np.float64) / D)[:, :, None]
    out = np.asarray(src, dtype=np.float64).copy()
    out[y1:y2, x1:x2] = alpha * FC.bilinear_f64(pred, (x2 - x1, y2 - y1)) + (1.0 - alpha) * out[y1:y2, x1:x2]
    return out


# ---------------------------------------------------------------- the division
MAX_D = (MAX_FEATHER + 1) ** 2
MAX_NUMERATOR = MAX_D * 255 + MAX_D // 2          # 4225 * 255 + 2112


def reciprocal(D):
    """the kernels' multiplier for D >= 2, as they compute it in 32 bits: 0xFFFFFFFF / D + 1 = ceil(2^32 / D)"""
    assert D >= 2
    return 0xFFFFFFFF // D + 1


def divide_by_reciprocal(n, D):
    """the kernels' quotient: the high 32 bits of the 64-bit product n * reciprocal(D)"""
    return (np.asarray(n, dtype=np.uint64) * np.uint64(reciprocal(D))) >> np.uint64(32)


# ---------------------------------------------------------------- compose rows
def thinned_sweep(step=7):
    """every `step`-th row of _frame_cases.compose_sweep(): 7 is coprime to the 15 alignment modes and to the 3 boxes per shape, so
    every mode, every box kind and every width stay in"""
    rows = FC.compose_sweep()[::step]
    modes = {(r[4], r[5]) for r in rows}
    assert modes == set(FC.ALIGN_MODES) and {r[2] for r in rows} == set(FC.COMPOSE_WIDTHS)
    assert {r[0].split("_")[2] for r in rows} == {"col0", "to", "full"}
    return rows
