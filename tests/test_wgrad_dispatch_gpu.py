"""The four weight-gradient paths at training batches and at the edges of their work splits, through the C ABI: the fp32 direct
GEMM with its small-head kernel and its split-operand bf16 variant (csrc/conv_wgrad.hip), the fp32 Winograd kernel
(csrc/conv_wino_wgrad.hip), the bf16 boxes (csrc/wgrad_bf16.hip) and the thin 1x1 kernel (csrc/thin_bf16.hip).

CASE SELECTION.  Nothing is picked by hand: REGIMES names every work-split regime a launcher has, as a predicate over the launcher's
own dry run (w2l_conv_wgrad_resolve / w2l_conv_wgrad_bf16_resolve / w2l_thin1x1_wgrad_blocks: the planning function the launch
itself executes).  The candidates are the layer signatures of test_conv_gpu.SIGS, test_train_gpu.WGRAD_SIGS and WINO_WGRAD_SIGS plus
EXTRA_SIGS (boundary shapes of wino_wgrad_ok and the small head's column limit, which no layer of the models sits on) at
N = 320 and 512, then at the smaller batches of SMALL_N.  A regime takes a case an earlier regime already selected if one fits, else
the cheapest candidate (training batches before small ones, then by operand bytes).  Every test asserts its regime from the dry
run, so a later change of a rule cannot quietly empty a regime; `python tests/test_wgrad_dispatch_gpu.py` prints the table below.

EXACT CHECK.  Operands are integers from {-1, 0, 1} (a third zeros, fixed seed); pad channels are zero as the ABI demands, neighbour
channels of wider buffers hold other integers.  Products and partial sums of such values are integers below 2^24 in magnitude as
long as the reduction length K = N*Hp*Wp is below 2^24 (asserted), so fp32 and bf16 hold every intermediate exactly in ANY
summation order and the result must EQUAL the float64 reference.  No tolerance.  One lost, doubled or shifted pixel is an integer
difference.  Every output buffer is pre-filled with NaN, every case runs twice and must be bit-identical.
  Winograd: the kernel sums U (.) V over 2x2 tiles with U = G g G^T, V = B^T d B and applies A^T . A.  |G| has row sums 1, so
|U| <= 1 in multiples of 1/4; |B^T| has row sums 2, so |V| <= 4 (integers); |A^T| has row sums 3, so an output is bounded by
9 * 4 * (tiles with a non-zero dz pixel) in multiples of 1/4: every intermediate is exact while
    WINO_GROWTH * live tiles < 2^24,   WINO_GROWTH = 9 * 4 * 4 = 144.
A training-size case has more tiles than that, so its dz is split by image index into disjoint masks (image n is live in run
n % masks), one exact run per mask with x dense: every dz pixel and every x pixel is non-zero in at least one exact run.

ACCURACY CHECK.  One run per kernel family with Gaussian operands (bf16-rounded for the bf16 paths) against float64 over the same
operands: L-inf error <= 2e-4 of the gradient's L-inf scale (the project's bound).  torch's own float32 weight gradient of the
same operands is measured against float64 too; were it above a third of 2e-4 the bound would be 3x its distance.

LARGE OFFSETS.  One exact case per launcher with its larger activation buffer between 1 GiB and the 2 GiB guard, data in the first
and the last image; the guard's error return just above 2 GiB (nothing is launched: the dry run must refuse first).

SELECTION TABLE (generated from the dry run; path: f32 = w2l_conv_wgrad_prec fp32, bf16c = the same with W2L_PREC_BF16)
  bf16 several boxes per split, full last split                  bf16  conv 512->512 1x1 s1x1 p0 @1x1 N=512 | ni 16 box 1x1, 32 boxes = 8 splits x 4, tg 1 x 1, ncq 8 mt 2 qp 2
  bf16 several boxes per split, short last split                 bf16  conv 512->512 1x1 s1x1 p0 @1x1 N=320 | ni 16 box 1x1, 20 boxes = 7 splits x 3, tg 1 x 1, ncq 8 mt 2 qp 2
  bf16 last split of exactly one box                             bf16  conv 128->256 3x3 s3x2 p1 @9x6 N=512 | ni 5 box 3x3, 103 boxes = 52 splits x 2, tg 1 x 9, ncq 2 mt 2 qp 2
  bf16 ni > 1, N % ni != 0, several boxes per split              bf16  conv 128->256 3x3 s3x2 p1 @9x6 N=512 | ni 5 box 3x3, 103 boxes = 52 splits x 2, tg 1 x 9, ncq 2 mt 2 qp 2
  bf16 ragged bh and bw, several boxes per split                 bf16  conv 64->64 3x3 s1x1 p1 @37x41 N=320 | ni 1 box 8x14, 4800 boxes = 480 splits x 10, tg 1 x 9, ncq 1 mt 2 qp 2
  bf16 5x5: short last tap group                                 bf16  conv 64->128 5x5 s2x2 p2 @24x24 N=320 | ni 1 box 12x4, 960 boxes = 80 splits x 12, tg 3 x 9, ncq 1 mt 2 qp 2
  bf16 7x7: short last tap group                                 bf16  conv 64->64 7x7 s1x1 p3 @12x12 N=320 | ni 1 box 12x6, 640 boxes = 80 splits x 8, tg 6 x 9, ncq 1 mt 2 qp 2
  bf16 ncq > 1                                                   bf16  conv 512->512 1x1 s1x1 p0 @1x1 N=512 | ni 16 box 1x1, 32 boxes = 8 splits x 4, tg 1 x 1, ncq 8 mt 2 qp 2
  bf16 mt 1 qp 1                                                 bf16  conv 32->3 1x1 s1x1 p0 @10x10 N=320 | ni 1 box 10x10, 320 boxes = 320 splits x 1, tg 1 x 1, ncq 1 mt 1 qp 1
  bf16 mt 1 qp 2                                                 bf16  conv 512->1 1x1 s1x1 p0 @1x1 N=320 | ni 16 box 1x1, 20 boxes = 20 splits x 1, tg 1 x 1, ncq 8 mt 1 qp 2
  bf16 mt 2 qp 1                                                 bf16  conv 32->64 3x3 s3x1 p1 @80x16 N=320 | ni 1 box 9x16, 960 boxes = 480 splits x 2, tg 1 x 9, ncq 1 mt 2 qp 1
  bf16 mt 2 qp 2                                                 bf16  conv 512->512 1x1 s1x1 p0 @1x1 N=512 | ni 16 box 1x1, 32 boxes = 8 splits x 4, tg 1 x 1, ncq 8 mt 2 qp 2
  bf16 stride-2 conv                                             bf16  conv 64->128 5x5 s2x2 p2 @24x24 N=320 | ni 1 box 12x4, 960 boxes = 80 splits x 12, tg 3 x 9, ncq 1 mt 2 qp 2
  bf16 transposed                                                bf16  convT 768->384 3x3 s2x2 p1+1 @3x3 N=320 | ni 5 box 3x3, 64 boxes = 7 splits x 10, tg 1 x 9, ncq 6 mt 2 qp 2
  bf16 one split, many boxes                                     bf16  conv 1024->1024 5x5 s1x1 p2 @6x6 N=320 | ni 3 box 6x6, 107 boxes = 1 splits x 107, tg 3 x 9, ncq 16 mt 2 qp 2
  bf16 operands are slices of wider buffers                      bf16  conv 64->64 3x3 s1x1 p1 @24x24 N=320 cs 160/96 | ni 1 box 24x6, 1280 boxes = 427 splits x 3, tg 1 x 9, ncq 1 mt 2 qp 2
  f32 direct: heuristic picks cfg 0                              f32   conv 512->512 1x1 s1x1 p0 @1x1 N=320 | direct cfg 0, K 320 = 1 x 320 (step 32), reduce 1024
  f32 direct: heuristic picks cfg 1                              f32   conv 47->64 3x3 s1x1 p1 @12x12 N=320 | direct cfg 1, K 46080 = 360 x 128 (step 16), reduce 108
  f32 direct: heuristic picks cfg 2                              f32   conv 64->64 3x3 s1x1 p1 @4x9 N=320 | direct cfg 2, K 11520 = 45 x 256 (step 32), reduce 144
  f32 direct: heuristic picks cfg 3                              f32   conv 6->16 7x7 s1x1 p3 @32x32 N=320 | direct cfg 3, K 327680 = 380 x 864 (step 16), reduce 25
  f32 direct: heuristic picks cfg 4                              f32   conv 1->32 3x3 s1x1 p1 @80x16 N=320 | direct cfg 4, K 409600 = 753 x 544 (step 32), reduce 5
  f32 direct: cfg 0 forced on a 3x3 s1 layer                     f32   conv 256->256 3x3 s1x1 p1 @3x3 N=320 force 0 wino 0 | direct cfg 0, K 2880 = 10 x 288 (step 32), reduce 2304
  f32 direct: cfg 1 forced on a 3x3 s1 layer                     f32   conv 256->256 3x3 s1x1 p1 @3x3 N=320 force 1 wino 0 | direct cfg 1, K 2880 = 20 x 144 (step 16), reduce 2304
  f32 direct: cfg 2 forced on a 3x3 s1 layer                     f32   conv 256->256 3x3 s1x1 p1 @3x3 N=320 force 2 wino 0 | direct cfg 2, K 2880 = 10 x 288 (step 32), reduce 2304
  f32 direct: cfg 3 forced on a 3x3 s1 layer                     f32   conv 80->32 3x3 s1x1 p1 @21x19 N=320 force 3 wino 0 | direct cfg 3, K 127680 = 250 x 512 (step 16), reduce 90
  f32 direct: cfg 4 forced on a 3x3 s1 layer                     f32   conv 80->32 3x3 s1x1 p1 @21x19 N=320 force 4 wino 0 | direct cfg 4, K 127680 = 125 x 1024 (step 32), reduce 90
  f32 direct: cfg 0 forced on a stride-2 layer                   f32   conv 256->512 3x3 s2x2 p1 @6x6 N=320 force 0 wino 1 | direct cfg 0, K 2880 = 7 x 416 (step 32), reduce 4608
  f32 direct: cfg 1 forced on a stride-2 layer                   f32   conv 256->512 3x3 s2x2 p1 @6x6 N=320 force 1 wino 1 | direct cfg 1, K 2880 = 10 x 288 (step 16), reduce 4608
  f32 direct: cfg 2 forced on a stride-2 layer                   f32   conv 256->512 3x3 s2x2 p1 @6x6 N=320 force 2 wino 1 | direct cfg 2, K 2880 = 5 x 576 (step 32), reduce 4608
  f32 direct: cfg 3 forced on a stride-2 layer                   f32   conv 16->32 3x3 s2x2 p1 @32x32 N=320 force 3 wino 1 | direct cfg 3, K 81920 = 640 x 128 (step 16), reduce 18
  f32 direct: cfg 4 forced on a stride-2 layer                   f32   conv 16->32 3x3 s2x2 p1 @32x32 N=320 force 4 wino 1 | direct cfg 4, K 81920 = 320 x 256 (step 32), reduce 18
  f32 direct: ksplit 1                                           f32   conv 512->512 1x1 s1x1 p0 @1x1 N=320 | direct cfg 0, K 320 = 1 x 320 (step 32), reduce 1024
  f32 direct: ksplit > 256                                       f32   conv 47->64 3x3 s1x1 p1 @12x12 N=320 | direct cfg 1, K 46080 = 360 x 128 (step 16), reduce 108
  f32 direct: K % chunk != 0                                     f32   conv 6->16 7x7 s1x1 p3 @32x32 N=320 | direct cfg 3, K 327680 = 380 x 864 (step 16), reduce 25
  f32 direct: K % K-step != 0                                    f32   conv 36->44 3x3 s1x1 p1 @17x30 N=1 | direct cfg 2, K 510 = 1 x 512 (step 32), reduce 56
  f32 direct: reduce grid at its 8192 cap                        f32   conv 512->512 3x3 s1x1 p0 @3x3 N=320 | direct cfg 0, K 320 = 1 x 320 (step 32), reduce 8192
  bf16c cfg 0                                                    bf16c conv 512->512 1x1 s1x1 p0 @1x1 N=320 | direct cfg 0, K 320 = 1 x 320 (step 32), reduce 1024
  bf16c cfg 1                                                    bf16c conv 128->128 3x3 s1x1 p1 @23x24 N=320 | direct cfg 1, K 176640 = 28 x 6336 (step 32), reduce 576
  bf16c cfg 2                                                    bf16c conv 64->64 3x3 s1x1 p1 @4x9 N=320 | direct cfg 2, K 11520 = 45 x 256 (step 32), reduce 144
  bf16c cfg 3                                                    bf16c conv 256->64 1x1 s1x1 p0 @8x8 N=320 | direct cfg 3, K 20480 = 80 x 256 (step 32), reduce 64
  bf16c cfg 4                                                    bf16c conv 80->32 3x3 s1x1 p1 @21x19 N=320 | direct cfg 4, K 127680 = 125 x 1024 (step 32), reduce 90
  bf16c cfg 5                                                    bf16c conv 6->16 7x7 s1x1 p3 @32x32 N=320 | direct cfg 5, K 327680 = 190 x 1728 (step 32), reduce 25
  bf16c ksplit > 1, ragged last chunk                            bf16c conv 128->128 3x3 s1x1 p1 @23x24 N=320 | direct cfg 1, K 176640 = 28 x 6336 (step 32), reduce 576
  small head: several blocks                                     f32   conv 512->1 1x1 s1x1 p0 @1x1 N=320 | small cfg -1, K 320 = 2 x 160 (step 2), reduce 2
  small head: 1024-block cap                                     f32   conv 256->1 2x2 s2x2 p0 @24x24 N=512 | small cfg -1, K 73728 = 1024 x 72 (step 1), reduce 4
  small head: ragged last chunk                                  f32   conv 32->3 1x1 s1x1 p0 @10x10 N=320 | small cfg -1, K 32000 = 15 x 2134 (step 32), reduce 1
  small head: ncols 1024                                         f32   conv 256->1 2x2 s2x2 p0 @24x24 N=512 | small cfg -1, K 73728 = 1024 x 72 (step 1), reduce 4
  small head: cout 1                                             f32   conv 512->1 1x1 s1x1 p0 @1x1 N=320 | small cfg -1, K 320 = 2 x 160 (step 2), reduce 2
  small head: cout 3                                             f32   conv 32->3 1x1 s1x1 p0 @10x10 N=320 | small cfg -1, K 32000 = 15 x 2134 (step 32), reduce 1
  wino: odd H and W at a training batch                          f32   conv 64->64 3x3 s1x1 p1 @5x9 N=320 | wino cfg -1, K 4800 = 150 x 32 (step 8), reduce 144
  wino: ksplit > 1, ragged last chunk                            f32   conv 256->256 3x3 s1x1 p1 @6x6 N=320 | wino cfg -1, K 2880 = 16 x 184 (step 8), reduce 2304
  wino: more tiles than the exactness bound (dz masks)           f32   conv 64->64 3x3 s1x1 p1 @37x41 N=320 | wino cfg -1, K 127680 = 254 x 504 (step 8), reduce 144
  wino: fill ratio exactly 3/4 (48 x 64)                         f32   conv 48->64 3x3 s1x1 p1 @12x12 N=37 | wino cfg -1, K 1332 = 34 x 40 (step 8), reduce 108
  wino: fill ratio below 3/4 (47 x 64) -> direct                 f32   conv 47->64 3x3 s1x1 p1 @12x12 N=37 | direct cfg 1, K 5328 = 37 x 144 (step 16), reduce 108
  wino: H = 5                                                    f32   conv 64->64 3x3 s1x1 p1 @5x9 N=64 | wino cfg -1, K 960 = 30 x 32 (step 8), reduce 144
  wino: H = 4 -> direct                                          f32   conv 64->64 3x3 s1x1 p1 @4x9 N=64 | direct cfg 2, K 2304 = 9 x 256 (step 32), reduce 144
  wino: W = 5                                                    f32   conv 64->64 3x3 s1x1 p1 @9x5 N=64 | wino cfg -1, K 960 = 30 x 32 (step 8), reduce 144
  wino: W = 4 -> direct                                          f32   conv 64->64 3x3 s1x1 p1 @9x4 N=64 | direct cfg 2, K 2304 = 9 x 256 (step 32), reduce 144
  wino: T = 64 kKT                                               f32   conv 64->64 3x3 s1x1 p1 @16x16 N=8 | wino cfg -1, K 512 = 16 x 32 (step 8), reduce 144
  wino: T < 64 kKT -> direct                                     f32   conv 64->64 3x3 s1x1 p1 @16x16 N=7 | direct cfg 2, K 1792 = 7 x 256 (step 32), reduce 144
  wino: T / tiles = 4 kKT                                        f32   conv 512->512 3x3 s1x1 p1 @6x6 N=228 | wino cfg -1, K 2052 = 4 x 520 (step 8), reduce 8192
  wino: T / tiles < 4 kKT -> direct                              f32   conv 512->512 3x3 s1x1 p1 @6x6 N=227 | direct cfg 0, K 8172 = 3 x 2752 (step 32), reduce 8192
  thin: one block                                                thin  conv 32->3 1x1 s1x1 p0 @10x10 N=1 | 1 blocks
  thin: 1 < blocks < 512                                         thin  conv 32->3 1x1 s1x1 p0 @10x10 N=320 | 16 blocks
  thin: 512-block cap, ragged tail, 320 x 96 x 96 pixels         thin  conv 32->3 1x1 s1x1 p0 @96x96 N=320 | 512 blocks
  f32 direct: forced cfg 3 / 4 on a layer of more than 32 P channels unreachable: wgrad_plan ignores a forced configuration whose row tile is smaller than the heuristic's class (bm >= 64 wanted): the forced cases above use <= 32 P channels, where all five are admitted

ACCURACY TABLE (measured on an MI355X: L-inf error / L-inf scale of the float64 gradient)
  bf16 boxes           conv 512->512 1x1 s1x1 p0 @1x1 N=320                 kernel / fp64 1.04e-07   torch fp32 / fp64 2.78e-07   bound 2.0e-04
  fp32 direct          conv 6->16 7x7 s1x1 p3 @32x32 N=320                  kernel / fp64 7.87e-07   torch fp32 / fp64 7.92e-07   bound 2.0e-04
  split-operand bf16   conv 128->128 3x3 s1x1 p1 @23x24 N=320               kernel / fp64 5.81e-07   torch fp32 / fp64 3.97e-07   bound 2.0e-04
  small head           conv 256->1 2x2 s2x2 p0 @24x24 N=512                 kernel / fp64 9.45e-07   torch fp32 / fp64 5.72e-07   bound 2.0e-04
  Winograd             conv 256->256 3x3 s1x1 p1 @6x6 N=320                 kernel / fp64 4.52e-07   torch fp32 / fp64 4.81e-07   bound 2.0e-04
  thin 1x1             conv 32->3 1x1 s1x1 p0 @96x96 N=320                  kernel / fp64 6.90e-08   torch fp32 / fp64 6.97e-07   bound 2.0e-04
"""
import ctypes as C
import functools
import time

import pytest
import torch
import torch.nn.functional as F

from test_conv_gpu import SIGS
from test_train_gpu import WGRAD_SIGS, WINO_WGRAD_SIGS
from wav2lip_amd import _lib
from wav2lip_amd._lib import (ACT_NONE, PREC_BF16, PREC_F32, WGRAD_DIRECT, WGRAD_SMALL, WGRAD_WINO, ConvGeom, WgradBf16Info, WgradInfo,
                              check, ptr)

pytestmark = pytest.mark.gpu

TRAIN_N = (320, 512)
SMALL_N = (64, 37, 8, 3, 2, 1)
WINO_GROWTH = 144
LIMIT = 1 << 24


def _pair(v):
    return tuple(v) if isinstance(v, tuple) else (v, v)


def _sig(tr, cin, cout, k, s, p, op, H, W, x_extra=0, dz_extra=0):
    return (int(tr), cin, cout, k) + _pair(s) + _pair(p) + _pair(op) + (H, W, x_extra, dz_extra)


# boundary shapes no layer of the models sits on: both sides of every clause of wino_wgrad_ok (fill ratio 3/4: 48 x 64 channels is
# exactly 3/4 of a 64 x 64 tile; H or W of 5 against 4; T = N*TH*TW against 64*kKT = 512; T / channel tiles against 4*kKT = 32 is
# reached by the models' 512 -> 512 layer at 6x6: 9 tiles per image, 64 channel tiles, 2052 / 64 >= 32 > 2043 / 64),
# the small head's column limit (ncols = taps * cin_p = 1024) and operands inside wider buffers at a training batch
EXTRA_SIGS = [
    _sig(0, 48, 64, 3, 1, 1, 0, 12, 12), _sig(0, 47, 64, 3, 1, 1, 0, 12, 12),
    _sig(0, 64, 64, 3, 1, 1, 0, 5, 9), _sig(0, 64, 64, 3, 1, 1, 0, 4, 9), _sig(0, 64, 64, 3, 1, 1, 0, 9, 5), _sig(0, 64, 64, 3, 1, 1, 0, 9, 4),
    _sig(0, 64, 64, 3, 1, 1, 0, 16, 16),                                              # 64 tiles per image: T = 512 at N = 8
    _sig(0, 1024, 3, 1, 1, 0, 0, 24, 24), _sig(0, 256, 1, 2, 2, 0, 0, 24, 24),
    _sig(0, 64, 64, 3, 1, 1, 0, 24, 24, 96, 32), _sig(0, 32, 32, 3, 1, 1, 0, 48, 48, 16, 8),
    # bf16 boxes: a 7x7 layer wide enough for tap groups (64 Q channels: 9 taps per group, 49 = 5 * 9 + 4), prime extents that no box divides,
    # and enough (cp, cq, tap group) tiles - 16 * 16 * 3 - that the K axis is not split at all
    _sig(0, 64, 64, 7, 1, 3, 0, 12, 12), _sig(0, 64, 64, 3, 1, 1, 0, 37, 41), _sig(0, 1024, 1024, 5, 1, 2, 0, 6, 6),
]


def _pool():
    out = []
    for kind, k, s, p, cin, cout, H, W, _res, op in SIGS:
        out.append(_sig(kind == "t", cin, cout, k, s, p, op, H, W))
    for tr, cin, cout, k, s, p, op, H, W in WGRAD_SIGS:
        out.append(_sig(tr, cin, cout, k, s, p, op, H, W))
    for cin, cout, H, W, _n, xcs, dcs in WINO_WGRAD_SIGS:
        out.append(_sig(0, cin, cout, 3, 1, 1, 0, H, W, xcs - (cin + 7) // 8 * 8 if xcs > cin else 0, dcs - (cout + 7) // 8 * 8 if dcs > cout else 0))
    seen, uniq = set(), []
    for s in out + EXTRA_SIGS:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def _geom(sig):
    tr, cin, cout, k, sh, sw, ph, pw, oph, opw = sig[:10]
    return ConvGeom(tr, cin, cout, k, k, sh, sw, ph, pw, oph, opw, ACT_NONE)


def _out_hw(sig):
    ho, wo = C.c_int(), C.c_int()
    g = _geom(sig)
    check(_lib.load().w2l_conv_out_hw(C.byref(g), sig[10], sig[11], C.byref(ho), C.byref(wo)), "out_hw")
    return ho.value, wo.value


class Case:
    """one launch: path ('bf16', 'f32', 'bf16c', 'thin'), layer signature, batch, forced tile configuration, Winograd switch"""

    def __init__(self, path, sig, N, force=-1, wino=1):
        self.path, self.sig, self.N, self.force, self.wino = path, sig, N, force, wino
        tr, cin, cout = sig[:3]
        self.H, self.W = sig[10], sig[11]
        self.Ho, self.Wo = _out_hw(sig)
        self.Hp, self.Wp = (self.H, self.W) if tr else (self.Ho, self.Wo)       # the coarse grid: K = N * Hp * Wp
        al = 4 if path in ("f32", "bf16c") else 8
        self.cin_p, self.cout_p = (cin + al - 1) // al * al, (cout + al - 1) // al * al
        self.x_cs, self.dz_cs = self.cin_p + sig[12], self.cout_p + sig[13]
        self.K = N * self.Hp * self.Wp
        esz = 4 if path in ("f32", "bf16c") else 2
        self.bytes = esz * N * (self.H * self.W * self.x_cs + self.Ho * self.Wo * self.dz_cs)
        self._info = None

    def key(self):
        return (self.path, self.sig, self.N, self.force, self.wino)

    def info(self):
        """the launcher's own dry run; None where the launcher refuses the call"""
        if self._info is None:
            lib, g = _lib.load(), _geom(self.sig)
            if self.path == "bf16":
                i = WgradBf16Info()
                rc = lib.w2l_conv_wgrad_bf16_resolve(C.byref(g), self.N, self.H, self.W, self.x_cs, self.dz_cs, C.byref(i))
            elif self.path == "thin":
                i, rc = lib.w2l_thin1x1_wgrad_blocks(self.K), 0
            else:
                i = WgradInfo()
                check(lib.w2l_conv_wgrad_set_cfg(self.force, self.wino), "set_cfg")
                rc = lib.w2l_conv_wgrad_resolve(C.byref(g), self.N, self.H, self.W, self.x_cs, self.dz_cs,
                                                PREC_BF16 if self.path == "bf16c" else PREC_F32, C.byref(i))
                check(lib.w2l_conv_wgrad_set_cfg(-1, 1), "set_cfg")
            self._info = (rc, i)
        return self._info[1] if self._info[0] == 0 else None

    def thin_ok(self):
        tr, cin, cout, k, sh, sw, ph, pw = self.sig[:8]
        return not tr and k == 1 and (sh, sw, ph, pw) == (1, 1, 0, 0) and cin <= 32 and cout <= 4

    def describe(self):
        tr, cin, cout, k, sh, sw, ph, pw, oph, opw, H, W, xe, de = self.sig
        s = "%s %d->%d %dx%d s%dx%d p%d%s @%dx%d N=%d" % ("convT" if tr else "conv", cin, cout, k, k, sh, sw, ph,
                                                          "+%d" % oph if oph else "", H, W, self.N)
        if xe or de:
            s += " cs %d/%d" % (self.x_cs, self.dz_cs)
        if self.force >= 0 or not self.wino:
            s += " force %d wino %d" % (self.force, self.wino)
        i = self.info()
        if self.path == "bf16":
            s += " | ni %d box %dx%d, %d boxes = %d splits x %d, tg %d x %d, ncq %d mt %d qp %d" % (
                i.ni, i.bh, i.bw, i.nboxes, i.splits, i.boxes_per_split, i.ntg, i.tg, i.ncq, i.mt, i.qp)
        elif self.path == "thin":
            s += " | %d blocks" % i
        else:
            s += " | %s cfg %d, K %d = %d x %d (step %d), reduce %d" % (("wino", "direct", "small")[i.family], i.cfg, i.K, i.ksplit, i.chunk,
                                                                        i.kstep, i.reduce_blocks)
        return s


# ------------------------------------------------------------------------------------------------ regimes
def _last(i):
    return i.nboxes - (i.splits - 1) * i.boxes_per_split


def _bf16(pred):
    return ("bf16", lambda c: c.info() is not None and pred(c, c.info()), {})


def _f32(pred, **kw):
    return ("f32", lambda c: c.info() is not None and pred(c, c.info()), kw)


def _b16c(pred):
    return ("bf16c", lambda c: c.info() is not None and pred(c, c.info()), {})


def _thin(pred):
    return ("thin", lambda c: c.thin_ok() and pred(c, c.info()), {})


def _train(c):
    return c.N in TRAIN_N


def _s1k3(c):
    return c.sig[0] == 0 and c.sig[3:8] == (3, 1, 1, 1, 1)


def _wino_pair(cin, cout, H, W, N, fam):
    """one side of a clause of wino_wgrad_ok: exactly this shape, which must resolve to family `fam`"""
    return _f32(lambda c, i: c.sig[:3] == (0, cin, cout) and _s1k3(c) and (c.H, c.W, c.N) == (H, W, N) and c.sig[12:] == (0, 0) and i.family == fam,
                ns=(N,))


REGIMES = {
    # ---- bf16 boxes
    "bf16 several boxes per split, full last split": _bf16(lambda c, i: i.boxes_per_split > 1 and _last(i) == i.boxes_per_split and i.splits > 1),
    "bf16 several boxes per split, short last split": _bf16(lambda c, i: i.boxes_per_split > 1 and 1 < _last(i) < i.boxes_per_split),
    "bf16 last split of exactly one box": _bf16(lambda c, i: i.boxes_per_split > 1 and i.splits > 1 and _last(i) == 1),
    "bf16 ni > 1, N % ni != 0, several boxes per split": _bf16(lambda c, i: i.ni > 1 and c.N % i.ni != 0 and i.boxes_per_split > 1),
    "bf16 ragged bh and bw, several boxes per split": _bf16(lambda c, i: i.ni == 1 and c.Hp % i.bh and c.Wp % i.bw and i.boxes_per_split > 1),
    "bf16 5x5: short last tap group": _bf16(lambda c, i: c.sig[3] == 5 and i.ntg > 1 and 25 % i.tg != 0),
    "bf16 7x7: short last tap group": _bf16(lambda c, i: c.sig[3] == 7 and i.ntg > 1 and 49 % i.tg != 0),
    "bf16 ncq > 1": _bf16(lambda c, i: i.ncq > 1 and _train(c)),
    "bf16 mt 1 qp 1": _bf16(lambda c, i: (i.mt, i.qp) == (1, 1) and _train(c)),
    "bf16 mt 1 qp 2": _bf16(lambda c, i: (i.mt, i.qp) == (1, 2) and _train(c)),
    "bf16 mt 2 qp 1": _bf16(lambda c, i: (i.mt, i.qp) == (2, 1) and _train(c)),
    "bf16 mt 2 qp 2": _bf16(lambda c, i: (i.mt, i.qp) == (2, 2) and _train(c)),
    "bf16 stride-2 conv": _bf16(lambda c, i: c.sig[0] == 0 and c.sig[4:6] == (2, 2) and _train(c)),
    "bf16 transposed": _bf16(lambda c, i: c.sig[0] == 1 and c.sig[4:6] == (2, 2) and _train(c)),
    "bf16 one split, many boxes": _bf16(lambda c, i: i.splits == 1 and i.nboxes >= 8),
    "bf16 operands are slices of wider buffers": _bf16(lambda c, i: c.sig[12] > 0 and c.sig[13] > 0 and _train(c) and i.boxes_per_split > 1),
    # ---- fp32 direct GEMM
    **{"f32 direct: heuristic picks cfg %d" % k: _f32(lambda c, i, k=k: i.family == WGRAD_DIRECT and i.cfg == k and _train(c)) for k in range(5)},
    **{"f32 direct: cfg %d forced on a 3x3 s1 layer" % k: _f32(lambda c, i, k=k: _s1k3(c) and i.family == WGRAD_DIRECT and i.cfg == k and _train(c),
                                                                force=k, wino=0) for k in range(5)},
    **{"f32 direct: cfg %d forced on a stride-2 layer" % k: _f32(lambda c, i, k=k: c.sig[4:6] == (2, 2) and i.family == WGRAD_DIRECT and i.cfg == k
                                                                  and _train(c), force=k) for k in range(5)},
    "f32 direct: ksplit 1": _f32(lambda c, i: i.family == WGRAD_DIRECT and i.ksplit == 1 and i.K > i.kstep),
    "f32 direct: ksplit > 256": _f32(lambda c, i: i.family == WGRAD_DIRECT and i.ksplit > 256),
    "f32 direct: K % chunk != 0": _f32(lambda c, i: i.family == WGRAD_DIRECT and i.ksplit > 1 and i.K % i.chunk and _train(c)),
    "f32 direct: K % K-step != 0": _f32(lambda c, i: i.family == WGRAD_DIRECT and i.K % i.kstep and i.K > 8 * i.kstep),
    "f32 direct: reduce grid at its 8192 cap": _f32(lambda c, i: i.family == WGRAD_DIRECT and i.reduce_blocks == 8192),
    # ---- split-operand bf16
    **{"bf16c cfg %d" % k: _b16c(lambda c, i, k=k: i.cfg == k and i.family == WGRAD_DIRECT) for k in range(6)},
    "bf16c ksplit > 1, ragged last chunk": _b16c(lambda c, i: i.family == WGRAD_DIRECT and i.ksplit > 1 and i.K % i.chunk and _train(c)),
    # ---- small head
    "small head: several blocks": _f32(lambda c, i: i.family == WGRAD_SMALL and 1 < i.ksplit < 1024),
    "small head: 1024-block cap": _f32(lambda c, i: i.family == WGRAD_SMALL and i.ksplit == 1024),
    "small head: ragged last chunk": _f32(lambda c, i: i.family == WGRAD_SMALL and i.ksplit > 1 and i.K % i.chunk),
    "small head: ncols 1024": _f32(lambda c, i: i.family == WGRAD_SMALL and c.sig[3] ** 2 * c.cin_p == 1024 and i.ksplit > 1),
    "small head: cout 1": _f32(lambda c, i: i.family == WGRAD_SMALL and c.sig[2] == 1 and i.ksplit > 1),
    "small head: cout 3": _f32(lambda c, i: i.family == WGRAD_SMALL and c.sig[2] == 3 and i.ksplit > 1),
    # ---- Winograd
    "wino: odd H and W at a training batch": _f32(lambda c, i: i.family == WGRAD_WINO and c.H % 2 and c.W % 2 and _train(c)),
    "wino: ksplit > 1, ragged last chunk": _f32(lambda c, i: i.family == WGRAD_WINO and i.ksplit > 1 and i.K % i.chunk and _train(c)),
    "wino: more tiles than the exactness bound (dz masks)": _f32(lambda c, i: i.family == WGRAD_WINO and WINO_GROWTH * i.K >= LIMIT),
    "wino: fill ratio exactly 3/4 (48 x 64)": _wino_pair(48, 64, 12, 12, 37, WGRAD_WINO),
    "wino: fill ratio below 3/4 (47 x 64) -> direct": _wino_pair(47, 64, 12, 12, 37, WGRAD_DIRECT),
    "wino: H = 5": _wino_pair(64, 64, 5, 9, 64, WGRAD_WINO),
    "wino: H = 4 -> direct": _wino_pair(64, 64, 4, 9, 64, WGRAD_DIRECT),
    "wino: W = 5": _wino_pair(64, 64, 9, 5, 64, WGRAD_WINO),
    "wino: W = 4 -> direct": _wino_pair(64, 64, 9, 4, 64, WGRAD_DIRECT),
    "wino: T = 64 kKT": _wino_pair(64, 64, 16, 16, 8, WGRAD_WINO),
    "wino: T < 64 kKT -> direct": _wino_pair(64, 64, 16, 16, 7, WGRAD_DIRECT),
    "wino: T / tiles = 4 kKT": _wino_pair(512, 512, 6, 6, 228, WGRAD_WINO),
    "wino: T / tiles < 4 kKT -> direct": _wino_pair(512, 512, 6, 6, 227, WGRAD_DIRECT),
    # ---- thin 1x1
    "thin: one block": _thin(lambda c, nb: nb == 1),
    "thin: 1 < blocks < 512": _thin(lambda c, nb: 1 < nb < 512),
    "thin: 512-block cap, ragged tail, 320 x 96 x 96 pixels": _thin(lambda c, nb: nb == 512 and c.K == 320 * 96 * 96 and c.K % (512 * 256)),
}
# regimes no admissible shape reaches, with the launcher's reason
UNREACHABLE = {
    "f32 direct: forced cfg 3 / 4 on a layer of more than 32 P channels": "wgrad_plan ignores a forced configuration whose row tile is "
    "smaller than the heuristic's class (bm >= 64 wanted): the forced cases above use <= 32 P channels, where all five are admitted",
}


@functools.lru_cache(maxsize=None)
def selection():
    """regime -> Case, greedy in the order of REGIMES"""
    pool = _pool() + [_sig(0, 32, 3, 1, 1, 0, 0, 96, 96), _sig(0, 32, 3, 1, 1, 0, 0, 10, 10)]
    chosen, picked = {}, []
    for name, (path, pred, kw) in REGIMES.items():
        force, wino, ns = kw.get("force", -1), kw.get("wino", 1), kw.get("ns", TRAIN_N + SMALL_N)
        hit = next((c for c in picked if (c.path, c.force, c.wino) == (path, force, wino) and c.N in ns and pred(c)), None)
        if hit is None:
            cands = [Case(path, s, N, force, wino) for N in ns for s in pool]
            cands = [c for c in cands if c.K < LIMIT and c.bytes < (3 << 30) and pred(c)]
            if cands:
                hit = min(cands, key=lambda c: (c.N not in TRAIN_N, c.bytes))
                picked.append(hit)
        chosen[name] = hit
    return chosen


def selection_table():
    rows = ["  %-62s %-5s %s" % (name, c.path if c else "-", c.describe() if c else "NO CASE") for name, c in selection().items()]
    rows += ["  %-62s unreachable: %s" % (k, v) for k, v in UNREACHABLE.items()]
    return "\n".join(rows)


# ------------------------------------------------------------------------------------------------ reference
def wgrad_ref(x, dz, sig, n_chunk=32):
    """float64 weight gradient, a plain sum over shifted slices: x [N,H,W,cin], dz [N,Ho,Wo,cout] (any dtype, any device) ->
    torch layout [cout][cin][k][k] ([cin][cout][k][k] for a transposed conv).  P = the tensor on the coarse grid (dz of a conv, x of a
    transposed conv), Q the other: dW[cp][cq][ky][kx] = sum_pix P[pix][cp] * Q[pix * s - pad + (ky, kx)][cq]."""
    tr, cin, cout, k, sh, sw, ph, pw = sig[:8]
    P, Q = (x, dz) if tr else (dz, x)
    N, Hp, Wp, CP = P.shape
    Hq, Wq, CQ = Q.shape[1:]
    out = torch.zeros(CP, CQ, k, k, dtype=torch.float64, device=x.device)
    # Q rows / columns needed: from -pad to (Hp - 1) * s - pad + k - 1
    hb, wb = max((Hp - 1) * sh - ph + k - Hq, 0), max((Wp - 1) * sw - pw + k - Wq, 0)
    for n0 in range(0, N, n_chunk):
        p64 = P[n0:n0 + n_chunk].double().reshape(-1, CP)
        q64 = F.pad(Q[n0:n0 + n_chunk].double(), (0, 0, pw, wb, ph, hb))
        for ky in range(k):
            for kx in range(k):
                qs = q64[:, ky:ky + (Hp - 1) * sh + 1:sh, kx:kx + (Wp - 1) * sw + 1:sw, :].reshape(-1, CQ)
                out[:, :, ky, kx] += p64.t() @ qs
    return out


@pytest.mark.parametrize("sig,N", [(_sig(0, 5, 7, 3, 2, 1, 0, 9, 8), 3), (_sig(1, 6, 4, 3, 2, 1, 1, 5, 4), 2), (_sig(0, 3, 5, 5, (1, 2), (2, 1), 0, 7, 11), 2),
                                   (_sig(1, 4, 3, 3, 1, 0, 0, 1, 1), 3), (_sig(0, 6, 2, 7, 1, 3, 0, 8, 6), 1)])
def test_reference_equals_float64_autograd(sig, N):
    """the reference of this file against F.conv2d / F.conv_transpose2d autograd in float64 on the CPU: conv, transposed, anisotropic"""
    tr, cin, cout, k, sh, sw, ph, pw, oph, opw, H, W = sig[:12]
    torch.manual_seed(1)
    x = torch.randn(N, cin, H, W, dtype=torch.float64)
    w = torch.zeros((cin, cout, k, k) if tr else (cout, cin, k, k), dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(x, w, None, (sh, sw), (ph, pw), (oph, opw)) if tr else F.conv2d(x, w, None, (sh, sw), (ph, pw))
    dz = torch.randn_like(y)
    y.backward(dz)
    got = wgrad_ref(x.permute(0, 2, 3, 1), dz.permute(0, 2, 3, 1), sig, n_chunk=2)
    assert got.shape == w.grad.shape and float((got - w.grad).abs().max()) <= 1e-12 * float(w.grad.abs().max())


# ------------------------------------------------------------------------------------------------ running a case
def _dtype(path):
    return torch.float32 if path in ("f32", "bf16c") else torch.bfloat16


def _operand(shape, C_valid, C_pad, dtype, dev, gen, mode, neighbour):
    """[N,H,W,cs]: channels [0, C_valid) data, [C_valid, C_pad) zero (the ABI's pad channels), the rest a neighbour's integers"""
    N, H, W, cs = shape
    t = torch.zeros(shape, dtype=dtype, device=dev)
    if mode == "exact":
        t[..., :C_valid] = torch.randint(-1, 2, (N, H, W, C_valid), device=dev, generator=gen, dtype=torch.int8).to(dtype)
    else:
        t[..., :C_valid] = torch.randn((N, H, W, C_valid), device=dev, generator=gen).to(dtype)
    if cs > C_pad:
        t[..., C_pad:] = neighbour
    return t


def _launch(c, x, dz, N=None):
    """two launches into NaN-filled outputs, bit-identical; returns the gradient in torch layout"""
    lib, g = _lib.load(), _geom(c.sig)
    tr, cin, cout, k = c.sig[:4]
    N = N or c.N
    shape = (cout, cin) if c.path == "thin" else ((cin, cout, k, k) if tr else (cout, cin, k, k))
    outs = []
    for _ in range(2):
        dw = torch.full(shape, float("nan"), device=x.device)
        s = _lib.current_stream()
        if c.path == "bf16":
            rc = lib.w2l_conv_wgrad_bf16(C.byref(g), s, N, c.H, c.W, ptr(x), x.shape[-1], ptr(dz), dz.shape[-1], ptr(dw))
        elif c.path == "thin":
            rc = lib.w2l_thin1x1_wgrad_bf16(s, N * c.H * c.W, cin, cout, ptr(x), x.shape[-1], ptr(dz), dz.shape[-1], ptr(dw), None)
        else:
            check(lib.w2l_conv_wgrad_set_cfg(c.force, c.wino), "set_cfg")
            try:
                rc = lib.w2l_conv_wgrad_prec(C.byref(g), s, N, c.H, c.W, ptr(x), x.shape[-1], ptr(dz), dz.shape[-1], ptr(dw),
                                             PREC_BF16 if c.path == "bf16c" else PREC_F32)
            finally:
                check(lib.w2l_conv_wgrad_set_cfg(-1, 1), "set_cfg")
        check(rc, c.path)
        torch.cuda.synchronize()
        outs.append(dw)
    assert torch.equal(outs[0], outs[1]) and not torch.isnan(outs[0]).any(), "two runs differ, or an element was never written"
    return outs[0].reshape(shape + (1, 1)) if c.path == "thin" else outs[0]


_VERIFIED = {}


def run_exact(c, cuda):
    """the exact check of one case (once per case, whatever number of regimes selected it)"""
    if c.key() in _VERIFIED:
        return _VERIFIED[c.key()]
    tr, cin, cout = c.sig[:3]
    assert c.K < LIMIT, "partial sums of {-1,0,1} products must stay below 2^24"
    i = c.info()
    wino = c.path == "f32" and i.family == WGRAD_WINO
    masks = 1
    if wino:
        tiles_per_image = i.K // c.N
        while WINO_GROWTH * ((c.N + masks - 1) // masks) * tiles_per_image >= LIMIT:
            masks += 1
        assert masks <= c.N
    gen = torch.Generator(device=cuda).manual_seed(len(c.describe()) + c.N)
    dt = _dtype(c.path)
    x = _operand((c.N, c.H, c.W, c.x_cs), cin, c.cin_p, dt, cuda, gen, "exact", 2.0)
    dz_full = _operand((c.N, c.Ho, c.Wo, c.dz_cs), cout, c.cout_p, dt, cuda, gen, "exact", -3.0)
    img = torch.arange(c.N, device=cuda)
    worst = 0.0
    for m in range(masks):
        dz = dz_full if masks == 1 else dz_full * (img % masks == m).to(dt).view(-1, 1, 1, 1)
        if masks > 1:
            dz[..., c.cout_p:] = dz_full[..., c.cout_p:]          # the neighbour's channels stay dense
        got = _launch(c, x, dz)
        ref = wgrad_ref(x[..., :cin], dz[..., :cout], c.sig)
        assert float(ref.abs().max()) > 0
        worst = max(worst, float((got.double() - ref).abs().max()))
        assert torch.equal(got.double(), ref), "%s (mask %d of %d): %d of %d elements differ, max |diff| %g" % (
            c.describe(), m, masks, int((got.double() != ref).sum()), ref.numel(), worst)
        del dz, got, ref
    _VERIFIED[c.key()] = masks
    return masks


@pytest.mark.parametrize("regime", list(REGIMES))
def test_regime_is_reached_and_exact(regime, cuda):
    c = selection()[regime]
    assert c is not None, "no candidate shape reaches the regime '%s' any more: a launch rule changed" % regime
    path, pred, _ = REGIMES[regime]
    assert pred(c), "the dry run no longer puts %s into '%s'" % (c.describe(), regime)      # the regime, from the launcher's own plan
    masks = run_exact(c, cuda)
    if "dz masks" in regime:
        assert masks > 1


# ------------------------------------------------------------------------------------------------ accuracy
ACCURACY_CASES = {
    "bf16 boxes": "bf16 several boxes per split, short last split",
    "fp32 direct": "f32 direct: K % chunk != 0",
    "split-operand bf16": "bf16c ksplit > 1, ragged last chunk",
    "small head": "small head: 1024-block cap",
    "Winograd": "wino: ksplit > 1, ragged last chunk",
    "thin 1x1": "thin: 512-block cap, ragged tail, 320 x 96 x 96 pixels",
}
BOUND = 2e-4


@pytest.mark.parametrize("family", list(ACCURACY_CASES))
def test_accuracy_on_gaussian_operands(family, cuda):
    c = selection()[ACCURACY_CASES[family]]
    assert c is not None
    tr, cin, cout, k, sh, sw, ph, pw, oph, opw = c.sig[:10]
    gen = torch.Generator(device=cuda).manual_seed(7)
    dt = _dtype(c.path)
    x = _operand((c.N, c.H, c.W, c.x_cs), cin, c.cin_p, dt, cuda, gen, "gauss", 5.0)
    dz = _operand((c.N, c.Ho, c.Wo, c.dz_cs), cout, c.cout_p, dt, cuda, gen, "gauss", -3.0)
    if c.path == "bf16c":                # operands rounded to bf16 inside the kernel: the reference takes the rounded values
        x, dz = x.to(torch.bfloat16).float(), dz.to(torch.bfloat16).float()
    got = _launch(c, x, dz).double()
    ref = wgrad_ref(x[..., :cin], dz[..., :cout], c.sig)
    # torch's own float32 weight gradient of the same operands
    xt = x[..., :cin].float().permute(0, 3, 1, 2)
    w = torch.zeros(ref.shape, device=cuda, requires_grad=True)
    y = F.conv_transpose2d(xt, w, None, (sh, sw), (ph, pw), (oph, opw)) if tr else F.conv2d(xt, w, None, (sh, sw), (ph, pw))
    y.backward(dz[..., :cout].float().permute(0, 3, 1, 2))
    scale = float(ref.abs().max())
    e_kernel, e_torch = float((got - ref).abs().max()) / scale, float((w.grad.double() - ref).abs().max()) / scale
    bound = BOUND if e_torch <= BOUND / 3 else 3 * e_torch
    print("ACCURACY %-20s %-70s kernel %.2e  torch fp32 %.2e  bound %.1e" % (family, c.describe().split(" | ")[0], e_kernel, e_torch, bound))
    assert e_kernel <= bound, "%s: %.3e of the gradient's scale (torch fp32: %.3e)" % (c.describe(), e_kernel, e_torch)


# ------------------------------------------------------------------------------------------------ large offsets
GIB = 1 << 30
LARGE = {   # launcher -> (path, signature, batch): the larger activation buffer lies between 1 GiB and the 2 GiB guard
    "fp32 direct": ("f32", _sig(0, 64, 128, 3, 2, 1, 0, 48, 48), 2400),
    "Winograd": ("f32", _sig(0, 64, 64, 3, 1, 1, 0, 96, 96), 700),
    "bf16 boxes": ("bf16", _sig(0, 64, 64, 3, 1, 1, 0, 96, 96), 1400),
}


@pytest.mark.parametrize("launcher", list(LARGE))
def test_byte_offsets_beyond_one_gib(launcher, cuda):
    path, sig, N = LARGE[launcher]
    c = Case(path, sig, N)
    tr, cin, cout = sig[:3]
    esz = 4 if path == "f32" else 2
    big = esz * N * max(c.H * c.W * c.x_cs, c.Ho * c.Wo * c.dz_cs)
    assert GIB < big < 2 * GIB
    i = c.info()
    assert i is not None and (path == "bf16" or i.family == (WGRAD_WINO if launcher == "Winograd" else WGRAD_DIRECT))
    dt, gen = _dtype(path), torch.Generator(device=cuda).manual_seed(3)
    x = torch.zeros((N, c.H, c.W, c.x_cs), dtype=dt, device=cuda)
    dz = torch.zeros((N, c.Ho, c.Wo, c.dz_cs), dtype=dt, device=cuda)
    for n in (0, N - 1):                                  # non-zero data in the first AND the last image: offsets pass 2^30
        x[n, ..., :cin] = torch.randint(-1, 2, (c.H, c.W, cin), device=cuda, generator=gen, dtype=torch.int8).to(dt)
        dz[n, ..., :cout] = torch.randint(-1, 2, (c.Ho, c.Wo, cout), device=cuda, generator=gen, dtype=torch.int8).to(dt)
    live_pixels = 2 * c.Hp * c.Wp                         # the sum of |terms| of any output element
    assert (WINO_GROWTH if launcher == "Winograd" else 1) * live_pixels < LIMIT
    got = _launch(c, x, dz)
    ends = [0, N - 1]
    ref = wgrad_ref(x[ends][..., :cin], dz[ends][..., :cout], sig)      # every other image is zero
    assert float(ref.abs().max()) > 0 and torch.equal(got.double(), ref), "%s: %d elements differ" % (c.describe(), int((got.double() != ref).sum()))


@pytest.mark.parametrize("launcher", list(LARGE))
def test_two_gib_guard(launcher, cuda):
    """just above 2 GiB the launcher refuses: first asked of the dry run (nothing can be launched), then of the entry point itself"""
    path, sig, N = LARGE[launcher]
    lib = _lib.load()
    esz = 4 if path == "f32" else 2
    c0 = Case(path, sig, 1)
    per_image = esz * max(c0.H * c0.W * c0.x_cs, c0.Ho * c0.Wo * c0.dz_cs)
    n_ok, n_bad = (2 * GIB - 1) // per_image, (2 * GIB - 1) // per_image + 1
    assert Case(path, sig, n_ok).info() is not None
    bad = Case(path, sig, n_bad)
    assert bad.info() is None and b"2 GiB" in lib.w2l_last_error()
    x = torch.zeros((1, c0.H, c0.W, c0.x_cs), dtype=_dtype(path), device=cuda)
    dz = torch.zeros((1, c0.Ho, c0.Wo, c0.dz_cs), dtype=_dtype(path), device=cuda)
    dw = torch.full((64, 64, 3, 3) if launcher != "fp32 direct" else (128, 64, 3, 3), float("nan"), device=cuda)
    g, s = _geom(sig), _lib.current_stream()
    if path == "bf16":
        rc = lib.w2l_conv_wgrad_bf16(C.byref(g), s, n_bad, c0.H, c0.W, ptr(x), c0.x_cs, ptr(dz), c0.dz_cs, ptr(dw))
    else:
        rc = lib.w2l_conv_wgrad_prec(C.byref(g), s, n_bad, c0.H, c0.W, ptr(x), c0.x_cs, ptr(dz), c0.dz_cs, ptr(dw), PREC_F32)
    torch.cuda.synchronize()
    assert rc != 0 and b"2 GiB" in lib.w2l_last_error() and bool(torch.isnan(dw).all())


if __name__ == "__main__":
    t0 = time.time()
    print(selection_table())
    print("%d regimes, %d distinct cases (%.1f s)" % (len(REGIMES), len({c.key() for c in selection().values() if c}), time.time() - t0))
