"""Cases, references and exactness bounds of tests/test_conv_exact_gpu.py (the forward conv kernels held to EQUALITY on integer
operands inside guard-banded buffers) and of tests/test_conv_cases_cpu.py.  Everything here runs on the host: the float64 references
are torch CPU convolutions, and the case selection asks the library's planning functions, which are host code
(w2l_tune_entry_applicable, w2l_wino4_block_plan, w2l_conv_block_plan, w2l_convb_resolve_geom, w2l_conv_out_hw,
w2l_conv_num_igemm_tiles, w2l_convb_num_tiles).  w2l_igemm_block_order is not a selection criterion: the order a launch uses is not
reported, and tests/test_abi.py already holds every order to a permutation of the tiles.

CANDIDATES are grids over the smallest shapes at which a kernel family can go wrong (never the workload's 96x96 at batch 128); a
REGIME is a named predicate over a candidate and what the planning functions say about it.  select() gives every regime the cheapest
candidate that satisfies it; the GPU tests assert the predicate again and the kernel that ran, so a later rule change cannot empty a
regime quietly.

EXACTNESS.  x, res and w are integers from {-1, 0, 1} (a third zeros, fixed seeds), scale is from {+-1, +-2, +-1/2}, shift an integer
in [-3, 3], the activation none or ReLU.  While every intermediate is an integer (or a dyadic fraction with as many significant
bits) below 2^24 in magnitude, fp32 holds it exactly in ANY summation order, so the result must equal the float64 reference; three
bf16 pieces carry such a value exactly too (the split-operand families).  The bound per family, asserted per case (exact_bound):
  direct / implicit GEMM / transposed:  kh*kw*cin * max|scale| + |shift| + |res| + 1 < 2^24.
  F(2x2,3x3):  U = G g G^T with |G| row sums <= 3/2: multiples of 1/4, |U| <= 9/4.  V = B^T d B with |B^T| row sums 2: integers,
    |V| <= 4.  A position sum over cin channels is a multiple of 1/4 below 9*cin; |A^T| has row sums <= 3, so an output is a multiple
    of 1/4 below 81*cin: in quarter units, WINO2_GROWTH * cin * max(|scale|, 1) + 4*(|shift| + |res|) + 1 < 2^24, WINO2_GROWTH = 324
    (the scale may be 1/2: one more bit, hence the factor 2 in exact_bound).
  F(4x4,3x3):  G holds sixths and twenty-fourths; the packer forms U in float64 and rounds once, so U is exact when it is an integer:
    weights are multiples of 576 = 24^2.  With DENSE taps |U| <= 576 * (1)^2 (the last row of G is (0, 0, 1)), |V| <= 10 * 10
    (|B^T| row sums <= 10), |A^T| row sums <= 19: 361 * 576 * 100 * cin > 2^24 already at cin = 1.  The exact cases therefore use
    ONE tap per (cout, cin) pair, drawn from the four taps (0..1, 0..1): columns 0 and 1 of G have |entries| <= 1/4, so
    |U| <= 576 / 16 = 36 and an output is an integer below WINO4_GROWTH * cin, WINO4_GROWTH = 361 * 36 * 100 = 1299600: cin = 8
    gives 10396800 < 2^24 with |scale| <= 1 (scale is drawn from {+-1, +-1/2} for this family).  x stays dense.  A case with more
    input channels (the residual that aliases the input needs cin = cout = 64) gives every cout W4_LIVE_CIN = 8 live input channels
    and zero weights on the others: the same bound.  The Gaussian
    accuracy run covers dense taps.  No regime of conv_wino4 had to fall back from equality to a bound check.

BACKWARD (tests/test_conv_backward_exact_gpu.py).  The data gradient of a layer is the forward kernel on the other interpretation of
the layer's weight tensor (dgrad_of: roles swapped, no activation, scale 1, shift 0, the output padding that restores what the strided
conv's floor division dropped), and an accumulating launch passes the OUTPUT slice as its residual (res = 3): the slice is pre-loaded
with a prior gradient of integers in [-3, 3] and must come back as prior + reference.  IN-PLACE BOUND: the prior takes the residual's
place in every bound above with |prior| <= 3 instead of |res| <= 1 (extra = |shift| + 3 in exact_bound); the sum is still an integer
(a multiple of 1/4 for F(2x2)) below 2^24, so "prior + reference" has ONE value whatever the order in which an epilogue adds the prior,
and a kernel that read the prior after a store to that address, twice, or not at all cannot produce it.  For bf16 storage the prior is
exact in bf16, the kernel adds it in fp32 and rounds ONCE: the result equals the float64 "prior + reference" rounded once to bf16.
"""
import ctypes as C
import itertools

import numpy as np
import torch
import torch.nn.functional as F

LIMIT = 1 << 24
WINO2_GROWTH = 324          # quarter units per input channel: 4 * (3 * 3) * (9/4 * 4)
WINO4_GROWTH = 361 * 36 * 100
W4_LIVE_CIN = 8             # conv_wino4 cases with more input channels keep 8 live ones per cout (the rest have zero weights)
ACT_NONE, ACT_RELU = 0, 1

# tile shapes (rows of output pixels x couts) of the implicit-GEMM configuration ids, in id order: kTiles of csrc/conv_igemm.hip
# (ids 0..5, and again for the split-operand ids 13..18) and kBTiles of csrc/conv_bf16.hip.  The GPU test checks them against the
# executed-FLOP count the launcher reports (padded tiles), so a changed table fails there.
F32_TILES = ((128, 128), (128, 64), (64, 128), (64, 64), (128, 32), (32, 128))
BF16_TILES = ((128, 128), (128, 64), (64, 128), (64, 64), (128, 32), (256, 256))
KSTEP = {"f32": 32, "bf16": 64}      # K elements per step (kBK / kBKH): kp = roundup(taps * cin_p, KSTEP)
GUARD_PIXELS = 512                   # conv_wino4 stores 32 tile slots x 16 pixels per work item: the largest block any family stores
GUARD_MIN_BYTES = 64 * 1024

# fp32 configuration ids by family name (wav2lip_amd._lib.FAMILY_NAMES order; ids are append-only across library versions)
WINO_IDS = {"wino": (6, 7), "wino2": (8, 9, 12), "wino4": (11,), "wino2s": (19,)}
# (cin, cout) at which each Winograd id is exercised: its minimum channel counts
WINO_CH = {6: (8, 64), 7: (16, 128), 8: (8, 64), 9: (8, 32), 12: (8, 32), 11: (8, 64), 19: (16, 64)}
WINO_HW = ((1, 1), (2, 3), (5, 4), (3, 3), (13, 11), (12, 12), (23, 24))
TP2_SIGS = ((8, 64, 5, 7), (16, 128, 1, 1), (64, 64, 9, 16))
STEM_CIN = (3, 5, 6, 15)
STEM_HW = ((5, 3), (16, 16), (50, 37))
K3S_CIN = (16, 48, 80)
K3S_HW = ((1, 1), (5, 7), (20, 24))
IGEMM_CIN = (1, 3, 6, 15, 32, 80)
GROUPED = ("wino2", "wino2s", "tp2", "tp2s", "k3s")      # families whose work items hold bh x bw blocks of ni images (besides wino4)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def lib():
    from wav2lip_amd import _lib
    return _lib.load()


def num_tiles(path):
    """implicit-GEMM tiles the library has (w2l_conv_num_igemm_tiles / w2l_convb_num_tiles); the tile tables above must list them all"""
    n = lib().w2l_conv_num_igemm_tiles() if path == "f32" else lib().w2l_convb_num_tiles()
    tiles = F32_TILES if path == "f32" else BF16_TILES
    assert n == len(tiles), "%s: the library has %d implicit-GEMM tiles, the test's table %d" % (path, n, len(tiles))
    return n


def config_id(family, index=0):
    from wav2lip_amd import _lib
    return _lib.config_ids(lib(), family)[index]


class Case:
    """one launch.  path: 'f32' (w2l_conv_*), 'bf16' (w2l_convb_*) or 'thin' (w2l_thin1x1_forward_bf16); force: fp32 configuration id
    or bf16 tile (-1: the launcher's own choice); ks: forced split-K (0: none); res: 0 none, 1 its own buffer, 2 the input slice,
    3 the OUTPUT slice (an accumulating data-gradient launch: y holds a prior gradient, integers in [-3, 3]); bwd: scale 1, shift 0
    (what NodeF gives a data-gradient handle); fwd: the forward layer (signature, H, W) a dgrad_of() case belongs to; declines:
    configuration ids that must refuse this launch (w2l_tune_entry_applicable), whichever id the case itself runs on;
    sliced: x / y / res are channel slices of wider buffers at non-zero offsets; wide: channel stride of x, y, res (0: dense) - the
    large-offset cases reach 1 GiB with it; wmode: 'dense' taps or 'w4' (see the module docstring)"""

    def __init__(self, path, family, tr, cin, cout, k, s, p, op, N, H, W, force=-1, ks=0, res=0, act=ACT_RELU, sliced=False, wide=0,
                 seed=0, head=0, x_wide=0, bwd=False, fwd=None, declines=()):
        self.path, self.family = path, family
        self.tr, self.cin, self.cout = int(tr), cin, cout
        self.k, self.s, self.p, self.op = _pair(k), _pair(s), _pair(p), _pair(op)
        self.N, self.H, self.W = N, H, W
        self.force, self.ks, self.res, self.act, self.sliced, self.wide, self.seed = force, ks, res, act, sliced, wide, seed
        self.x_wide = x_wide                                                  # channel stride of x where it is not derived from `wide`
        self.head = head                                                      # channels of a fused 1x1 head WITHOUT activation (0: none)
        self.esz = 4 if path == "f32" else 2
        al = 4 if path == "f32" else 8
        self.cin_p = (cin + al - 1) // al * al
        self.cout_w = cout if path == "f32" else (cout + 7) // 8 * 8          # channels of a pixel the launch writes
        if head:
            self.cout_w = head                                                # fp32 scalars, for either storage
        self.wmode = "w4" if family == "wino4" else "dense"
        self.bwd, self.fwd, self.declines = bwd, fwd, tuple(declines)

    # ---- geometry
    def geom(self):
        from wav2lip_amd._lib import ConvGeom
        return ConvGeom(self.tr, self.cin, self.cout, self.k[0], self.k[1], self.s[0], self.s[1], self.p[0], self.p[1], self.op[0],
                        self.op[1], self.act)

    def out_hw(self):
        if self.path == "thin":
            return self.H, self.W
        ho, wo = C.c_int(), C.c_int()
        g = self.geom()
        rc = lib().w2l_conv_out_hw(C.byref(g), self.H, self.W, C.byref(ho), C.byref(wo))
        return (ho.value, wo.value) if rc == 0 else None

    def strides(self):
        """(x_cs, x_off, y_cs, y_off, r_cs, r_off) in elements; offsets keep every slice 16-byte aligned"""
        if self.wide:
            return (self.wide_x(), 0, self.wide, 0, self.wide, 0)
        if self.head:          # the head writes scalars: the plan's stride of 4, or a slice of a wider pixel
            return (self.cin_p + 24, 8, 12, 4, 0, 0) if self.sliced else (self.cin_p, 0, 4, 0, 0, 0)
        if self.sliced:
            return (self.cin_p + 24, 8, self.cout_w + 24, 8, self.cout_w + (24 if self.res == 3 else 16), 8)
        return (self.cin_p, 0, self.cout_w, 0, self.cout_w, 0)

    def wide_x(self):
        """the x stride of a large-offset case: the y stride scaled by the ratio of output to input pixels, so that both buffers
        land between 1 GiB and 2 GiB"""
        if self.x_wide:
            return self.x_wide
        ho, wo = self.out_hw()
        r = (ho * wo) / float(self.H * self.W)
        return max(self.cin_p, int(round(self.wide * r / 8)) * 8)

    def nbytes(self):
        ho, wo = self.out_hw()
        xs, _, ys, _, rs, _ = self.strides()
        return (self.N * self.H * self.W * xs * self.esz, self.N * ho * wo * ys * self.esz, self.N * ho * wo * rs * self.esz if self.res in (1, 2) else 0)

    def macs(self):
        ho, wo = self.out_hw()
        px = self.H * self.W if self.tr else ho * wo
        return self.N * px * self.cin * self.cout * self.k[0] * self.k[1]

    # ---- what the planning functions say
    def tune_key(self):
        return (self.tr, self.cin, self.cout, self.k[0], self.k[1], self.s[0], self.s[1], self.p[0], self.p[1], self.op[0], self.op[1], 0,
                int(self.res != 0), self.head, self.N, self.H, self.W)

    def applicable(self, cid=None):
        """w2l_tune_entry_applicable: can configuration id `cid` run this launch (config_fits, the launcher's own shape rule)"""
        key = (C.c_int * 17)(*self.tune_key())
        return bool(lib().w2l_tune_entry_applicable(key, self.force if cid is None else cid))

    def wino4_plan(self):
        """w2l_wino4_block_plan: dict form / blocks / r / c / ni"""
        out = (C.c_int * 8)()
        assert lib().w2l_wino4_block_plan(self.N, self.H, self.W, out) == 0
        return dict(zip(("form", "blocks", "r", "c", "ni", "pitch", "pad", "cells"), [int(v) for v in out]))

    def group_plan(self):
        """w2l_conv_block_plan: (bh, bw, ni) of the block the grouped family's launcher picks, None for the other families"""
        if self.path != "f32" or self.family not in GROUPED:
            return None
        out = (C.c_int * 3)()
        assert lib().w2l_conv_block_plan(self.force, self.N, self.H, self.W, out) == 0
        return tuple(int(v) for v in out)

    def group_past_batch(self):
        """several images per block and a last image group that runs past the batch"""
        pl = self.group_plan()
        return pl is not None and pl[2] > 1 and self.N % pl[2] != 0

    def convb_resolve(self):
        """w2l_convb_resolve_geom for the automatic tile: (family, tile, ksplit)"""
        from wav2lip_amd import bf16
        return bf16.ConvB.resolve_geom(self.geom(), self.N, self.H, self.W, res=bool(self.res))

    def gemm_rows(self):
        """M of the implicit GEMM: output pixels, of one phase for a strided transposed conv"""
        ho, wo = self.out_hw()
        if self.tr and self.s != (1, 1):
            return self.N * (-(-ho // self.s[0])) * (-(-wo // self.s[1]))
        return self.N * ho * wo

    def tile(self):
        if self.path == "bf16":
            return BF16_TILES[self.force] if self.force >= 0 else None
        idx = self.force if self.family == "igemm" else self.force - config_id("split")
        return F32_TILES[idx]

    def ksteps(self):
        """K-steps of the deepest phase (what split-K divides): taps of that phase x padded channels, in steps of KSTEP"""
        taps = self.k[0] * self.k[1]
        if self.tr and self.s != (1, 1):
            taps = (-(-self.k[0] // self.s[0])) * (-(-self.k[1] // self.s[1]))
        elif self.tr and (self.H, self.W) == (1, 1):
            taps = 1                                                    # unit input: every output pixel is one tap
        step = KSTEP[self.path]
        return -(-taps * self.cin_p // step)

    def splits(self):
        """(split-K the launcher resolves to, K-steps per split) for the forced ks"""
        steps = self.ksteps()
        ks = max(1, min(self.ks or 1, steps))
        per = -(-steps // ks)
        return -(-steps // per), per

    # ---- exactness
    def exact_bound(self):
        """the largest magnitude an intermediate can reach, counted in the finest unit that occurs (so that it is an integer); must be
        < LIMIT.  A is the accumulator's bound in its own unit q (1, or 1/4 for F(2x2)); A * scale is exact for a power-of-two scale;
        adding shift and residual (|.| <= extra) to A * 2 needs 2 A + extra / q, to A / 2 (unit q / 2) needs A + 2 extra / q."""
        extra = 3 + (3 if self.res == 3 else 1 if self.res else 0)      # |shift| <= 3, |res| <= 1, |prior| <= 3 (in place)
        smax = max(abs(s) for s in self.scales())
        if self.head:          # a sum of cout such values times weights from {-1, 0, 1}, plus a bias |.| <= 3
            inner = Case(self.path, "k3s" if self.family == "k3s_head" else self.family, self.tr, self.cin, self.cout, self.k, self.s,
                         self.p, self.op, self.N, self.H, self.W)
            return self.cout * inner.exact_bound() + 8 * 3 + 1
        if self.family in ("wino", "wino2", "wino2s"):
            return int(smax * WINO2_GROWTH * self.cin) + 8 * extra + 1
        if self.family == "wino4":
            return int(smax * WINO4_GROWTH * min(self.cin, W4_LIVE_CIN)) + 2 * extra + 1
        return int(smax * self.k[0] * self.k[1] * self.cin) + 2 * extra + 1

    def scales(self):
        return (1.0, -1.0, 0.5, -0.5) if self.family == "wino4" else (1.0, -1.0, 2.0, -2.0, 0.5, -0.5)

    def describe(self):
        s = "%s %d->%d %dx%d s%dx%d p%d%s @%dx%d N=%d" % ("convT" if self.tr else "conv", self.cin, self.cout, self.k[0], self.k[1],
                                                          self.s[0], self.s[1], self.p[0],
                                                          "+(%d,%d)" % self.op if self.op[0] != self.op[1] else "+%d" % self.op[0] if self.op[0] else "",
                                                          self.H, self.W, self.N)
        if self.force >= 0:
            s += " id %d" % self.force
        if self.ks:
            s += " ks %d" % self.ks
        if self.res:
            s += " res" + {1: "", 2: "=x", 3: "=y"}[self.res]
        if self.head:
            s += " head %d" % self.head
        if self.sliced:
            s += " sliced"
        if self.wide:
            s += " cs %d" % self.wide
        return s

    def key(self):
        return (self.path, self.family, self.tr, self.cin, self.cout, self.k, self.s, self.p, self.op, self.N, self.H, self.W, self.force,
                self.ks, self.res, self.act, self.sliced, self.wide, self.head, self.bwd, self.declines)

    def with_seed(self, seed):
        """the same launch with operands from another seed"""
        import copy
        c = copy.copy(self)
        c.seed = seed
        return c

    def __repr__(self):
        return "%s/%s %s" % (self.path, self.family, self.describe())


# ---------------------------------------------------------------- operands and references
def image_map(case):
    """(number of distinct images D, [N] index of each batch image into the stack of D).  Small batches: every image its own.  The
    batches that only exist to fill the chip (the bf16 special-case kernels) repeat 7 distinct images, an odd period that no
    power-of-two grouping of images aligns with; a large-offset case has data in its first and last image and zeros between (image
    2 of its stack).  The reference is computed once per distinct image."""
    if case.wide:
        return 3, [0] + [2] * (case.N - 2) + [1]
    if case.N > 16:
        return 7, [n % 7 for n in range(case.N)]
    return case.N, list(range(case.N))



def int_operands(case):
    """(x [D,cin,H,W], w (torch layout), scale [cout], shift [cout], res [D,cout,Ho,Wo] or None) as float64 tensors of integers /
    dyadic fractions, a third zeros, from the case's seed; D distinct images (image_map)"""
    g = torch.Generator().manual_seed(1000 + case.seed)
    ho, wo = case.out_hw()
    D = image_map(case)[0]

    def tern(*shape):
        return (torch.randint(0, 3, shape, generator=g) - 1).double()
    x = tern(D, case.cin, case.H, case.W)
    wshape = (case.cin, case.cout) if case.tr else (case.cout, case.cin)
    if case.wmode == "w4":                                               # one tap of (0..1, 0..1) per channel pair, times 576
        w = torch.zeros(wshape + (3, 3), dtype=torch.float64)
        val = tern(*wshape) * 576.0
        ti = torch.randint(0, 2, wshape, generator=g)
        tj = torch.randint(0, 2, wshape, generator=g)
        a, b = torch.meshgrid(torch.arange(wshape[0]), torch.arange(wshape[1]), indexing="ij")
        w[a, b, ti, tj] = val
        if case.cin > W4_LIVE_CIN:                                       # at most W4_LIVE_CIN live input channels per cout
            co_axis = 1 if case.tr else 0
            keep = torch.zeros(wshape, dtype=torch.bool)
            for o in range(case.cout):
                live = torch.randperm(case.cin, generator=g)[:W4_LIVE_CIN]
                if case.tr:
                    keep[live, o] = True
                else:
                    keep[o, live] = True
            w = w * keep[:, :, None, None].double()
    else:
        w = tern(*(wshape + case.k))
    sc = torch.tensor(case.scales(), dtype=torch.float64)
    scale = sc[torch.randint(0, len(sc), (case.cout,), generator=g)]
    shift = (torch.randint(0, 7, (case.cout,), generator=g) - 3).double()
    res = None
    if case.res == 1:
        res = tern(D, case.cout, ho, wo)
    elif case.res == 2:
        assert case.cin == case.cout and (ho, wo) == (case.H, case.W)
        res = x
    elif case.res == 3:                                                  # the prior gradient the output slice already holds
        res = (torch.randint(0, 7, (D, case.cout, ho, wo), generator=g) - 3).double()
    if case.bwd:
        scale, shift = torch.ones_like(scale), torch.zeros_like(shift)
    if case.wide:
        x[2] = 0
        if case.res == 1:
            res[2] = 0
    if case.path == "thin":
        scale = torch.ones_like(scale)
    return x, w, scale, shift, res


def head_operands(case):
    """(head_w [head_c, cout], head_b [head_c]) of a fused 1x1 head: integers from {-1, 0, 1} and [-3, 3]"""
    g = torch.Generator().manual_seed(3000 + case.seed)
    hw = (torch.randint(0, 3, (case.head, case.cout), generator=g) - 1).double()
    hb = (torch.randint(0, 7, (case.head,), generator=g) - 3).double()
    return hw, hb


def head_ref(h, hw, hb):
    """the 1x1 head without activation over the block's output h [D, cout, H, W], float64"""
    return torch.einsum("oc,nchw->nohw", hw, h) + hb.view(1, -1, 1, 1)


def gauss_operands(case):
    """Gaussian operands of the accuracy run (weights scaled by 1/sqrt(fan-in)); bf16-rounded for the bf16 kernels"""
    g = torch.Generator().manual_seed(5000 + case.seed)
    ho, wo = case.out_hw()
    D = image_map(case)[0]
    x = torch.randn(D, case.cin, case.H, case.W, generator=g)
    wshape = ((case.cin, case.cout) if case.tr else (case.cout, case.cin)) + case.k
    w = torch.randn(wshape, generator=g) / float(np.sqrt(case.cin * case.k[0] * case.k[1]))
    scale = torch.rand(case.cout, generator=g) + 0.5
    shift = torch.randn(case.cout, generator=g) * 0.2
    res = torch.randn(D, case.cout, ho, wo, generator=g) if case.res in (1, 3) else (x if case.res == 2 else None)
    if case.bwd:
        scale, shift = torch.ones_like(scale), torch.zeros_like(shift)
    if case.path == "thin":
        scale = torch.ones_like(scale)
    if case.path != "f32":
        x, w = x.bfloat16().float(), w.bfloat16().float()
        res = None if res is None else res.bfloat16().float()
    return x.double(), w.double(), scale.double(), shift.double(), None if res is None else res.double()


def ref64(case, x, w, scale, shift, res, dtype=torch.float64):
    """act( conv(x, w) * scale + shift (+ res) ) with torch's CPU convolution in `dtype` (float64: THE reference)"""
    x, w = x.to(dtype), w.to(dtype)
    if case.tr:
        z = F.conv_transpose2d(x, w, None, case.s, case.p, case.op)
    else:
        z = F.conv2d(x, w, None, case.s, case.p)
    z = z * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    if res is not None:
        z = z + res.to(dtype)
    if case.act == ACT_RELU:
        z = z.clamp_min(0)
    return z


def conv_loops(x, w, tr, s, p, op, scale, shift, res, relu):
    """the same operation as plain numpy loops (no torch): x [N,cin,H,W], w in torch layout -> [N,cout,Ho,Wo], float64"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, cin, H, W = x.shape
    kh, kw = w.shape[2:]
    if tr:
        cout = w.shape[1]
        Ho, Wo = (H - 1) * s[0] - 2 * p[0] + kh + op[0], (W - 1) * s[1] - 2 * p[1] + kw + op[1]
    else:
        cout = w.shape[0]
        Ho, Wo = (H + 2 * p[0] - kh) // s[0] + 1, (W + 2 * p[1] - kw) // s[1] + 1
    z = np.zeros((N, cout, Ho, Wo))
    for n in range(N):
        for o in range(cout):
            for c in range(cin):
                for i in range(kh):
                    for j in range(kw):
                        wv = w[c, o, i, j] if tr else w[o, c, i, j]
                        if wv == 0.0:
                            continue
                        for yy in range(H if tr else Ho):
                            for xx in range(W if tr else Wo):
                                if tr:     # input pixel (yy, xx) scatters to output (yy*s - p + i, xx*s - p + j)
                                    oy, ox = yy * s[0] - p[0] + i, xx * s[1] - p[1] + j
                                    if 0 <= oy < Ho and 0 <= ox < Wo:
                                        z[n, o, oy, ox] += wv * x[n, c, yy, xx]
                                else:      # output pixel (yy, xx) gathers input (yy*s - p + i, xx*s - p + j)
                                    iy, ix = yy * s[0] - p[0] + i, xx * s[1] - p[1] + j
                                    if 0 <= iy < H and 0 <= ix < W:
                                        z[n, o, yy, xx] += wv * x[n, c, iy, ix]
    z = z * np.asarray(scale, np.float64).reshape(1, -1, 1, 1) + np.asarray(shift, np.float64).reshape(1, -1, 1, 1)
    if res is not None:
        z = z + np.asarray(res, np.float64)
    return np.maximum(z, 0.0) if relu else z


def guard_elems(cs, esz):
    """elements of one guard band of a buffer with channel stride cs: GUARD_PIXELS pixels' worth, at least GUARD_MIN_BYTES, a
    multiple of 16 bytes (the tensor between the guards stays 16-byte aligned)"""
    n = max(GUARD_PIXELS * cs, GUARD_MIN_BYTES // esz)
    return (n + 7) // 8 * 8


# ---------------------------------------------------------------- candidates
# every (transposed, k, stride, pad, output padding) combination of test_conv_gpu.SIGS in order of first appearance, with the extent
# of that first signature reduced to <= 13 x 11 (sigs_geoms() derives it; test_conv_cases_cpu.py holds the two equal)
SIGS_GEOMS = (
    (False, 3, (1, 1), 1, 0, 13, 11), (False, 3, (3, 1), 1, 0, 13, 11), (False, 3, (3, 3), 1, 0, 13, 11),
    (False, 3, (3, 2), 1, 0, 9, 6), (False, 3, (1, 1), 0, 0, 3, 3), (False, 1, (1, 1), 0, 0, 1, 1),
    (False, 7, (1, 1), 3, 0, 13, 11), (False, 3, (2, 2), 1, 0, 13, 11), (True, 3, (1, 1), 0, 0, 1, 1),
    (True, 3, (2, 2), 1, 1, 3, 3), (False, 5, (1, 2), 1, 0, 13, 11), (False, 5, (1, 2), 2, 0, 13, 11),
    (False, 5, (1, 1), 2, 0, 13, 11), (False, 5, (2, 2), 2, 0, 13, 11),
)


def sigs_geoms(sigs):
    """SIGS_GEOMS from a list of signatures in the form of test_conv_gpu.SIGS"""
    seen, out = set(), []
    for kind, k, s, p, _cin, _cout, H, W, _res, op in sigs:
        key = (kind == "t", k, _pair(s), p, op)
        if key in seen:
            continue
        seen.add(key)
        out.append(key + (min(H, 13), min(W, 11)))
    return tuple(out)


def igemm_candidates(path, family):
    """every SIGS geometry on every tile, cin rotating through IGEMM_CIN (cin_p > cin occurs), cout = tile width + 8 (ragged), N = 3;
    the split-K triple 2 / 3 / more splits than K-steps on 3x3 layers of 32 and 15 channels and a strided transposed one; residual and
    channel-slice forms"""
    tiles = (F32_TILES if path == "f32" else BF16_TILES)[:num_tiles(path)]
    base = 0 if family != "split" else config_id("split")
    out = []
    for gi, (tr, k, s, p, op, H, W) in enumerate(SIGS_GEOMS):
        for ti, (bm, bn) in enumerate(tiles):
            cin = IGEMM_CIN[(gi + ti) % len(IGEMM_CIN)]
            out.append(Case(path, family, tr, cin, bn + 8, k, s, p, op, 3, H, W, force=base + ti, seed=gi * 8 + ti))
    for ti, (bm, bn) in enumerate(tiles):
        for ks in (2, 3, 64):
            for cin in (32, 15):
                out.append(Case(path, family, 0, cin, bn + 8, 3, 1, 1, 0, 3, 9, 7, force=base + ti, ks=ks, seed=100 + ti))
            out.append(Case(path, family, 1, 80, bn + 8, 3, 2, 1, 1, 2, 5, 3, force=base + ti, ks=ks, seed=120 + ti))
        out.append(Case(path, family, 0, 15, bn + 8, 3, 1, 1, 0, 3, 9, 7, force=base + ti, res=1, seed=140 + ti))
        out.append(Case(path, family, 0, 64, 64, 3, 1, 1, 0, 3, 9, 7, force=base + ti, res=2, seed=150 + ti))
        out.append(Case(path, family, 0, 15, bn + 8, 3, 1, 1, 0, 3, 9, 7, force=base + ti, res=1, sliced=True, seed=160 + ti))
        out.append(Case(path, family, 0, 64, 64, 3, 1, 1, 0, 2, 9, 7, force=base + ti, res=2, sliced=True, ks=2, seed=170 + ti))
    if path == "f32":     # cout <= 16 at x-stride 1: the launcher pairs adjacent output pixels when the width is even
        out.append(Case(path, family, 0, 6, 16, 7, 1, 3, 0, 2, 10, 12, force=base + 4, seed=180))
        out.append(Case(path, family, 0, 3, 12, 5, 1, 2, 0, 2, 7, 6, force=base + 4, seed=181))
    return out


def wino_candidates(cid):
    fam = [f for f, ids in WINO_IDS.items() if cid in ids][0]
    cin, cout = WINO_CH[cid]
    out = []
    ns = (1, 3, 9) + ((2, 4, 5, 6, 7, 8, 10, 11, 13, 17) if fam == "wino4" else (5,))
    for (H, W), N in itertools.product(WINO_HW, ns):
        out.append(Case("f32", fam, 0, cin, cout, 3, 1, 1, 0, N, H, W, force=cid, seed=cid * 100 + H + N))
    for N in (3,):
        out.append(Case("f32", fam, 0, cin, cout, 3, 1, 1, 0, N, 5, 4, force=cid, res=1, seed=cid * 100 + 50))
        out.append(Case("f32", fam, 0, cin, cout, 3, 1, 1, 0, N, 13, 11, force=cid, res=1, sliced=True, seed=cid * 100 + 51))
        c2 = max(cin, cout)
        out.append(Case("f32", fam, 0, c2, c2, 3, 1, 1, 0, N, 5, 4, force=cid, res=2, seed=cid * 100 + 52))
        out.append(Case("f32", fam, 0, c2, c2, 3, 1, 1, 0, N, 5, 4, force=cid, res=2, sliced=True, seed=cid * 100 + 53))
    return out


def tp2_candidates(family):
    cid = config_id(family)
    out = []
    sigs = TP2_SIGS + (((16, 64, 5, 7),) if family == "tp2s" else ())      # conv_tp2s takes multiples of 16 input channels
    for (cin, cout, H, W), N in itertools.product(sigs, (1, 3, 7)):
        out.append(Case("f32", family, 1, cin, cout, 3, 2, 1, 1, N, H, W, force=cid, seed=300 + cin + N))
        if family == "tp2s":
            for ks in (2, 3, 64):
                out.append(Case("f32", family, 1, cin, cout, 3, 2, 1, 1, N, H, W, force=cid, ks=ks, seed=320 + cin + N))
    out.append(Case("f32", family, 1, 64, 64, 3, 2, 1, 1, 3, 9, 16, force=cid, sliced=True, seed=340))
    if family == "tp2s":      # five K-steps: three splits of 2, 2, 1
        out.append(Case("f32", family, 1, 80, 64, 3, 2, 1, 1, 2, 3, 2, force=cid, ks=3, seed=341))
    return out


def stem7s_candidates():
    cid = config_id("stem7s")
    out = [Case("f32", "stem7s", 0, cin, 16, 7, 1, 3, 0, N, H, W, force=cid, seed=400 + cin + H)
           for cin, (H, W), N in itertools.product(STEM_CIN, STEM_HW, (1, 3))]
    out.append(Case("f32", "stem7s", 0, 6, 16, 7, 1, 3, 0, 2, 16, 16, force=cid, sliced=True, seed=440))
    return out


def k3s_candidates():
    cid = config_id("k3s")
    out = [Case("f32", "k3s", 0, cin, 32, 3, 1, 1, 0, N, H, W, force=cid, seed=500 + cin + H)
           for cin, (H, W), N in itertools.product(K3S_CIN, K3S_HW, (1, 3, 5, 9))]
    out.append(Case("f32", "k3s", 0, 16, 32, 3, 1, 1, 0, 3, 5, 7, force=cid, res=1, seed=540))
    out.append(Case("f32", "k3s", 0, 32, 32, 3, 1, 1, 0, 3, 5, 7, force=cid, res=2, seed=541))
    out.append(Case("f32", "k3s", 0, 32, 32, 3, 1, 1, 0, 3, 5, 7, force=cid, res=2, sliced=True, seed=542))
    return out


def convb_special_candidates():
    """the bf16 launcher's special-case kernels are rules of the SHAPE (w2l_convb_resolve_geom): each needs enough tiles to fill the
    chip, so the batch is what grows, never the extent"""
    out = []
    for cin, (H, W), N in itertools.product(STEM_CIN, STEM_HW, (3, 1024, 1030)):
        for cout in (16, 32):
            out.append(Case("bf16", "stem", 0, cin, cout, 7, 1, 3, 0, N, H, W, seed=600 + cin + H))
    for N in (2048, 2051):
        out.append(Case("bf16", "stem", 0, 32, 32, 3, 1, 1, 0, N, 16, 16, res=1, seed=620))
        out.append(Case("bf16", "stem", 0, 80, 32, 3, 1, 1, 0, N, 16, 16, seed=621))
        out.append(Case("bf16", "box64", 0, 64, 64, 3, 1, 1, 0, N, 16, 16, seed=630))
        out.append(Case("bf16", "box64", 0, 64, 64, 3, 1, 1, 0, N, 16, 16, res=2, seed=631))
        out.append(Case("bf16", "box64", 0, 64, 60, 3, 1, 1, 0, N, 15, 15, res=1, sliced=True, seed=632))
    for (cin, cout, H, W), N in itertools.product(((32, 32, 5, 7), (64, 24, 1, 1), (32, 32, 9, 16)), (3, 520, 2049)):
        out.append(Case("bf16", "tp2b", 1, cin, cout, 3, 2, 1, 1, N, H, W, seed=640 + cin + N % 7))
    out.append(Case("bf16", "tp2b", 1, 32, 32, 3, 2, 1, 1, 1030, 5, 7, sliced=True, seed=650))
    out.append(Case("bf16", "stem", 0, 6, 16, 7, 1, 3, 0, 1030, 16, 16, sliced=True, seed=651))
    return out


def head_candidates():
    """a 3x3 block with a fused 1x1 head that has NO activation (both ABIs accept it; the sigmoid head is not exact and stays with
    the existing tests): every implicit-GEMM and split-operand tile that holds 32 couts in one row, conv_wino2's two 32-cout shapes,
    conv_k3s, and the bf16-storage output block"""
    out = []
    for base in (0, config_id("split")):
        fam = "igemm" if base == 0 else "split"
        for ti in range(len(F32_TILES)):
            out.append(Case("f32", fam, 0, 15, 32, 3, 1, 1, 0, 3, 9, 7, force=base + ti, head=3, seed=1000 + base + ti))
    for cid in (9, 12):
        for (H, W), hc in (((13, 11), 3), ((5, 4), 1), ((1, 1), 4)):
            out.append(Case("f32", "wino2", 0, 8, 32, 3, 1, 1, 0, 3, H, W, force=cid, head=hc, seed=1020 + cid + H))
        out.append(Case("f32", "wino2", 0, 8, 32, 3, 1, 1, 0, 3, 5, 4, force=cid, head=3, sliced=True, seed=1030 + cid))
    for path, fam, cid in (("f32", "k3s", config_id("k3s")), ("bf16", "k3s_head", -1)):
        for cin, (H, W), N, hc in ((16, (5, 7), 3, 3), (80, (20, 24), 1, 4), (48, (1, 1), 9, 1)):
            out.append(Case(path, fam, 0, cin, 32, 3, 1, 1, 0, N, H, W, force=cid, head=hc, seed=1040 + cin))
        out.append(Case(path, fam, 0, 16, 32, 3, 1, 1, 0, 3, 5, 7, force=cid, head=3, sliced=True, seed=1050))
    return out


def thin_candidates():
    out = []
    for cin, cout, npix in itertools.product((5, 16, 32), (1, 3, 4), (1, 255, 777)):      # one image of 1 x npix pixels
        # a handful of outputs: no activation, so that the reference is not all zero after the ReLU
        out.append(Case("thin", "thin", 0, cin, cout, 1, 1, 0, 0, 1, 1, npix, act=ACT_NONE if npix == 1 else ACT_RELU,
                        seed=710 + cin + 3 * cout))
    out.append(Case("thin", "thin", 0, 32, 3, 1, 1, 0, 0, 1, 1, 777, sliced=True, seed=740))
    return out


def large_candidates():
    """one case per launcher with x and y (and the residual where the family has one) between 1 GiB and the 2 GiB guard: wide channel
    strides, small channel counts, data in the first and last image only"""
    out = []

    def f32(family, cid, tr, cin, cout, k, s, p, op, N, H, W, wide, res=0, ks=0):
        out.append(Case("f32", family, tr, cin, cout, k, s, p, op, N, H, W, force=cid, ks=ks, res=res, wide=wide, seed=800 + cid))
    f32("igemm", 3, 0, 8, 72, 3, 1, 1, 0, 4096, 12, 12, 512, res=1)
    f32("igemm", 1, 0, 8, 72, 3, 2, 1, 0, 4096, 12, 12, 2048, ks=2)          # strided: y has a quarter of the pixels
    f32("split", config_id("split") + 3, 0, 8, 72, 3, 1, 1, 0, 4096, 12, 12, 512, res=1)
    for cid in (6, 7, 8, 9, 12, 11, 19):
        fam = [f for f, ids in WINO_IDS.items() if cid in ids][0]
        cin, cout = WINO_CH[cid]
        f32(fam, cid, 0, cin, cout, 3, 1, 1, 0, 4096, 12, 12, 512, res=1)
    f32("tp2", config_id("tp2"), 1, 8, 64, 3, 2, 1, 1, 16384, 5, 7, 128)
    f32("tp2s", config_id("tp2s"), 1, 16, 64, 3, 2, 1, 1, 16384, 5, 7, 128)
    f32("tp2s", config_id("tp2s"), 1, 32, 64, 3, 2, 1, 1, 16384, 5, 7, 128, ks=2)
    f32("stem7s", config_id("stem7s"), 0, 6, 16, 7, 1, 3, 0, 4096, 12, 12, 512)
    f32("k3s", config_id("k3s"), 0, 16, 32, 3, 1, 1, 0, 4096, 12, 12, 512, res=1)
    out.append(Case("bf16", "igemm", 0, 8, 72, 3, 1, 1, 0, 4096, 12, 12, force=3, res=1, wide=1024, seed=900))
    out.append(Case("bf16", "igemm", 0, 8, 72, 3, 1, 1, 0, 4096, 12, 12, force=1, ks=2, wide=1024, seed=901))
    out.append(Case("bf16", "stem", 0, 6, 16, 7, 1, 3, 0, 4200, 16, 16, wide=512, seed=902))
    out.append(Case("bf16", "box64", 0, 64, 64, 3, 1, 1, 0, 4200, 16, 16, res=1, wide=512, seed=903))
    out.append(Case("bf16", "tp2b", 1, 32, 32, 3, 2, 1, 1, 16384, 5, 7, wide=256, seed=904))
    out.append(Case("thin", "thin", 0, 32, 3, 1, 1, 0, 0, 600, 1, 1000, wide=1024, seed=905))
    return out


# ---------------------------------------------------------------- the backward pass: data-gradient launches and weight re-packs
def dgrad_op(tr, k, s, p, H, W):
    """the output padding of the data-gradient launch of a layer over an [H, W] input, restated from the definition: the gradient of a
    transposed layer is a plain conv (no output padding); a conv's floor division drops (H + 2p - k) % s rows (columns) of the padded
    input, and its gradient - a transposed conv over the conv's output - must produce them again"""
    k, s, p = _pair(k), _pair(s), _pair(p)
    if tr:
        return (0, 0)
    return ((H + 2 * p[0] - k[0]) % s[0], (W + 2 * p[1] - k[1]) % s[1])


def dgrad_of(path, family, sig, N, H, W, **kw):
    """the Case of the data-gradient launch of the forward layer sig = (tr, cin, cout, k, s, p, op) over an [N, H, W] input, as
    autograd.NodeF builds it: the other interpretation of the same weight tensor, channel roles swapped, no activation, scale 1, shift 0;
    its input is dz (the forward output's extent), its output the gradient of x.  None if the forward layer has no output."""
    tr, cin, cout, k, s, p, op = sig
    hw = Case(path, "igemm", tr, cin, cout, k, s, p, op, N, H, W).out_hw()
    if hw is None or min(hw) < 1:
        return None
    return Case(path, family, 0 if tr else 1, cout, cin, k, s, p, dgrad_op(tr, k, s, p, H, W), N, hw[0], hw[1], act=ACT_NONE, bwd=True,
                fwd=(sig, H, W), **kw)


def geom_label(tr, k, s, p, op):
    s = _pair(s)
    return "%s %dx%d s%s p%d%s" % ("convT" if tr else "conv", k, k, "%d" % s[0] if s[0] == s[1] else "(%d,%d)" % s, p, "+%d" % op if op else "")


# forward input extents per (transposed, k, stride, pad, output padding) row of SIGS_GEOMS: the smallest at which the backward form can
# go wrong.  Stride 3 takes {4, 5, 6} (output padding 0, 1, 2), stride 2 takes {5, 6}, each against a small odd extent on the other axis.
BWD_EXTENTS = {
    (False, 3, (1, 1), 1, 0): ((1, 1), (5, 4)),
    (False, 3, (3, 1), 1, 0): ((4, 3), (5, 3), (6, 5)),
    (False, 3, (3, 3), 1, 0): ((4, 5), (5, 7), (6, 5), (5, 6), (3, 4)),
    (False, 3, (3, 2), 1, 0): ((4, 5), (5, 6), (6, 5), (4, 6)),
    (False, 3, (1, 1), 0, 0): ((3, 3), (4, 5)),                  # 3x3 -> 1x1: the backward launch is the unit-input variant
    (False, 1, (1, 1), 0, 0): ((1, 1), (5, 4)),
    (False, 7, (1, 1), 3, 0): ((5, 3), (10, 12)),
    (False, 3, (2, 2), 1, 0): ((5, 3), (6, 5), (5, 6), (6, 6)),
    (True, 3, (1, 1), 0, 0): ((1, 1), (3, 2)),                   # backward: a plain 3x3 s1 p0 conv
    (True, 3, (2, 2), 1, 1): ((3, 3), (2, 3)),                   # backward: a 3x3 s2 p1 conv
    (False, 5, (1, 2), 1, 0): ((6, 7), (6, 8)),
    (False, 5, (1, 2), 2, 0): ((6, 7), (6, 8)),
    (False, 5, (1, 1), 2, 0): ((5, 4),),
    (False, 5, (2, 2), 2, 0): ((5, 6), (6, 5), (6, 6)),
}


def bwd_igemm_candidates(path, family):
    """the data gradient of every SIGS geometry at every extent of BWD_EXTENTS, tiles and the forward cout (the launch's cin) rotating,
    forward cin (the launch's cout) = tile width + 8 (ragged), N in {2, 3}; on every tile the accumulating forms: in place, in place
    with split-K 2 and 3 (ten fp32 / five bf16 K-steps), in place into a channel slice, in place for a stride-1 layer and for a
    transposed layer (whose gradient is a plain conv), in place with 15 couts; once the x-paired variant"""
    tiles = (F32_TILES if path == "f32" else BF16_TILES)[:num_tiles(path)]
    base = 0 if family != "split" else config_id("split")
    out = []
    for gi, (tr, k, s, p, op, _H, _W) in enumerate(SIGS_GEOMS):
        for ei, hw in enumerate(BWD_EXTENTS[(tr, k, s, p, op)]):
            ti = (gi + ei) % len(tiles)
            ch = IGEMM_CIN[(gi + 2 * ei) % len(IGEMM_CIN)]
            out.append(dgrad_of(path, family, (tr, tiles[ti][1] + 8, ch, k, s, p, op), 2 + (gi + ei) % 2, hw[0], hw[1], force=base + ti,
                                seed=2000 + gi * 8 + ei))
    for ti, (_bm, bn) in enumerate(tiles):
        f, c = base + ti, bn + 8
        out.append(dgrad_of(path, family, (0, c, 15, 3, 2, 1, 0), 3, 6, 5, force=f, res=3, seed=2200 + ti))
        for ks in (2, 3):
            out.append(dgrad_of(path, family, (0, c, 80, 3, 2, 1, 0), 2, 6, 5, force=f, res=3, ks=ks, seed=2210 + ti))
        out.append(dgrad_of(path, family, (0, c, 15, 3, 2, 1, 0), 3, 5, 6, force=f, res=3, sliced=True, seed=2220 + ti))
        out.append(dgrad_of(path, family, (0, c, 80, 3, 2, 1, 0), 2, 6, 6, force=f, res=3, sliced=True, ks=2, seed=2230 + ti))
        out.append(dgrad_of(path, family, (0, c, 15, 3, 1, 1, 0), 3, 5, 4, force=f, res=3, seed=2240 + ti))
        out.append(dgrad_of(path, family, (1, c, 15, 3, 2, 1, 1), 3, 3, 2, force=f, res=3, seed=2250 + ti))
        # 15 couts: rows that are no multiple of 16 bytes in fp32, so the epilogue that adds the prior is the scalar one
        out.append(dgrad_of(path, family, (0, 15, 32, 3, 2, 1, 0), 3, 6, 5, force=f, res=3, seed=2260 + ti))
        out.append(dgrad_of(path, family, (0, 15, 80, 3, 2, 1, 0), 2, 6, 5, force=f, res=3, ks=2, seed=2270 + ti))
    # the gradient of a transposed s1 p0 layer with 16 input channels is a plain conv with 16 couts and an even output width: the
    # fp32 launcher takes its x-paired variant
    out.append(dgrad_of(path, family, (1, 16, 15, 3, 1, 0, 0), 2, 3, 2, force=base + 4, seed=2280))
    return [c for c in out if c is not None]


BWD_WINO_HW = ((1, 1), (3, 3), (5, 4), (13, 11))


def bwd_wino_candidates(cid):
    """a Winograd kernel run with transposed = 1 (the data gradient of a 3x3 s1 p1 layer: the packer reads the weights flipped, channel
    roles swapped) at the launch's minimum channel counts"""
    fam = [f for f, ids in WINO_IDS.items() if cid in ids][0]
    cin, cout = WINO_CH[cid]
    sig = (0, cout, cin, 3, 1, 1, 0)                                     # the forward layer: its cout is the launch's cin
    out = []
    for (H, W), N in itertools.product(BWD_WINO_HW, (2, 3, 5)):
        out.append(dgrad_of("f32", fam, sig, N, H, W, force=cid, seed=2400 + cid * 20 + H + N))
    for (H, W), N in (((1, 1), 5), ((5, 4), 3), ((13, 11), 2), ((13, 11), 5)):
        out.append(dgrad_of("f32", fam, sig, N, H, W, force=cid, res=3, seed=2410 + cid * 20 + H))
    for (H, W), N in (((5, 4), 3), ((13, 11), 3)):
        out.append(dgrad_of("f32", fam, sig, N, H, W, force=cid, res=3, sliced=True, seed=2415 + cid * 20 + H))
    return out


def bwd_tp2_candidates(family):
    """conv_tp2 / conv_tp2s as the data gradient of a 3x3 s2 p1 conv over EVEN extents (output padding 1 on both axes); in the "tp2"
    pool also the launches the two kernels must decline - an accumulating launch (neither kernel has a residual operand) and an odd
    extent (output padding 0) - which run on an implicit-GEMM tile instead"""
    cid = config_id(family)
    c0 = 16 if family == "tp2s" else 8
    out = []
    for (cin, cout, H, W), N in itertools.product(((c0, 64, 3, 2), (16, 128, 1, 1), (64, 64, 2, 3)), (2, 3)):
        sig = (0, cout, cin, 3, 2, 1, 0)
        out.append(dgrad_of("f32", family, sig, N, 2 * H, 2 * W, force=cid, seed=2600 + cin + N))
        if family == "tp2s":
            out.append(dgrad_of("f32", family, sig, N, 2 * H, 2 * W, force=cid, ks=2, seed=2620 + cin + N))
    if family == "tp2":
        both = (config_id("tp2"), config_id("tp2s"))
        sig = (0, 64, 16, 3, 2, 1, 0)
        out.append(dgrad_of("f32", "igemm", sig, 3, 6, 4, force=3, res=3, declines=both, seed=2640))
        for H, W in ((5, 5), (5, 6), (6, 5)):
            out.append(dgrad_of("f32", "igemm", sig, 2, H, W, force=3, declines=both, seed=2641 + H + 2 * W))
    return out


def bwd_convb_special_candidates():
    """the bf16 launcher's special-case kernels in backward form: box64 with transposed = 1 (the data gradient of a 64 -> 64 3x3 s1 p1
    layer), tp2b as the data gradient of a 3x3 s2 p1 conv; each plain and accumulating in place; batches that fill the chip, seven
    distinct images (image_map)"""
    out = []
    for N in (2048, 2051):
        for res in (0, 3):
            out.append(dgrad_of("bf16", "box64", (0, 64, 64, 3, 1, 1, 0), N, 16, 16, res=res, seed=2700 + res))
    for (c, H, W), N in itertools.product(((32, 10, 14), (32, 2, 2)), (1030, 2049)):
        for res in (0, 3):
            out.append(dgrad_of("bf16", "tp2b", (0, c, c, 3, 2, 1, 0), N, H, W, res=res, seed=2720 + H + res))
    out.append(dgrad_of("bf16", "tp2b", (0, 32, 32, 3, 2, 1, 0), 1030, 10, 14, res=3, sliced=True, seed=2740))
    return out


def update_candidates():
    """one small launch per packed weight form that w2l_conv_update / w2l_convb_update(_many) must refresh"""
    sp, out = config_id("split"), []

    def f32(family, cid, tr, cin, cout, k, s, p, op, N, H, W, **kw):
        out.append(Case("f32", family, tr, cin, cout, k, s, p, op, N, H, W, force=cid, seed=3100 + len(out), **kw))
    for fam, base in (("igemm", 0), ("split", sp)):                      # w_dev of each variant, then its lazily built w_split planes
        f32(fam, base + 4, 0, 15, 40, 3, 1, 1, 0, 2, 5, 4)               # generic
        f32(fam, base + 4, 1, 6, 40, 3, 1, 0, 0, 3, 1, 1)                # unit-input: transposed s1 over a 1x1 input
        f32(fam, base + 4, 0, 6, 16, 7, 1, 3, 0, 2, 5, 4)                # x-paired: cout <= 16, even output width, no residual
        f32(fam, base + 3, 1, 15, 72, 3, 2, 1, 1, 2, 3, 2)               # generic, four phases
    for cid in (6, 7, 8, 9, 12, 11, 19):
        fam = [f for f, ids in WINO_IDS.items() if cid in ids][0]
        cin, cout = WINO_CH[cid]
        for tr in (0, 1):
            f32(fam, cid, tr, cin, cout, 3, 1, 1, 0, 2, 5, 4, act=ACT_NONE if tr else ACT_RELU)
    f32("tp2", config_id("tp2"), 1, 8, 64, 3, 2, 1, 1, 2, 3, 2)
    f32("tp2s", config_id("tp2s"), 1, 32, 64, 3, 2, 1, 1, 2, 3, 2)
    f32("tp2s", config_id("tp2s"), 1, 32, 64, 3, 2, 1, 1, 2, 3, 2, ks=2)
    f32("stem7s", config_id("stem7s"), 0, 6, 16, 7, 1, 3, 0, 2, 5, 3)
    f32("k3s", config_id("k3s"), 0, 16, 32, 3, 1, 1, 0, 3, 5, 7)
    f32("k3s", config_id("k3s"), 0, 16, 32, 3, 1, 1, 0, 3, 5, 7, head=3)

    def b16(family, tr, cin, cout, k, s, p, op, N, H, W, **kw):
        out.append(Case("bf16", family, tr, cin, cout, k, s, p, op, N, H, W, seed=3200 + len(out), **kw))
    b16("igemm", 0, 15, 40, 3, 1, 1, 0, 2, 5, 4, force=4)                # generic
    b16("igemm", 1, 6, 40, 3, 1, 0, 0, 3, 1, 1, force=4)                 # unit-input
    b16("igemm", 1, 15, 72, 3, 2, 1, 1, 2, 3, 2, force=3)                # four phases
    b16("stem", 0, 3, 16, 7, 1, 3, 0, 1024, 16, 16)                      # stem1
    b16("stem", 0, 80, 32, 3, 1, 1, 0, 2048, 16, 16)                     # stem2
    b16("stem", 0, 32, 32, 3, 1, 1, 0, 2048, 16, 16, res=1)              # stem3
    b16("box64", 0, 64, 64, 3, 1, 1, 0, 2048, 16, 16)
    b16("tp2b", 1, 32, 32, 3, 2, 1, 1, 1030, 5, 7)
    b16("k3s_head", 0, 16, 32, 3, 1, 1, 0, 3, 5, 7, head=3)
    return out


def update_operands(case):
    """(x, w0, w1, scale, shift, scale2, shift2, res): w0 and w1 from different seeds, a second scale / shift draw"""
    x, w0, scale, shift, res = int_operands(case)
    _x, w1, _s, _h, _r = int_operands(case.with_seed(case.seed + 7919))
    _x, _w, scale2, shift2, _r = int_operands(case.with_seed(case.seed + 104729))
    return x, w0, w1, scale, shift, scale2, shift2, res


def update_refs(case):
    """(ref(w0), ref(w1), ref(w1) under the second scale / shift) in float64, fused head applied"""
    x, w0, w1, scale, shift, scale2, shift2, res = update_operands(case)
    refs = [ref64(case, x, w, sc, sh, res) for w, sc, sh in ((w0, scale, shift), (w1, scale, shift), (w1, scale2, shift2))]
    if case.head:
        refs = [head_ref(r, *head_operands(case)) for r in refs]
    return refs


_CACHE = {}


def candidates(name):
    if name not in _CACHE:
        if name in ("f32 igemm", "f32 split", "bf16 igemm"):
            path, fam = name.split()
            _CACHE[name] = igemm_candidates(path, fam)
        elif name.startswith("wino id "):
            _CACHE[name] = wino_candidates(int(name.split()[-1]))
        elif name in ("tp2", "tp2s"):
            _CACHE[name] = tp2_candidates(name)
        elif name in ("bwd f32 igemm", "bwd f32 split", "bwd bf16 igemm"):
            _bwd, path, fam = name.split()
            _CACHE[name] = bwd_igemm_candidates(path, fam)
        elif name.startswith("bwd wino id "):
            _CACHE[name] = bwd_wino_candidates(int(name.split()[-1]))
        elif name in ("bwd tp2", "bwd tp2s"):
            _CACHE[name] = bwd_tp2_candidates(name.split()[1])
        elif name == "bwd bf16 special":
            _CACHE[name] = bwd_convb_special_candidates()
        elif name == "update":
            _CACHE[name] = update_candidates()
        else:
            _CACHE[name] = {"stem7s": stem7s_candidates, "k3s": k3s_candidates, "bf16 special": convb_special_candidates,
                            "thin": thin_candidates, "large": large_candidates, "heads": head_candidates}[name]()
    return _CACHE[name]


POOLS = ["f32 igemm", "f32 split"] + ["wino id %d" % i for i in (6, 7, 8, 9, 12, 11, 19)] + ["tp2", "tp2s", "stem7s", "k3s", "bf16 igemm",
                                                                                              "bf16 special", "thin", "heads"]
BWD_POOLS = ["bwd f32 igemm", "bwd f32 split", "bwd bf16 igemm"] + ["bwd wino id %d" % i for i in (6, 7, 8, 9, 12, 11, 19)] + [
    "bwd tp2", "bwd tp2s", "bwd bf16 special"]


def eligible(case):
    """does the kernel the case names run it, by the launcher's own rule?  fp32: w2l_tune_entry_applicable (plus the two buffer rules
    of io_fits that depend on the strides: conv_stem7s reads 8 channels per pixel); bf16: w2l_convb_resolve_geom names the family (a
    forced tile or split-K always means the implicit GEMM)"""
    if case.out_hw() is None or min(case.out_hw()) < 1:
        return False
    if case.path == "thin":
        return True
    if case.path == "f32":
        return case.applicable() and (case.family != "stem7s" or case.strides()[0] >= 8)
    if case.head:              # the bf16 head is the layer's only kernel: a 3x3 s1 p1 conv, cin % 16 == 0, 32 couts
        return (case.k, case.s, case.p) == ((3, 3), (1, 1), (1, 1)) and case.cin % 16 == 0 and case.cout == 32
    if case.force >= 0 or case.ks:
        return case.family == "igemm"
    return case.convb_resolve()[0].startswith(case.family)


def exact_cases(pool):
    """the eligible candidates of a pool, duplicates dropped"""
    seen, out = set(), []
    for c in candidates(pool):
        if c.key() not in seen and eligible(c):
            seen.add(c.key())
            out.append(c)
    return out


# ---------------------------------------------------------------- regimes
def _seg_blocks(c):
    """(first unit, last unit, tile rows per image) of every work item of conv_wino4's segment form"""
    pl = c.wino4_plan()
    th = (c.H + 3) // 4
    units = c.N * th
    return [(b * pl["r"], min((b + 1) * pl["r"], units) - 1, th) for b in range(pl["blocks"]) if b * pl["r"] < units]


def _ragged(c, m=True, n=True):
    bm, bn = c.tile()
    M = c.gemm_rows()
    return (not m or (M > bm and M % bm != 0)) and (not n or (c.cout > bn and c.cout % bn != 0))


REGIMES = []


def _regime(name, pool, pred):
    REGIMES.append((name, pool, pred))


for _p in ("f32 igemm", "f32 split", "bf16 igemm"):
    for _t in range(len(BF16_TILES if _p == "bf16 igemm" else F32_TILES)):
        def _tile_pred(c, t=_t, p=_p):
            base = config_id("split") if p == "f32 split" else 0
            return c.force == base + t and not c.ks and _ragged(c)
        _regime("%s tile %d: ragged M and ragged cout" % (_p, _t), _p, _tile_pred)

        def _ks_pred(c, t=_t, p=_p):
            base = config_id("split") if p == "f32 split" else 0
            n, per = c.splits()
            return c.force == base + t and c.ks >= 2 and n >= 2 and c.ksteps() % per != 0
        _regime("%s tile %d: split-K with a short last split" % (_p, _t), _p, _ks_pred)
    _regime("%s: more splits asked than K-steps" % _p, _p, lambda c: c.ks > c.ksteps() and c.splits()[0] == c.ksteps())
    _regime("%s: split-K 3" % _p, _p, lambda c: c.ks == 3 and c.splits()[0] == 3)
    _regime("%s: cin_p > cin" % _p, _p, lambda c: c.cin_p > c.cin and not c.ks)
    _regime("%s: transposed s1 p0" % _p, _p, lambda c: c.tr and c.s == (1, 1))
    _regime("%s: transposed s2 p1 output padding 1, split-K" % _p, _p, lambda c: c.tr and c.s == (2, 2) and c.op == (1, 1) and c.ks >= 2)
    _regime("%s: 7x7" % _p, _p, lambda c: c.k == (7, 7))
    _regime("%s: 5x5 s(1,2)" % _p, _p, lambda c: c.k == (5, 5) and c.s == (1, 2))
    _regime("%s: 3x3 s(3,2)" % _p, _p, lambda c: c.k == (3, 3) and c.s == (3, 2))
    _regime("%s: residual in its own buffer" % _p, _p, lambda c: c.res == 1 and not c.sliced)
    _regime("%s: residual aliases the input" % _p, _p, lambda c: c.res == 2 and not c.sliced)
    _regime("%s: channel slices of wider buffers" % _p, _p, lambda c: c.sliced)

for _cid in (6, 7, 8, 9, 12, 11, 19):
    _p = "wino id %d" % _cid
    _regime("%s: a single pixel" % _p, _p, lambda c: (c.H, c.W) == (1, 1) and not c.res)
    _regime("%s: odd extents, several tiles" % _p, _p, lambda c: c.H % 2 == 1 and c.W % 2 == 1 and c.H > 4 and not c.res)
    _regime("%s: residual in its own buffer" % _p, _p, lambda c: c.res == 1 and not c.sliced)
    _regime("%s: residual aliases the input" % _p, _p, lambda c: c.res == 2 and not c.sliced)
    _regime("%s: channel slices of wider buffers" % _p, _p, lambda c: c.sliced)
for _cid in (8, 9, 12, 19):
    _regime("wino id %d: several images per block, last group past the batch" % _cid, "wino id %d" % _cid,
            lambda c: c.group_past_batch() and not c.res)
    _regime("wino id %d: the same with several tiles per image" % _cid, "wino id %d" % _cid,
            lambda c: c.group_past_batch() and c.H > 2 and not c.res)
_regime("wino4: rectangles", "wino id 11", lambda c: c.wino4_plan()["form"] == 0 and not c.res)
_regime("wino4: rectangles, several images per block, last group past the batch", "wino id 11",
        lambda c: c.wino4_plan()["form"] == 0 and c.wino4_plan()["ni"] > 1 and c.N % c.wino4_plan()["ni"] != 0 and not c.res)
_regime("wino4: segments", "wino id 11", lambda c: c.wino4_plan()["form"] == 1 and not c.res)
_regime("wino4: segments, a block starts in the middle of an image", "wino id 11",
        lambda c: c.wino4_plan()["form"] == 1 and any(a % th for a, _b, th in _seg_blocks(c)))
_regime("wino4: segments, a block covers three images", "wino id 11",
        lambda c: c.wino4_plan()["form"] == 1 and any(b // th - a // th >= 2 for a, b, th in _seg_blocks(c)))
_regime("wino4: segments, the last block is short", "wino id 11",
        lambda c: c.wino4_plan()["form"] == 1 and (c.N * ((c.H + 3) // 4)) % c.wino4_plan()["r"] != 0)
for _p in ("tp2", "tp2s"):
    _regime("%s: a single input pixel" % _p, _p, lambda c: (c.H, c.W) == (1, 1) and not c.ks)
    _regime("%s: odd extents, odd batch" % _p, _p, lambda c: c.H % 2 == 1 and c.W % 2 == 1 and c.H > 1 and c.N == 7 and not c.ks and not c.sliced)
    _regime("%s: channel slices of wider buffers" % _p, _p, lambda c: c.sliced)
for _p in ("tp2", "tp2s", "k3s"):
    _regime("%s: several images per block, last group past the batch" % _p, _p, lambda c: c.group_past_batch() and not c.res and not c.ks)
    _regime("%s: the same with several pixels per image" % _p, _p, lambda c: c.group_past_batch() and c.H > 1 and not c.res and not c.ks)
_regime("tp2s: split-K 2", "tp2s", lambda c: c.ks == 2 and c.cin // 16 >= 2)
_regime("tp2s: split-K 3 with a short last split", "tp2s", lambda c: c.ks == 3 and (c.cin // 16) % (-(-(c.cin // 16) // 3)) != 0)
_regime("tp2s: more splits asked than K-steps", "tp2s", lambda c: c.ks > c.cin // 16)
_regime("stem7s: image smaller than a block", "stem7s", lambda c: c.H < 16 and c.W < 16)
_regime("stem7s: ragged blocks in both directions", "stem7s", lambda c: c.H > 16 and c.H % 16 and c.W > 16 and c.W % 16)
_regime("stem7s: 5 input channels (cin_p > cin)", "stem7s", lambda c: c.cin == 5)
_regime("stem7s: channel slices of wider buffers", "stem7s", lambda c: c.sliced)
_regime("k3s: a single pixel", "k3s", lambda c: (c.H, c.W) == (1, 1))
_regime("k3s: five K-steps", "k3s", lambda c: c.cin == 80)
_regime("k3s: residual in its own buffer", "k3s", lambda c: c.res == 1)
_regime("k3s: residual aliases the input", "k3s", lambda c: c.res == 2 and not c.sliced)
_regime("k3s: channel slices of wider buffers", "k3s", lambda c: c.sliced)
_regime("bf16 stem: 7x7, cin_p 8", "bf16 special", lambda c: c.family == "stem" and c.k == (7, 7) and c.cin_p == 8 and c.convb_resolve()[0] == "stem1")
_regime("bf16 stem: 7x7, cin_p 16", "bf16 special", lambda c: c.family == "stem" and c.k == (7, 7) and c.cin_p == 16 and c.convb_resolve()[0] == "stem1")
_regime("bf16 stem: 80 -> 32 output block", "bf16 special", lambda c: c.convb_resolve()[0] == "stem2")
_regime("bf16 stem: 32 -> 32 with a residual", "bf16 special", lambda c: c.convb_resolve()[0] == "stem3" and c.res)
_regime("bf16 stem: tiles not a multiple of the grid", "bf16 special", lambda c: c.family == "stem" and c.N % 256 != 0)
_regime("bf16 stem: channel slices of wider buffers", "bf16 special", lambda c: c.convb_resolve()[0] == "stem1" and c.sliced)
_regime("bf16 box64: no residual", "bf16 special", lambda c: c.convb_resolve()[0] == "box64" and not c.res)
_regime("bf16 box64: residual aliases the input", "bf16 special", lambda c: c.convb_resolve()[0] == "box64" and c.res == 2)
_regime("bf16 box64: ragged tiles, 60 couts, slices", "bf16 special", lambda c: c.convb_resolve()[0] == "box64" and c.sliced and c.H % 16)
_regime("bf16 tp2b: odd extents", "bf16 special", lambda c: c.convb_resolve()[0] == "tp2b" and c.H % 2 and c.H > 1 and not c.sliced)
_regime("bf16 tp2b: a single input pixel", "bf16 special", lambda c: c.convb_resolve()[0] == "tp2b" and (c.H, c.W) == (1, 1))
_regime("bf16 tp2b: channel slices of wider buffers", "bf16 special", lambda c: c.convb_resolve()[0] == "tp2b" and c.sliced)
for _f in ("igemm", "split", "k3s", "k3s_head"):
    _regime("head without activation: %s" % _f, "heads", lambda c, f=_f: c.family == f and c.head and not c.sliced)
for _cid in (9, 12):
    _regime("head without activation: wino2 id %d" % _cid, "heads", lambda c, i=_cid: c.force == i and c.head == 3 and not c.sliced)
_regime("head without activation: output slice of a wider pixel", "heads", lambda c: c.head and c.sliced and c.path == "f32")
_regime("thin: one pixel", "thin", lambda c: c.W == 1)
_regime("thin: several blocks, ragged tail", "thin", lambda c: c.W > 256 and c.W % 256 and not c.sliced)
_regime("thin: cin not a multiple of 8", "thin", lambda c: c.cin % 8 != 0)
_regime("thin: channel slices of wider buffers", "thin", lambda c: c.sliced)


# ---- the backward pass (tests/test_conv_backward_exact_gpu.py)
BWD_REGIMES = []


def _bwd_regime(name, pool, pred):
    BWD_REGIMES.append((name, pool, pred))


def _row(c):
    """the SIGS_GEOMS row (transposed, k, stride, pad, output padding) of the forward layer a dgrad_of() case belongs to"""
    (tr, _ci, _co, k, s, p, op), _H, _W = c.fwd
    return (bool(tr), k, _pair(s), p, op)


for _p in ("f32 igemm", "f32 split", "bf16 igemm"):
    for _g in SIGS_GEOMS:
        _bwd_regime("%s: data gradient of %s" % (_p, geom_label(*_g[:5])), "bwd " + _p,
                    lambda c, row=_g[:5]: _row(c) == row and not c.res and not c.ks)
    _bwd_regime("%s: output padding differs between the axes" % _p, "bwd " + _p, lambda c: c.op[0] != c.op[1] and not c.res)
    _bwd_regime("%s: output padding 2" % _p, "bwd " + _p, lambda c: 2 in c.op and not c.res)
    _bwd_regime("%s: the unit-input variant (gradient of 3x3 p0 over 3x3)" % _p, "bwd " + _p,
                lambda c: c.tr and c.s == (1, 1) and (c.H, c.W) == (1, 1) and c.k == (3, 3))
    _bwd_regime("%s: accumulate in place" % _p, "bwd " + _p,
                lambda c: c.res == 3 and not c.ks and not c.sliced and c.s == (2, 2) and c.tr and c.cout > 16)
    _bwd_regime("%s: accumulate in place, split-K 2" % _p, "bwd " + _p,
                lambda c: c.res == 3 and c.ks == 2 and c.splits()[0] == 2 and not c.sliced and c.cout > 16)
    _bwd_regime("%s: accumulate in place, split-K 3" % _p, "bwd " + _p,
                lambda c: c.res == 3 and c.ks == 3 and c.splits()[0] == 3 and not c.sliced)
    _bwd_regime("%s: accumulate in place into a channel slice of a wider buffer" % _p, "bwd " + _p,
                lambda c: c.res == 3 and c.sliced and not c.ks)
    _bwd_regime("%s: in place into a channel slice, split-K 2" % _p, "bwd " + _p, lambda c: c.res == 3 and c.sliced and c.ks == 2)
    _bwd_regime("%s: accumulate in place, 15 couts (fp32: scalar epilogue)" % _p, "bwd " + _p, lambda c: c.res == 3 and c.cout == 15 and not c.ks)
    _bwd_regime("%s: in place, 15 couts, split-K 2" % _p, "bwd " + _p, lambda c: c.res == 3 and c.cout == 15 and c.ks == 2)
    _bwd_regime("%s: gradient of a transposed layer with 16 input channels (fp32: x-paired variant)" % _p, "bwd " + _p,
                lambda c: not c.tr and c.cout == 16 and c.out_hw()[1] % 2 == 0 and not c.res)
    _bwd_regime("%s: accumulate in place, stride 1" % _p, "bwd " + _p, lambda c: c.res == 3 and c.tr and c.s == (1, 1))
    _bwd_regime("%s: accumulate in place, gradient of a transposed layer" % _p, "bwd " + _p, lambda c: c.res == 3 and not c.tr)
for _cid in (6, 7, 8, 9, 12, 11, 19):
    _p = "wino id %d" % _cid
    _bwd_regime("%s transposed: a single pixel" % _p, "bwd " + _p, lambda c: (c.H, c.W) == (1, 1) and not c.res)
    _bwd_regime("%s transposed: odd extents, several tiles" % _p, "bwd " + _p, lambda c: (c.H, c.W) == (13, 11) and not c.res)
    if _cid in (8, 9, 12, 19):      # conv_wino (ids 6, 7) holds one image per block
        _bwd_regime("%s transposed: several images per block, last group past the batch" % _p, "bwd " + _p,
                    lambda c: c.group_past_batch() and not c.res)
    _bwd_regime("%s transposed: accumulate in place" % _p, "bwd " + _p, lambda c: c.res == 3 and not c.sliced)
    _bwd_regime("%s transposed: accumulate in place, sliced" % _p, "bwd " + _p, lambda c: c.res == 3 and c.sliced)
for _f, _n in ((0, "rectangles"), (1, "segments")):
    _bwd_regime("wino4 transposed: %s" % _n, "bwd wino id 11", lambda c, f=_f: c.wino4_plan()["form"] == f and not c.res)
    _bwd_regime("wino4 transposed: %s, accumulate in place" % _n, "bwd wino id 11",
                lambda c, f=_f: c.wino4_plan()["form"] == f and c.res == 3 and not c.sliced)
_bwd_regime("wino4 transposed: rectangles, several images per block, last group past the batch", "bwd wino id 11",
            lambda c: c.wino4_plan()["form"] == 0 and c.wino4_plan()["ni"] > 1 and c.N % c.wino4_plan()["ni"] != 0 and not c.res)
for _p in ("tp2", "tp2s"):
    _bwd_regime("%s: data gradient of conv 3x3 s2 p1 at even extents" % _p, "bwd " + _p,
                lambda c, f=_p: c.family == f and not c.ks and c.H * c.W > 1)
    _bwd_regime("%s: the same over a single pixel of dz" % _p, "bwd " + _p, lambda c, f=_p: c.family == f and not c.ks and c.H * c.W == 1)
_bwd_regime("tp2s: data gradient with split-K 2", "bwd tp2s", lambda c: c.ks == 2 and c.cin // 16 >= 2)
# FINDING: neither kernel has a residual operand (config_fits: "plain"), so an accumulating data gradient never runs on them
_bwd_regime("tp2 / tp2s DECLINE accumulate in place (no residual operand): the implicit GEMM runs it", "bwd tp2",
            lambda c: bool(c.declines) and c.res == 3 and c.op == (1, 1))
_bwd_regime("tp2 / tp2s DECLINE an odd extent (output padding 0 on both axes): the implicit GEMM runs it", "bwd tp2",
            lambda c: bool(c.declines) and c.op == (0, 0))
_bwd_regime("tp2 / tp2s DECLINE output padding (0, 1): the implicit GEMM runs it", "bwd tp2", lambda c: bool(c.declines) and c.op == (0, 1))
_bwd_regime("tp2 / tp2s DECLINE output padding (1, 0): the implicit GEMM runs it", "bwd tp2", lambda c: bool(c.declines) and c.op == (1, 0))
_bwd_regime("bf16 box64 transposed", "bwd bf16 special", lambda c: c.family == "box64" and c.tr and not c.res)
_bwd_regime("bf16 box64 transposed: accumulate in place", "bwd bf16 special", lambda c: c.family == "box64" and c.tr and c.res == 3)
_bwd_regime("bf16 box64 transposed: batch not a multiple of the 7-image period", "bwd bf16 special",
            lambda c: c.family == "box64" and c.N % 7 != 0 and c.N > 16)
_bwd_regime("bf16 tp2b: data gradient of conv 3x3 s2 p1", "bwd bf16 special", lambda c: c.family == "tp2b" and not c.res and c.H > 1)
_bwd_regime("bf16 tp2b: the same over a single pixel of dz", "bwd bf16 special", lambda c: c.family == "tp2b" and not c.res and c.H == 1)
_bwd_regime("bf16 tp2b: accumulate in place", "bwd bf16 special", lambda c: c.family == "tp2b" and c.res == 3 and not c.sliced)
_bwd_regime("bf16 tp2b: accumulate in place, sliced", "bwd bf16 special", lambda c: c.family == "tp2b" and c.res == 3 and c.sliced)


def select(regimes=None):
    """[(regime name, pool, case or None)]: the cheapest eligible candidate of the pool that satisfies the predicate"""
    out = []
    for name, pool, pred in (REGIMES if regimes is None else regimes):
        fits = [c for c in exact_cases(pool) if pred(c)]
        fits.sort(key=lambda c: (c.macs(), sum(c.nbytes())))
        out.append((name, pool, fits[0] if fits else None))
    return out


def regime_pred(name, regimes=None):
    return [p for n, _pool, p in (REGIMES if regimes is None else regimes) if n == name][0]


def table(ran=None, regimes=None):
    """the selection table; ran: {regime name: text of the kernel that ran} from a GPU run"""
    lines = []
    for name, _pool, c in select(regimes):
        lines.append("  %-72s %s%s" % (name, c.describe() if c else "EMPTY", " | " + ran[name] if ran and name in ran else ""))
    return "\n".join(lines)
