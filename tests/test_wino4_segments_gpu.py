"""conv_wino4.hip's segment form (configuration id 11 on shapes whose tile rows pack better as runs across image boundaries than
as rectangles) against the oracle's block() in float64, through the same plan entry and at the same tolerance as
tests/test_conv_gpu.py's F(4x4) cases (1e-4 abs + rel).

Which form runs is the host's cost rule, items x (1 + 0.05 halo), and not the test's choice: 12x12 at N = 7 or 1 and 10x10 at
N = 2 need as many items either way and stay rectangular (they are kept as cases of the entry), so the runs that cross image
boundaries, the ragged last block and the ragged last tile row / column inside a segment are exercised at N = 10 and 13, the
smallest batches at which ten rows per block save an item."""
import ctypes

import pytest
import torch

from oracle import models_ref
from test_conv_gpu import _geom_string, _make

pytestmark = pytest.mark.gpu

# (kind, N, H, W, cin, cout, residual, items of the segment form per 64 couts or None where the rectangles are kept)
CASES = [
    ("c", 7, 12, 12, 8, 64, 0, None),       # 21 units: three blocks either way
    ("c", 1, 12, 12, 16, 64, 0, None),      # one image, one item
    ("c", 3, 24, 24, 8, 128, 0, 4),         # 18 units in runs of 5: 5 | 1+4 | 2+3 | 3, two cout tiles
    ("c", 2, 10, 10, 8, 64, 0, None),
    ("c", 2, 22, 22, 8, 64, 0, 3),          # ragged last tile row and column, 12 units: 5 | 1+4 | 2
    ("c", 10, 12, 12, 8, 64, 0, 3),         # 30 units in runs of 10: 3+3+3+1 | 2+3+3+2 | 1+3+3+3 (rectangles: 4 items)
    ("c", 13, 12, 12, 8, 64, 0, 4),         # ragged last block of 9 units (rectangles: 5 items)
    ("c", 10, 10, 10, 8, 64, 0, 3),         # ragged last tile row and column inside every segment
    ("c", 13, 12, 12, 64, 64, 1, 4),        # the residual input
    ("t", 10, 12, 12, 64, 128, 0, 3),       # transposed weights: flipped kernel, swapped channel roles
]


def _reference(m, kind, x, residual):
    sd = {"b." + key: v.double() for key, v in m.state_dict().items()}
    with torch.no_grad():
        return models_ref.block(x.double(), sd, "b", _geom_string(kind, 3, 1, 1, residual, 0), norm=(kind != "n"))


def _query(N, H, W):
    from wav2lip_amd import _lib
    out = (ctypes.c_int * 8)()
    assert _lib.load().w2l_wino4_block_plan(N, H, W, out) == 0
    return tuple(out)


def _run(kind, N, H, W, cin, cout, residual, cuda, seed):
    """-> (output NCHW on the host, float64 reference, work items from the dry-run FLOP query)"""
    from wav2lip_amd import engine
    m = _make(kind, 3, 1, 1, cin, cout, residual, 0, seed)
    x = torch.randn(N, cin, H, W)
    ref = _reference(m, kind, x, residual)
    layer = m.to(cuda).fused()
    assert layer.cin_p == cin
    xin = x.permute(0, 2, 3, 1).contiguous().to(cuda)
    y = torch.full((N, H, W, cout), 3.0, device=cuda)
    plan = engine.Plan()
    a_in = engine.Act(xin, 0, cin)
    plan.add("l", layer, a_in, engine.Act(y, 0, cout), a_in if residual else None)
    plan.tuned = True
    plan.set_config(0, 11, 1)
    name, flops, family, cfg = plan.resolved()[0]
    assert family == "wino4", plan.resolved()
    plan.run()
    items, rem = divmod(flops, 2 * 36 * 32 * 64 * cin)
    assert rem == 0
    return y.permute(0, 3, 1, 2).cpu(), ref, items


def _close(got, ref):
    err = (got.double() - ref).abs()
    print("max err %.3e at |ref| up to %.3e" % (err.max().item(), ref.abs().max().item()))
    assert bool((err <= 1e-4 + 1e-4 * ref.abs()).all()), "max err %.3e" % err.max().item()


@pytest.mark.parametrize("idx", range(len(CASES)))
def test_segment_blocks_match_float64(idx, cuda):
    kind, N, H, W, cin, cout, residual, seg_items = CASES[idx]
    got, ref, items = _run(kind, N, H, W, cin, cout, residual, cuda, 900 + idx)
    q = _query(N, H, W)
    assert q[0] == (seg_items is not None) and items == q[1] * (cout // 64), (q, items)
    if seg_items is not None:
        assert items == seg_items * (cout // 64)
    _close(got, ref)


def test_dispatcher_takes_the_segment_form(cuda):
    """by the item count of the dry-run FLOP query: 13 images of 3 x 3 tiles are 39 tile rows = 4 runs of ten (the 3x3x3
    rectangles need 5 items), 128 frames 39 (43), and 128 frames of 24x24 154 runs of five per cout tile (172)"""
    from wav2lip_amd import engine
    for N, H, cin, cout, want in ((13, 12, 8, 64, 4), (128, 12, 8, 384, 39 * 6), (128, 24, 8, 256, 154 * 4)):
        layer = _make("c", 3, 1, 1, cin, cout, 0, 0, 5).to(cuda).fused()
        xin = torch.zeros(N, H, H, cin, device=cuda)
        y = torch.zeros(N, H, H, cout, device=cuda)
        plan = engine.Plan()
        plan.add("l", layer, engine.Act(xin, 0, cin), engine.Act(y, 0, cout), None)
        plan.tuned = True
        plan.set_config(0, 11, 1)
        name, flops, family, cfg = plan.resolved()[0]
        assert family == "wino4" and flops == 2 * 36 * want * 32 * 64 * cin, (N, H, flops)


def test_channel_sliced_input_and_output(cuda):
    """the concat layout: input and aliasing residual read from a channel slice of a wider buffer, output written into one"""
    from wav2lip_amd import engine
    m = _make("c", 3, 1, 1, 64, 64, 1, 0, 77)
    N, H, W = 10, 12, 12
    assert _query(N, H, W)[0] == 1
    src = torch.randn(N, H, W, 96)
    x = src[..., 32:96].permute(0, 3, 1, 2).contiguous()
    ref = _reference(m, "c", x, 1)
    layer = m.to(cuda).fused()
    layer.set_tile(11)
    src = src.to(cuda)
    dst = torch.full((N, H, W, 80), 7.0, device=cuda)
    a_in, a_out = engine.Act(src, 32, 64), engine.Act(dst, 8, 64)
    layer.forward_raw(N, H, W, a_in.ptr, a_in.cs, a_out.ptr, a_out.cs, a_in.ptr, a_in.cs)
    _close(dst[..., 8:72].permute(0, 3, 1, 2).cpu(), ref)
    assert bool((dst[..., :8] == 7.0).all()) and bool((dst[..., 72:] == 7.0).all()), "wrote outside its slice"


@pytest.mark.parametrize("N,H,cin,cout,items", [(1, 96, 8, 64, 18), (2, 48, 8, 128, 9 * 2)])
def test_full_rectangles_are_kept_and_packing_does_not_change_a_bit(N, H, cin, cout, items, cuda):
    """96x96 and 48x48 fill their 4x8x1 / 4x4x2 rectangles and keep them (item count).  A tile's arithmetic does not depend on
    how tiles are packed into items, so the whole batch equals, bit for bit, the same layer run on one image or one crop-free
    sub-batch at a time; the same holds between the two forms: 24x24 at N = 3 runs as segments, each of its images alone
    as rectangles."""
    from wav2lip_amd import engine

    def run(layer, xin):
        n = xin.shape[0]
        y = torch.full((n, xin.shape[1], xin.shape[2], cout), 3.0, device=cuda)
        plan = engine.Plan()
        plan.add("l", layer, engine.Act(xin, 0, cin), engine.Act(y, 0, cout), None)
        plan.tuned = True
        plan.set_config(0, 11, 1)
        fl = plan.resolved()[0][1]
        plan.run()
        torch.cuda.synchronize()
        return y, fl // (2 * 36 * 32 * 64 * cin)

    m = _make("c", 3, 1, 1, cin, cout, 0, 0, 31)
    x = torch.randn(N, cin, H, H)
    ref = _reference(m, "c", x, 0)
    layer = m.to(cuda).fused()
    xin = x.permute(0, 2, 3, 1).contiguous().to(cuda)
    assert _query(N, H, H)[0] == 0
    y, got_items = run(layer, xin)
    assert got_items == items
    _close(y.permute(0, 3, 1, 2).cpu(), ref)
    if N > 1:
        for n in range(N):
            y1, _ = run(layer, xin[n:n + 1].contiguous())
            assert torch.equal(y1[0], y[n])
    # segments against rectangles on the same inputs
    xs = torch.randn(3, 24, 24, cin, device=cuda)
    assert _query(3, 24, 24)[0] == 1 and _query(1, 24, 24)[0] == 0
    ys, _ = run(layer, xs)
    for n in range(3):
        y1, _ = run(layer, xs[n:n + 1].contiguous())
        assert torch.equal(y1[0], ys[n])
