"""The detector glue of csrc/detect.hip (w2l_s3fd_decode and, on the fp32 and the bf16 instantiation of their one body each,
w2l_maxpool2x2, w2l_l2norm_scale, w2l_s3fd_pack) and the input packing of csrc/api.hip (w2l_datagen_pack,
w2l_datagen_pack_bf16, w2l_frames_to_u8, w2l_nchw_to_nhwc, w2l_nhwc_to_nchw) at their edges, through the C ABI.
Cases, float64 references and derived bounds: tests/_glue_cases.py (tests/test_glue_cases_cpu.py holds numpy restatements to the same bounds and shows that the inputs tell the named wrong variants apart).  Every destination
starts as a sentinel with a sentinel tail behind it, and every input channel that a stride leaves free is NaN: a read or a write
outside the stated channels shows.  Each kernel also runs once at a size where its grid-stride loop takes a second trip, with
inputs generated and compared on the device.

Largest observed error as a fraction of its bound (MI355X; the numpy fp32 restatements reach 0.30, 0.19 and 0.16):
    w2l_l2norm_scale                 0.30
    w2l_l2norm_scale_bf16            0.99  (the bound is all but the half ulp of the one bf16 rounding, which a store can reach)
    w2l_s3fd_decode, coordinates     0.17
    w2l_s3fd_decode, score           0.16
    w2l_s3fd_decode, two-trip case   0.31
    every other comparison (maxpool, pack, datagen fp32 / bf16, frames_to_u8, the layout transposes) is bit-exact: 0 differences"""
import ctypes as C

import numpy as np
import pytest
import torch

import _glue_cases as G
from oracle import datagen_ref, s3fd_ref

pytestmark = pytest.mark.gpu
TAIL = 64                     # sentinel elements behind every destination
HEAD = 8                      # and before the destinations whose base pointer moves
NAN = float("nan")
U8_SENT = 0xA5


def _lib3():
    from wav2lip_amd import _lib
    return _lib.load(), _lib.current_stream(), _lib.ptr


def _up(a, cuda):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    assert t.data_ptr() % 16 == 0
    return t


def _dest(n, cuda, dtype=torch.float32, head=0):
    """a SENT-filled buffer: a destination of n elements with `head` elements before and TAIL after it"""
    buf = torch.full((head + n + TAIL,), U8_SENT if dtype == torch.uint8 else G.SENT, dtype=dtype, device=cuda)
    assert buf.data_ptr() % 16 == 0
    return buf


def _at(t, elems):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def _read(buf, n, what, head=0):
    """the n destination elements as numpy, after checking the sentinels either side"""
    torch.cuda.synchronize()
    sent = U8_SENT if buf.dtype == torch.uint8 else G.SENT
    h = buf.float().cpu().numpy() if buf.dtype == torch.bfloat16 else buf.cpu().numpy()
    assert (h[:head] == sent).all(), "%s: written before the destination" % what
    assert (h[head + n:] == sent).all(), "%s: written past the destination" % what
    return h[head:head + n]


# the two storages of the detector glue: kind -> (dtype, suffix of the entry point)
GLUE = {"fp32": (torch.float32, ""), "bf16": (torch.bfloat16, "_bf16")}


def _kind_cases(fp32, bf16):
    """[(kind, case)] with their ids: the fp32 cases keep the ids they had before the bf16 ones joined them"""
    return dict(argvalues=[("fp32", c) for c in fp32] + [("bf16", c) for c in bf16],
                ids=[str(c) for c in fp32] + ["bf16-%s" % (c,) for c in bf16])


def _up_as(a, cuda, kind):
    """fp32 values (already rounded to bf16 where kind is bf16: the conversion is exact) as a device tensor of the kind's dtype"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda).to(GLUE[kind][0])
    assert t.data_ptr() % 16 == 0
    return t


def _frac(err, bound):
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def _bits_equal(what, got, want):
    got, want = G.bits(got), G.bits(want)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d of %d values differ in their bits, first at %s" % (what, len(bad), want.size, tuple(bad[0]))


# ---------------------------------------------------------------- w2l_s3fd_decode
@pytest.mark.parametrize("case", G.DECODE_CASES, ids=str)
def test_s3fd_decode_stays_inside_the_float64_bounds(cuda, case):
    """against dense_boxes in float64 (the max-out, the softmax, the priors, the variances), every position and coordinate:
    coordinates within R (M + A), the score within R, saturated rows exactly 0.0 or 1.0 and never NaN; channels >= ncls of conf
    and >= 4 of loc are NaN; nothing past out[B FH FW 5] is written"""
    lib, s, ptr = _lib3()
    B, FH, FW, ncls, stride, cls_cs, reg_cs = case
    conf, loc = G.decode_inputs(case, seed=sum(case))
    ref, bound = G.decode_case_ref(case, conf, loc)
    P = B * FH * FW
    cd, ld, out = _up(conf, cuda), _up(loc, cuda), _dest(P * 5, cuda)
    assert lib.w2l_s3fd_decode(s, B, FH, FW, stride, ptr(cd), cls_cs, ncls, ptr(ld), reg_cs, ptr(out)) == 0, lib.w2l_last_error()
    got = _read(out, P * 5, "decode %s" % (case,)).reshape(P, 5).astype(np.float64)
    assert not np.isnan(got).any(), "decode %s: NaN at %s" % (case, np.argwhere(np.isnan(got))[:4].tolist())
    err = np.abs(got - ref)
    fc, fs = _frac(err[:, :4], bound[:, :4]), _frac(err[:, 4:], bound[:, 4:])
    print("GLUE_FRACTION decode_coord %.4f\nGLUE_FRACTION decode_score %.4f" % (fc, fs))
    bad = G.leaves(got, ref, bound)
    assert not bad.any(), "decode %s: %d values outside their bound, first (position, column) %s; worst %.2f of the bound " \
        "(coordinates), %.2f (score)" % (case, int(bad.sum()), np.argwhere(bad)[0].tolist(), fc, fs)
    bg, fg = G.decode_bg_fg(conf, ncls)
    sat = np.abs(bg - fg) >= G.SAT_GAP
    assert sat.any() and np.array_equal(got[sat, 4], (fg[sat] > bg[sat]).astype(np.float64)), \
        "decode %s: saturated scores %s" % (case, got[sat, 4].tolist())


def test_s3fd_decode_second_grid_stride_trip(cuda):
    """2049 x 2048 positions, 2048 more than 16384 workgroups of 256 hold: inputs, the float64 reference and the comparison on
    the device.  Saturated rows lie on both sides of the trip boundary"""
    lib, s, ptr = _lib3()
    B, FH, FW, ncls, stride, cls_cs, reg_cs = G.DECODE_BIG
    P = B * FH * FW
    gen = torch.Generator(device=cuda).manual_seed(5)
    conf = torch.full((P, cls_cs), NAN, device=cuda)
    loc = torch.full((P, reg_cs), NAN, device=cuda)
    conf[:, :ncls] = torch.randn((P, ncls), generator=gen, device=cuda) * 3
    loc[:, :4] = torch.randn((P, 4), generator=gen, device=cuda) * 2
    sat_rows = torch.tensor(G.SAT_ROWS, device=cuda)
    edge = 16384 * 256
    for r0 in (edge - 4, P - len(G.SAT_ROWS)):
        conf[r0:r0 + len(G.SAT_ROWS), :2] = sat_rows
    out = _dest(P * 5, cuda)
    assert lib.w2l_s3fd_decode(s, B, FH, FW, stride, ptr(conf), cls_cs, ncls, ptr(loc), reg_cs, ptr(out)) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    i = torch.arange(P, device=cuda)
    ref, bound = G.decode_ref(conf[:, :ncls].double(), loc[:, :4].double(), (i % FW).double(), ((i // FW) % FH).double(), ncls,
                              stride, xp=torch)
    got = out[:P * 5].view(P, 5).double()
    assert bool((out[P * 5:] == G.SENT).all()), "written past the table"
    assert not bool(torch.isnan(got).any())
    err = (got - ref).abs()
    bad = ~(err <= bound)
    frac = float((err / bound).max())
    print("GLUE_FRACTION decode_big %.4f" % frac)
    assert not bool(bad.any()), "%d values outside their bound, first %s (second trip from position %d), worst %.2f of the bound" % (
        int(bad.sum()), torch.nonzero(bad)[0].tolist(), edge, frac)
    d = conf[:, 1].double() - conf[:, 0].double()
    sat = d.abs() >= G.SAT_GAP
    assert int(sat.sum()) == 2 * len(G.SAT_ROWS) and torch.equal(got[sat, 4], (d[sat] > 0).double())
    del conf, loc, out, ref, bound, got, err
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- w2l_maxpool2x2
@pytest.mark.parametrize("kind,case", **_kind_cases(G.POOL_CASES, G.POOL_CASES_BF16))
def test_maxpool2x2_equals_the_four_strided_slices(cuda, kind, case):
    """equal in value to the maximum of the four strided slices: odd H and W drop the last row and column (which hold +inf here),
    +-inf and negative-only windows, channels >= C of x NaN and of y untouched.  NaN and windows that mix +0 and -0 are left
    out: fmaxf and torch differ there by definition, and post-ReLU activations hold neither.  bf16: a maximum of bf16 values is
    exact, so the comparison is the same equality"""
    lib, s, ptr = _lib3()
    dtype, sfx = GLUE[kind]
    N, H, W, C_, x_cs, y_cs = case
    x = G.pool_inputs(case, seed=sum(case), kind=kind)
    ref = G.pool_ref(x, C_)
    n = N * (H // 2) * (W // 2) * y_cs
    xd, y = _up_as(x, cuda, kind), _dest(n, cuda, dtype=dtype)
    assert getattr(lib, "w2l_maxpool2x2" + sfx)(s, N, H, W, C_, ptr(xd), x_cs, ptr(y), y_cs) == 0, lib.w2l_last_error()
    got = _read(y, n, "maxpool %s %s" % (kind, case)).reshape(N, H // 2, W // 2, y_cs)
    bad = np.argwhere(got[..., :C_] != ref)
    assert len(bad) == 0, "maxpool %s: %d of %d values differ, first at %s" % (case, len(bad), ref.size, bad[0].tolist())
    assert (got[..., C_:] == G.SENT).all(), "maxpool %s: channels >= C of y were written" % (case,)


@pytest.mark.parametrize("kind", list(GLUE))
def test_maxpool2x2_second_grid_stride_trip(cuda, kind):
    """1025 x 1024 x 16 items of 16 bytes (float4, or 8 bf16), 16384 more than 65536 workgroups of 256 hold; generated and compared
    on the device"""
    lib, s, ptr = _lib3()
    dtype, sfx = GLUE[kind]
    N, H, W, C_, x_cs, y_cs = G.POOL_BIG_BF16 if kind == "bf16" else G.POOL_BIG
    assert G.pool_trips(N, H, W, C_, kind) == 2 and G.pool_items(N, H, W, C_, kind) - G.POOL_GRID_CAP * G.BLOCK == 16384
    gen = torch.Generator(device=cuda).manual_seed(6)
    x = torch.empty((N, H, W, x_cs), device=cuda, dtype=dtype).normal_(generator=gen)
    Ho, Wo = H // 2, W // 2
    n = N * Ho * Wo * y_cs
    y = _dest(n, cuda, dtype=dtype)
    assert getattr(lib, "w2l_maxpool2x2" + sfx)(s, N, H, W, C_, ptr(x), x_cs, ptr(y), y_cs) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    ref = torch.maximum(torch.maximum(x[:, 0:2 * Ho:2, 0:2 * Wo:2], x[:, 0:2 * Ho:2, 1:2 * Wo:2]),
                        torch.maximum(x[:, 1:2 * Ho:2, 0:2 * Wo:2], x[:, 1:2 * Ho:2, 1:2 * Wo:2]))
    got = y[:n].view(N, Ho, Wo, y_cs)
    nbad = int((got != ref).sum())
    assert nbad == 0, "%d of %d values differ, first at %s" % (nbad, ref.numel(), torch.nonzero(got != ref)[0].tolist())
    assert bool((y[n:] == G.SENT).all())
    del x, y, ref, got
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- w2l_l2norm_scale
@pytest.mark.parametrize("kind,shape", **_kind_cases(G.L2_SHAPES, G.L2_SHAPES_BF16))
def test_l2norm_scale_stays_inside_the_float64_bound(cuda, kind, shape):
    """x / (sqrt(sum x^2) + 1e-10) w[c] within (K2(C) / 2 + 4) U |ref| for 1, 5 and 70 rows: one and several 256-channel trips,
    the last trip taken by lane 0 alone (C = 260), an all-zero row (exactly 0), a row at 1e-10 where the eps counts, a row whose
    only value is its last channel; channels >= C of x are NaN, of y untouched.  bf16 (1 and 5 rows, 512-channel trips: lane 0
    alone at C = 8, one full trip at 512, lane 0 alone in the second at 520): x holds bf16 values, and the bound grows by the one
    rounding of the stored result (G.l2norm_bound)"""
    lib, s, ptr = _lib3()
    dtype, sfx = GLUE[kind]
    C_, x_cs, y_cs = shape
    worst = 0.0
    for _, _, _, rows, rot in [c for c in G.l2norm_cases(kind) if c[0] == C_]:
        what = "l2norm %s C=%d x_cs=%d y_cs=%d rows=%d kinds %s" % (kind, C_, x_cs, y_cs, rows, G.l2norm_kinds(rows, rot)[:4])
        x, w = G.l2norm_inputs(C_, rows, rot, seed=C_ + rows + rot, kind=kind)
        ref = G.l2norm_ref(x, w)
        bound = G.l2norm_bound(ref, C_, kind)
        xb = np.full((rows, x_cs), np.nan, np.float32)
        xb[:, :C_] = x
        wb = np.full(C_ + 4, np.nan, np.float32)
        wb[:C_] = w
        xd, wd, y = _up_as(xb, cuda, kind), _up(wb, cuda), _dest(rows * y_cs, cuda, dtype=dtype)
        assert getattr(lib, "w2l_l2norm_scale" + sfx)(s, rows, C_, ptr(xd), x_cs, ptr(wd), ptr(y), y_cs) == 0, lib.w2l_last_error()
        got = _read(y, rows * y_cs, what).reshape(rows, y_cs)
        assert (got[:, C_:] == G.SENT).all(), "%s: channels >= C of y were written" % what
        got = got[:, :C_].astype(np.float64)
        bad = G.leaves(got, ref, bound)
        f = _frac(np.abs(got - ref), bound)
        assert not bad.any(), "%s: %d values outside the bound, first (row, channel) %s, worst %.2f of the bound" % (
            what, int(bad.sum()), np.argwhere(bad)[0].tolist(), f)
        assert (got[ref == 0] == 0).all(), "%s: a zero of the reference is not exactly 0" % what
        worst = max(worst, f)
    print("GLUE_FRACTION l2norm%s %.4f" % (sfx, worst))


# ---------------------------------------------------------------- w2l_s3fd_pack
@pytest.mark.parametrize("kind,y_cs", **_kind_cases(G.PACK_YCS, G.PACK_YCS_BF16))
def test_s3fd_pack_equals_the_oracle_bit_for_bit(cuda, kind, y_cs):
    """against s3fd_ref.preprocess on every byte value in every channel: channel 3 is 0 exactly when the 16-byte store is taken
    (y_cs % 4 == 0), channels >= 4 are untouched; an odd stride needs no aligned base.  bf16: the fp32 pack's values (integers
    with |v| <= 152: exact) and zeros in every other channel of every 8-channel group, the second group of y_cs = 16 included"""
    lib, s, ptr = _lib3()
    dtype, sfx = GLUE[kind]
    for npix in G.PACK_NPIX:
        for off in ((0,) if kind == "bf16" or G.pack_vector_path(y_cs) else (0, 1)):
            what = "pack %s npix=%d y_cs=%d base + %d" % (kind, npix, y_cs, off)
            bgr = G.pack_inputs(npix)
            rgb = s3fd_ref.preprocess(bgr.reshape(1, 1, npix, 3)).permute(0, 2, 3, 1).reshape(npix, 3).numpy()
            y = _dest(npix * y_cs, cuda, dtype=dtype, head=HEAD + off)
            assert getattr(lib, "w2l_s3fd_pack" + sfx)(s, npix, ptr(_up(bgr, cuda)), _at(y, HEAD + off), y_cs) == 0, lib.w2l_last_error()
            got = _read(y, npix * y_cs, what, head=HEAD + off).reshape(npix, y_cs)
            _bits_equal(what, got, G.pack_expected(rgb, y_cs, kind))


@pytest.mark.parametrize("kind,y_cs", **_kind_cases([4, 3], [8]))
def test_s3fd_pack_second_grid_stride_trip(cuda, kind, y_cs):
    """three pixels (bf16: one) more than the launch's cap of workgroups of 256 hold: 16384 for fp32, 65536 for bf16"""
    lib, s, ptr = _lib3()
    dtype, sfx = GLUE[kind]
    npix = G.PACK_BIG_BF16 if kind == "bf16" else G.PACK_BIG
    assert G.pack_trips(npix, kind) == 2
    gen = torch.Generator(device=cuda).manual_seed(7)
    x = torch.randint(0, 256, (npix, 3), dtype=torch.uint8, device=cuda, generator=gen)
    y = _dest(npix * y_cs, cuda, dtype=dtype)
    assert getattr(lib, "w2l_s3fd_pack" + sfx)(s, npix, ptr(x), ptr(y), y_cs) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    want = torch.full((npix, y_cs), 0.0 if kind == "bf16" else G.SENT, device=cuda)
    want[:, :3] = x[:, [2, 1, 0]].float() - torch.tensor([104.0, 117.0, 123.0], device=cuda)
    if kind == "fp32" and G.pack_vector_path(y_cs):
        want[:, 3] = 0
    diff = _as_bits(y[:npix * y_cs].view(npix, y_cs)) != _as_bits(want.to(dtype))
    nbad = int(diff.sum())
    assert nbad == 0, "%d values differ, first at %s" % (nbad, torch.nonzero(diff)[0].tolist())
    assert bool((y[npix * y_cs:].float() == G.SENT).all())
    del x, y, want, diff
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- w2l_datagen_pack / w2l_datagen_pack_bf16
DTYPES = {"fp32": (torch.float32, "w2l_datagen_pack"), "bf16": (torch.bfloat16, "w2l_datagen_pack_bf16")}


def _as_bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("S", G.DATAGEN_S)
@pytest.mark.parametrize("kind", list(DTYPES))
def test_datagen_pack_equals_the_oracle_bit_for_bit(cuda, kind, S):
    """against datagen_ref.datagen_batch (bf16: rounded by torch's .to(bfloat16)) at even and odd S - the mask rule is
    row >= S // 2 - through the vector store, the scalar stores forced by the stride, by c_zero_to and by a base pointer one
    element off a 16-byte boundary; zeros in [6, c_zero_to), channels from there on untouched"""
    lib, s, ptr = _lib3()
    dtype, fn = DTYPES[kind]
    N = G.DATAGEN_N
    faces = G.datagen_inputs(N, S, seed=S)
    six = datagen_ref.datagen_batch(faces, np.zeros((N, 80, 16), np.float32), img_size=S)[0].astype(np.float32)
    fd = _up(faces, cuda)
    for y_cs, czt, off in G.DATAGEN_LAYOUTS:
        path = G.datagen_store_path(torch.empty(0, dtype=dtype).element_size(), y_cs, czt, off)
        what = "%s S=%d y_cs=%d c_zero_to=%d base + %d (%s)" % (fn, S, y_cs, czt, off, path)
        n = N * S * S * y_cs
        y = _dest(n, cuda, dtype=dtype, head=HEAD + off)
        assert (y.data_ptr() + (HEAD + off) * y.element_size()) % 16 == (off * y.element_size()) % 16
        assert getattr(lib, fn)(s, N, S, ptr(fd), _at(y, HEAD + off), y_cs, czt) == 0, lib.w2l_last_error()
        torch.cuda.synchronize()
        want = torch.full((HEAD + off + n + TAIL,), G.SENT)
        want[HEAD + off:HEAD + off + n] = torch.from_numpy(G.datagen_expected(six, y_cs, czt)).view(-1)
        want = want.to(dtype)
        bad = torch.nonzero(_as_bits(y.cpu()) != _as_bits(want))
        assert len(bad) == 0, "%s: %d elements differ (sentinels before and after included), first at element %d of the pixel table" % (
            what, len(bad), int(bad[0]) - HEAD - off)


@pytest.mark.parametrize("kind", list(DTYPES))
def test_datagen_pack_second_grid_stride_trip(cuda, kind):
    """N = 228 at S = 96: above the 227 faces that 8192 workgroups of 256 hold; the vector store and a scalar one"""
    lib, s, ptr = _lib3()
    dtype, fn = DTYPES[kind]
    N, S = G.DATAGEN_BIG
    gen = torch.Generator(device=cuda).manual_seed(8)
    faces = torch.randint(0, 256, (N, S, S, 3), dtype=torch.uint8, device=cuda, generator=gen)
    v = (faces.double() / 255.0).float()
    m = v.clone()
    m[:, S // 2:] = 0
    six = torch.cat([m, v], 3).view(-1, 6)
    for y_cs, czt in ((8, 8), (6, 6)):
        n = N * S * S * y_cs
        y = _dest(n, cuda, dtype=dtype)
        assert getattr(lib, fn)(s, N, S, ptr(faces), ptr(y), y_cs, czt) == 0, lib.w2l_last_error()
        torch.cuda.synchronize()
        want = torch.full((N * S * S, y_cs), G.SENT, device=cuda)
        want[:, :6] = six
        want[:, 6:czt] = 0
        want = want.to(dtype)
        diff = _as_bits(y[:n].view(-1, y_cs)) != _as_bits(want)
        assert not bool(diff.any()), "%s y_cs=%d: %d elements differ, first (pixel, channel) %s" % (
            fn, y_cs, int(diff.sum()), torch.nonzero(diff)[0].tolist())
        assert bool((y[n:].float() == G.SENT).all())


# ---------------------------------------------------------------- w2l_frames_to_u8
@pytest.mark.parametrize("x_cs", G.FRAMES_XCS + ("slice",))
def test_frames_to_u8_equals_the_oracle(cuda, x_cs):
    """against datagen_ref.frames_to_u8 on k / 255 and its fp32 neighbours below and above for every k: the value below truncates
    to k - 1.  Values outside [0, 1] are out of scope: the conversion is undefined for them in the reference too.  "slice": three
    channels at channel offset 2 of a NaN-filled 8-channel buffer"""
    lib, s, ptr = _lib3()
    x = G.frames_inputs()
    off, cs = (2, 8) if x_cs == "slice" else (0, x_cs)
    xb = np.full((x.shape[0], cs), np.nan, np.float32)
    xb[:, off:off + 3] = x
    xd = _up(xb, cuda)
    for N, H, W in G.FRAMES_SHAPES:
        want = datagen_ref.frames_to_u8(x.reshape(N, H, W, 3).transpose(0, 3, 1, 2)).reshape(-1)
        y = _dest(want.size, cuda, dtype=torch.uint8)
        assert lib.w2l_frames_to_u8(s, N, H, W, _at(xd, off), cs, ptr(y)) == 0, lib.w2l_last_error()
        got = _read(y, want.size, "frames_to_u8 x_cs=%s" % (x_cs,))
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "x_cs=%s %s: %d of %d bytes differ, first at byte %d: %d for %r, want %d" % (
            x_cs, (N, H, W), len(bad), want.size, bad[0, 0], got[bad[0, 0]], float(x.reshape(-1)[bad[0, 0]]), want[bad[0, 0]])


def test_frames_to_u8_second_grid_stride_trip(cuda):
    lib, s, ptr = _lib3()
    N, H, W = G.FRAMES_BIG
    npix = N * H * W
    gen = torch.Generator(device=cuda).manual_seed(9)
    x = torch.rand((npix, 4), device=cuda, generator=gen)
    x[:768, :3] = _up(G.frames_inputs(), cuda)
    x[-768:, :3] = _up(G.frames_inputs(), cuda)
    x[:, 3] = NAN
    y = _dest(npix * 3, cuda, dtype=torch.uint8)
    assert lib.w2l_frames_to_u8(s, N, H, W, ptr(x), 4, ptr(y)) == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    want = (x[:, :3] * 255.0).to(torch.int32).to(torch.uint8).view(-1)
    assert np.array_equal(want[:768 * 3].cpu().numpy(), G.frames_f32(G.frames_inputs()).reshape(-1))
    diff = y[:npix * 3] != want
    assert not bool(diff.any()), "%d bytes differ, first at %s" % (int(diff.sum()), torch.nonzero(diff)[0].tolist())
    assert bool((y[npix * 3:] == U8_SENT).all())


# ---------------------------------------------------------------- w2l_nchw_to_nhwc / w2l_nhwc_to_nchw
def test_layout_case_table_holds_the_bf16_shapes():
    import test_bf16_train_ops_gpu as T
    for name, shape in T.LAYOUT_CASES.items():
        assert G.LAYOUT_CASES[name] == shape, name


@pytest.mark.parametrize("name", list(G.LAYOUT_CASES))
def test_layout_kernels_fp32_move_every_bit(cuda, name):
    """nchw_to_nhwc: the transpose bit for bit (+-0, +-inf, a denormal), zeros in [C, c_zero_to), the sentinel from there to y_cs;
    nhwc_to_nchw reads the first C channels of a slice of a NaN-filled buffer and writes nothing past its output"""
    lib, s, ptr = _lib3()
    N, C_, H, W, y_cs, czt = G.LAYOUT_CASES[name]
    x = G.layout_inputs(N, C_, H, W, seed=len(name))
    xd = _up(x, cuda)
    n = N * H * W * y_cs
    y = _dest(n, cuda)
    assert lib.w2l_nchw_to_nhwc(s, N, C_, H, W, ptr(xd), ptr(y), y_cs, czt) == 0, lib.w2l_last_error()
    _bits_equal("nchw_to_nhwc " + name, _read(y, n, name).reshape(N, H, W, y_cs), G.layout_expected(x, y_cs, czt))
    x_cs = y_cs + 16
    fence = np.full((N, H, W, x_cs), np.nan, np.float32)
    fence[..., 8:8 + C_] = x.transpose(0, 2, 3, 1)
    fd = _up(fence, cuda)
    out = _dest(x.size, cuda)
    assert lib.w2l_nhwc_to_nchw(s, N, C_, H, W, _at(fd, 8), x_cs, ptr(out)) == 0, lib.w2l_last_error()
    _bits_equal("nhwc_to_nchw " + name, _read(out, x.size, name).reshape(x.shape), x)


# ---------------------------------------------------------------- refusals
def _refusals(lib, fn, bad):
    """every call returns non-zero and leaves its own message (a known other message is planted before each)"""
    for name, args in bad.items():
        assert lib.w2l_adam_create(0, None, C.byref(C.c_void_p())) != 0
        mark = lib.w2l_last_error()
        rc = getattr(lib, fn)(*args)
        msg = lib.w2l_last_error()
        assert rc != 0, "%s accepted: %s" % (fn, name)
        assert msg and msg != mark, "%s refused %s without a message of its own" % (fn, name)


def _untouched(buf, what):
    torch.cuda.synchronize()
    sent = U8_SENT if buf.dtype == torch.uint8 else G.SENT
    assert bool((buf.float() == sent).all()), "%s: a refused call wrote to its output" % what


@pytest.mark.parametrize("kind", list(GLUE))
def test_detector_glue_refuses_bad_arguments_and_writes_nothing(cuda, kind):
    """bf16: C or a stride that is no multiple of 8, a base pointer 8 bytes off a 16-byte boundary, and shapes that reach 2 GiB
    in one buffer (the rule of the w2l_convb launches that consume these tensors; fp32 has no such rule) - shapes only, behind
    small buffers: the refusal comes before any launch"""
    lib, s, ptr = _lib3()
    z = torch.zeros(4096, device=cuda)
    zu = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    if kind == "fp32":
        out = _dest(4096, cuda)
        x, o = ptr(z), ptr(out)
        _refusals(lib, "w2l_s3fd_decode", {
            "ncls = 3": (s, 1, 4, 4, 4, x, 4, 3, x, 4, o), "cls_cs < ncls": (s, 1, 4, 4, 4, x, 3, 4, x, 4, o),
            "cls_cs < ncls = 2": (s, 1, 4, 4, 4, x, 1, 2, x, 4, o), "reg_cs < 4": (s, 1, 4, 4, 4, x, 4, 2, x, 3, o),
            "no cls": (s, 1, 4, 4, 4, None, 4, 2, x, 4, o), "no reg": (s, 1, 4, 4, 4, x, 4, 2, None, 4, o),
            "no out": (s, 1, 4, 4, 4, x, 4, 2, x, 4, None)})
        _refusals(lib, "w2l_maxpool2x2", {
            "C % 4 != 0": (s, 1, 4, 4, 6, x, 8, o, 8), "H < 2": (s, 1, 1, 4, 8, x, 8, o, 8), "x_cs < C": (s, 1, 4, 4, 8, x, 4, o, 8),
            "misaligned x": (s, 1, 4, 4, 8, _at(z, 1), 8, o, 8), "misaligned y": (s, 1, 4, 4, 8, x, 8, _at(out, 1), 8)})
        _refusals(lib, "w2l_l2norm_scale", {
            "C % 4 != 0": (s, 4, 6, x, 8, x, o, 8), "y_cs < C": (s, 4, 8, x, 8, x, o, 4), "misaligned weight": (s, 4, 8, x, 8, _at(z, 2), o, 8)})
        _refusals(lib, "w2l_s3fd_pack", {
            "y_cs < 3": (s, 16, ptr(zu), o, 2), "misaligned y with y_cs % 4 == 0": (s, 16, ptr(zu), _at(out, 1), 4),
            "misaligned y with y_cs = 8": (s, 16, ptr(zu), _at(out, 2), 8)})
        _untouched(out, "detector glue")
        assert lib.w2l_s3fd_pack(s, 16, ptr(zu), _at(out, 1), 5) == 0, "an odd stride needs no alignment"
        torch.cuda.synchronize()
        return
    zb = torch.zeros(4096, dtype=torch.bfloat16, device=cuda)
    out = _dest(4096, cuda, dtype=torch.bfloat16)
    x, w, o = ptr(zb), ptr(z), ptr(out)
    assert _at(zb, 4).value % 16 == 8 and _at(out, 4).value % 16 == 8 and _at(z, 2).value % 16 == 8
    _refusals(lib, "w2l_maxpool2x2_bf16", {
        "C % 8 != 0": (s, 1, 4, 4, 12, x, 16, o, 16), "x_cs % 8 != 0": (s, 1, 4, 4, 8, x, 12, o, 8),
        "y_cs % 8 != 0": (s, 1, 4, 4, 8, x, 8, o, 12), "H < 2": (s, 1, 1, 4, 8, x, 8, o, 8), "x_cs < C": (s, 1, 4, 4, 16, x, 8, o, 16),
        "x 8 bytes off": (s, 1, 4, 4, 8, _at(zb, 4), 8, o, 8), "y 8 bytes off": (s, 1, 4, 4, 8, x, 8, _at(out, 4), 8),
        "x of 2 GiB": (s, 1, 32768, 4096, 8, x, 8, o, 8)})
    _refusals(lib, "w2l_l2norm_scale_bf16", {
        "C % 8 != 0": (s, 4, 12, x, 16, w, o, 16), "x_cs % 8 != 0": (s, 4, 8, x, 12, w, o, 8), "y_cs % 8 != 0": (s, 4, 8, x, 8, w, o, 12),
        "y_cs < C": (s, 4, 16, x, 16, w, o, 8), "weight 8 bytes off": (s, 4, 8, x, 8, _at(z, 2), o, 8),
        "x 8 bytes off": (s, 4, 8, _at(zb, 4), 8, w, o, 8), "y 8 bytes off": (s, 4, 8, x, 8, w, _at(out, 4), 8),
        "x of 2 GiB": (s, 1 << 27, 8, x, 8, w, o, 8), "y of 2 GiB": (s, 1 << 26, 8, x, 8, w, o, 16)})
    _refusals(lib, "w2l_s3fd_pack_bf16", {
        "y_cs < 8": (s, 16, ptr(zu), o, 4), "y_cs % 8 != 0": (s, 16, ptr(zu), o, 12), "y 8 bytes off": (s, 16, ptr(zu), _at(out, 4), 8),
        "y of 2 GiB": (s, 1 << 27, ptr(zu), o, 8)})
    _untouched(out, "detector glue, bf16")


def test_input_packing_refuses_bad_arguments_and_writes_nothing(cuda):
    lib, s, ptr = _lib3()
    z = torch.zeros(4096, device=cuda)
    zu = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    out, outb, outu = _dest(4096, cuda), _dest(4096, cuda, dtype=torch.bfloat16), _dest(4096, cuda, dtype=torch.uint8)
    for fn, o in (("w2l_datagen_pack", ptr(out)), ("w2l_datagen_pack_bf16", ptr(outb))):
        _refusals(lib, fn, {"S < 2": (s, 1, 1, ptr(zu), o, 8, 8), "c_zero_to = 9": (s, 1, 4, ptr(zu), o, 16, 9),
                            "y_cs < c_zero_to": (s, 1, 4, ptr(zu), o, 7, 8), "y_cs < 6": (s, 1, 4, ptr(zu), o, 5, 0)})
    _refusals(lib, "w2l_frames_to_u8", {"x_cs < 3": (s, 1, 4, 4, ptr(z), 2, ptr(outu))})
    for buf in (out, outb, outu):
        _untouched(buf, "input packing")
