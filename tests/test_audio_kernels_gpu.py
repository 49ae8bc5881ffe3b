"""The audio front end's kernels (csrc/audio_mel.hip) and w2l_bn_fold through the C ABI at their edges.  tests/_audio_cases.py holds
the cases, the float64 references and the derivation of the bounds; tests/test_audio_cases_cpu.py pins them without a GPU.

- w2l_melspectrogram against the all-float64 spectrogram within the per-element bound (a few 1e-6; no element left out, the
  clipped ones included), bit-for-bit locality under a change of one sample, and w2l_mel_stream_cols bit for bit against it;
- the four mel window gathers bit for bit against one numpy expression: starts on both sides of both ends of the spectrogram,
  T = 16, channel strides with and without channels the kernel must leave alone, the second grid-stride trip, sentinel guard
  bands around every output, and every refusal;
- w2l_resample_sinc bit for bit against oracle/resample_ref.py at 1 - 4 input samples, around the 128-thread block and at the
  smallest table step, and its refusals;
- w2l_bn_fold against float64 under every NULL pattern.
Every output lies between two guard bands of a sentinel that must survive."""
import ctypes as C

import numpy as np
import pytest
import torch

import _audio_cases as ac
from _audio_cases import F32, SENT
from oracle import resample_ref
from wav2lip_amd import _lib, audio
from wav2lip_amd._lib import check, current_stream, ptr

pytestmark = pytest.mark.gpu

GUARD = 64
SENT_BF16 = int(ac.bf16_bits(np.array([SENT], F32))[0])


def _dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _guarded(n, cuda, dtype=torch.float32):
    """(buffer of GUARD + n + GUARD sentinel cells, the n cells in the middle a kernel may write)"""
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=cuda)
    return buf, buf[GUARD:GUARD + n]


def _bits(t):
    """bit patterns of a device tensor on the host: uint32 for fp32, uint16 for bf16"""
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.contiguous().cpu().numpy().view(np.uint32)


def _guards_intact(buf):
    b = _bits(buf)
    sent = SENT_BF16 if buf.dtype == torch.bfloat16 else F32(SENT).view(np.uint32)
    return bool((b[:GUARD] == sent).all()) and bool((b[-GUARD:] == sent).all())


def _marker(lib, by_bn_fold=False):
    """put a known message into w2l_last_error, so that the next refusal is seen to write its own (by_bn_fold: from an entry
    point whose message differs from the plain "NULL argument" of w2l_mel_create and w2l_resample_sinc)"""
    if by_bn_fold:
        assert lib.w2l_bn_fold(current_stream(), 0, None, None, None, None, None, 1e-5, None, None) != 0
    else:
        assert lib.w2l_mel_create(None, None, None) != 0
    return lib.w2l_last_error()


# ---------------------------------------------------------------- w2l_melspectrogram
def _mel(wav, cuda):
    """[80, T] fp32 on the host, through the C entry point into a guarded buffer"""
    lib = _lib.load()
    w = _dev(np.array(wav, F32), cuda)
    T = lib.w2l_mel_num_frames(len(wav))
    assert T == 1 + len(wav) // 200
    buf, out = _guarded(80 * T, cuda)
    check(lib.w2l_melspectrogram(audio._context(cuda), current_stream(), ptr(w), len(wav), ptr(out)), "melspectrogram")
    torch.cuda.synchronize()
    assert _guards_intact(buf), "w2l_melspectrogram wrote outside [80, T]"
    return out.cpu().numpy().reshape(80, T)


@pytest.mark.parametrize("name", list(ac.mel_cases()))
def test_melspectrogram_is_inside_the_float64_bound(name, cuda):
    """every element of every case, clipped or not, within the derived bound of the all-float64 spectrogram.  Measured on the
    MI355X: the largest error over all cases is 1.2e-6, the largest error / bound 0.42 (the per-case figures are printed)"""
    v, M, bound = ac.mel_reference(name)
    got = _mel(ac.mel_cases()[name], cuda)
    assert got.shape == v.shape and got.dtype == np.float32 and not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - v)
    print("mel %s: max |error| %.3e, max error / bound %.3f" % (name, err.max(), (err / bound).max()))
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d of %d elements outside the bound, worst error / bound %.2f" % (name, int(bad.sum()), bad.size,
                                                                                               float((err / bound).max()))
    assert got.min() >= -4 and got.max() <= 4


@pytest.fixture(scope="module")
def locality_base(cuda):
    return _mel(ac.locality_wav(), cuda)


@pytest.mark.parametrize("k", ac.LOCALITY_K)
def test_melspectrogram_columns_depend_on_their_own_window_only(k, locality_base, cuda):
    """one sample replaced: the columns whose reflected window (or its pre-emphasis predecessor) holds it may change, every
    other column is the untouched run bit for bit, and something does change"""
    wav = ac.locality_wav()
    wav[k] = wav[k] + F32(0.25)
    assert np.isfinite(wav[k]) and wav[k] != ac.locality_wav()[k]
    got = _mel(wav, cuda)
    may = ac.locality_columns(ac.LOCALITY_N, k)
    others = np.setdiff1d(np.arange(got.shape[1]), may)
    assert len(others) >= 1 and np.array_equal(got[:, others].view(np.uint32), locality_base[:, others].view(np.uint32)), \
        "sample %d changed a column outside %s" % (k, may.tolist())
    assert (got[:, may] != locality_base[:, may]).any()


# ---------------------------------------------------------------- w2l_mel_stream_cols
def _stream_columns(wav_d, held, total, cols, cap, cuda):
    """one stream holding samples [0, held) of a signal of `total` samples (-1: open), the listed columns into a guarded
    sentinel window [80, cap]; the tables are streaming.MEL_STREAM / MEL_COL, as tests/test_streaming_gpu.py builds them"""
    from wav2lip_amd import streaming
    lib = _lib.load()
    buf, flat = _guarded(80 * cap, cuda)
    st = np.zeros(1, streaming.MEL_STREAM)
    st[0] = (wav_d.data_ptr(), 0, total, flat.data_ptr(), held, cap, 0)
    ct = np.zeros(len(cols), streaming.MEL_COL)
    ct[:] = [(0, 0, c) for c in cols]
    sd, cd = (_dev(t.view(np.uint8).copy(), cuda) for t in (st, ct))
    check(lib.w2l_mel_stream_cols(audio._context(cuda), current_stream(), ptr(sd), 1, ptr(cd), len(cols)), "mel_stream_cols")
    torch.cuda.synchronize()
    assert _guards_intact(buf), "w2l_mel_stream_cols wrote outside its window"
    return flat.cpu().numpy().reshape(80, cap)


@pytest.mark.parametrize("N", ac.STREAM_LENGTHS)
def test_stream_columns_equal_the_whole_signal_kernel_bit_for_bit(N, cuda):
    """the whole signal held (first = 0, held = total = N), every column listed: w2l_melspectrogram's bits.  Then the open stream
    (total = -1), which has no end to reflect at: the columns t <= (N - 400) // 200, whose window ends at sample 200 t + 399 <= N - 1,
    are final and equal; the columns behind them are not listed and keep the sentinel"""
    wav = ac.mel_cases()["noise%d" % N]
    assert len(wav) == N
    whole = _mel(wav, cuda)
    T = whole.shape[1]
    wd = _dev(np.array(wav, F32), cuda)
    closed = _stream_columns(wd, N, N, list(range(T)), T, cuda)
    assert np.array_equal(closed.view(np.uint32), whole.view(np.uint32))
    n_open = ac.open_stream_columns(N)
    assert 1 <= n_open < T and 200 * (n_open - 1) + 399 <= N - 1 < 200 * n_open + 399
    opened = _stream_columns(wd, N, -1, list(range(n_open)), T, cuda)
    assert np.array_equal(opened[:, :n_open].view(np.uint32), whole[:, :n_open].view(np.uint32))
    assert (opened[:, n_open:] == SENT).all()


# ---------------------------------------------------------------- the mel window gathers
GATHER_KINDS = [("f32", cs, cz) for cs, cz in ac.GATHER_STRIDES_F32] + [("bf16", cs, cz) for cs, cz in ac.GATHER_STRIDES_BF16]
GATHER_SHAPES = [(ac.GATHER_T, len(ac.GATHER_STARTS)), (16, len(ac.GATHER_T16_STARTS)), (ac.GATHER_T, ac.GATHER_B_SECOND_TRIP)]


def _expected(win, kind, cs, cz):
    """bit patterns of the whole output from the fp32 windows [B, 80, 16]"""
    if kind == "bf16":
        return ac.gather_expect(ac.bf16_bits(win).reshape(win.shape), cs, cz, np.uint16(SENT_BF16))
    return ac.gather_expect(win, cs, cz, F32(SENT)).view(np.uint32)


def _out_for(kind, n, cuda):
    return _guarded(n, cuda, torch.bfloat16 if kind == "bf16" else torch.float32)


@pytest.mark.parametrize("kind,cs,cz", GATHER_KINDS, ids=["%s-cs%d-z%d" % k for k in GATHER_KINDS])
@pytest.mark.parametrize("T,B", GATHER_SHAPES, ids=["T%d-B%d" % s for s in GATHER_SHAPES])
def test_mel_gather_is_the_numpy_expression_bit_for_bit(T, B, kind, cs, cz, cuda):
    """out[b, m, j, 0] = mel[m, s + j] inside the spectrogram, +0 outside; channels 1 .. c_zero_to - 1 zero; channels from
    max(c_zero_to, 1) on and both guard bands still the sentinel.  bf16: the fp32 value rounded once to nearest even.  B = 820 is
    the first batch whose last row is written on the kernel's second grid-stride trip; every row is compared"""
    lib = _lib.load()
    mel = ac.gather_mel(T, T)
    starts = ac.gather_starts(B, ac.GATHER_STARTS if T == ac.GATHER_T else ac.GATHER_T16_STARTS)
    assert B * 80 * 16 > ac.GATHER_GRID_ITEMS or B < 100
    md, sd = _dev(mel, cuda), _dev(np.array(starts, np.int32), cuda)
    buf, out = _out_for(kind, B * 80 * 16 * cs, cuda)
    fn = lib.w2l_mel_gather_bf16 if kind == "bf16" else lib.w2l_mel_gather
    check(fn(current_stream(), ptr(md), T, ptr(sd), B, ptr(out), cs, cz), "mel_gather")
    torch.cuda.synchronize()
    assert _guards_intact(buf), "mel_gather wrote outside its output"
    got = _bits(out).reshape(B, 80, 16, cs)
    want = _expected(ac.gather_windows(mel, starts), kind, cs, cz)
    if not np.array_equal(got, want):
        b, m, j, c = (int(i[0]) for i in np.nonzero(got != want))
        raise AssertionError("row %d (start %d) mel %d column %d channel %d: got bits %#x, want %#x (%d cells differ)" % (
            b, starts[b], m, j, c, got[b, m, j, c], want[b, m, j, c], int((got != want).sum())))


@pytest.mark.parametrize("kind,cs,cz", GATHER_KINDS, ids=["%s-cs%d-z%d" % k for k in GATHER_KINDS])
@pytest.mark.parametrize("B", [45, ac.GATHER_B_SECOND_TRIP])
def test_mel_gather_rows_is_the_numpy_expression_bit_for_bit(B, kind, cs, cz, cuda):
    """one spectrogram per row: three of T = 37, 16 and 50, every row on another one than its neighbours, the starts of the plain
    gather per spectrogram; the same numpy expression per row"""
    from wav2lip_amd import multiclip
    lib = _lib.load()
    mels = [ac.gather_mel(T, 10 + T) for T in ac.ROWS_T]
    mds = [_dev(m, cuda) for m in mels]
    rows = ac.gather_rows(B)
    assert all(rows[i][0] != rows[i + 1][0] for i in range(B - 1))
    table = np.zeros(B, multiclip.MEL_ROW)
    table[:] = [(mds[c].data_ptr(), ac.ROWS_T[c], s) for c, s in rows]
    td = _dev(table.view(np.uint8).copy(), cuda)
    buf, out = _out_for(kind, B * 80 * 16 * cs, cuda)
    fn = lib.w2l_mel_gather_rows_bf16 if kind == "bf16" else lib.w2l_mel_gather_rows
    check(fn(current_stream(), ptr(td), B, ptr(out), cs, cz), "mel_gather_rows")
    torch.cuda.synchronize()
    assert _guards_intact(buf), "mel_gather_rows wrote outside its output"
    win = np.zeros((B, 80, 16), F32)
    for c in range(3):
        idx = [i for i, r in enumerate(rows) if r[0] == c]
        win[idx] = ac.gather_windows(mels[c], [rows[i][1] for i in idx])
    got, want = _bits(out).reshape(B, 80, 16, cs), _expected(win, kind, cs, cz)
    if not np.array_equal(got, want):
        b, m, j, c = (int(i[0]) for i in np.nonzero(got != want))
        raise AssertionError("row %d (T %d, start %d) mel %d column %d channel %d: got bits %#x, want %#x (%d cells differ)" % (
            b, ac.ROWS_T[rows[b][0]], rows[b][1], m, j, c, got[b, m, j, c], want[b, m, j, c], int((got != want).sum())))


def test_mel_gather_refusals_name_the_function_and_write_nothing(cuda):
    """T < 16, B < 1, a NULL pointer, out_cs < c_zero_to; for the row forms also B > 65535 and a table off its 16-byte alignment"""
    from wav2lip_amd import multiclip
    lib, s = _lib.load(), current_stream()
    T, B = 16, 2
    md, sd = _dev(ac.gather_mel(T, 3), cuda), _dev(np.zeros(B, np.int32), cuda)
    table = np.zeros(B + 1, multiclip.MEL_ROW)
    table[:] = [(md.data_ptr(), T, 0)] * (B + 1)
    td = _dev(table.view(np.uint8).copy(), cuda)
    assert td.data_ptr() % 16 == 0
    outs = {"f32": _guarded(B * 80 * 16 * 8, cuda)[0], "bf16": _guarded(B * 80 * 16 * 8, cuda, torch.bfloat16)[0]}
    for kind, plain, rowsf in (("f32", lib.w2l_mel_gather, lib.w2l_mel_gather_rows),
                               ("bf16", lib.w2l_mel_gather_bf16, lib.w2l_mel_gather_rows_bf16)):
        o = ptr(outs[kind])
        calls = {
            "T=15": lambda: plain(s, ptr(md), 15, ptr(sd), B, o, 8, 8),
            "B=0": lambda: plain(s, ptr(md), T, ptr(sd), 0, o, 8, 8),
            "B=-1": lambda: plain(s, ptr(md), T, ptr(sd), -1, o, 8, 8),
            "mel NULL": lambda: plain(s, None, T, ptr(sd), B, o, 8, 8),
            "starts NULL": lambda: plain(s, ptr(md), T, None, B, o, 8, 8),
            "out NULL": lambda: plain(s, ptr(md), T, ptr(sd), B, None, 8, 8),
            "out_cs < c_zero_to": lambda: plain(s, ptr(md), T, ptr(sd), B, o, 4, 8),
            "out_cs = 0": lambda: plain(s, ptr(md), T, ptr(sd), B, o, 0, 0),
            "rows NULL": lambda: rowsf(s, None, B, o, 8, 8),
            "rows out NULL": lambda: rowsf(s, ptr(td), B, None, 8, 8),
            "rows B=0": lambda: rowsf(s, ptr(td), 0, o, 8, 8),
            "rows B=65536": lambda: rowsf(s, ptr(td), 65536, o, 8, 8),
            "rows misaligned": lambda: rowsf(s, C.c_void_p(td.data_ptr() + 8), B, o, 8, 8),
            "rows out_cs < c_zero_to": lambda: rowsf(s, ptr(td), B, o, 4, 8),
        }
        for name, call in calls.items():
            mark = _marker(lib)
            rc = call()
            msg = lib.w2l_last_error()
            assert rc != 0, "%s %s: accepted" % (kind, name)
            assert msg != mark and (b"mel_gather_rows" if name.startswith("rows") else b"mel_gather") in msg, (kind, name, msg)
    torch.cuda.synchronize()
    for kind, t in outs.items():
        b = _bits(t)
        assert (b == (SENT_BF16 if kind == "bf16" else F32(SENT).view(np.uint32))).all(), "a refused %s gather wrote its output" % kind


# ---------------------------------------------------------------- w2l_resample_sinc
@pytest.mark.parametrize("orig_sr,n", list(ac.RESAMPLE_CASES), ids=["%d-%d" % k for k in ac.RESAMPLE_CASES])
def test_resample_edges_are_bit_exact(orig_sr, n, cuda):
    """1 - 4 input samples (both wings cut by the signal's ends), n_out = 128, 128 and 129 (the 128-thread block), and 8.192 MHz,
    whose ratio 1 / 512 gives the smallest table step (index_step == 1)"""
    x = ac.resample_input(orig_sr, n)
    got = audio.resample(x, orig_sr, 16000)
    ref = resample_ref.librosa_resample(x, orig_sr, 16000)
    assert got.dtype == np.float32 and got.shape == ref.shape == (ac.RESAMPLE_CASES[(orig_sr, n)][1],)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (got, ref)


def _resample_buffers(cuda):
    win = np.linspace(1.0, 0.0, 1025)
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    x, tr = _dev(np.ones(8, F32), cuda), _dev(np.zeros(2, np.float64), cuda)
    return x, tr, _dev(win, cuda), _dev(delta, cuda)


def test_resample_refuses_a_ratio_below_the_table_step(cuda):
    """sample_ratio = 1 / 1024 with 512 table samples per zero crossing: index_step = int(0.5) = 0, which would divide by zero"""
    lib, s = _lib.load(), current_stream()
    x, tr, win, delta = _resample_buffers(cuda)
    buf, y = _guarded(2, cuda)
    assert ac.resample_index_step(16000 * 1024) == 0
    mark = _marker(lib, by_bn_fold=True)
    rc = lib.w2l_resample_sinc(s, ptr(x), 8, ptr(tr), 2, 1.0 / 1024, ptr(win), ptr(delta), 1025, 512, ptr(y))
    msg = lib.w2l_last_error()
    assert rc != 0 and msg != mark and b"table" in msg, msg
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    # the same call at the smallest ratio the table allows runs
    check(lib.w2l_resample_sinc(s, ptr(x), 8, ptr(tr), 2, 1.0 / 512, ptr(win), ptr(delta), 1025, 512, ptr(y)), "resample_sinc")
    torch.cuda.synchronize()
    assert _guards_intact(buf) and bool((y != SENT).all())


def test_resample_refusals_write_nothing(cuda):
    lib, s = _lib.load(), current_stream()
    x, tr, win, delta = _resample_buffers(cuda)
    buf, y = _guarded(2, cuda)
    X, TR, W, D, Y = ptr(x), ptr(tr), ptr(win), ptr(delta), ptr(y)
    calls = {
        "x NULL": lambda: lib.w2l_resample_sinc(s, None, 8, TR, 2, 0.5, W, D, 1025, 512, Y),
        "tr NULL": lambda: lib.w2l_resample_sinc(s, X, 8, None, 2, 0.5, W, D, 1025, 512, Y),
        "win NULL": lambda: lib.w2l_resample_sinc(s, X, 8, TR, 2, 0.5, None, D, 1025, 512, Y),
        "delta NULL": lambda: lib.w2l_resample_sinc(s, X, 8, TR, 2, 0.5, W, None, 1025, 512, Y),
        "y NULL": lambda: lib.w2l_resample_sinc(s, X, 8, TR, 2, 0.5, W, D, 1025, 512, None),
        "n_in=0": lambda: lib.w2l_resample_sinc(s, X, 0, TR, 2, 0.5, W, D, 1025, 512, Y),
        "n_out=0": lambda: lib.w2l_resample_sinc(s, X, 8, TR, 0, 0.5, W, D, 1025, 512, Y),
        "nwin=1": lambda: lib.w2l_resample_sinc(s, X, 8, TR, 2, 0.5, W, D, 1, 512, Y),
        "num_table=0": lambda: lib.w2l_resample_sinc(s, X, 8, TR, 2, 0.5, W, D, 1025, 0, Y),
        "ratio=0": lambda: lib.w2l_resample_sinc(s, X, 8, TR, 2, 0.0, W, D, 1025, 512, Y),
        "ratio<0": lambda: lib.w2l_resample_sinc(s, X, 8, TR, 2, -1.0, W, D, 1025, 512, Y),
    }
    for name, call in calls.items():
        mark = _marker(lib, by_bn_fold=True)
        rc = call()
        assert rc != 0 and lib.w2l_last_error() != mark, name
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()), "a refused resample wrote y"


# ---------------------------------------------------------------- w2l_bn_fold
@pytest.mark.parametrize("pattern", ac.BN_PATTERNS)
@pytest.mark.parametrize("C_", ac.BN_C)
def test_bn_fold_against_float64(C_, pattern, cuda):
    """scale = gamma / sqrt(var + eps), shift = (bias - mean) scale + beta within the fp32 roundings of the five operations; var = 0
    and 1e-12 under eps = 1e-5, 1e10 and 1e30; without the BatchNorm tensors scale is exactly 1 and shift exactly the bias (0
    without one)"""
    lib = _lib.load()
    bias, gamma, beta, mean, var = ac.bn_inputs(C_, C_)
    bn, has_bias = pattern in ("all", "no_bias"), pattern in ("all", "no_bn")
    dev = [_dev(t, cuda) for t in (bias, gamma, beta, mean, var)]
    args = [ptr(dev[0]) if has_bias else None] + [ptr(t) if bn else None for t in dev[1:]]
    sbuf, scale = _guarded(C_, cuda)
    hbuf, shift = _guarded(C_, cuda)
    check(lib.w2l_bn_fold(current_stream(), C_, *args, 1e-5 if bn else 0.0, ptr(scale), ptr(shift)), "bn_fold")
    torch.cuda.synchronize()
    assert _guards_intact(sbuf) and _guards_intact(hbuf), "bn_fold wrote outside [0, C)"
    gs, gh = scale.cpu().numpy(), shift.cpu().numpy()
    rs, rh, ts = ac.bn_ref(pattern, bias, gamma, beta, mean, var)
    bs, bh = ac.bn_bounds(pattern, rs, rh, ts)
    assert np.isfinite(gs).all() and np.isfinite(gh).all()
    es, eh = np.abs(gs - rs), np.abs(gh - rh)
    if bn:
        print("bn_fold C%d %s: scale error / bound %.3f, shift error / bound %.3f" % (
            C_, pattern, (es[bs > 0] / bs[bs > 0]).max(), (eh[bh > 0] / bh[bh > 0]).max()))
    assert (es <= bs).all() and (eh <= bh).all(), (pattern, float(es.max()), float(eh.max()))


def test_bn_fold_refusals_write_nothing(cuda):
    lib, s = _lib.load(), current_stream()
    sbuf, scale = _guarded(4, cuda)
    hbuf, shift = _guarded(4, cuda)
    for C_, sc, sh in ((0, ptr(scale), ptr(shift)), (-1, ptr(scale), ptr(shift)), (4, None, ptr(shift)), (4, ptr(scale), None)):
        mark = _marker(lib)
        assert lib.w2l_bn_fold(s, C_, None, None, None, None, None, 1e-5, sc, sh) != 0
        msg = lib.w2l_last_error()
        assert msg != mark and b"bn_fold" in msg
    torch.cuda.synchronize()
    assert bool((sbuf == SENT).all()) and bool((hbuf == SENT).all())
