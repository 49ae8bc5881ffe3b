"""Cases, float64 references and error bounds shared by tests/test_audio_kernels_gpu.py (the HIP kernels of csrc/audio_mel.hip,
w2l_bn_fold, w2l_lse_score_segments) and tests/test_audio_cases_cpu.py (which pins the tables and checks the bounds against the
CPU oracle).  No fixtures, no tests, nothing that needs a device: numpy only (the project's fp32 mel basis is built by
wav2lip_amd.audio on the host).

The mel bound, per element, u = 2^-24 (fp32 unit roundoff), first order in u with a 1e-4 relative margin for the second order
(every relative error below is under 1e-5):

  the kernel computes, per column, frame = window * preemph(reflect(wav)) and its 800-point DFT in float64, casts re and im to
  fp32, takes mag = hypotf(re, im), M = sum_k basis[m, k] * mag[k] with fmaf in fp32, L = log10f(max(1e-5f, M)), S = 20 L - 20,
  v = clip(8 ((S + 100) / 100) - 4, -4, 4).  Inside the clip v = 1.6 log10(M) + 2.4: v = -4 at M = 1e-4, v = +4 at M = 10, so
  the 1e-5 floor lies under the lower clip and |dv| = (1.6 / ln 10) |dM| / M = 0.695 |dM| / M.

  dM, relative: every term basis * mag is non-negative, so sum|terms| = M.  A zero basis entry adds exactly nothing
  (fmaf(0, x, acc) == acc), so a filter with n non-zero taps performs n roundings: n u M.  Each mag carries the two casts (u: a
  relative perturbation of both components by at most u moves their norm by at most u) and hypotf's error, HYPOT_ULP ulp =
  2 HYPOT_ULP u.  Together (n + 1 + 2 HYPOT_ULP) u M, n counted per filter from the basis itself (mel_taps()).
  dM, absolute: the float64 DFT's own rounding, on the device (a recursive sum of 800 fma terms: at most 800 * 2^-53 * sum|frame|
  per component, the twiddles' roundings included to first order) and in the reference's FFT (far smaller); both components and
  both sides are covered by 1600 * 2^-53 * sum|frame| per bin, times the filter's row sum.  It only matters next to an M near
  the lower clip.  3 * 2^-149 per bin for casts that land in the denormals.
  The logarithm turns dM into -log1p(-dM / max(M, 1e-5)) (max is 1-Lipschitz, so the floor needs no case of its own).
  log10f: LOG10_ULP ulp of L = 2 LOG10_ULP u |L|.
  Then one rounding each for 20 L, - 20, + 100, / 100 (IEEE division: hipcc's default for fp32) and - 4, each u times the
  magnitude of its result, carried through the remaining factors (x 8 is exact).  |S| <= 120, so these add about 1.5e-6.
  A contraction of 20 L - 20 or 8 q - 4 into one fma only removes a rounding.
  clip is 1-Lipschitz and continuous: |clip(a) - clip(b)| <= |a - b|, so the bound on the unclipped value holds for the clipped
  one and no element is left out.

  HYPOT_ULP = 4 and LOG10_ULP = 3 are the figures of the OpenCL C specification's table of relative errors (section 7.4:
  hypot <= 4 ulp, log10 <= 3 ulp), the contract the device math library (OCML) is written to; HIP's own math API page reports 1
  and 2.  glibc documents hypotf at 1 and log10f at 2 ulp, so the CPU oracle (np.abs of complex64, sgemm, np.log10 in fp32) is
  covered by the same figures; its sgemm adds the non-zero taps in another order, with at most a handful of extra additions for
  the vector lanes' partial sums, which the slack between 2 HYPOT_ULP u and glibc's 2 u covers.
  The result is 1.5e-6 .. 6.3e-6 on these inputs (test_audio_cases_cpu.py asserts < 1e-5); the CPU oracle reaches 0.34 of it, the
  kernel 0.42.

w2l_bn_fold, scale = g / sqrt(var + eps): the addition (u, halved by the root), the root, the division and the product: 3.5 u,
rounded up to 4 u |scale| for the second order.  shift = (bias - mu) scale + beta: the difference t (u), the inherited 3.5 u of
scale, the product's own u: 5.5 u |t scale|, rounded up to 6 u, plus u |shift| for the last addition (an fma removes one).  With
no BatchNorm tensors scale is exactly 1 and shift exactly bias; with nothing at all 1 and 0.

The mel gather and the resampler are exact (bit patterns); the LSE scores take their NaN expectations from oracle/lse_ref.py."""
import numpy as np

U = 2.0 ** -24
F32 = np.float32
SENT = 12352.0                       # exactly representable in bf16 (193 * 64)
N_FFT, HOP, PAD, N_MELS, BINS = 800, 200, 400, 80, 401
PREEMPH = 0.97
MIN_LEVEL = float(F32(1e-5))         # the floor as the kernel holds it
HYPOT_ULP, LOG10_ULP = 4, 3
DFT_ABS = 1600 * 2.0 ** -53
SECOND_ORDER = 1.0001
MEL_BOUND_CEILING = 1e-5             # a derived bound above this means the derivation needs another look

_BASIS = None


def basis():
    """the project's fp32 mel basis [80, 401] (the table w2l_mel_create receives)"""
    global _BASIS
    if _BASIS is None:
        from wav2lip_amd import audio
        _BASIS = audio._build_mel_basis()
        assert _BASIS.dtype == np.float32 and _BASIS.shape == (N_MELS, BINS)
    return _BASIS


def mel_taps():
    """non-zero taps per mel filter, counted from the basis"""
    return (basis() != 0).sum(1)


# ---------------------------------------------------------------- the spectrogram in float64
def reflect_index(N, T=None):
    """[T, 800] sample index read at window position n of column t: np.pad(mode='reflect') by 400 on both sides"""
    T = 1 + N // HOP if T is None else T
    j = HOP * np.arange(T, dtype=np.int64)[:, None] + np.arange(N_FFT, dtype=np.int64)[None, :] - PAD
    j = np.where(j < 0, -j, j)
    return np.where(j >= N, 2 * (N - 1) - j, j)


def hann():
    """scipy.signal.get_window('hann', 800, fftbins=True): the periodic Hann window, float64"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)


def mel_f64(wav):
    """audio_ref.melspectrogram with nothing rounded below float64 -> (v [80, T] clipped, M [80, T] before the logarithm,
    sum|frame| [T])"""
    from scipy import signal
    x = np.asarray(wav, dtype=np.float64)
    y = signal.lfilter([1, -PREEMPH], [1], x)
    yp = np.pad(y, PAD, mode="reflect")
    T = 1 + (len(yp) - N_FFT) // HOP
    idx = np.arange(N_FFT)[:, None] + HOP * np.arange(T)[None, :]
    frames = signal.get_window("hann", N_FFT, fftbins=True)[:, None] * yp[idx]            # [800, T]
    mag = np.abs(np.fft.rfft(frames, axis=0))                                                # [401, T] float64
    M = basis().astype(np.float64) @ mag
    S = 20.0 * np.log10(np.maximum(MIN_LEVEL, M)) - 20.0
    v = np.clip(8.0 * ((S + 100.0) / 100.0) - 4.0, -4.0, 4.0)
    return v, M, np.abs(frames).sum(0)


def mel_bound(M, fsum):
    """per-element bound on |fp32 implementation - mel_f64| (module docstring)"""
    b = basis().astype(np.float64)
    rel = (mel_taps() + 1 + 2 * HYPOT_ULP)[:, None] * U
    dM = rel * M + b.sum(1)[:, None] * (DFT_ABS * fsum[None, :] + 3 * 2.0 ** -149)
    Mc = np.maximum(M, MIN_LEVEL)
    L = np.log10(Mc)
    dL = -np.log1p(-np.minimum(dM / Mc, 0.5)) / np.log(10.0) + 2 * LOG10_ULP * U * np.abs(L)
    S20 = 20.0 * L
    S = S20 - 20.0
    A = S + 100.0
    q = A / 100.0
    v = 8.0 * q - 4.0
    dS = 20.0 * dL + U * np.abs(S20) + U * np.abs(S)
    dq = (dS + U * np.abs(A)) / 100.0 + U * np.abs(q)
    return SECOND_ORDER * (8.0 * dq + U * np.abs(v))


def _noise(n, sigma, seed):
    return (np.random.default_rng(seed).standard_normal(n) * sigma).astype(F32)


def _impulse(k, n=1000):
    x = np.zeros(n, F32)
    x[k] = 1.0
    return x


MEL_NOISE_LENGTHS = (401, 599, 600, 601, 799, 800, 801, 1000, 16123)
MEL_IMPULSES = (0, 1, 399, 400, 401, 998, 999)
_MEL_CASES = None


def mel_cases():
    """name -> fp32 signal (built once; callers must not modify them)"""
    global _MEL_CASES
    if _MEL_CASES is None:
        c = {}
        for i, n in enumerate(MEL_NOISE_LENGTHS):
            c["noise%d" % n] = _noise(n, 0.1, 100 + i)
        for k in MEL_IMPULSES:
            c["impulse%d" % k] = _impulse(k)
        c["dc"] = np.ones(1000, F32)
        c["sine440"] = np.sin(2 * np.pi * 440.0 * np.arange(4000) / 16000.0).astype(F32)
        # 440 Hz is bin 22 exactly, so away from the signal's ends only three bins of sine440 are non-zero.  450 Hz lies between
        # two bins and leaks into all of them: bins that are small next to the DFT's partial sums, where an accumulator narrower
        # than float64 shows (test_audio_cases_cpu.py: an fp32 accumulator stays inside the bound on every other case)
        c["sine450"] = np.sin(2 * np.pi * 450.0 * np.arange(4000) / 16000.0).astype(F32)
        c["tone_noise"] = (30.0 * np.sin(2 * np.pi * 450.0 * np.arange(4000) / 16000.0)
                           + 1e-3 * np.random.default_rng(123).standard_normal(4000)).astype(F32)
        c["ramp"] = (np.random.default_rng(120).standard_normal(6000) * np.logspace(-6, 3, 6000)).astype(F32)
        c["loud"] = _noise(3000, 3000.0, 121)
        c["quiet"] = _noise(3000, 3e-5, 122)
        for w in c.values():
            w.setflags(write=False)
        _MEL_CASES = c
    return _MEL_CASES


_MEL_REFS = {}


def mel_reference(name):
    """(v, M, bound) of a case, computed once"""
    if name not in _MEL_REFS:
        v, M, fsum = mel_f64(mel_cases()[name])
        _MEL_REFS[name] = (v, M, mel_bound(M, fsum))
    return _MEL_REFS[name]


# locality: which columns may change when sample k changes
LOCALITY_N = 2000
LOCALITY_K = (0, 1, 400, 1000, 1998, 1999)


def locality_wav():
    return _noise(LOCALITY_N, 0.1, 130)


def locality_columns(N, k):
    """columns whose reflected 800-sample window contains sample k, or contains k + 1 as a sample with a pre-emphasis
    predecessor (every sample but 0 has one)"""
    j = reflect_index(N)
    hit = (j == k) | ((j - 1 == k) & (j != 0))
    return np.flatnonzero(hit.any(1))


# the stream path: lengths, and the columns an open stream (total = -1) can compute from N held samples - column t reads up to
# sample 200 t + 399 without an end to reflect at, so t <= (N - 400) // 200
STREAM_LENGTHS = (401, 600, 801, 1000)


def open_stream_columns(N):
    return (N - PAD) // HOP + 1


# ---------------------------------------------------------------- the mel window gather
GATHER_T = 37
GATHER_STARTS = (-2 ** 30, -17, -16, -15, -1, 0, 21, 22, 36, 37, 38, 2 ** 30)
GATHER_T16_STARTS = (-1, 0, 1)
GATHER_STRIDES_F32 = ((1, 1), (4, 4), (4, 1), (8, 4), (4, 0))          # (out_cs, c_zero_to)
GATHER_STRIDES_BF16 = ((8, 8), (8, 1), (16, 8), (8, 0))
GATHER_B_SECOND_TRIP = 820                                             # the grid caps at 4096 x 256 items = 819.2 rows
GATHER_GRID_ITEMS = 4096 * 256
ROWS_T = (37, 16, 50)
ROWS_STARTS = (GATHER_STARTS, GATHER_T16_STARTS, (-16, -1, 0, 34, 35, 49, 50))


def gather_mel(T, seed):
    """uniform(-4, 4) [80, T] with exact +-4, +-0 and values on bf16 rounding ties (low 16 bits 0x8000, the kept bit even and
    odd) scattered over it, column 0 and column T - 1 included"""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-4, 4, (N_MELS, T)).astype(F32)
    bits = m.view(np.uint32)                                          # shares m's memory
    flat = bits.reshape(-1)
    tie = rng.permutation(flat.size)[:36]
    flat[tie] = (flat[tie] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    flat[tie[::2]] |= np.uint32(0x10000)                              # odd kept bit: the tie rounds up
    flat[tie[1::2]] &= np.uint32(0xFFFEFFFF)                          # even kept bit: the tie rounds down
    m[0, 0], m[1, T - 1], m[2, 0], m[3, T - 1], m[4, 5], m[5, 7] = 4.0, -4.0, -0.0, 0.0, -4.0, 4.0
    for r, c in ((6, 0), (7, T - 1)):
        bits[r, c] = (bits[r, c] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    return m


def bf16_bits(x):
    """fp32 -> bf16 bit patterns, round to nearest even (finite input)"""
    b = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def gather_windows(mel, starts):
    """[B, 80, 16] fp32: out[b, m, j] = mel[m, s + j] if 0 <= s + j < T else +0"""
    T = mel.shape[1]
    s = np.asarray(starts, np.int64)[:, None] + np.arange(16, dtype=np.int64)[None, :]
    ok = (s >= 0) & (s < T)
    w = mel[:, np.clip(s, 0, T - 1)].transpose(1, 0, 2)               # [B, 80, 16]
    return np.where(ok[:, None, :], w, F32(0.0)).astype(F32)


def gather_expect(win, out_cs, c_zero_to, sent):
    """the whole output from channel 0's values (or bits): channels 1 .. max(c_zero_to, 1) - 1 zero, the rest still `sent`"""
    out = np.full(win.shape + (out_cs,), sent, win.dtype)
    out[..., 0] = win
    out[..., 1:max(c_zero_to, 1)] = 0
    return out


def gather_starts(B, starts=GATHER_STARTS):
    return [starts[i % len(starts)] for i in range(B)]


def gather_rows(B):
    """B rows over the three spectrograms of ROWS_T, neighbours always on different ones: [(spectrogram, start)]"""
    return [(i % 3, ROWS_STARTS[i % 3][(i // 3) % len(ROWS_STARTS[i % 3])]) for i in range(B)]


# ---------------------------------------------------------------- the resampler
# (orig_sr, n_in) -> (resampy's n_out = int(n_in * ratio), librosa's fixed length = ceil(n_in * ratio)), target 16 kHz
RESAMPLE_CASES = {
    (8000, 1): (2, 2), (8000, 2): (4, 4), (8000, 3): (6, 6), (4000, 1): (4, 4), (48000, 3): (1, 1), (48000, 4): (1, 2),
    (32000, 2): (1, 1), (15999, 1): (1, 2), (16001, 2): (1, 2),
    (8000, 64): (128, 128), (48000, 384): (128, 128), (48000, 387): (129, 129),      # n_out around the 128-thread block
    (8192000, 1100): (2, 3),                                                          # ratio 1 / 512: index_step == 1
}


def resample_input(orig_sr, n):
    return _noise(n, 0.3, orig_sr % 97 + n)


def resample_index_step(orig_sr, num_table=512):
    ratio = 16000.0 / orig_sr
    return int(min(1.0, ratio) * num_table)


# ---------------------------------------------------------------- w2l_bn_fold
BN_C = (1, 255, 256, 257, 1000)
BN_PATTERNS = ("all", "no_bn", "no_bias", "none")
BN_EPS = float(F32(1e-5))
BN_VAR_EDGES = (0.0, 1e-12, 1e10, 1e30)


def bn_inputs(C, seed):
    """bias, gamma, beta, mean, var (fp32): var starts with 0, 1e-12 (both far under eps), 1e10 and 1e30 as far as C allows;
    gamma has both signs and, from C = 255 on, a zero"""
    rng = np.random.default_rng(seed)
    bias, gamma, beta, mean = (rng.standard_normal(C).astype(F32) for _ in range(4))
    var = rng.uniform(0.01, 4.0, C).astype(F32)
    k = min(C, len(BN_VAR_EDGES))
    var[:k] = BN_VAR_EDGES[:k]
    if C > 8:
        gamma[7] = 0.0
    return bias, gamma, beta, mean, var


def bn_ref(pattern, bias, gamma, beta, mean, var):
    """-> (scale, shift, t * scale) in float64 for a NULL pattern"""
    C = len(var)
    bn = pattern in ("all", "no_bias")
    has_bias = pattern in ("all", "no_bn")
    g, b, mu = (t.astype(np.float64) if bn else np.full(C, c) for t, c in ((gamma, 1.0), (beta, 0.0), (mean, 0.0)))
    inv = 1.0 / np.sqrt(var.astype(np.float64) + BN_EPS) if bn else np.ones(C)
    scale = g * inv
    t = (bias.astype(np.float64) if has_bias else np.zeros(C)) - mu
    return scale, t * scale + b, t * scale


def bn_bounds(pattern, scale, shift, ts):
    if pattern in ("no_bn", "none"):
        return np.zeros_like(scale), np.zeros_like(shift)
    return 4 * U * np.abs(scale), 6 * U * np.abs(ts) + U * np.abs(shift)


# ---------------------------------------------------------------- w2l_lse_score_segments: the NaN order
LSE_C, LSE_VSHIFT = 70, 2
LSE_NAN_N = (1, 6)
LSE_PDIST_TOL = 1e-5     # two fp32 sums of 70 squares (<= 4 in all) in different orders, one root: 70 u * 4 / (2 * 1) and change


def lse_nan_inputs(n):
    """unit rows f1, f2 [n, 70]; one NaN in f2, in row 0 (n = 1) or row 3"""
    rng = np.random.default_rng(40 + n)
    f1, f2 = (rng.standard_normal((n, LSE_C)) for _ in range(2))
    f1, f2 = ((f / np.linalg.norm(f, axis=1, keepdims=True)).astype(F32) for f in (f1, f2))
    f2[0 if n == 1 else 3, 5] = np.nan
    return f1, f2
