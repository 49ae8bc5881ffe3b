"""tests/_audio_cases.py without a GPU: the tables are pinned, the conditions on the inputs hold against the float64 reference
(not against code under test), the CPU oracle lies inside the mel bound at every element of every case - the bound is reachable
by a correct fp32 implementation - while an fp32 DFT leaves it, the resampler's lengths are the oracle's, and the NaN
expectations of the LSE scores are what oracle/lse_ref.py returns."""
import numpy as np
import pytest
import torch

import _audio_cases as ac
from _audio_cases import F32
from oracle import audio_ref, lse_ref, resample_ref


# ---------------------------------------------------------------- the table
def test_the_case_table_is_pinned():
    c = ac.mel_cases()
    assert list(c) == (["noise%d" % n for n in (401, 599, 600, 601, 799, 800, 801, 1000, 16123)] +
                       ["impulse%d" % k for k in (0, 1, 399, 400, 401, 998, 999)] + ["dc", "sine440", "sine450", "tone_noise", "ramp", "loud", "quiet"])
    assert all(w.dtype == np.float32 and w.ndim == 1 and len(w) > 400 and not w.flags.writeable for w in c.values())
    assert [len(c[k]) for k in ("dc", "sine440", "sine450", "tone_noise", "ramp", "loud", "quiet")] == [1000, 4000, 4000, 4000, 6000, 3000, 3000]
    for k in ac.MEL_IMPULSES:
        w = c["impulse%d" % k]
        assert len(w) == 1000 and w[k] == 1 and np.count_nonzero(w) == 1
    assert (c["dc"] == 1).all()
    assert 0.09 < c["noise16123"].std() < 0.11 and 2700 < c["loud"].std() < 3300 and 2.7e-5 < c["quiet"].std() < 3.3e-5
    # the frame count on both sides of 1 + N // 200, the tail reflection in one, two and three frames
    assert [1 + n // 200 for n in ac.MEL_NOISE_LENGTHS] == [3, 3, 4, 4, 4, 5, 5, 6, 81]
    assert ac.GATHER_STARTS == (-2 ** 30, -17, -16, -15, -1, 0, 21, 22, 36, 37, 38, 2 ** 30) and ac.GATHER_T == 37
    assert ac.GATHER_T16_STARTS == (-1, 0, 1)
    assert ac.GATHER_STRIDES_F32 == ((1, 1), (4, 4), (4, 1), (8, 4), (4, 0))
    assert ac.GATHER_STRIDES_BF16 == ((8, 8), (8, 1), (16, 8), (8, 0))
    assert all(abs(s) + 15 < 2 ** 31 for st in ac.ROWS_STARTS for s in st)
    # the grid of the gather caps at 4096 blocks of 256 items: 820 rows is the first count whose last row takes a second trip
    assert 819 * 80 * 16 <= ac.GATHER_GRID_ITEMS < ac.GATHER_B_SECOND_TRIP * 80 * 16
    assert ac.BN_C == (1, 255, 256, 257, 1000) and ac.LOCALITY_K == (0, 1, 400, 1000, 1998, 1999) and ac.LOCALITY_N == 2000
    assert ac.STREAM_LENGTHS == (401, 600, 801, 1000) and [ac.open_stream_columns(n) for n in ac.STREAM_LENGTHS] == [1, 2, 3, 4]
    assert [1 + n // 200 for n in ac.STREAM_LENGTHS] == [3, 4, 5, 6]


def test_the_basis_and_window_are_the_oracles():
    assert np.array_equal(ac.basis(), audio_ref.mel_basis())
    assert np.abs(ac.hann() - audio_ref.hann_window()).max() < 1e-15
    taps = ac.mel_taps()
    assert taps.min() >= 1 and taps.max() <= 40 and int(taps.sum()) == int((audio_ref.mel_basis() != 0).sum())
    print("non-zero taps per filter: %d .. %d" % (taps.min(), taps.max()))


# ---------------------------------------------------------------- the mel bound
@pytest.mark.parametrize("name", list(ac.mel_cases()))
def test_the_oracle_is_inside_the_mel_bound_everywhere(name):
    wav = ac.mel_cases()[name]
    v, M, bound = ac.mel_reference(name)
    got = audio_ref.melspectrogram(wav)
    assert got.shape == v.shape == (80, 1 + len(wav) // 200) and got.dtype == np.float32
    assert np.isfinite(bound).all() and (bound > 0).all() and bound.max() < ac.MEL_BOUND_CEILING, bound.max()
    err = np.abs(got.astype(np.float64) - v)
    print("%s: oracle max |error| %.3e, max error / bound %.3f, bound %.2e .. %.2e" % (name, err.max(), (err / bound).max(),
                                                                                       bound.min(), bound.max()))
    assert (err <= bound).all(), (name, float((err / bound).max()))


def _mel_with_fp32_dft_accumulators(wav):
    """the kernel's steps with the two DFT accumulators held in fp32: float64 frame, twiddles and products, the running sums
    rounded to fp32 after every term"""
    y = audio_ref.preemphasis(wav)
    frames = ac.hann()[None, :] * y[ac.reflect_index(len(wav))]                               # [T, 800] float64
    k = np.arange(ac.BINS)
    acc = np.zeros((ac.BINS, frames.shape[0]), np.complex64)
    for n in range(ac.N_FFT):
        acc = (acc + np.exp(-2j * np.pi * (k * n % ac.N_FFT) / ac.N_FFT)[:, None] * frames[None, :, n]).astype(np.complex64)
    Mf = ac.basis() @ np.abs(acc)                                                             # fp32
    return np.clip(8 * ((20 * np.log10(np.maximum(F32(1e-5), Mf)) - 20 + 100) / 100) - 4, -4, 4)


@pytest.mark.parametrize("name,leaves", [("sine450", True), ("tone_noise", True), ("sine440", False), ("noise1000", False)])
def test_an_fp32_dft_leaves_the_mel_bound(name, leaves):
    """what a tolerance of 1e-4 let pass.  The two signals between bins take an fp32 accumulator 20 and 100 bounds away from float64;
    on white noise and on the sine that sits on a bin its error is a fraction of the bound, which is why those two signals are
    in the table"""
    v, M, bound = ac.mel_reference(name)
    err = np.abs(_mel_with_fp32_dft_accumulators(ac.mel_cases()[name]).astype(np.float64) - v)
    print("fp32 DFT accumulators, %s: max |error| %.3e, max error / bound %.1f" % (name, err.max(), (err / bound).max()))
    assert err.max() < 1e-3 and ((err / bound).max() > 5) == leaves


def test_the_mel_inputs_reach_the_interior_and_both_clips():
    inside = low = high = total = 0
    smallest = np.inf
    for name in ac.mel_cases():
        v, M, _ = ac.mel_reference(name)
        i = (v > -4) & (v < 4)
        inside, low, high, total = inside + int(i.sum()), low + int((v == -4).sum()), high + int((v == 4).sum()), total + v.size
        if i.any():
            smallest = min(smallest, float(M[i].min()))
    print("interior %.1f %%, clipped low %.1f %%, high %.1f %%, smallest unclipped M %.2e" % (
        100. * inside / total, 100. * low / total, 100. * high / total, smallest))
    assert inside >= 0.10 * total and low >= 1 and high >= 1 and smallest < 2e-4
    v, M, _ = ac.mel_reference("ramp")                                       # the one signal that reaches all three
    assert (v == -4).any() and (v == 4).any() and ((v > -4) & (v < 4)).mean() > 0.3
    assert (ac.mel_reference("loud")[0] == 4).mean() > 0.5 and (ac.mel_reference("quiet")[0] == -4).all()
    assert ac.mel_reference("sine440")[1].min() < 1e-3                      # far bins approach the lower clip


@pytest.mark.parametrize("k", ac.LOCALITY_K)
def test_locality_columns_follow_the_reflect_rule(k):
    """the index arithmetic against the float64 reference: every column that changes is in the set; the set is the columns whose
    padded window [200 t - 400, 200 t + 400) holds k, k + 1 or one of their mirror images"""
    N = ac.LOCALITY_N
    cols = ac.locality_columns(N, k)
    wav = ac.locality_wav()
    w2 = wav.copy()
    w2[k] = wav[k] + F32(0.25)
    changed = np.flatnonzero((ac.mel_f64(wav)[1] != ac.mel_f64(w2)[1]).any(0))
    assert len(changed) >= 1 and set(changed) <= set(cols) and len(cols) < 1 + N // 200
    brute = set()
    for t in range(1 + N // 200):
        for p in range(200 * t - 400, 200 * t + 400):
            j = -p if p < 0 else (2 * (N - 1) - p if p >= N else p)
            if j == k or (j == k + 1):
                brute.add(t)
    assert set(cols) == brute
    assert {0: [0, 1, 2], 1999: [8, 9, 10]}.get(k, list(cols)) == list(cols)


# ---------------------------------------------------------------- the gather
def test_gather_reference_and_bf16_rounding():
    mel = ac.gather_mel(ac.GATHER_T, 1)
    bits = mel.view(np.uint32)
    assert mel.dtype == np.float32 and (np.abs(mel) <= 4).all()
    assert (mel == 4).sum() >= 2 and (mel == -4).sum() >= 2 and (bits == 0x80000000).any() and (bits == 0).any()
    ties = (bits & 0xFFFF) == 0x8000
    assert ties.sum() >= 30 and (bits[ties] & 0x10000 != 0).any() and (bits[ties] & 0x10000 == 0).any()
    assert ties[:, 0].any() and ties[:, -1].any()
    want = torch.from_numpy(mel).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(ac.bf16_bits(mel), want)                           # torch's cast is the rounding the kernel must do
    up = ac.bf16_bits(mel)[ties].astype(np.uint32) << 16
    assert (up > bits[ties]).any() and (up < bits[ties]).any()               # ties go both ways
    w = ac.gather_windows(mel, ac.GATHER_STARTS)
    assert w.shape == (12, 80, 16)
    for b, s in enumerate(ac.GATHER_STARTS):
        for j in range(16):
            col = mel[:, s + j] if 0 <= s + j < ac.GATHER_T else np.zeros(80, F32)
            assert np.array_equal(w[b, :, j].view(np.uint32), col.view(np.uint32))
    assert not w[0].any() and not w[-1].any() and not w[1].any() and not w[2].any()          # -2**30, 2**30, -17, -16
    assert w[3][:, 15].any() and not w[3][:, :15].any()                                       # -15: column 0 in the last slot
    assert w[8][:, 0].any() and not w[8][:, 1:].any() and not w[9].any()
    e = ac.gather_expect(w, 8, 4, F32(ac.SENT))
    assert np.array_equal(e[..., 0], w) and not e[..., 1:4].any() and (e[..., 4:] == ac.SENT).all()
    e = ac.gather_expect(w, 4, 0, F32(ac.SENT))
    assert (e[..., 1:] == ac.SENT).all()
    assert float(torch.tensor(ac.SENT).to(torch.bfloat16)) == ac.SENT
    rows = ac.gather_rows(45)
    assert all(rows[i][0] != rows[i + 1][0] for i in range(44)) and {r[0] for r in rows} == {0, 1, 2}
    assert {s for c, s in rows if c == 1} == set(ac.GATHER_T16_STARTS) and {s for c, s in rows if c == 0} == set(ac.GATHER_STARTS)


# ---------------------------------------------------------------- the resampler
@pytest.mark.parametrize("orig_sr,n", list(ac.RESAMPLE_CASES))
def test_resample_lengths_are_the_oracles(orig_sr, n):
    n_out, fixed = ac.RESAMPLE_CASES[(orig_sr, n)]
    x = ac.resample_input(orig_sr, n)
    assert x.shape == (n,) and x.dtype == np.float32 and x.any()
    assert resample_ref.resampy_resample(x, orig_sr, 16000).shape == (n_out,)
    y = resample_ref.librosa_resample(x, orig_sr, 16000)
    assert y.shape == (fixed,) and y.dtype == np.float32 and np.isfinite(y).all() and y[:n_out].any()


def test_resample_table_reaches_its_edges():
    outs = sorted(v[0] for v in ac.RESAMPLE_CASES.values())
    assert 127 < outs[-3] == 128 == outs[-2] < outs[-1] == 129                # both sides of the 128-thread block
    assert ac.resample_index_step(8192000) == 1 and ac.resample_index_step(16384000) == 0
    assert min(n for _, n in ac.RESAMPLE_CASES) == 1 and sum(n <= 4 for _, n in ac.RESAMPLE_CASES) == 9


# ---------------------------------------------------------------- bn_fold
@pytest.mark.parametrize("C", ac.BN_C)
def test_bn_fold_bounds_hold_for_an_fp32_restatement(C):
    bias, gamma, beta, mean, var = ac.bn_inputs(C, C)
    assert var[0] == 0 and (C < 4 or (var[1] == F32(1e-12) and var[2] == F32(1e10) and var[3] == F32(1e30)))
    assert C < 9 or ((gamma < 0).any() and (gamma > 0).any() and gamma[7] == 0)
    for pattern in ac.BN_PATTERNS:
        scale, shift, ts = ac.bn_ref(pattern, bias, gamma, beta, mean, var)
        bs, bsh = ac.bn_bounds(pattern, scale, shift, ts)
        assert np.isfinite(scale).all() and np.isfinite(shift).all()
        bn, has_bias = pattern in ("all", "no_bias"), pattern in ("all", "no_bn")
        one, zero = np.ones(C, F32), np.zeros(C, F32)
        inv = one / np.sqrt(var + F32(ac.BN_EPS)) if bn else one
        s32 = (gamma if bn else one) * inv
        sh32 = ((bias if has_bias else zero) - (mean if bn else zero)) * s32 + (beta if bn else zero)
        assert s32.dtype == sh32.dtype == np.float32
        assert (np.abs(s32 - scale) <= bs).all() and (np.abs(sh32 - shift) <= bsh).all(), pattern
        if not bn:
            assert (scale == 1).all() and np.array_equal(shift, bias.astype(np.float64) if has_bias else np.zeros(C))
    # without + eps the var = 0 channel is not finite: the case the bound exists for
    with np.errstate(divide="ignore"):
        assert not np.isfinite(F32(1) / np.sqrt(var[:1]))[0]


# ---------------------------------------------------------------- the LSE scores' NaN order
@pytest.mark.parametrize("n", ac.LSE_NAN_N)
def test_the_nan_expectations_come_from_lse_ref(n):
    f1, f2 = ac.lse_nan_inputs(n)
    assert f1.shape == f2.shape == (n, ac.LSE_C) and int(np.isnan(f2).sum()) == 1 and not np.isnan(f1).any()
    offset, conf, minval, mdist = lse_ref.scores(torch.from_numpy(f1), torch.from_numpy(f2), vshift=ac.LSE_VSHIFT)
    nan = np.isnan(mdist.numpy())
    assert mdist.shape == (5,) and np.isnan(conf) and np.isnan(minval)
    if n == 1:
        assert nan.tolist() == [False, False, True, False, False] and offset == 0     # the minimum is the NaN, at its index
    else:
        assert nan.all() and offset == ac.LSE_VSHIFT                                   # all NaN: the first one, index 0
