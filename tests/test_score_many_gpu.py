"""Filelist scoring on the device: w2l_sync_window_rows bit for bit against the numpy expression of oracle/lse_ref.py,
w2l_lse_score_segments bit for bit against w2l_shifted_pdist per segment plus a numpy restatement of the reduction,
`evaluation.lse_many` against a replay of its own batches and against `lse_like` per clip, and
`python -m wav2lip_amd.calculate_scores` on three synthetic AVIs."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from oracle import lse_ref
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu


def _sync_state_dict():
    from wav2lip_amd import models
    return synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.SyncNet_color().state_dict().items()}, seed=2)


def _syncnet(cuda):
    from wav2lip_amd import models
    S = models.SyncNet_color()
    S.load_state_dict(_sync_state_dict())
    return S.to(cuda).eval()


def _ulps(a, b):
    """distance in units in the last place between two float32 arrays of non-negative values"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---------------------------------------------------------------- w2l_sync_window_rows
@pytest.mark.parametrize("shift", [0, 1])
def test_window_rows_kernel_is_the_numpy_expression_bit_for_bit(cuda, shift):
    """three rows drawn from two clips (T = 6 and 9, mel lengths 16 and 37; starts 0, 0 and 21, the last legal ones of both) into
    NaN-filled buffers.  shift = 1 puts the frames on an odd address: the kernel's byte path"""
    from wav2lip_amd import _lib, evaluation
    from wav2lip_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    r = np.random.default_rng(5)
    clips_np = [r.integers(0, 256, (T, 96, 96, 3), dtype=np.uint8) for T in (6, 9)]
    mels_np = [r.uniform(-4, 4, (80, Tm)).astype(np.float32) for Tm in (16, 37)]
    store = [torch.zeros(c.size + 16, dtype=torch.uint8, device=cuda) for c in clips_np]
    clips = []
    for s, c in zip(store, clips_np):
        s[shift:shift + c.size] = torch.from_numpy(c.reshape(-1)).to(cuda)
        clips.append(s[shift:shift + c.size].view(c.shape))
        assert clips[-1].data_ptr() % 4 == shift
    mels = [torch.from_numpy(m).to(cuda) for m in mels_np]
    rows = [(0, 1, 0), (1, 0, 0), (1, 4, 21)]                                  # (clip, first frame, first mel column)
    table = np.zeros(len(rows), evaluation.SYNC_ROW)
    for k, (c, v, s) in enumerate(rows):
        table[k] = (clips[c].data_ptr() + v * 96 * 96 * 3, mels[c].data_ptr(), mels[c].shape[1], s, (0, 0))
    table_dev = torch.from_numpy(table.view(np.uint8)).to(cuda)
    face_in = torch.full((len(rows), 48, 96, 16), float("nan"), device=cuda)
    mel_in = torch.full((len(rows), 80, 16, 4), float("nan"), device=cuda)
    check(lib.w2l_sync_window_rows(current_stream(), len(rows), ptr(table_dev), 96, ptr(face_in), 16, ptr(mel_in), 4), "sync_window_rows")
    got_f, got_m = face_in.cpu().numpy(), mel_in.cpu().numpy()
    for k, (c, v, s) in enumerate(rows):
        x = clips_np[c][v:v + 5, 48:].astype(np.float32) / np.float32(255.)   # [5,48,96,3], oracle/lse_ref.py's expression
        want = np.zeros((48, 96, 16), np.float32)
        want[:, :, :15] = x.transpose(1, 2, 0, 3).reshape(48, 96, 15)          # channel 3*t + c
        assert np.array_equal(got_f[k], want), (k, float(np.nanmax(np.abs(got_f[k] - want))))
        wm = np.zeros((80, 16, 4), np.float32)
        wm[:, :, 0] = mels_np[c][:, s:s + 16]
        assert np.array_equal(got_m[k], wm), k
    # the existing device path (torch's division, then the layout kernel): within 1 ulp
    faces_t, mels_t = evaluation.sync_windows(clips[1], mels[1], 25.)
    assert faces_t.shape[0] == 5
    old_f = torch.full((5, 48, 96, 16), float("nan"), device=cuda)
    old_m = torch.full((5, 80, 16, 4), float("nan"), device=cuda)
    check(lib.w2l_nchw_to_nhwc(current_stream(), 5, 15, 48, 96, ptr(faces_t), ptr(old_f), 16, 16), "nchw_to_nhwc")
    check(lib.w2l_nchw_to_nhwc(current_stream(), 5, 1, 80, 16, ptr(mels_t), ptr(old_m), 4, 4), "nchw_to_nhwc")
    old_f, old_m = old_f.cpu().numpy(), old_m.cpu().numpy()
    worst = max(int(_ulps(got_f[1], old_f[0]).max()), int(_ulps(got_f[2], old_f[4]).max()))
    print("sync_windows path vs the row kernel: at most %d ulp" % worst)
    assert worst <= 1
    assert np.array_equal(got_m[1], old_m[0])                                  # window 0 starts at column 0 there too


def test_window_rows_kernel_reads_columns_outside_the_spectrogram_as_zero_and_reports_argument_errors(cuda):
    from wav2lip_amd import _lib, evaluation
    from wav2lip_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    frames = torch.from_numpy(synth.face_crops_u8(5, seed=3)).to(cuda)
    mel = torch.arange(80 * 20, dtype=torch.float32, device=cuda).reshape(80, 20) + 1
    table = np.zeros(2, evaluation.SYNC_ROW)
    table[0] = (frames.data_ptr(), mel.data_ptr(), 20, -3, (0, 0))
    table[1] = (frames.data_ptr(), mel.data_ptr(), 20, 10, (0, 0))
    table_dev = torch.from_numpy(table.view(np.uint8)).to(cuda)
    face_in = torch.full((2, 48, 96, 20), float("nan"), device=cuda)           # a wider channel stride: channels 15..19 zeroed
    mel_in = torch.full((2, 80, 16, 8), float("nan"), device=cuda)
    check(lib.w2l_sync_window_rows(current_stream(), 2, ptr(table_dev), 96, ptr(face_in), 20, ptr(mel_in), 8), "sync_window_rows")
    m = mel_in.cpu().numpy()
    want = np.zeros((2, 80, 16), np.float32)
    want[0, :, 3:] = mel.cpu().numpy()[:, :13]
    want[1, :, :10] = mel.cpu().numpy()[:, 10:]
    assert np.array_equal(m[..., 0], want) and not m[..., 1:].any()
    f = face_in.cpu().numpy()
    assert not f[..., 15:].any() and np.array_equal(f[0], f[1]) and not np.isnan(f).any()
    s = current_stream()
    assert lib.w2l_sync_window_rows(s, 0, ptr(table_dev), 96, ptr(face_in), 20, ptr(mel_in), 8) != 0
    assert lib.w2l_sync_window_rows(s, 2, None, 96, ptr(face_in), 20, ptr(mel_in), 8) != 0
    assert lib.w2l_sync_window_rows(s, 2, ptr(table_dev), 96, ptr(face_in), 15, ptr(mel_in), 8) != 0
    assert lib.w2l_sync_window_rows(s, 2, ptr(table_dev), 96, ptr(face_in), 20, ptr(mel_in), 3) != 0
    big = torch.zeros(128, dtype=torch.uint8, device=cuda)
    assert lib.w2l_sync_window_rows(s, 1, ptr(big[8:]), 96, ptr(face_in), 20, ptr(mel_in), 8) != 0
    assert b"16-byte" in lib.w2l_last_error()


# ---------------------------------------------------------------- w2l_lse_score_segments
def _restate(mdist, vshift, n):
    """(min, conf, offset, n) of one mdist row in numpy: stable sort, rank (win-1)/2, first argmin; fp32 arithmetic"""
    order = np.argsort(mdist, kind="stable")
    amin = int(np.argmin(mdist))
    assert order[0] == amin
    med = mdist[order[(len(mdist) - 1) // 2]]
    return np.array([mdist[amin], np.float32(med - mdist[amin]), np.float32(vshift - amin), np.float32(n)], np.float32)


def _score(lib, cuda, segs, C, vshift, f1, f2, fill=float("nan")):
    from wav2lip_amd import evaluation
    from wav2lip_amd._lib import check, current_stream, ptr
    win = 2 * vshift + 1
    t = np.zeros(len(segs), evaluation.LSE_SEGMENT)
    for k, s in enumerate(segs):
        t[k] = s
    t_dev = torch.from_numpy(t.view(np.uint8)).to(cuda)
    mdist = torch.full((len(segs), win), fill, device=cuda)
    scores = torch.full((len(segs), 4), fill, device=cuda)
    check(lib.w2l_lse_score_segments(current_stream(), len(segs), ptr(t_dev), C, vshift, ptr(f1), ptr(f2), ptr(mdist), ptr(scores)),
          "lse_score_segments")
    return mdist.cpu().numpy(), scores.cpu().numpy()


def _pdist_alone(lib, cuda, f1, f2, vshift):
    from wav2lip_amd._lib import check, current_stream, ptr
    a, b = f1.clone().contiguous(), f2.clone().contiguous()
    d = torch.empty((a.shape[0], 2 * vshift + 1), device=cuda)
    check(lib.w2l_shifted_pdist(current_stream(), a.shape[0], a.shape[1], vshift, ptr(a), ptr(b), ptr(d)), "shifted_pdist")
    return d.cpu().numpy()


def _fenced_segments_equal_pdist_and_numpy(cuda, C, vshift, lengths):
    """segments side by side, fenced by rows of large distinct values: one read across a boundary changes a distance by hundreds.
    Unit rows keep every distance in [2**-16, 4), so with n < 2**12 the fp64 sum of a column is exact in any order, and the mean
    is one correctly rounded division: bit-equality is the right bar."""
    from wav2lip_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 * vshift + C)
    total = sum(lengths) + 2 * (len(lengths) + 1)
    f1 = 1e3 + torch.arange(total * C, dtype=torch.float32).reshape(total, C)          # the fences (and everything else, for now)
    f2 = -2e3 - torch.arange(total * C, dtype=torch.float32).reshape(total, C)
    segs, row = [], 2
    for n in lengths:
        for f in (f1, f2):
            f[row:row + n] = torch.nn.functional.normalize(torch.randn(n, C, generator=g), dim=1)
        segs.append((row, n))
        row += n + 2
    f1, f2 = f1.to(cuda), f2.to(cuda)
    mdist, scores = _score(lib, cuda, segs, C, vshift, f1, f2)
    for k, (row0, n) in enumerate(segs):
        d = _pdist_alone(lib, cuda, f1[row0:row0 + n], f2[row0:row0 + n], vshift)
        assert d.min() >= 2.0 ** -16 and d.max() < 4 and n < 2 ** 12                   # the precondition for exactness
        want = d.astype(np.float64).mean(0).astype(np.float32)
        assert np.array_equal(mdist[k], want), (k, n, float(np.abs(mdist[k] - want).max()))
        assert np.array_equal(scores[k], _restate(want, vshift, n)), (k, n, scores[k], _restate(want, vshift, n))


@pytest.mark.parametrize("C", [512, 7])
@pytest.mark.parametrize("vshift", [0, 3, 15])
def test_score_segments_equals_pdist_per_segment_and_a_numpy_reduction(cuda, C, vshift):
    """segments of 1, 2, vshift+1 and 40 rows (_fenced_segments_equal_pdist_and_numpy)"""
    _fenced_segments_equal_pdist_and_numpy(cuda, C, vshift, [1, 2, vshift + 1, 40])


@pytest.mark.parametrize("C", [512, 7])
@pytest.mark.parametrize("vshift", [0, 3])
def test_score_segments_at_the_sixteen_wave_round_boundary(cuda, C, vshift):
    """16, 17, 32 and 33 rows: the kernel takes the rows sixteen at a time, one wave each - a full round, a round and one row,
    two full rounds, two and one row"""
    _fenced_segments_equal_pdist_and_numpy(cuda, C, vshift, [16, 17, 32, 33])


@pytest.mark.parametrize("n", [1, 6])
def test_score_segments_orders_nan_as_the_reference_does(cuda, n):
    """one NaN in f2 (tests/_audio_cases.py; tests/test_audio_cases_cpu.py pins what oracle/lse_ref.py makes of it): with n = 1 and
    vshift = 2 exactly one of the five mean distances is NaN, the minimum is that NaN, at its index, and the confidence is NaN;
    with n = 6 every entry is NaN and the offset is that of index 0"""
    import _audio_cases as ac
    from wav2lip_amd import _lib
    lib = _lib.load()
    f1, f2 = (torch.from_numpy(f) for f in ac.lse_nan_inputs(n))
    off, conf, minval, ref = lse_ref.scores(f1, f2, vshift=ac.LSE_VSHIFT)
    ref = ref.numpy()
    assert np.isnan(conf) and np.isnan(minval) and int(np.isnan(ref).sum()) == (1 if n == 1 else 5)
    mdist, scores = _score(lib, cuda, [(0, n)], ac.LSE_C, ac.LSE_VSHIFT, f1.to(cuda), f2.to(cuda), fill=7.0)
    assert np.array_equal(np.isnan(mdist[0]), np.isnan(ref)), (mdist[0], ref)
    live = ~np.isnan(ref)
    assert (np.abs(mdist[0][live] - ref[live]) <= ac.LSE_PDIST_TOL).all()
    assert np.isnan(scores[0, 0]) and np.isnan(scores[0, 1]), scores[0]
    assert scores[0, 2] == off == (0 if n == 1 else ac.LSE_VSHIFT) and scores[0, 3] == n


def test_score_segments_writes_an_empty_segment_as_nan_and_reads_nothing_for_it(cuda):
    """a segment of no rows between two live ones, its row0 far behind both arenas: its mean distances are NaN, its scores
    (NaN, NaN, NaN, 0), and its neighbours' rows are the bits of a run without it"""
    from wav2lip_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(77)
    C, vshift = 70, 3
    f1 = torch.nn.functional.normalize(torch.randn(12, C, generator=g), dim=1).to(cuda)
    f2 = torch.nn.functional.normalize(torch.randn(12, C, generator=g), dim=1).to(cuda)
    mdist, scores = _score(lib, cuda, [(0, 5), (10 ** 6, 0), (5, 7)], C, vshift, f1, f2, fill=7.0)
    m2, s2 = _score(lib, cuda, [(0, 5), (5, 7)], C, vshift, f1, f2, fill=7.0)
    assert np.isnan(mdist[1]).all() and np.isnan(scores[1, :3]).all() and scores[1, 3] == 0
    assert not np.isnan(m2).any() and not np.isnan(s2).any() and not (m2 == 7.0).any()
    assert mdist[[0, 2]].tobytes() == m2.tobytes() and scores[[0, 2]].tobytes() == s2.tobytes()
    assert s2[:, 3].tolist() == [5.0, 7.0]


def test_score_segments_takes_the_lowest_index_among_equal_minima(cuda):
    """n = 1, vshift = 1, f1 = e, f2 = -e: offsets 0 and 2 both see a zero-padding row and tie for the minimum; offset 1 sees -e"""
    from wav2lip_amd import _lib
    lib = _lib.load()
    e = torch.zeros((1, 8), device=cuda)
    e[0, 3] = 1.
    mdist, scores = _score(lib, cuda, [(0, 1)], 8, 1, e, -e)
    assert mdist[0, 0] == mdist[0, 2] < mdist[0, 1]
    assert scores[0].tolist() == [float(mdist[0, 0]), 0.0, 1.0, 1.0]


def test_score_segments_agrees_with_the_reference_expressions(cuda):
    """oracle/lse_ref.py `scores` (calc_pdist + mean + min + median, torch CPU) on the same embeddings.  1e-4 is the derived worst case
    for two fp32 sums of 512 terms in different orders plus an fp32 mean of 64 values of at most 2"""
    from wav2lip_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(9)
    lengths = [1, 2, 16, 40, 64]
    f1 = torch.nn.functional.normalize(torch.randn(sum(lengths), 512, generator=g), dim=1)
    f2 = torch.nn.functional.normalize(torch.randn(sum(lengths), 512, generator=g), dim=1)
    segs, row = [], 0
    for n in lengths:
        segs.append((row, n))
        row += n
    for vshift in (3, 15):
        mdist, scores = _score(lib, cuda, segs, 512, vshift, f1.to(cuda), f2.to(cuda))
        for k, (row0, n) in enumerate(segs):
            off, conf, minval, ref = lse_ref.scores(f1[row0:row0 + n], f2[row0:row0 + n], vshift=vshift)
            err = max(float(np.abs(mdist[k] - ref.numpy()).max()), abs(float(scores[k, 0]) - minval), abs(float(scores[k, 1]) - conf))
            print("vshift %d n %d: largest difference %.2e" % (vshift, n, err))
            assert err <= 1e-4 and scores[k, 3] == n
            two = np.sort(ref.numpy())[:2]
            assert scores[k, 2] == off or two[1] - two[0] <= 2e-4                     # both sides within 1e-4 of the truth


def test_score_segments_refuses_bad_arguments_without_launching(cuda):
    from wav2lip_amd import _lib, evaluation
    from wav2lip_amd._lib import current_stream, ptr
    lib = _lib.load()
    f = torch.ones((4, 8), device=cuda)
    t = np.zeros(1, evaluation.LSE_SEGMENT)
    t[0] = (0, 4)
    t_dev = torch.from_numpy(t.view(np.uint8)).to(cuda)
    mdist = torch.full((1, 255), 7., device=cuda)
    scores = torch.full((1, 4), 7., device=cuda)
    s = current_stream()
    for n_seg, C, vshift in ((0, 8, 1), (-1, 8, 1), (1, 0, 1), (1, 8, -1), (1, 8, 128)):
        assert lib.w2l_lse_score_segments(s, n_seg, ptr(t_dev), C, vshift, ptr(f), ptr(f), ptr(mdist), ptr(scores)) != 0
        assert b"lse_score_segments" in lib.w2l_last_error()
    assert lib.w2l_lse_score_segments(s, 1, None, 8, 1, ptr(f), ptr(f), ptr(mdist), ptr(scores)) != 0
    assert lib.w2l_lse_score_segments(s, 1, ptr(t_dev), 8, 1, ptr(f), None, ptr(mdist), ptr(scores)) != 0
    torch.cuda.synchronize()
    assert bool((mdist == 7).all()) and bool((scores == 7).all())                   # nothing ran
    assert lib.w2l_lse_score_segments(s, 1, ptr(t_dev), 8, 127, ptr(f), ptr(f), ptr(mdist), ptr(scores)) == 0      # win = 255 fits
    assert float(scores[0, 3]) == 4


# ---------------------------------------------------------------- evaluation.lse_many
VSHIFT = 3
LENGTHS = (5, 9, 12, 23, 4)          # frames; windows 1, 5, 8, 19 and none


@pytest.fixture(scope="module")
def many(cuda):
    """five clips through lse_many three times on one fresh model (device faces with the batches recorded, the same again, host
    faces), then `lse_like` per clip on a model of its own"""
    from wav2lip_amd import evaluation
    from wav2lip_amd.models import syncnet
    r = np.random.default_rng(17)
    faces = [r.integers(0, 256, (T, 96, 96, 3), dtype=np.uint8) for T in LENGTHS]
    mels = [torch.from_numpy(r.uniform(-4, 4, (80, 16 + int(3.2 * T))).astype(np.float32)).to(cuda) for T in LENGTHS]
    faces_dev = [torch.from_numpy(f).to(cuda) for f in faces]
    S = _syncnet(cuda)
    built, batches = [], []
    real_graph, real_embed = syncnet._SyncGraph, S.embed_rows

    def counting_graph(*a, **k):
        assert (a[5:] + (k.get("precision", "f32"),))[0] == "f32"                 # this module scores in fp32 only
        built.append(a[1:4])
        return real_graph(*a, **k)

    def recording_embed(rows, B, audio_out, face_out, offset=0):
        batches.append((rows.clone(), B, offset, tuple(audio_out.shape)))
        return real_embed(rows, B, audio_out, face_out, offset)

    def jobs(fs):
        return (evaluation.ScoreJob("clip%d" % i, f, m) for i, (f, m) in enumerate(zip(fs, mels)))

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(syncnet, "_SyncGraph", counting_graph)
        mp.setattr(S, "embed_rows", recording_embed, raising=False)
        first = evaluation.lse_many(S, jobs(faces_dev), vshift=VSHIFT, batch_size=8)
        mp.undo()
        mp.setattr(syncnet, "_SyncGraph", counting_graph)
        again = evaluation.lse_many(S, jobs(faces_dev), vshift=VSHIFT, batch_size=8)
        host = evaluation.lse_many(S, jobs(faces), vshift=VSHIFT, batch_size=8)
    L = _syncnet(cuda)
    per_clip = [evaluation.lse_like(L, f, m, vshift=VSHIFT) for f, m in list(zip(faces_dev, mels))[:-1]]
    return dict(S=S, faces_dev=faces_dev, mels=mels, built=built, batches=batches, first=first, again=again, host=host,
                per_clip=per_clip)


def _same_bytes(a, b):
    assert [r["key"] for r in a] == [r["key"] for r in b]
    for x, y in zip(a, b):
        assert (x["n"], x["offset"]) == (y["n"], y["offset"])
        if x["n"]:
            assert np.float32(x["lse_c"]).tobytes() == np.float32(y["lse_c"]).tobytes()
            assert np.float32(x["lse_d"]).tobytes() == np.float32(y["lse_d"]).tobytes()
            assert x["mdist"].tobytes() == y["mdist"].tobytes()


def test_lse_many_builds_one_graph_and_repeats_itself(cuda, many):
    assert many["built"] == [(8, 48, 96)]                                       # three runs, one _SyncGraph
    assert [r["key"] for r in many["first"]] == ["clip%d" % i for i in range(5)]
    assert [r["n"] for r in many["first"]] == [1, 5, 8, 19, 0]
    last = many["first"][-1]
    assert last["offset"] is None and last["lse_c"] is None and last["lse_d"] is None and last["mdist"] is None
    assert [(b[1], b[2], b[3]) for b in many["batches"]] == [(8, lo, (40, 512)) for lo in range(0, 40, 8)]
    _same_bytes(many["first"], many["again"])
    _same_bytes(many["first"], many["host"])


def test_lse_many_equals_a_replay_of_its_batches_bit_for_bit(cuda, many):
    """the recorded row tables through embed_rows again, then w2l_shifted_pdist per clip and the numpy restatement"""
    from wav2lip_amd import _lib
    lib = _lib.load()
    S = many["S"]
    a = torch.full((40, 512), float("nan"), device=cuda)
    v = torch.full((40, 512), float("nan"), device=cuda)
    for rows, B, offset, _ in many["batches"]:
        S.embed_rows(rows, B, a, v, offset)
    row0 = 0
    for res in many["first"][:-1]:
        n = res["n"]
        d = _pdist_alone(lib, cuda, v[row0:row0 + n], a[row0:row0 + n], VSHIFT)
        mdist = d.astype(np.float64).mean(0).astype(np.float32)
        want = _restate(mdist, VSHIFT, n)
        assert res["mdist"].tobytes() == mdist.tobytes(), res["key"]
        assert (np.float32(res["lse_d"]), np.float32(res["lse_c"]), res["offset"], n) == (want[0], want[1], int(want[2]), int(want[3]))
        row0 += n
    assert row0 == 33


def test_lse_many_agrees_with_lse_like_per_clip(cuda, many):
    """the bars of test_lse_like_scores_match_the_cpu_scoring for the same quantities"""
    worst = 0.
    for got, ref in zip(many["first"], many["per_clip"]):
        assert got["n"] == ref["n"]
        two = np.sort(ref["mdist"])[:2]
        assert got["offset"] == ref["offset"] or two[1] - two[0] <= 2e-3
        err = max(abs(got["lse_d"] - ref["lse_d"]), abs(got["lse_c"] - ref["lse_c"]))
        worst = max(worst, err)
        assert err <= 1e-3, (got["key"], err)
    print("lse_many vs lse_like: largest difference of lse_d / lse_c %.3e" % worst)


def test_embed_rows_is_an_inference_path_with_checked_arguments(cuda, many):
    S, (rows, B, offset, _) = many["S"], many["batches"][0]
    a = torch.empty((8, 512), device=cuda)
    v = torch.empty((8, 512), device=cuda)
    with pytest.raises(ValueError):
        S.embed_rows(rows, B, a, v, 1)                                           # rows 1..9 of 8
    with pytest.raises(ValueError):
        S.embed_rows(rows, B, a, v.double(), 0)
    with pytest.raises(ValueError):
        S.embed_rows(rows[:100], B, a, v, 0)
    S.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            S.embed_rows(rows, B, a, v, 0)
    finally:
        S.eval()


# ---------------------------------------------------------------- python -m wav2lip_amd.calculate_scores
def test_cli_scores_a_directory_and_prints_the_reference_averages(cuda, tmp_path):
    from wav2lip_amd import audio, calculate_scores as cs, container, evaluation
    r = np.random.default_rng(3)
    box = (10, 106, 16, 112)
    clips = {}
    for name, T, seconds in (("b_long", 20, 1.0), ("a_short", 12, 0.6), ("c_tiny", 3, 0.5)):
        frames = r.integers(0, 256, (T, 120, 128, 3), dtype=np.uint8)
        pcm = (synth.noise_wav(int(16000 * seconds), seed=T) * 20000).astype(np.int16).reshape(-1, 1)
        container.write_avi(str(tmp_path / (name + ".avi")), frames, 25, audio=pcm, audio_sr=16000)
        clips[name] = (frames, pcm)
    (tmp_path / "notes.txt").write_text("not a clip")
    torch.save({"state_dict": {"module." + k: v for k, v in _sync_state_dict().items()}, "optimizer": None, "global_step": 1,
                "global_epoch": 0}, str(tmp_path / "sync.pth"))
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        scored = cs.main(["--data_root", str(tmp_path), "--checkpoint_path", str(tmp_path / "sync.pth"), "--box"] + [str(b) for b in box])
    lines = out.getvalue().strip().splitlines()
    assert [s["key"] for s in scored] == ["a_short.avi", "b_long.avi"] and [s["n"] for s in scored] == [8, 16]
    assert len(lines) == 4 and lines[0].startswith("a_short.avi: offset ") and lines[1].startswith("b_long.avi: offset ")
    assert lines[0].endswith("windows 8") and "confidence %.3f, minimum distance %.3f" % (scored[0]["lse_c"], scored[0]["lse_d"]) in lines[0]
    assert "c_tiny.avi: skipped: too short" in err.getvalue() and "notes" not in err.getvalue()
    # the same clips through lse_many by hand: the averages are over its results
    jobs = []
    for name in ("a_short", "b_long"):
        frames, pcm = clips[name]
        wav = pcm[:, 0].astype(np.float32) / np.float32(32768.0)
        jobs.append(evaluation.ScoreJob(name, cs.face_crops(frames, [box] * len(frames), cuda), audio.melspectrogram_device(wav, cuda)))
    want = evaluation.lse_many(_syncnet(cuda), jobs, batch_size=20)
    assert lines[2] == "Average Confidence: {}".format(sum(w["lse_c"] for w in want) / 2)
    assert lines[3] == "Average Minimum Distance: {}".format(sum(w["lse_d"] for w in want) / 2)
    assert [w["offset"] for w in want] == [s["offset"] for s in scored]
