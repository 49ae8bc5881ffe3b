"""The opt-in bf16 path of SyncNet scoring (`precision="bf16"`) on the device: w2l_sync_window_rows_bf16 bit for bit against the
fp32 kernel rounded once, w2l_sync_embeddings_bf16 against fp64, whole batches against the fp64 oracle within the bf16 error
model's yardstick, the two doors (`forward` and `embed_rows`) against each other, the one-live-graph rule, and
`evaluation.lse_many` / `lse_like` / `python -m wav2lip_amd.calculate_scores` in bf16 against their fp32 selves.

Yardstick: oracle.error_models.bf16_storage_noise jitters every conv input, weight and output of the exact graph by the bf16
rounding bound; the largest move it causes over three seeds is what bf16 storage alone can do.  The HIP plan may be at most twice
that far from the clean fp64 embeddings (the project's standing rule for bf16 plans).

Scores: every distance of the scorer is 1-Lipschitz in each embedding (and so are a mean and a min, and a median), so with E the
largest per-row move of a clip's face embeddings plus the same of its audio embeddings, LSE-D moves by at most E and LSE-C by at
most 2E."""
import contextlib
import io

import numpy as np
import pytest
import torch

from oracle import error_models, models_ref
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


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _same(a, b):
    """two fp32 tensors hold the same bytes"""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------- 1. w2l_sync_window_rows_bf16
def _tie_values():
    """fp32 values for the spectrogram: exact round-to-nearest-even ties (low 16 bits 0x8000) above an even and above an odd bf16
    mantissa, their neighbours at +-1 ulp, all of them negated, and +-4.0"""
    ties = np.array([0x3F808000, 0x3F818000, 0x40308000, 0x40318000, 0x3E7E8000, 0x3E7F8000], dtype=np.int64)
    bits = np.concatenate([ties, ties - 1, ties + 1])
    bits = np.concatenate([bits, bits | 0x80000000])
    vals = bits.astype(np.uint32).view(np.float32)
    return np.concatenate([vals, np.array([4.0, -4.0], np.float32)])


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("S", [96, 10])
def test_window_rows_bf16_is_the_fp32_kernel_rounded_once(cuda, S, shift):
    """S = 10: five output lines of three groups, the last one of 2 pixels.  shift = 1: frames on an odd address, the byte path.
    Three rows, the first repeated as the third; starts -3 and 10 of T = 20 (one before the spectrogram, one past its end);
    face_cs = 24 and mel_cs = 16 over sentinel-filled buffers, so every pad channel has to be written"""
    from wav2lip_amd import _lib, evaluation
    from wav2lip_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    r = np.random.default_rng(100 * S + shift)
    frames_np = r.integers(0, 256, (6, S, S, 3), dtype=np.uint8)
    store = torch.zeros(frames_np.size + 16, dtype=torch.uint8, device=cuda)
    store[shift:shift + frames_np.size] = torch.from_numpy(frames_np.reshape(-1)).to(cuda)
    frames = store[shift:shift + frames_np.size]
    assert frames.data_ptr() % 4 == shift
    T = 20
    mel_np = r.uniform(-4, 4, (80, T)).astype(np.float32)
    ties = _tie_values()
    mel_np.reshape(-1)[r.permutation(80 * T)[:4 * len(ties)]] = np.tile(ties, 4)
    assert (mel_np.view(np.uint32) & 0xFFFF == 0x8000).sum() >= 24
    mel = torch.from_numpy(mel_np).to(cuda)
    table = np.zeros(3, evaluation.SYNC_ROW)
    table[0] = (frames.data_ptr(), mel.data_ptr(), T, -3, (0, 0))
    table[1] = (frames.data_ptr() + S * S * 3, mel.data_ptr(), T, 10, (0, 0))
    table[2] = table[0]
    table_dev = torch.from_numpy(table.view(np.uint8)).to(cuda)
    Ho = S // 2
    s = current_stream()
    f32 = torch.full((3, Ho, S, 24), float("nan"), device=cuda)
    m32 = torch.full((3, 80, 16, 16), float("nan"), device=cuda)
    check(lib.w2l_sync_window_rows(s, 3, ptr(table_dev), S, ptr(f32), 24, ptr(m32), 16), "sync_window_rows")
    fb = torch.full((3, Ho, S, 24), 7.0, dtype=torch.bfloat16, device=cuda)
    mb = torch.full((3, 80, 16, 16), 7.0, dtype=torch.bfloat16, device=cuda)
    check(lib.w2l_sync_window_rows_bf16(s, 3, ptr(table_dev), S, ptr(fb), 24, ptr(mb), 16), "sync_window_rows_bf16")
    torch.cuda.synchronize()
    assert not torch.isnan(f32).any() and not torch.isnan(m32).any()
    assert torch.equal(_bits(fb), _bits(f32.to(torch.bfloat16)))
    assert torch.equal(_bits(mb), _bits(m32.to(torch.bfloat16)))
    assert not _bits(fb[..., 15:]).any() and not _bits(mb[..., 1:]).any()         # pad channels 15..23 and 1..15: zeros
    assert _bits(fb[..., :15]).any() and torch.equal(_bits(fb[0]), _bits(fb[2])) and torch.equal(_bits(mb[0]), _bits(mb[2]))
    # the windows themselves: columns outside [0, T) read as zero, the rest is the spectrogram rounded once
    want = np.zeros((2, 80, 16), np.float32)
    want[0, :, 3:] = mel_np[:, :13]
    want[1, :, :10] = mel_np[:, 10:]
    assert torch.equal(_bits(mb[:2, :, :, 0]), _bits(torch.from_numpy(want).to(torch.bfloat16)))
    # argument errors: refused without a launch
    fb.fill_(7.0)
    mb.fill_(7.0)
    big = torch.zeros(128, dtype=torch.uint8, device=cuda)
    assert lib.w2l_sync_window_rows_bf16(s, 0, ptr(table_dev), S, ptr(fb), 24, ptr(mb), 16) != 0
    assert lib.w2l_sync_window_rows_bf16(s, 65536, ptr(table_dev), S, ptr(fb), 24, ptr(mb), 16) != 0
    assert lib.w2l_sync_window_rows_bf16(s, 3, None, S, ptr(fb), 24, ptr(mb), 16) != 0
    assert lib.w2l_sync_window_rows_bf16(s, 3, ptr(table_dev), S, ptr(fb), 20, ptr(mb), 16) != 0
    assert lib.w2l_sync_window_rows_bf16(s, 3, ptr(table_dev), S, ptr(fb), 24, ptr(mb), 4) != 0
    assert b"multiples of 8" in lib.w2l_last_error()
    assert lib.w2l_sync_window_rows_bf16(s, 3, ptr(table_dev), S, fb.data_ptr() + 8, 24, ptr(mb), 16) != 0
    assert b"16-byte" in lib.w2l_last_error()
    assert lib.w2l_sync_window_rows_bf16(s, 3, ptr(table_dev), S, ptr(fb), 24, mb.data_ptr() + 2, 16) != 0
    assert lib.w2l_sync_window_rows_bf16(s, 1, ptr(big[8:]), S, ptr(fb), 24, ptr(mb), 16) != 0
    torch.cuda.synchronize()
    assert bool((fb == 7).all()) and bool((mb == 7).all())                          # nothing ran


# ---------------------------------------------------------------- 2. w2l_sync_embeddings_bf16
@pytest.mark.parametrize("B", [1, 5, 130])
def test_embeddings_kernel_against_fp64(cuda, B):
    """C = 512; the audio input has stride 512, the face input is a 520-wide slice whose channels past C hold NaN (a read of them
    shows in the result); both start two rows into larger arenas, and the outputs are rows [3, 3 + B) of sentinel-filled arenas.
    Audio row B // 2 is all zero.  Per element |y - ref| <= (C + 8) * 2**-24 * |ref| + 1e-12: the worst case of an fp32 sum of C
    exact squares (C - 1 additions), a square root, a divide, with room for the order of the additions"""
    from wav2lip_amd import _lib
    from wav2lip_amd._lib import check, current_stream, ptr
    lib = _lib.load()
    C = 512
    g = torch.Generator().manual_seed(B)
    ax = torch.full((B + 4, 512), 9.0, dtype=torch.bfloat16)
    fx = torch.full((B + 4, 520), float("nan"), dtype=torch.bfloat16)
    ax[2:2 + B] = (torch.randn(B, 512, generator=g) * torch.rand(B, 1, generator=g) * 3).to(torch.bfloat16)
    fx[2:2 + B, :C] = torch.relu(torch.randn(B, C, generator=g)).to(torch.bfloat16)        # half zeros, as after a ReLU
    ax[2 + B // 2] = 0
    axd, fxd = ax.to(cuda), fx.to(cuda)
    a_out = torch.full((B + 7, C), -5.0, device=cuda)
    f_out = torch.full((B + 7, C), -5.0, device=cuda)
    check(lib.w2l_sync_embeddings_bf16(current_stream(), B, C, ptr(axd[2:]), 512, ptr(fxd[2:]), 520, a_out.data_ptr() + 4 * C * 3,
                                       f_out.data_ptr() + 4 * C * 3), "sync_embeddings_bf16")
    torch.cuda.synchronize()
    for name, x, out in (("audio", ax[2:2 + B], a_out.cpu()), ("face", fx[2:2 + B, :C], f_out.cpu())):
        x64 = x.double()
        ref = x64 / x64.norm(dim=1, keepdim=True).clamp_min(1e-12)
        got = out[3:3 + B].double()
        assert not torch.isnan(got).any(), name
        excess = ((got - ref).abs() - ((C + 8) * 2.0 ** -24 * ref.abs() + 1e-12)).max()
        if bool((ref != 0).any()):
            rel = ((got - ref).abs() / ref.abs().clamp_min(1e-30))[ref != 0].max() / 2.0 ** -24
            print("B=%d %s: largest error %.2f x 2**-24 relative (bound %d)" % (B, name, float(rel), C + 8))
        assert float(excess) <= 0, (name, float(excess))
        assert bool((out[:3] == -5).all()) and bool((out[3 + B:] == -5).all()), name       # rows outside [offset, offset + B)
    assert not a_out[3 + B // 2].any()                                                       # the zero row gives zeros
    s = current_stream()
    a_out.fill_(-5.0)
    for args in ((0, C, ptr(axd), 512, ptr(fxd), 520, ptr(a_out), ptr(f_out)), (B, C, None, 512, ptr(fxd), 520, ptr(a_out), ptr(f_out)),
                 (B, C, ptr(axd), 504, ptr(fxd), 520, ptr(a_out), ptr(f_out)), (B, C, ptr(axd), 512, ptr(fxd), 516, ptr(a_out), ptr(f_out)),
                 (B, C, axd.data_ptr() + 2, 512, ptr(fxd), 520, ptr(a_out), ptr(f_out)),
                 (B, C, ptr(axd), 512, ptr(fxd), 520, a_out.data_ptr() + 4, ptr(f_out))):
        assert lib.w2l_sync_embeddings_bf16(s, *args) != 0
    torch.cuda.synchronize()
    assert bool((a_out == -5).all())


# ---------------------------------------------------------------- 3. the whole network against the fp64 oracle
def _windows():
    """8 windows as evaluation.sync_windows builds them: frames v .. v+4 of 12 crops, lower halves, / 255, stacked on channels"""
    frames = synth.face_crops_u8(12, seed=5)
    x = torch.from_numpy(frames)[:, 48:].permute(0, 3, 1, 2).float() / 255.
    faces = torch.stack([x[v:v + 5].reshape(15, 48, 96) for v in range(8)]).contiguous()
    mels = torch.from_numpy(synth.mel_windows(8, seed=5)).unsqueeze(1).contiguous()
    return frames, faces, mels


def _measures(got, clean):
    d = (got.double() - clean).abs()
    return {"linf": float(d.max()), "mean": float(d.mean()), "row": float(d.pow(2).sum(1).sqrt().max())}


@pytest.fixture(scope="module")
def oracle():
    """the clean fp64 embeddings of the 8 windows and the yardstick: per stream, the largest move over seeds 0-2 of
    bf16_storage_noise on L-inf, mean |d| and the largest per-row ||d||_2"""
    _, faces, mels = _windows()
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in _sync_state_dict().items()}
    f64, m64 = faces.double(), mels.double()
    clean = dict(zip(("audio", "face"), models_ref.syncnet_forward(sd64, m64, f64)))
    yard = {k: {"linf": 0.0, "mean": 0.0, "row": 0.0} for k in clean}
    for seed in range(3):
        with error_models.bf16_storage_noise(seed):
            noisy = dict(zip(("audio", "face"), models_ref.syncnet_forward(sd64, m64, f64)))
        for k in clean:
            for name, val in _measures(noisy[k], clean[k]).items():
                yard[k][name] = max(yard[k][name], val)
    for k in ("audio", "face"):
        print("bf16 yardstick, %s (max over 3 seeds, 8 windows): L-inf %.2e, mean %.2e, per-row L2 %.2e; %.0f%% non-zero"
              % (k, yard[k]["linf"], yard[k]["mean"], yard[k]["row"], 100 * float((clean[k] != 0).double().mean())))
    return dict(clean=clean, yard=yard, faces=faces, mels=mels)


@pytest.fixture(scope="module")
def net(cuda):
    return _syncnet(cuda)


@pytest.mark.parametrize("N", [8, 1, 7])
def test_forward_bf16_stays_within_twice_the_error_model_of_the_fp64_oracle(cuda, oracle, net, N):
    a, v = net(oracle["mels"][:N].to(cuda), oracle["faces"][:N].to(cuda), precision="bf16")
    assert a.dtype == v.dtype == torch.float32 and tuple(a.shape) == tuple(v.shape) == (N, 512)
    worst = 0.0
    for name, got in (("audio", a.cpu()), ("face", v.cpu())):
        m = _measures(got, oracle["clean"][name][:N])
        mult = {k: m[k] / oracle["yard"][name][k] for k in m}
        print("N=%d %s: L-inf %.2e (%.2f x), mean %.2e (%.2f x), per-row L2 %.2e (%.2f x the yardstick)"
              % (N, name, m["linf"], mult["linf"], m["mean"], mult["mean"], m["row"], mult["row"]))
        worst = max(worst, max(mult.values()))
    assert worst <= 2.0, worst


# ---------------------------------------------------------------- 4. two doors, one result
def _row_table(cuda, frames_dev, spec, n=8):
    """w2l_sync_row table of windows 0 .. n-1 of a clip whose window v is columns [16 v, 16 v + 16) of `spec`"""
    from wav2lip_amd import evaluation
    table = np.zeros(n, evaluation.SYNC_ROW)
    for v in range(n):
        table[v] = (frames_dev.data_ptr() + v * 96 * 96 * 3, spec.data_ptr(), spec.shape[1], 16 * v, (0, 0))
    return torch.from_numpy(table.view(np.uint8)).to(cuda)


def test_embed_rows_bf16_equals_forward_bf16_bit_for_bit(cuda, oracle, net):
    """both doors round the same fp32 input values to bf16 once and run the same plan at the same batch"""
    frames, faces, mels = _windows()
    frames_dev = torch.from_numpy(frames).to(cuda)
    spec = mels[:, 0].permute(1, 0, 2).reshape(80, 8 * 16).contiguous().to(cuda)
    rows = _row_table(cuda, frames_dev, spec)
    a, v = net(mels.to(cuda), faces.to(cuda), precision="bf16")
    a2 = torch.full((8, 512), float("nan"), device=cuda)
    v2 = torch.full((8, 512), float("nan"), device=cuda)
    net.embed_rows(rows, 8, a2, v2, precision="bf16")
    assert _same(a, a2) and _same(v, v2)
    a3 = torch.full((16, 512), -3.0, device=cuda)
    v3 = torch.full((16, 512), -3.0, device=cuda)
    net.embed_rows(rows, 8, a3, v3, 3, precision="bf16")
    assert _same(a, a3[3:11]) and _same(v, v3[3:11])
    for t in (a3, v3):
        assert bool((t[:3] == -3).all()) and bool((t[11:] == -3).all())
    with pytest.raises(ValueError, match="precision"):
        net.embed_rows(rows, 8, a2, v2, precision="fp16")
    with pytest.raises(ValueError, match="precision"):
        net(mels.to(cuda), faces.to(cuda), precision="fp16")


# ---------------------------------------------------------------- 5. one live graph
def test_one_live_graph_and_the_switch_is_inference_only(cuda, oracle, monkeypatch):
    from wav2lip_amd.models import syncnet
    S = _syncnet(cuda)
    built = []
    real = syncnet._SyncGraph

    def counting(*a, **k):
        if (a[5:] + (k.get("precision", "f32"),))[0] == "bf16":                            # counts the bf16 graphs, as before
            built.append(a[1:4])
        return real(*a, **k)

    monkeypatch.setattr(syncnet, "_SyncGraph", counting)
    m, f = oracle["mels"].to(cuda), oracle["faces"].to(cuda)
    a0, v0 = S(m, f)
    assert len(S._graphs) == 1 and built == []
    ab, vb = S(m, f, precision="bf16")
    assert len(S._graphs) == 1 and built == [(8, 48, 96)]
    assert next(iter(S._graphs.values()))[1].precision == "bf16"
    ab2, vb2 = S(m, f, precision="bf16")
    assert built == [(8, 48, 96)] and _same(ab, ab2) and _same(vb, vb2)          # the second call builds nothing new
    names = [d[0] for d in next(iter(S._graphs.values()))[1].dispatch()]
    assert len(names) == 17 + 14 and names[0] == "face_encoder.0" and names[-1] == "audio_encoder.13"
    a1, v1 = S(m, f)
    assert len(S._graphs) == 1 and next(iter(S._graphs.values()))[1].precision == "f32"
    assert _same(a0, a1) and _same(v0, v1)
    assert not _same(a0, ab)                                                        # and bf16 was a different computation
    S.train()
    try:
        with pytest.raises(ValueError, match="inference"):
            S(m, f, precision="bf16")
        with pytest.raises(RuntimeError, match="eval"):
            S.embed_rows(torch.zeros(32 * 8, dtype=torch.uint8, device=cuda), 8, a0.clone(), v0.clone(), precision="bf16")
    finally:
        S.eval()
    with pytest.raises(ValueError, match="inference"):                              # eval mode, but a gradient is asked for
        S(m, f.clone().requires_grad_(True), precision="bf16")


# ---------------------------------------------------------------- 6. evaluation.lse_many in bf16
VSHIFT = 3
LENGTHS = (5, 9, 12, 23, 4)          # frames; windows 1, 5, 8, 19 and none
WINDOWS = (1, 5, 8, 19)


def _clips(cuda):
    r = np.random.default_rng(17)
    faces = [r.integers(0, 256, (T, 96, 96, 3), dtype=np.uint8) for T in LENGTHS]
    mels = [torch.from_numpy(r.uniform(-4, 4, (80, 16 + int(3.2 * T))).astype(np.float32)).to(cuda) for T in LENGTHS]
    return [torch.from_numpy(f).to(cuda) for f in faces], mels


def _replay(S, batches, cuda, precision):
    """the recorded row tables through embed_rows again -> (audio, face) arenas"""
    a = torch.full((40, 512), float("nan"), device=cuda)
    v = torch.full((40, 512), float("nan"), device=cuda)
    for rows, B, offset in batches:
        S.embed_rows(rows, B, a, v, offset, precision=precision)
    return a, v


def _row_moves(x, y):
    return (x.double() - y.double()).pow(2).sum(1).sqrt().cpu().numpy()


@pytest.fixture(scope="module")
def many(cuda):
    """the five clips through lse_many in bf16 (batches recorded), again, on a fresh model, and in fp32; then both replays"""
    from wav2lip_amd import evaluation
    faces, mels = _clips(cuda)
    S = _syncnet(cuda)
    batches = []
    real_embed = S.embed_rows

    def recording_embed(rows, B, audio_out, face_out, offset=0, precision="f32"):
        batches.append((rows.clone(), B, offset, precision, tuple(audio_out.shape)))
        return real_embed(rows, B, audio_out, face_out, offset, precision=precision)

    def jobs():
        return (evaluation.ScoreJob("clip%d" % i, f, m) for i, (f, m) in enumerate(zip(faces, mels)))

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(S, "embed_rows", recording_embed, raising=False)
        first = evaluation.lse_many(S, jobs(), vshift=VSHIFT, batch_size=8, precision="bf16")
    again = evaluation.lse_many(S, jobs(), vshift=VSHIFT, batch_size=8, precision="bf16")
    fresh = evaluation.lse_many(_syncnet(cuda), jobs(), vshift=VSHIFT, batch_size=8, precision="bf16")
    f32 = evaluation.lse_many(S, jobs(), vshift=VSHIFT, batch_size=8)
    tables = [b[:3] for b in batches]
    ab, vb = _replay(S, tables, cuda, "bf16")
    a32, v32 = _replay(S, tables, cuda, "f32")
    return dict(S=S, faces=faces, mels=mels, batches=batches, first=first, again=again, fresh=fresh, f32=f32,
                bf16_emb=(ab, vb), f32_emb=(a32, v32))


def _same_bytes(a, b):
    assert [r["key"] for r in a] == [r["key"] for r in b]
    for x, y in zip(a, b):
        assert (x["n"], x["offset"]) == (y["n"], y["offset"])
        if x["n"]:
            assert np.float32(x["lse_c"]).tobytes() == np.float32(y["lse_c"]).tobytes()
            assert np.float32(x["lse_d"]).tobytes() == np.float32(y["lse_d"]).tobytes()
            assert x["mdist"].tobytes() == y["mdist"].tobytes()


def test_lse_many_bf16_equals_a_replay_of_its_batches_and_repeats_itself(cuda, many):
    from wav2lip_amd import evaluation
    assert [(b[1], b[2], b[3], b[4]) for b in many["batches"]] == [(8, lo, "bf16", (40, 512)) for lo in range(0, 40, 8)]
    ab, vb = many["bf16_emb"]
    segs = np.zeros(4, evaluation.LSE_SEGMENT)
    segs["n"] = WINDOWS
    segs["row0"] = np.concatenate([[0], np.cumsum(WINDOWS)[:-1]])
    win = 2 * VSHIFT + 1
    out = torch.full((4 * (4 + win),), float("nan"), device=cuda)
    evaluation._score_segments(4, torch.from_numpy(segs.view(np.uint8)).to(cuda), VSHIFT, vb, ab, out)
    res = out.cpu().numpy()
    scores, mdist = res[:16].reshape(4, 4), res[16:].reshape(4, win)
    assert [r["n"] for r in many["first"]] == [1, 5, 8, 19, 0]
    for k, r in enumerate(many["first"][:-1]):
        assert r["mdist"].tobytes() == mdist[k].tobytes(), r["key"]
        assert (np.float32(r["lse_d"]), np.float32(r["lse_c"]), r["offset"], r["n"]) == (scores[k, 0], scores[k, 1], int(scores[k, 2]),
                                                                                         int(scores[k, 3]))
    _same_bytes(many["first"], many["again"])
    _same_bytes(many["first"], many["fresh"])


def _check_lipschitz(got, ref, E, what):
    dd, dc = abs(got["lse_d"] - ref["lse_d"]), abs(got["lse_c"] - ref["lse_c"])
    print("%s %s: E %.3e, |d LSE-D| %.3e, |d LSE-C| %.3e, offsets %s / %s" % (what, got["key"], E, dd, dc, got["offset"], ref["offset"]))
    assert dd <= E + 1e-5, (got["key"], dd, E)
    assert dc <= 2 * E + 2e-5, (got["key"], dc, E)
    two = np.sort(ref["mdist"])[:2]
    if two[1] - two[0] > 2 * E:
        assert got["offset"] == ref["offset"], got["key"]


def test_lse_many_bf16_moves_the_scores_by_no_more_than_the_embeddings_moved(cuda, many):
    (ab, vb), (a32, v32) = many["bf16_emb"], many["f32_emb"]
    da, dv = _row_moves(ab, a32), _row_moves(vb, v32)
    assert [r["n"] for r in many["f32"]] == [r["n"] for r in many["first"]] == [1, 5, 8, 19, 0]
    last = many["first"][-1]
    assert last["offset"] is None and last["lse_c"] is None and last["lse_d"] is None and last["mdist"] is None
    row0 = 0
    for got, ref in zip(many["first"][:-1], many["f32"][:-1]):
        n = got["n"]
        E = float(dv[row0:row0 + n].max() + da[row0:row0 + n].max())
        assert 0 < E < 0.1
        _check_lipschitz(got, ref, E, "bf16 vs f32")
        row0 += n
    assert row0 == 33


# ---------------------------------------------------------------- 7. evaluation.lse_like in bf16
def test_lse_like_bf16_agrees_with_lse_many_bf16_per_clip(cuda, many):
    """one clip per call, batches of the clip's own size: launch configurations may differ from the packed batches of 8, so the
    bar is the Lipschitz bound with E taken between the embeddings of the two batchings"""
    from wav2lip_amd import evaluation
    L = _syncnet(cuda)
    seen = []
    real_forward = L.forward

    def recording_forward(audio, face, precision="f32"):
        out = real_forward(audio, face, precision=precision)
        seen.append((precision,) + tuple(out))
        return out

    L.forward = recording_forward
    ab, vb = many["bf16_emb"]
    row0 = 0
    for k, want in enumerate(many["first"][:-1]):
        del seen[:]
        got = evaluation.lse_like(L, many["faces"][k], many["mels"][k], vshift=VSHIFT, precision="bf16")
        got["key"] = want["key"]
        n = want["n"]
        assert got["n"] == n and [s[0] for s in seen] == ["bf16"]
        E = float(_row_moves(seen[0][2], vb[row0:row0 + n]).max() + _row_moves(seen[0][1], ab[row0:row0 + n]).max())
        _check_lipschitz(got, want, E, "lse_like vs lse_many")
        row0 += n
    with pytest.raises(ValueError, match="clip too short"):
        evaluation.lse_like(L, many["faces"][4], many["mels"][4], vshift=VSHIFT, precision="bf16")


# ---------------------------------------------------------------- 8. python -m wav2lip_amd.calculate_scores --precision bf16
def test_cli_scores_a_directory_in_bf16(cuda, tmp_path):
    from wav2lip_amd import audio, calculate_scores as cs, container, evaluation
    r = np.random.default_rng(3)
    box = (10, 106, 16, 112)
    clips = {}
    for name, T, seconds in (("b_long", 20, 1.0), ("a_short", 12, 0.6), ("c_tiny", 3, 0.5)):
        frames = r.integers(0, 256, (T, 120, 128, 3), dtype=np.uint8)
        pcm = (synth.noise_wav(int(16000 * seconds), seed=T) * 20000).astype(np.int16).reshape(-1, 1)
        container.write_avi(str(tmp_path / (name + ".avi")), frames, 25, audio=pcm, audio_sr=16000)
        clips[name] = (frames, pcm)
    torch.save({"state_dict": {"module." + k: v for k, v in _sync_state_dict().items()}, "optimizer": None, "global_step": 1,
                "global_epoch": 0}, str(tmp_path / "sync.pth"))
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        scored = cs.main(["--data_root", str(tmp_path), "--checkpoint_path", str(tmp_path / "sync.pth"), "--precision", "bf16", "--box"]
                         + [str(b) for b in box])
    lines = out.getvalue().strip().splitlines()
    assert [s["key"] for s in scored] == ["a_short.avi", "b_long.avi"] and [s["n"] for s in scored] == [8, 16]
    assert len(lines) == 4 and lines[0].startswith("a_short.avi: offset ") and lines[1].startswith("b_long.avi: offset ")
    assert lines[0].endswith("windows 8") and "confidence %.3f, minimum distance %.3f" % (scored[0]["lse_c"], scored[0]["lse_d"]) in lines[0]
    assert "c_tiny.avi: skipped: too short" in err.getvalue()
    jobs = []
    for name in ("a_short", "b_long"):
        frames, pcm = clips[name]
        wav = pcm[:, 0].astype(np.float32) / np.float32(32768.0)
        jobs.append(evaluation.ScoreJob(name + ".avi", cs.face_crops(frames, [box] * len(frames), cuda), audio.melspectrogram_device(wav, cuda)))
    S = _syncnet(cuda)
    want = evaluation.lse_many(S, jobs, batch_size=20, precision="bf16")
    _same_bytes(scored, want)
    assert lines[2] == "Average Confidence: {}".format(sum(w["lse_c"] for w in want) / 2)
    assert lines[3] == "Average Minimum Distance: {}".format(sum(w["lse_d"] for w in want) / 2)
    f32 = evaluation.lse_many(S, jobs, batch_size=20)
    assert any(np.float32(a["lse_d"]).tobytes() != np.float32(b["lse_d"]).tobytes() for a, b in zip(want, f32))    # the flag took effect
