"""Streaming lip-sync on the device (wav2lip_amd/streaming.py, w2l_mel_stream_cols in csrc/audio_mel.hip): the incremental
many-stream spectrogram bit for bit against `audio.melspectrogram_device` of the whole signal (which the existing tests pin to
the oracle), the entry point's argument errors, every delivered frame against a replay of the recorded batches through
`multiclip.BatchRunner` on the OFFLINE spectrograms, the streamed frames against `inference.lipsync`, bounded memory over a
60 s stream, the plans a run with many ragged ticks leaves, determinism, and the command line."""
import os

import numpy as np
import pytest
import torch

from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu


def _state_dict():
    from wav2lip_amd import models
    return synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.Wav2Lip().state_dict().items()}, seed=0)


def _model(cuda):
    from wav2lip_amd import models
    m = models.Wav2Lip()
    m.load_state_dict(_state_dict())
    return m.to(cuda).eval()


# ---------------------------------------------------------------- the spectrogram
MEL_LENGTHS = (4000, 4001, 4199, 7777, 3000, 9800)       # N % 200 in {0, 1, 199} among them


def _state(streaming, key, cap=64):
    return streaming.StreamState(key, [np.zeros((96, 96, 3), np.uint8)], [(0, 96, 0, 96)], False, 25., cap)


@pytest.mark.parametrize("chunk", [1, 199, 200, 640, 641, 3333, None])
def test_streamed_columns_equal_the_whole_signals_spectrogram_bit_for_bit(cuda, chunk):
    """several streams of different lengths, ONE launch per tick (`advance_columns` is one staged copy and one launch); at every
    point the final columns equal the same columns of the whole signal's spectrogram, after close all of it - the reflected
    start and end included"""
    from wav2lip_amd import audio, streaming
    wavs = [synth.noise_wav(n, seed=70 + i) * np.float32(0.5 + 0.1 * i) for i, n in enumerate(MEL_LENGTHS)]
    full = [audio.melspectrogram_device(w, cuda) for w in wavs]
    mel = streaming.DeviceMel(cuda)
    sts = [_state(streaming, i) for i in range(len(wavs))]
    pos, ticks, launches, compared = 0, 0, 0, 0
    step = chunk or max(MEL_LENGTHS)
    while pos < max(MEL_LENGTHS):
        for st, w in zip(sts, wavs):
            if pos < len(w):
                st.feed(w[pos:pos + step])
                if pos + step >= len(w):
                    st.closed = True
        pos += step
        launched = streaming.advance_columns(mel, sts)                        # one launch for all streams
        assert not streaming.advance_columns(mel, sts)                         # and nothing is left over
        ticks += 1
        launches += launched
        if chunk == 1 and not launched:
            continue
        for i, st in enumerate(sts):
            n = min(pos, len(wavs[i]))
            c = streaming.final_columns(n, st.closed)
            assert st.cols_done == c and (not st.closed or c == full[i].shape[1] == 1 + len(wavs[i]) // 200)
            if c:
                assert torch.equal(st.window[:, :c], full[i][:, :c]), (chunk, i, pos, c)
                compared += c
    assert compared >= sum(f.shape[1] for f in full) and all(st.closed for st in sts)
    for i, st in enumerate(sts):
        assert st.held.size == 0 and torch.equal(st.window[:, :st.cols_done], full[i])
    print("chunk %s: %d ticks, %d launches, %d columns compared" % (chunk, ticks, launches, compared))


def test_columns_survive_the_window_rolling_over(cuda):
    """a small window: the stream continues in fresh windows; every window holds the right columns at the right place"""
    from wav2lip_amd import audio, streaming
    wav = synth.noise_wav(16000 * 4 + 199, seed=3)
    full = audio.melspectrogram_device(wav, cuda)
    mel = streaming.DeviceMel(cuda)
    st = _state(streaming, "s", cap=64)
    windows = set()
    for pos in range(0, len(wav), 1000):
        st.feed(wav[pos:pos + 1000])
        if pos + 1000 >= len(wav):
            st.closed = True
        while streaming.advance_columns(mel, [st]):
            st.take_rows()
        st.take_rows()
        windows.add(st.col0)
        assert torch.equal(st.window[:, :st.cols_done - st.col0], full[:, st.col0:st.cols_done]), (pos, st.col0, st.cols_done)
    assert st.cols_done == full.shape[1] == 321 and len(windows) >= 5


def test_mel_stream_cols_reports_argument_errors_and_survives_a_bad_table(cuda):
    from wav2lip_amd import _lib, audio, streaming
    from wav2lip_amd._lib import current_stream, ptr
    lib = _lib.load()
    ctx = audio._context(cuda)
    buf = torch.zeros(256, dtype=torch.uint8, device=cuda)
    s = current_stream()
    assert lib.w2l_mel_stream_cols(None, s, ptr(buf), 1, ptr(buf[64:]), 1) != 0 and b"NULL" in lib.w2l_last_error()
    assert lib.w2l_mel_stream_cols(ctx, s, None, 1, ptr(buf[64:]), 1) != 0
    assert lib.w2l_mel_stream_cols(ctx, s, ptr(buf), 1, None, 1) != 0
    assert lib.w2l_mel_stream_cols(ctx, s, ptr(buf), 0, ptr(buf[64:]), 1) != 0
    assert lib.w2l_mel_stream_cols(ctx, s, ptr(buf), 65536, ptr(buf[64:]), 1) != 0
    assert lib.w2l_mel_stream_cols(ctx, s, ptr(buf), 1, ptr(buf[64:]), 0) != 0
    assert lib.w2l_mel_stream_cols(ctx, s, ptr(buf), 1, ptr(buf[64:]), (1 << 20) + 1) != 0
    assert lib.w2l_mel_stream_cols(ctx, s, ptr(buf[8:]), 1, ptr(buf[64:]), 1) != 0 and b"16-byte" in lib.w2l_last_error()
    assert lib.w2l_mel_stream_cols(ctx, s, ptr(buf), 1, ptr(buf[72:]), 1) != 0 and b"16-byte" in lib.w2l_last_error()
    # NOTE for whoever extends this: every ADDRESS in these tables is valid and must stay so.  The test varies only indices,
    # columns and counts, which the kernel's guards turn into a skipped entry or a clamped read inside the held samples; it must
    # never hand the kernel an invalid pointer, which no guard can catch and which would fault a device others share.
    # entries the kernel must skip or clamp, not follow: a stream index outside the table, a column outside the window, a stream
    # that holds nothing, and one whose held range does not cover the column (clamped: wrong numbers, no fault)
    wav = torch.from_numpy(synth.noise_wav(1000, seed=1)).to(cuda)
    window = torch.full((80, 8), 7.0, device=cuda)
    st = np.zeros(2, streaming.MEL_STREAM)
    st[0] = (wav.data_ptr(), 5000, -1, window.data_ptr(), 1000, 8, 0)
    st[1] = (wav.data_ptr(), 0, -1, window.data_ptr(), 0, 8, 0)
    ct = np.zeros(6, streaming.MEL_COL)
    ct[:] = [(2, 0, 0), (-1, 0, 0), (0, 0, 8), (0, 0, -1), (1, 0, 1), (0, 0, 3)]
    sd, cd = (torch.from_numpy(t.view(np.uint8).copy()).to(cuda) for t in (st, ct))
    assert lib.w2l_mel_stream_cols(ctx, s, ptr(sd), 2, ptr(cd), 6) == 0
    torch.cuda.synchronize()
    got = window.cpu().numpy()
    assert (np.delete(got, 3, axis=1) == 7.0).all() and np.isfinite(got[:, 3]).all() and (np.abs(got[:, 3]) <= 4).all()


# ---------------------------------------------------------------- end to end
def _streams_spec():
    r = np.random.default_rng(11)
    spec = {
        "a": dict(frames=list(r.integers(0, 256, (6, 120, 150, 3), dtype=np.uint8)), box=(10, 100, 20, 130), static=False, n=16000 * 2 + 1),
        "b": dict(frames=list(r.integers(0, 256, (3, 200, 210, 3), dtype=np.uint8)), box=(4, 196, 10, 202), static=True, n=16000 * 3),
        "c": dict(frames=list(r.integers(0, 256, (40, 97, 131, 3), dtype=np.uint8)), box=(1, 96, 5, 60), static=False, n=16000 + 199),
        "d": dict(frames=list(r.integers(0, 256, (2, 160, 160, 3), dtype=np.uint8)), box=(30, 140, 25, 135), static=False, n=23400),
    }
    for i, (k, s) in enumerate(spec.items()):
        s["wav"] = synth.noise_wav(s["n"], seed=90 + i)
    return spec


def _run_streamed(model, spec, precision, batch_size=16, seed=4, flush=False, mel_window=1024, chunks=(0, 1, 200, 640, 641, 1500, 3333)):
    """feed in a seeded interleaving with a step after each feed; "c" is opened mid-run; returns (frames per key, recorded
    batches, sink events)"""
    from wav2lip_amd import streaming
    rng = np.random.default_rng(seed)
    batches, events, out = [], [], {k: [] for k in spec}

    def sink(key, frame):
        events.append((key, frame is None))
        if frame is not None:
            out[key].append(frame)

    ls = streaming.LipsyncStreams(model, batch_size=batch_size, precision=precision, sink=sink, on_batch=batches.append, mel_window=mel_window)
    pos = dict.fromkeys(spec, 0)
    late = [k for k in spec if k == "c"]
    for k, s in spec.items():
        if k not in late:
            ls.open(k, s["frames"], [s["box"]] * len(s["frames"]), static=s["static"])
    opened = set(spec) - set(late)
    while any(pos[k] < spec[k]["n"] for k in spec):
        if late and sum(pos.values()) > 20000:
            k = late.pop()
            ls.open(k, spec[k]["frames"], [spec[k]["box"]] * len(spec[k]["frames"]), static=spec[k]["static"])
            opened.add(k)
        k = str(rng.choice(sorted(j for j in opened if pos[j] < spec[j]["n"])))
        c = min(int(rng.choice(chunks)), spec[k]["n"] - pos[k])
        ls.feed(k, spec[k]["wav"][pos[k]:pos[k] + c])
        pos[k] += c
        if pos[k] == spec[k]["n"]:
            ls.close(k)
        ls.step(flush=flush)
    ls.drain()
    assert ls.device_bytes() == 0 and not ls._streams
    return out, batches, events


def _replay(model, cuda, spec, batches, precision, batch_size=16):
    """every recorded batch again through BatchRunner, its rows on the spectrogram of the WHOLE audio"""
    from wav2lip_amd import audio, multiclip
    jobs, rows = {}, {}
    for k, s in spec.items():
        mel = audio.melspectrogram_device(s["wav"], cuda)
        rows[k] = multiclip.rows_inference(mel.shape[1], len(s["frames"]), [s["box"]] * len(s["frames"]), 25., s["static"])
        jobs[k] = multiclip.ClipJob(k, s["frames"], mel, rows[k])
    runner = multiclip.BatchRunner(model, batch_size, 2, precision)
    out = {k: [] for k in spec}
    for rec in batches:
        real = list(dict.fromkeys(rec))
        assert rec[:len(real)] == real and rec[len(real):] == [real[-1]] * (len(rec) - len(real))     # padding: the last row again
        item = runner.submit([(jobs[k], rows[k][i][0], rows[k][i][1], rows[k][i][2]) for k, i in real], pad_to=len(rec))
        for (k, i), f in zip(real, runner.result(item)):
            assert i == len(out[k])                                                                     # row order per stream
            out[k].append(f)
    return out, rows


@pytest.fixture(scope="module")
def streamed(cuda):
    spec = _streams_spec()
    return spec, {p: _run_streamed(_model(cuda), spec, p) for p in ("f32", "bf16")}


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_every_delivered_frame_equals_the_replay_on_the_offline_spectrograms(cuda, streamed, precision):
    spec, runs = streamed
    got, batches, events = runs[precision]
    want, rows = _replay(_model(cuda), cuda, spec, batches, precision)
    assert any(len({k for k, _ in b}) >= 3 for b in batches)                      # rows of three streams in one batch
    assert all(len(b) == 16 for b in batches[:-1]) and len(batches[-1]) in (8, 16)
    for k in spec:
        assert len(got[k]) == len(rows[k]) == len(want[k]) > 0
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.shape == spec[k]["frames"][0].shape and np.array_equal(a, b), (precision, k, i)
        mine = [e for e in events if e[0] == k]
        assert mine == [(k, False)] * len(rows[k]) + [(k, True)]                  # row order, then None once, last
    # a stream closed mid-batch: its last row is neither first nor last of its batch
    last = {k: (k, len(rows[k]) - 1) for k in spec}
    assert any(0 < b.index(last[k]) < len(dict.fromkeys(b)) - 1 for k in spec for b in batches if last[k] in b)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_streamed_frames_against_lipsync_on_the_whole_audio(cuda, streamed, precision):
    """the same rows as `lipsync`; outside the box the input bytes; f32 within one uint8 level (both sides are within the
    project's 1e-3 parity bar of the same oracle, and 1e-3 * 255 < 1).  The share of differing bytes is printed, not bounded."""
    from wav2lip_amd import inference
    spec, runs = streamed
    got = runs[precision][0]
    model = _model(cuda)
    for k, s in spec.items():
        ref = inference.lipsync(model, s["frames"], s["wav"], batch_size=16, static=s["static"], box=s["box"], precision=precision)
        assert len(ref) == len(got[k])
        y1, y2, x1, x2 = s["box"]
        worst, differing, total = 0, 0, 0
        for a, b in zip(got[k], ref):
            d = np.abs(a.astype(np.int32) - b.astype(np.int32))
            inside = d[y1:y2, x1:x2]
            assert int(d.sum()) == int(inside.sum())                               # outside the box: byte-equal
            worst, differing, total = max(worst, int(inside.max())), differing + int((inside != 0).sum()), total + inside.size
        print("stream %s %s: %d rows, max difference %d, differing bytes in the boxes %.3e" % (k, precision, len(ref), worst, differing / total))
        if precision == "f32":
            assert worst <= 1, (k, worst)


def test_a_long_stream_in_a_small_window_is_exact_and_its_memory_does_not_grow(cuda):
    from wav2lip_amd import streaming
    r = np.random.default_rng(13)
    n = 16000 * 60
    spec = {"long": dict(frames=list(r.integers(0, 256, (5, 100, 110, 3), dtype=np.uint8)), box=(8, 98, 6, 100), static=False, n=n,
                         wav=synth.noise_wav(n, seed=17))}
    model = _model(cuda)
    batches, out, at = [], [], {}
    ls = streaming.LipsyncStreams(model, batch_size=64, on_batch=batches.append, mel_window=64,
                                  sink=lambda k, f: out.append(f) if f is not None else None)
    ls.open("long", spec["long"]["frames"], [spec["long"]["box"]] * 5)
    for pos in range(0, n, 640):
        ls.feed("long", spec["long"]["wav"][pos:pos + 640])
        ls.step()
        if pos + 640 in (160000, 960000):
            st = ls._streams["long"]
            at[pos + 640] = (ls.device_bytes("long"), st.held.size, st.col0)
    ls.close("long")
    ls.drain()
    assert at[160000][0] == at[960000][0] == 80 * 64 * 4 and at[160000][1] <= 801 and at[960000][1] <= 801
    assert at[960000][2] > at[160000][2] > 0                                       # the window moved on
    want, rows = _replay(model, cuda, spec, batches, "f32", batch_size=64)
    assert len(out) == len(rows["long"]) == len(want["long"]) == 1497
    for i, (a, b) in enumerate(zip(out, want["long"])):
        assert np.array_equal(a, b), i


def test_ragged_ticks_leave_plans_of_the_bucket_sizes_only_and_runs_repeat_bit_for_bit(cuda):
    from wav2lip_amd import streaming
    spec = _streams_spec()
    model = _model(cuda)
    first = _run_streamed(model, spec, "f32", batch_size=32, seed=8, flush=True, chunks=(640, 1500, 3333, 5000, 9000))
    sizes = {k[0] for k in model._graphs}
    launched = sorted({len(b) for b in first[1]})
    print("plans of batch sizes %s for launches of %s; real rows per launch %s"
          % (sorted(sizes), launched, sorted({len(dict.fromkeys(b)) for b in first[1]})))
    assert sizes <= set(streaming.BUCKETS) | {32} and sizes == set(launched) and len({len(dict.fromkeys(b)) for b in first[1]}) > len(sizes)
    again = _run_streamed(model, spec, "f32", batch_size=32, seed=8, flush=True, chunks=(640, 1500, 3333, 5000, 9000))
    assert first[1] == again[1] and first[2] == again[2]
    for k in spec:
        assert len(first[0][k]) == len(again[0][k]) and all(np.array_equal(a, b) for a, b in zip(first[0][k], again[0][k]))


def test_command_line_writes_one_avi_per_stream(cuda, tmp_path):
    from scipy.io import wavfile
    from wav2lip_amd import container, multiclip, streaming
    r = np.random.default_rng(19)
    clips = [(r.integers(0, 256, (7, 120, 150, 3), dtype=np.uint8), 16000 + 1), (r.integers(0, 256, (30, 120, 150, 3), dtype=np.uint8), 9999)]
    argv = ["--checkpoint_path", str(tmp_path / "ckpt.pth"), "--outdir", str(tmp_path / "out"), "--box", "10", "100", "20", "130",
            "--wav2lip_batch_size", "16"]
    pcms = []
    for i, (frames, n) in enumerate(clips):
        pcm = np.clip(np.round(synth.noise_wav(n, seed=30 + i) * 20000.0), -32768, 32767).astype(np.int16)
        pcms.append(pcm)
        container.write_avi(str(tmp_path / ("v%d.avi" % i)), frames, 25)
        wavfile.write(str(tmp_path / ("a%d.wav" % i)), 16000, pcm)
        argv += ["--face", str(tmp_path / ("v%d.avi" % i)), "--audio", str(tmp_path / ("a%d.wav" % i))]
    torch.save({"state_dict": {"module." + k: v for k, v in _state_dict().items()}, "optimizer": None, "global_step": 7,
                "global_epoch": 1}, str(tmp_path / "ckpt.pth"))
    written = streaming.main(argv)
    assert written == [str(tmp_path / "out" / "0.avi"), str(tmp_path / "out" / "1.avi")]
    for i, (frames, n) in enumerate(clips):
        clip = container.read_avi(written[i])
        rows = multiclip.rows_inference(1 + n // 200, len(frames), [(10, 100, 20, 130)] * len(frames))
        assert len(clip["frames"]) == len(rows) and clip["fps"] == 25.0 and clip["audio_sr"] == 16000
        assert np.array_equal(clip["audio"][:, 0], pcms[i])
        for f, (fi, _, _) in zip(clip["frames"], rows):                            # outside the box: the cycled source frame
            d = f != frames[fi]
            d[10:100, 20:130] = False
            assert not d.any()
