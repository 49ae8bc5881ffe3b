"""Streaming at a source rate of its own on the device (wav2lip_amd/streaming.py, w2l_resample_stream in csrc/audio_mel.hip): the
final 16 kHz samples of many streams per launch bit for bit against oracle/resample_ref.py of the whole signals, the buffer and
the spectrogram window rolling over, bounded device memory, the entry point's refusals, every delivered frame of streams at
48 kHz, 44.1 kHz and 16 kHz against the whole-signal path, and the command line."""
import numpy as np
import pytest
import torch

import _audio_cases as ac
import _stream_resample_cases as sc
from oracle import resample_ref
from test_streaming_gpu import _model, _replay, _state_dict
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu

SENT = 12352.0


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _state(streaming, key, rate, cap16=1 << 14, cap=64):
    return streaming.StreamState(key, [np.zeros((96, 96, 3), np.uint8)], [(0, 96, 0, 96)], False, 25., cap, sample_rate=rate, cap16=cap16)


# ---------------------------------------------------------------- the kernel, through advance_samples
# (rate, source samples): 1 - 4 inputs (every output comes at close, both wings cut; (48000, 4) has the padded zero), then
# signals of 300 - 700 outputs at five rates; the oracle is a Python loop, so each is converted once and shared
TINY = [k for k in ac.RESAMPLE_CASES if k[0] in (8000, 48000) and k[1] <= 4]
LONGER = [(48000, 1801), (44100, 1500), (22050, 700), (8000, 301), (15999, 500), (16001, 450)]
_REFS = {}


def _case(rate, n):
    if (rate, n) not in _REFS:
        x = ac.resample_input(rate, n) if n <= 4 else sc.noise(n, rate % 97 + n)
        ref = resample_ref.librosa_resample(x, rate, 16000)
        x.setflags(write=False)
        ref.setflags(write=False)
        _REFS[(rate, n)] = (x, ref)
    return _REFS[(rate, n)]


def _run_cut(cuda, cases, chunk_of, compare_every=1):
    """all `cases` as streams of one DeviceResampler, fed chunk_of(rate) samples per tick, ONE launch per tick for all of them;
    at every compared tick each stream's final samples equal the whole signal's, after close all of them"""
    from wav2lip_amd import streaming
    res = streaming.DeviceResampler(cuda)
    sts = [_state(streaming, i, rate) for i, (rate, n) in enumerate(cases)]
    data = [_case(rate, n) for rate, n in cases]
    pos, tick, launches, compared, shared = [0] * len(cases), 0, 0, 0, 0
    while any(not st.closed for st in sts):
        for i, (st, (x, _)) in enumerate(zip(sts, data)):
            if st.closed:
                continue
            c = chunk_of(cases[i][0]) or len(x)
            st.feed(x[pos[i]:pos[i] + c])
            pos[i] = min(len(x), pos[i] + c)
            if pos[i] == len(x):
                st.end_audio()
        before = [st.rs.n16 for st in sts]
        launched = streaming.advance_samples(res, sts)
        assert not streaming.advance_samples(res, sts)                       # one launch took everything that was final
        launches += launched
        shared += sum(st.rs.n16 > b for st, b in zip(sts, before)) > 1       # a block table that goes from one stream to the next
        tick += 1
        if tick % compare_every and any(not st.closed for st in sts):
            continue
        for i, (st, (x, ref)) in enumerate(zip(sts, data)):
            rs = st.rs
            want = len(ref) if st.closed else sc.final_outputs(cases[i][0], pos[i])
            assert rs.n16 == want, (cases[i], pos[i])
            if want:
                assert np.array_equal(_bits(rs.buf[:want]), _bits(ref[:want])), (cases[i], pos[i], want)
                compared += want
    for st, (x, ref) in zip(sts, data):
        assert st.rs.n16 == st.rs.total16 == len(ref) and st.rs.held.size == 0
        assert np.array_equal(_bits(st.rs.buf[:len(ref)]), _bits(ref)) and bool((st.rs.buf[len(ref):] == 0).all())
    assert shared > 0 or len(cases) == 1
    print("%d streams: %d ticks, %d launches, %d samples compared" % (len(cases), tick, launches, compared))


@pytest.mark.parametrize("chunk", ["K", "K+1", 997, None])
def test_streamed_samples_equal_the_whole_signals_bit_for_bit(cuda, chunk):
    """streams of six rates and of 1 - 4 input samples in the same launches, fed K, K + 1 or 997 samples per tick, or whole"""
    def chunk_of(rate):
        K = sc.params(rate)[2]
        return {"K": K, "K+1": K + 1}.get(chunk, chunk)
    _run_cut(cuda, TINY + LONGER, chunk_of)


def test_one_sample_per_feed(cuda):
    """chunk size 1 on short signals: most ticks have nothing final, and then there is no launch"""
    _run_cut(cuda, TINY + [(8000, 301), (48000, 700)], lambda rate: 1, compare_every=16)


@pytest.mark.parametrize("n_out", [127, 128, 129])
def test_output_counts_around_the_block_of_128(cuda, n_out):
    """one stream, one launch, n_out outputs - per stream and per launch - and one launch of three such streams"""
    _run_cut(cuda, [(48000, 3 * n_out)], lambda rate: None)
    assert len(_case(48000, 3 * n_out)[1]) == n_out
    if n_out == 129:
        _run_cut(cuda, [(48000, 381), (48000, 384), (48000, 387), (8000, 64)], lambda rate: None)


# ---------------------------------------------------------------- rolling over, memory
def test_a_small_buffer_and_window_roll_over_and_memory_does_not_grow(cuda):
    """4 s at 48 kHz in 1000-sample feeds, a 16 kHz buffer of 2048 samples and a window of 64 columns: the whole
    melspectrogram_device(audio.resample(...)) bit for bit across the roll-overs; the device bytes of the stream are the same
    in its first and its last quarter"""
    from wav2lip_amd import audio, streaming
    x = synth.noise_wav(48000 * 4 + 77, seed=5)
    y = audio.resample(x, 48000, 16000)
    full = audio.melspectrogram_device(y, cuda)
    res, mel = streaming.DeviceResampler(cuda), streaming.DeviceMel(cuda)
    st = _state(streaming, "s", 48000, cap16=2048, cap=64)
    buffers, windows, bytes_at = set(), set(), []
    for pos in range(0, len(x), 1000):
        st.feed(x[pos:pos + 1000])
        if pos + 1000 >= len(x):
            st.end_audio()
        while streaming.advance_samples(res, [st]) | streaming.advance_columns(mel, [st]):
            st.take_rows()
        st.take_rows()
        rs = st.rs
        buffers.add(rs.buf_first)
        windows.add(st.col0)
        bytes_at.append(streaming.DeviceResampler.buffer_bytes(rs.buf)
                        + (streaming.DeviceMel.window_bytes(st.window) if st.window is not None else 0))
        assert rs.n16 == (len(y) if st.closed else sc.final_outputs(48000, min(pos + 1000, len(x))))
        assert np.array_equal(_bits(rs.buf[:rs.n16 - rs.buf_first]), _bits(y[rs.buf_first:rs.n16])), (pos, rs.buf_first, rs.n16)
        assert st.cols_done == streaming.final_columns(rs.n16, st.mel_closed())
        if st.cols_done:
            assert torch.equal(st.window[:, :st.cols_done - st.col0], full[:, st.col0:st.cols_done]), (pos, st.col0, st.cols_done)
    assert st.cols_done == full.shape[1] == 1 + len(y) // 200 and len(buffers) >= 20 and len(windows) >= 5
    q = len(bytes_at) // 4
    assert max(bytes_at[:q]) == max(bytes_at[-q:]) == 2048 * 4 + 80 * 64 * 4


# ---------------------------------------------------------------- refusals
def test_resample_stream_refusals_write_nothing(cuda):
    """host-side refusals only: every address in these tables is valid and stays so; what varies are NULL arguments, counts,
    alignment and index_step, which the entry point refuses before it launches"""
    from wav2lip_amd import _lib, audio, streaming
    from wav2lip_amd._lib import check, current_stream, ptr
    lib, s = _lib.load(), current_stream()
    win, delta = audio.resample_tables(cuda, 48000)
    ratio, inc, scale, index_step, K = streaming.resample_params(48000)
    x = torch.from_numpy(sc.noise(1200, 1)).to(cuda)
    buf = torch.full((64 + 128 + 64,), SENT, dtype=torch.float32, device=cuda)
    y = buf[64:192]

    def tables(**change):
        host = torch.zeros(512, dtype=torch.uint8, pin_memory=True)
        st = host.numpy()[:128].view(streaming.RESAMPLE_STREAM)
        st[0] = (x.data_ptr(), 0, 1200, 400, y.data_ptr(), 0, win.data_ptr(), delta.data_ptr(), 0, 0, scale, inc, 1200, 128,
                 index_step, win.numel(), 0, (0, 0, 0))
        for f, v in change.items():
            st[f][0] = v
        host.numpy()[128:160].view(streaming.RESAMPLE_BLOCKS)[0] = (0, 128, 0, 0.0, 0, 0)
        return host, host.to(cuda)

    host, dev = tables()
    H, D, B = host.data_ptr(), dev.data_ptr(), dev.data_ptr() + 128
    calls = {
        "host NULL": lambda: lib.w2l_resample_stream(s, None, D, 1, B, 1, 512),
        "streams NULL": lambda: lib.w2l_resample_stream(s, H, None, 1, B, 1, 512),
        "blocks NULL": lambda: lib.w2l_resample_stream(s, H, D, 1, None, 1, 512),
        "nstreams=0": lambda: lib.w2l_resample_stream(s, H, D, 0, B, 1, 512),
        "nstreams=65536": lambda: lib.w2l_resample_stream(s, H, D, 65536, B, 1, 512),
        "nblocks=0": lambda: lib.w2l_resample_stream(s, H, D, 1, B, 0, 512),
        "nblocks>2^20": lambda: lib.w2l_resample_stream(s, H, D, 1, B, (1 << 20) + 1, 512),
        "num_table=0": lambda: lib.w2l_resample_stream(s, H, D, 1, B, 1, 0),
        "host misaligned": lambda: lib.w2l_resample_stream(s, H + 8, D, 1, B, 1, 512),
        "streams misaligned": lambda: lib.w2l_resample_stream(s, H, D + 8, 1, B, 1, 512),
        "blocks misaligned": lambda: lib.w2l_resample_stream(s, H, D, 1, B + 8, 1, 512),
    }
    keep = [host, dev]
    for name, change in (("index_step=0", dict(index_step=0)), ("index_step<0", dict(index_step=-170)), ("src NULL", dict(src=0)),
                         ("dst NULL", dict(dst16=0)), ("win NULL", dict(win=0)), ("delta NULL", dict(delta=0)),
                         ("src_held=0", dict(src_held=0)), ("dst_cap=0", dict(dst_cap=0)), ("nwin=1", dict(nwin=1)),
                         ("carry_held without carry", dict(carry_held=4))):
        h, d = tables(**change)
        keep += [h, d]
        calls[name] = lambda h=h, d=d: lib.w2l_resample_stream(s, h.data_ptr(), d.data_ptr(), 1, d.data_ptr() + 128, 1, 512)
    for name, call in calls.items():
        assert lib.w2l_bn_fold(s, 0, None, None, None, None, None, 1e-5, None, None) != 0      # a known message first
        mark = lib.w2l_last_error()
        rc = call()
        msg = lib.w2l_last_error()
        assert rc != 0 and msg != mark and b"resample_stream" in msg, (name, msg)
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()), "a refused w2l_resample_stream wrote"
    # the same table as it stands runs: 128 outputs of a closed 1200-sample signal, and nothing outside them
    check(lib.w2l_resample_stream(s, H, D, 1, B, 1, 512), "resample_stream")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    ref = resample_ref.resampy_resample(x.cpu().numpy(), 48000, 16000)
    assert (got[:64] == SENT).all() and (got[192:] == SENT).all()
    assert np.array_equal(_bits(got[64:192]), _bits(ref[:128]))


# ---------------------------------------------------------------- end to end
RATE_OF = {"a": 48000, "b": 44100, "c": 16000}


def _spec():
    r = np.random.default_rng(23)
    spec = {
        "a": dict(frames=list(r.integers(0, 256, (6, 120, 150, 3), dtype=np.uint8)), box=(10, 100, 20, 130), static=False, n_src=48000 + 100),
        "b": dict(frames=list(r.integers(0, 256, (3, 100, 110, 3), dtype=np.uint8)), box=(4, 96, 10, 102), static=True, n_src=44100 + 2300),
        "c": dict(frames=list(r.integers(0, 256, (9, 97, 131, 3), dtype=np.uint8)), box=(1, 96, 5, 60), static=False, n_src=16000 + 199),
    }
    for i, (k, s) in enumerate(spec.items()):
        s["src"] = synth.noise_wav(s["n_src"], seed=50 + i)
    return spec


def _run(model, spec, precision, seed, chunk_ms):
    """a seeded interleaving, a step after each feed; returns (frames per key, recorded batches, device bytes of "a" per step)"""
    from wav2lip_amd import streaming
    rng = np.random.default_rng(seed)
    batches, out, held = [], {k: [] for k in spec}, []
    ls = streaming.LipsyncStreams(model, batch_size=8, precision=precision, on_batch=batches.append, mel_window=64, resample_buffer=2048,
                                  sink=lambda k, f: out[k].append(f) if f is not None else None)
    for k, s in spec.items():
        ls.open(k, s["frames"], [s["box"]] * len(s["frames"]), static=s["static"], sample_rate=RATE_OF[k])
    pos = dict.fromkeys(spec, 0)
    while any(pos[k] < spec[k]["n_src"] for k in spec):
        k = str(rng.choice(sorted(j for j in spec if pos[j] < spec[j]["n_src"])))
        c = min(int(RATE_OF[k] * float(rng.choice(chunk_ms)) / 1000), spec[k]["n_src"] - pos[k])
        ls.feed(k, spec[k]["src"][pos[k]:pos[k] + c])
        pos[k] += c
        if pos[k] == spec[k]["n_src"]:
            ls.close(k)
        ls.step()
        if "a" in ls._streams:
            held.append(ls.device_bytes("a"))
    ls.drain()
    assert ls.device_bytes() == 0 and not ls._streams and ls.resample_launches > 0
    return out, batches, held


@pytest.fixture(scope="module")
def whole(cuda):
    """the whole-signal path: every stream's audio converted at once"""
    from wav2lip_amd import audio
    spec = _spec()
    for k, s in spec.items():
        s["wav"] = s["src"] if RATE_OF[k] == 16000 else audio.resample(s["src"], RATE_OF[k], 16000)
        s["n"] = len(s["wav"])
    return spec


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_frames_of_streams_at_48_44_and_16_khz_equal_the_whole_signal_path(cuda, whole, precision):
    """the standard of test_streaming_gpu.py for 16 kHz streams: every delivered frame equals the replay of the recorded batches
    on the spectrogram of the WHOLE converted audio byte for byte, fp32 and bf16; against `lipsync` on it the same rows, the
    input bytes outside the box, and fp32 within one uint8 level.  Two different cuts give identical frames (every launch has
    the batch size 8, so a row runs under one plan whatever shares its batch)."""
    from wav2lip_amd import inference
    model = _model(cuda)
    got, batches, held = _run(model, whole, precision, seed=1, chunk_ms=(0, 1, 12, 40, 41, 130))
    want, rows = _replay(model, cuda, whole, batches, precision, batch_size=8)
    for k, s in whole.items():
        assert len(got[k]) == len(rows[k]) == len(want[k]) > 0 and len(rows[k]) == len(_rows_of(s))
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert np.array_equal(a, b), (precision, k, i)
        ref = inference.lipsync(model, s["frames"], s["wav"], batch_size=8, static=s["static"], box=s["box"], precision=precision)
        assert len(ref) == len(got[k])
        y1, y2, x1, x2 = s["box"]
        worst = 0
        for a, b in zip(got[k], ref):
            d = np.abs(a.astype(np.int32) - b.astype(np.int32))
            assert int(d.sum()) == int(d[y1:y2, x1:x2].sum())
            worst = max(worst, int(d.max()))
        print("stream %s %s: %d rows, max difference to lipsync %d" % (k, precision, len(ref), worst))
        if precision == "f32":
            assert worst <= 1, (k, worst)
    q = len(held) // 4
    assert max(held[-q:]) <= max(held[:q]) == 2048 * 4 + 80 * 64 * 4                   # bounded: no growth with the duration
    again, batches2, _ = _run(model, whole, precision, seed=2, chunk_ms=(7, 40, 333))
    assert batches2 != batches
    for k in whole:
        assert len(again[k]) == len(got[k]) and all(np.array_equal(a, b) for a, b in zip(again[k], got[k])), k


def _rows_of(s):
    from wav2lip_amd import multiclip
    return multiclip.rows_inference(1 + s["n"] // 200, len(s["frames"]), [s["box"]] * len(s["frames"]), 25., s["static"])


# ---------------------------------------------------------------- the command line
def test_native_rate_writes_the_same_avi_bytes(cuda, tmp_path):
    """a 44.1 kHz stereo WAV: with --native_rate (fed as the file holds it, converted as it streams) and without (converted up
    front) the written files are the same bytes"""
    from scipy.io import wavfile
    from wav2lip_amd import container, multiclip, streaming
    r = np.random.default_rng(29)
    frames = r.integers(0, 256, (7, 120, 150, 3), dtype=np.uint8)
    n = 44100 + 2300
    pcm = np.clip(np.round(np.stack([synth.noise_wav(n, seed=41), synth.noise_wav(n, seed=42)], 1) * 20000.0), -32768, 32767).astype(np.int16)
    container.write_avi(str(tmp_path / "v.avi"), frames, 25)
    wavfile.write(str(tmp_path / "a.wav"), 44100, pcm)
    torch.save({"state_dict": {"module." + k: v for k, v in _state_dict().items()}, "optimizer": None, "global_step": 7,
                "global_epoch": 1}, str(tmp_path / "ckpt.pth"))
    argv = ["--checkpoint_path", str(tmp_path / "ckpt.pth"), "--box", "10", "100", "20", "130", "--wav2lip_batch_size", "16",
            "--face", str(tmp_path / "v.avi"), "--audio", str(tmp_path / "a.wav")]
    plain = streaming.main(argv + ["--outdir", str(tmp_path / "plain")])
    native = streaming.main(argv + ["--outdir", str(tmp_path / "native"), "--native_rate"])
    a, b = open(plain[0], "rb").read(), open(native[0], "rb").read()
    assert len(a) > 100000 and a == b
    clip = container.read_avi(native[0])
    M = int(np.ceil(n * 16000.0 / 44100))
    assert len(clip["frames"]) == len(multiclip.rows_inference(1 + M // 200, 7, [(10, 100, 20, 130)] * 7)) and clip["audio_sr"] == 44100
