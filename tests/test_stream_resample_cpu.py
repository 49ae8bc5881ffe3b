"""Host side of streaming at a source rate of its own (wav2lip_amd/streaming.py: ResampleState, advance_samples) with the device
stubbed at the seams `DeviceResampler`, `DeviceMel` and `BatchRunner`: which 16 kHz samples are final (against
oracle/resample_ref.py), the time registers across any cut, coverage of every launch, the rows of any cut, the lengths, and the
errors of `open` / `feed` / `close`."""
import numpy as np
import pytest

import _stream_resample_cases as sc
from oracle import resample_ref
from test_streaming_cpu import StubRunner, _frames


@pytest.fixture
def stub(monkeypatch):
    from wav2lip_amd import streaming
    sc.StubMel.instances, sc.StubResampler.instances, StubRunner.instances = [], [], []
    monkeypatch.setattr(streaming, "BatchRunner", StubRunner)
    monkeypatch.setattr(streaming, "DeviceMel", sc.StubMel)
    monkeypatch.setattr(streaming, "DeviceResampler", sc.StubResampler)
    return streaming


def _source(n):
    return (np.arange(n) % 1000).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_parameters_of_the_rates_the_issue_names():
    from wav2lip_amd import streaming as s
    assert [s.resample_params(r)[3:] for r in (48000, 44100, 8000)] == [(170, 192), (185, 177), (512, 64)]
    for r in sc.RATES + (8192000,):
        ratio, inc, scale, index_step, K = s.resample_params(r)
        assert (ratio, index_step, K) == sc.params(r) and inc == 1.0 / ratio and scale == min(1.0, ratio)
    assert s.resample_params(8192000)[3] == 1


@pytest.mark.parametrize("rate", sc.RATES)
def test_outputs_called_final_equal_the_whole_signals_and_later_ones_do_not(rate):
    """the bookkeeping's count of final outputs after m samples is the rule's (n_t + K <= m - 1); those outputs are bit-equal
    between resampy_resample(x[:m]) and the whole signal's; and some output past the rule differs, so the rule is not vacuous"""
    from wav2lip_amd import streaming
    ratio, _, K = sc.params(rate)
    N = int(600 / ratio)
    x = sc.noise(N, rate % 89)
    whole = resample_ref.resampy_resample(x, rate, 16000)
    differs = 0
    for m in (K + 1, K + 2, N // 3, N // 2 + 1, N - 1):
        rs = streaming.ResampleState("s", rate, 1 << 20)
        rs.feed(x[:m])
        c, tr = rs.new_final(1 << 20)
        assert c == sc.final_outputs(rate, m), (rate, m)
        part = resample_ref.resampy_resample(x[:m], rate, 16000)
        assert c <= len(part) and np.array_equal(_bits(part[:c]), _bits(whole[:c])), (rate, m, c)
        differs += int((_bits(part[c:]) != _bits(whole[c:len(part)])).sum())
        if c:
            assert np.array_equal(tr.view(np.uint64), resample_ref.time_registers(len(whole), ratio)[:c].view(np.uint64))
    assert differs > 0, rate


@pytest.mark.parametrize("rate", sc.RATES)
def test_time_registers_across_any_cut_are_the_whole_signals(stub, rate):
    """fed in ragged chunks through `advance_samples`: every launch's registers (the stub compares each, block starts among
    them) and the running register after every commit equal resample_ref.time_registers of the whole, bit for bit"""
    ratio, _, K = sc.params(rate)
    N = int(5000 / ratio) + 7
    x, rng = _source(N), np.random.default_rng(rate)
    st = stub.StreamState("s", _frames(1), [(0, 9, 1, 8)], False, 25., 64, sample_rate=rate, cap16=1 << 20)
    res = stub.DeviceResampler(None)
    whole = resample_ref.time_registers(int(np.ceil(N * ratio)) + 1, ratio)
    pos = 0
    while pos < N:
        c = min(int(rng.choice([0, 1, K, K + 1, 129, 997])), N - pos)
        st.feed(x[pos:pos + c])
        pos += c
        if pos == N:
            st.end_audio()
        stub.advance_samples(res, [st])
        assert not stub.advance_samples(res, [st])                          # nothing is left over: the room is large
        rs = st.rs
        assert rs.n16 == (rs.total16 if rs.closed else sc.final_outputs(rate, pos))
        assert np.float64(rs.tr_next).view(np.uint64) == whole[rs.n16].view(np.uint64)
        assert rs.held.size <= (K + 1) + (N - pos if rs.closed else 0) + int(np.ceil(1 / ratio)) + 2 * K    # only what later wings read
    assert st.rs.n16 == st.rs.total16 == int(np.ceil(N * ratio)) and st.rs.held.size == 0
    assert not np.isnan(st.rs.buf[:st.rs.n16]).any() and np.isnan(st.rs.buf[st.rs.n16:]).all()


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_block_start_registers_and_the_additions_of_a_blocks_threads(rate):
    """a launch's block table: copy blocks first, then blocks of up to 128 outputs whose start register is the whole signal's;
    thread j's j sequential float64 additions of the increment land on the whole signal's register of its output, bit for bit"""
    from wav2lip_amd import streaming
    ratio = 16000.0 / rate
    inc = streaming.resample_params(rate)[1]
    whole = resample_ref.time_registers(3000, ratio)
    for t0, count, carry in ((0, 1, 0), (0, 128, 0), (5, 129, 0), (1000, 700, 300), (2200, 127, 128)):
        blocks = streaming.resample_blocks(3, t0, whole[t0:t0 + count], t0 - carry, carry)
        copies, work = blocks[blocks["copy"] != 0], blocks[blocks["copy"] == 0]
        assert (blocks["stream"] == 3).all() and len(copies) == -(-carry // 128) and (blocks["copy"][:len(copies)] == 1).all()
        assert copies["count"].sum() == carry and (copies["t0"] == t0 - carry + 128 * np.arange(len(copies))).all()
        assert work["count"].sum() == count and (work["count"][:-1] == 128).all() and 1 <= work["count"][-1] <= 128
        assert (work["t0"] == t0 + 128 * np.arange(len(work))).all()
        for b in work:
            tr, t = np.float64(b["tr0"]), int(b["t0"])
            for j in range(int(b["count"])):
                assert tr.view(np.uint64) == whole[t + j].view(np.uint64), (rate, t, j)
                tr = np.float64(tr + np.float64(inc))


@pytest.mark.parametrize("chunk", [1, 192, 193, 997, None, "empty"])
def test_rows_of_any_cut_of_a_48_khz_stream_are_rows_inference(stub, chunk):
    """chunks of 1, K, K + 1 and 997 samples, whole-in-one, and empty feeds between ragged ones; a small 16 kHz buffer and
    spectrogram window, so both roll over; the stubs check coverage and single writes in every launch"""
    from wav2lip_amd import multiclip
    N = 12001 if chunk == 1 else 48000 * 2 + 5
    M = int(np.ceil(N * 16000 / 48000))
    nf, boxes = 5, [(k % 3, 9 + k % 3, 1, 8 + k % 2) for k in range(5)]
    ls = stub.LipsyncStreams(None, batch_size=16, mel_window=64, resample_buffer=2048)
    ls.open("s", _frames(nf), boxes, sample_rate=48000)
    x, pos, rng = _source(N), 0, np.random.default_rng(3)
    while pos < N:
        c = N if chunk is None else int(rng.choice([0, 0, 5000, 31])) if chunk == "empty" else chunk
        ls.feed("s", x[pos:pos + c])
        pos = min(N, pos + c)
        if chunk != 1 or pos % 64 == 0 or pos == N:
            ls.step()
            rs = ls._streams["s"].rs
            assert rs.n16 == sc.final_outputs(48000, pos) and ls.device_bytes("s") <= 2048 * 4 + 80 * 64 * 4
    ls.close("s")
    got = ls.drain()
    res, mel = sc.StubResampler.instances[-1], sc.StubMel.instances[-1]
    assert sum(res.calls) == M and sum(mel.calls) == 1 + M // 200 and ls.resample_launches == len(res.calls)
    assert ls.launches == len(mel.calls)
    if chunk != 1:
        assert res.buffers >= M // 2048 and res.carried > 0 and mel.windows > 1          # both rolled over
    want = multiclip.rows_inference(1 + M // 200, nf, boxes, 25., False)
    rec = [r for b, _ in StubRunner.instances[-1].batches for r in b]
    assert [(fi, box) for _, fi, box, _ in rec] == [(fi, box) for fi, box, _ in want] and len(got["s"]) == len(want)
    for (_, _, _, cols), (_, _, start) in zip(rec, want):
        assert (cols == np.arange(start, start + 16)).all()
    assert ls.device_bytes() == 0


def test_streams_at_16_khz_launch_nothing_new_and_share_ticks_with_native_ones(stub):
    ls = stub.LipsyncStreams(None, batch_size=8)
    ls.open("a", _frames(2), [(0, 9, 1, 8)] * 2)
    ls.feed("a", _source(6400))
    ls.step()
    assert ls.launches == 1 and ls.resample_launches == 0 and not sc.StubResampler.instances and ls._resampler is None
    ls.open("b", _frames(2), [(0, 9, 1, 8)] * 2, sample_rate=44100)
    ls.open("c", _frames(2), [(0, 9, 1, 8)] * 2, sample_rate=8000)
    for t in range(10):
        ls.feed("a", _source(6400 + 640 * (t + 1))[-640:])
        ls.feed("b", _source(1764 * (t + 1))[-1764:])
        ls.feed("c", _source(320 * (t + 1))[-320:])
        ls.step()
    assert ls.resample_launches == len(sc.StubResampler.instances[-1].calls) == 10 and ls.launches == 11       # one each per tick


def test_lengths_are_librosas(stub):
    """total16 = ceil(N * ratio), n_res = int(N * ratio); 2300 samples at 44100 Hz: 834 resampled samples, length 835"""
    for rate, n in ((44100, 2300), (48000, 4), (48000, 3), (8000, 3), (15999, 1), (16001, 2), (48000, 387), (22050, 1001)):
        x = sc.noise(n, n)
        rs = stub.ResampleState("s", rate, 4096)
        rs.feed(x)
        rs.close()
        assert rs.n_res == len(resample_ref.resampy_resample(x, rate, 16000)), (rate, n)
        assert rs.total16 == len(resample_ref.librosa_resample(x, rate, 16000)), (rate, n)
    rs = stub.ResampleState("s", 44100, 4096)
    rs.feed(sc.noise(2300, 1))
    rs.close()
    assert (rs.n_res, rs.total16) == (834, 835)
    st = stub.StreamState("s", _frames(1), [(0, 9, 1, 8)], False, 25., 64, sample_rate=44100, cap16=4096)
    st.feed(_source(2300))
    st.end_audio()
    res = stub.DeviceResampler(None)
    assert stub.advance_samples(res, [st]) and st.rs.n16 == 835 and st.mel_closed() and st.target() == 1 + 835 // 200


def test_open_feed_and_close_errors(stub):
    ls = stub.LipsyncStreams(None)
    box = [(0, 9, 1, 8)]
    for bad in (8192001, 16000 * 1024, 0, -48000, 44100.0, "48000", True, None):
        with pytest.raises(ValueError, match="sample_rate"):
            ls.open("bad", _frames(1), box, sample_rate=bad)
    ls.open("top", _frames(1), box, sample_rate=8192000)                  # index_step == 1: the highest rate there is a table for
    with pytest.raises(TypeError):
        ls.open("pos", _frames(1), box, False, None, 48000)              # by keyword only
    with pytest.raises(ValueError, match="resample_buffer"):
        stub.LipsyncStreams(None, resample_buffer=1024)
    ls.open("n", _frames(1), box, sample_rate=48000)
    stereo = (np.arange(2 * 9600).reshape(9600, 2) % 2000 - 1000).astype(np.int16)
    ls.feed("n", stereo)
    ls.feed("n", stereo[:0])
    ls.feed("n", np.zeros(10, np.uint8))
    ls.feed("n", np.zeros((10, 1), np.int32))
    ls.feed("n", np.zeros(10, np.float64))
    st = ls._streams["n"]
    assert st.rs.n_src == 9630 and st.n_fed == 0
    from wav2lip_amd import audio
    want = audio._pcm_to_float32(stereo).T.mean(axis=0)                  # load_wav's own expressions
    assert np.array_equal(_bits(st.rs.samples()[:9600]), _bits(want))
    halves = np.concatenate([stub.native_samples(stereo[:4801]), stub.native_samples(stereo[4801:])])
    assert np.array_equal(_bits(halves), _bits(want))                    # sample-wise: the cut does not show
    for bad in (np.zeros(4, np.int64), np.zeros((2, 2, 2), np.int16), np.zeros(4, np.complex64)):
        with pytest.raises(ValueError, match="feed"):
            ls.feed("n", bad)
    ls.open("k", _frames(1), box)
    with pytest.raises(ValueError, match="1-D"):
        ls.feed("k", np.zeros((10, 2), np.float32))                      # a 16 kHz stream: float32 1-D, as before
    # close applies its length checks to the 16 kHz length ceil(N * ratio)
    ls.open("tiny", _frames(1), box, sample_rate=48000)
    ls.feed("tiny", np.zeros(1200, np.int16))                            # 400 samples at 16 kHz
    with pytest.raises(ValueError, match="reflect"):
        ls.close("tiny")
    ls.open("short", _frames(1), box, sample_rate=48000)
    ls.feed("short", np.zeros(8997, np.int16))                           # 2999
    with pytest.raises(RuntimeError, match="mel columns"):
        ls.close("short")
    ls.open("ok", _frames(1), box, sample_rate=48000)
    ls.feed("ok", _source(8998))                                         # ceil(8998 / 3) = 3000
    ls.close("ok")
    with pytest.raises(ValueError, match="closed"):
        ls.feed("ok", _source(1))
    assert "ok" in ls._streams and "tiny" not in ls._streams and "short" not in ls._streams


def test_cli_surface():
    from wav2lip_amd import streaming
    argv = ["--checkpoint_path", "c", "--face", "f0", "--audio", "a0"]
    assert streaming.build_parser().parse_args(argv).native_rate is False
    assert streaming.build_parser().parse_args(argv + ["--native_rate"]).native_rate is True
