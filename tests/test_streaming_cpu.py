"""Host side of streaming lip-sync (wav2lip_amd/streaming.py) with the device stubbed at the two seams `BatchRunner` and
`DeviceMel`: which columns are final, when a row is ready, that the rows of any feed split are `multiclip.rows_inference` of the
whole audio, what a ragged batch is padded to, and the spectrogram window filling and continuing."""
import numpy as np
import pytest


def _reads(col, total=-1):
    """every sample index column `col` reads, by the rule of the issue, one index at a time"""
    out = set()
    for n in range(800):
        j = col * 200 + n - 400
        if j < 0:
            j = -j
        if total >= 0 and j >= total:
            j = 2 * (total - 1) - j
        out.add(j)
        if j != 0:
            out.add(j - 1)
    return out


class StubMel:
    """DeviceMel on numpy: a column's "spectrogram" is its own absolute number; unwritten columns are NaN.  Checks on its own that
    the held samples cover what each column reads and that no column is ever written twice."""
    instances = []

    def __init__(self, device):
        self.calls, self.windows = [], 0
        StubMel.instances.append(self)

    def new_window(self, cap):
        self.windows += 1
        return np.full((80, cap), np.nan, np.float32)

    def carry(self, new, old, first, count):
        assert count <= 16 and not np.isnan(old[:, first:first + count]).any()
        new[:, :count] = old[:, first:first + count]

    @staticmethod
    def window_bytes(window):
        return window.nbytes

    def compute(self, items):
        self.calls.append(sum(it[7] for it in items))
        for x, first, total, window, cap, col0, lo, count in items:
            assert window.shape == (80, cap) and x.dtype == np.float32
            for col in range(lo, lo + count):
                need = _reads(col, total)
                assert first <= min(need) and max(need) < first + x.size, (col, total, first, x.size)
                assert (x[np.array(sorted(need)) - first] == np.array(sorted(need), np.float32) % 1000).all()   # the right samples
                assert 0 <= col - col0 < cap and np.isnan(window[:, col - col0]).all(), "a column is written once"
                window[:, col - col0] = col


class StubRunner:
    """BatchRunner without a device: a row's "output" is its input frame; records what every row's mel window holds"""
    instances = []

    def __init__(self, model, batch_size, depth, precision):
        self.device, self.batches = None, []
        StubRunner.instances.append(self)

    def submit(self, rows, pad_to=None):
        rec = []
        for st, fi, box, (window, cap, rel) in rows:
            assert window.shape[1] == cap and 0 <= rel and rel + 16 <= cap
            rec.append((st.key, fi, box, window[0, rel:rel + 16].copy()))
        self.batches.append((rec, pad_to))
        return [np.asarray(st.frames[fi]).copy() for st, fi, _, _ in rows]

    def result(self, item):
        return item

    @staticmethod
    def ready(item):
        return True


@pytest.fixture
def stub(monkeypatch):
    from wav2lip_amd import streaming
    StubMel.instances, StubRunner.instances = [], []
    monkeypatch.setattr(streaming, "BatchRunner", StubRunner)
    monkeypatch.setattr(streaming, "DeviceMel", StubMel)
    return streaming


def _audio(n):
    return (np.arange(n) % 1000).astype(np.float32)


def _frames(n, shape=(12, 10), tag=0):
    f = np.zeros((n,) + shape + (3,), np.uint8)
    for k in range(n):
        f[k, 0, 0] = (tag, k % 256, k // 256)
    return list(f)


def _splits(rng, n, kind):
    if kind == "whole":
        return [n]
    cuts, pos = [], 0
    while pos < n:
        c = int(rng.choice([0, 1, 199, 200, 201, 640, 3333, int(rng.integers(1, 5000))])) if kind == "mixed" else kind
        c = min(c, n - pos)
        cuts.append(c)
        pos += c
    return cuts


def test_final_columns_and_the_sample_range_of_a_column():
    from wav2lip_amd import streaming as s
    assert [s.final_columns(n) for n in (0, 400, 401, 599, 600, 799, 800, 3000, 3199, 3200, 3201)] == [0, 0, 1, 1, 2, 2, 3, 14, 14, 15, 15]
    assert [s.final_columns(n, True) for n in (401, 3199, 3200, 3201, 7777)] == [3, 16, 17, 17, 39]
    for n in (401, 1000, 3200, 7777):
        for t in range(s.final_columns(n)):                # a final column of an open stream reads only what was fed
            assert max(_reads(t)) < n and t * 200 + 400 <= max(n, 401)
        assert max(_reads(s.final_columns(n))) >= n        # and the next one does not
    for total in (401, 3000, 3199, 3200, 3201):
        for t in range(1 + total // 200):
            for tot in (-1, total):
                r = _reads(t, tot)
                assert s.column_sample_range(t, tot) == (min(r), max(r)), (t, tot)
    for col in range(0, 40):                               # what the host keeps covers every later column of an open stream
        assert s.first_sample_needed(col) == min(_reads(col)) or col < 3
        assert s.first_sample_needed(col) <= min(_reads(col))
    for n in range(0, 5000):                               # the tail the host keeps once the final columns are done
        assert n - s.first_sample_needed(s.final_columns(n)) <= 801


def test_a_ragged_batch_is_padded_to_the_next_table_size_within_the_batch_size():
    from wav2lip_amd import streaming as s
    assert s.BUCKETS == (8, 16, 32, 64, 128)
    assert [s.bucket(n, 128) for n in (1, 7, 8, 9, 16, 17, 33, 64, 65, 127, 128)] == [8, 8, 8, 16, 16, 32, 64, 64, 128, 128, 128]
    assert [s.bucket(n, 100) for n in (1, 8, 9, 60, 64, 65, 99)] == [8, 8, 16, 64, 64, 100, 100]
    assert [s.bucket(n, 4) for n in (1, 3, 4)] == [4, 4, 4]
    assert [s.bucket(n, 200) for n in (100, 128, 129, 199)] == [128, 128, 200, 200]
    assert [s.bucket(n, 8) for n in (1, 8)] == [8, 8]


@pytest.mark.parametrize("fps", [25., 30.])
@pytest.mark.parametrize("rem", [0, 1, 199])
def test_rows_of_any_feed_split_are_rows_inference_of_the_whole_audio(stub, fps, rem):
    from wav2lip_amd import multiclip
    rng = np.random.default_rng(int(fps) * 1000 + rem)
    for case, kind in enumerate(("mixed", "mixed", "mixed", 1600, "whole", 200, 641)):
        n = (20 + int(rng.integers(0, 60))) * 200 + rem
        nf = int(rng.integers(1, 9))
        static = case == 1
        boxes = [(k % 3, 9 + k % 3, 1, 8 + k % 2) for k in range(nf)]
        launched = []
        ls = stub.LipsyncStreams(None, batch_size=16, fps=fps, on_batch=launched.append, mel_window=64 if case % 2 else 1024)
        ls.open("s", _frames(nf), boxes, static=static)
        x, pos = _audio(n), 0
        for c in _splits(rng, n, kind):
            ls.feed("s", x[pos:pos + c])
            pos += c
            ls.step(flush=True)
            # the readiness rule: exactly the rows whose columns through start + 15 are final have run
            done = sum(len(set(b)) for b in launched)
            final = stub.final_columns(pos)
            want = 0
            while int(want * (80. / fps)) + 16 <= final:
                want += 1
            assert done == want, (kind, pos, done, want)
        ls.close("s")
        got = ls.drain()
        want = multiclip.rows_inference(1 + n // 200, nf, boxes, fps, static)
        rec = [r for b, _ in StubRunner.instances[-1].batches for r in b]
        assert [(fi, box) for _, fi, box, _ in rec] == [(fi, box) for fi, box, _ in want]
        for (_, _, _, cols), (_, _, start) in zip(rec, want):
            assert (cols == np.arange(start, start + 16)).all()
        assert len(rec) == len(want) == len(got["s"]) and want[-1][2] == 1 + n // 200 - 16
        for f, (fi, _, _) in zip(got["s"], want):
            assert tuple(f[0, 0]) == (0, fi % 256, fi // 256)
        assert [r for b in launched for _, r in dict.fromkeys(b)] == list(range(len(want)))
        for rows, (_, pad_to) in zip(launched, StubRunner.instances[-1].batches):     # padding: the last row again, to a table size
            real = len(dict.fromkeys(rows))
            assert len(rows) == pad_to == (16 if real == 16 else stub.bucket(real, 16)) and rows[real:] == [rows[real - 1]] * (pad_to - real)


def test_streams_interleave_in_open_order_and_batches_fill_across_streams(stub):
    from wav2lip_amd import multiclip
    rng = np.random.default_rng(5)
    lengths = {"a": 9000 + 1, "b": 20000, "c": 14000 + 199}
    launched, events = [], []
    ls = stub.LipsyncStreams(None, batch_size=8, depth=2, on_batch=launched.append, sink=lambda k, f: events.append((k, f is None)))
    x = {k: _audio(n) for k, n in lengths.items()}
    pos = dict.fromkeys(lengths, 0)
    ls.open("a", _frames(3, tag=1), [(0, 9, 1, 8)] * 3)
    ls.open("b", _frames(5, (20, 16), tag=2), [(2, 19, 1, 15)] * 5, static=True)
    opened_c = False
    while any(pos[k] < lengths[k] for k in lengths):
        if not opened_c and pos["b"] > 6000:
            ls.open("c", _frames(2, tag=3), [(0, 9, 1, 8)] * 2)          # opened mid-run
            opened_c = True
        for k in ("b", "a", "c"):
            if (k == "c" and not opened_c) or pos[k] >= lengths[k]:
                continue
            c = min(int(rng.integers(0, 1500)), lengths[k] - pos[k])
            ls.feed(k, x[k][pos[k]:pos[k] + c])
            pos[k] += c
            if pos[k] == lengths[k]:
                ls.close(k)
        ls.step()
    assert ls.drain() is None
    flat = [r for b in launched[:-1] for r in b] + list(dict.fromkeys(launched[-1]))
    assert all(len(b) == 8 for b in launched)                            # full batches; only the flushed one padded (to 8)
    assert any(len({k for k, _ in b}) > 1 for b in launched)             # rows of several streams share a batch
    for k, n in lengths.items():
        want = multiclip.rows_inference(1 + n // 200, {"a": 3, "b": 5, "c": 2}[k], [(0, 0, 0, 0)] * 5, 25., k == "b")
        assert [r for kk, r in flat if kk == k] == list(range(len(want)))
        assert [e for e in events if e[0] == k] == [(k, False)] * len(want) + [(k, True)]
    with pytest.raises(KeyError):
        ls.feed("a", x["a"][:10])                                        # finished streams are gone
    assert ls.device_bytes() == 0


def test_the_window_fills_and_continues_with_bounded_memory(stub):
    from wav2lip_amd import multiclip
    n = 16000 * 60 + 1
    x = _audio(n)
    ls = stub.LipsyncStreams(None, batch_size=32, mel_window=64)
    ls.open("long", _frames(4), [(0, 9, 1, 8)] * 4)
    sizes, held, pos = set(), [], 0
    rng = np.random.default_rng(9)
    while pos < n:
        c = min(int(rng.choice([640, 640, 640, 12800, 1, 7000])), n - pos)          # 12800 samples = 64 columns: a whole window at once
        ls.feed("long", x[pos:pos + c])
        pos += c
        ls.step()
        st = ls._streams["long"]
        sizes.add(ls.device_bytes("long"))
        held.append(st.held.size + sum(len(ch) for ch in st.chunks))
        assert st.cols_done == stub.final_columns(pos) and st.col0 <= st.cols_done <= st.col0 + 64
    assert sizes == {80 * 64 * 4} and max(held) <= 801                  # the device window and the host tail: bounded
    mel = StubMel.instances[-1]
    assert mel.windows >= (1 + n // 200) // 64                          # it did roll over, many times
    ls.close("long")
    got = ls.drain()
    want = multiclip.rows_inference(1 + n // 200, 4, [(0, 9, 1, 8)] * 4)
    rec = [r for b, _ in StubRunner.instances[-1].batches for r in b]
    assert len(got["long"]) == len(want) == len(rec)
    for (_, fi, _, cols), (wfi, _, start) in zip(rec, want):
        assert fi == wfi and (cols == np.arange(start, start + 16)).all()
    with pytest.raises(ValueError, match="mel_window"):
        stub.LipsyncStreams(None, mel_window=16)


def test_one_launch_per_tick_for_all_streams(stub):
    ls = stub.LipsyncStreams(None, batch_size=8)
    for k in range(5):
        ls.open(k, _frames(2), [(0, 9, 1, 8)] * 2)
    x = _audio(640 * 30)
    for t in range(30):
        for k in range(5):
            ls.feed(k, x[t * 640:(t + 1) * 640])
        ls.step()
    assert ls.launches == len(StubMel.instances[-1].calls) == 30 and set(StubMel.instances[-1].calls[1:]) <= {15, 20}


def test_close_fails_the_way_lipsync_fails_on_audio_that_is_too_short(stub):
    ls = stub.LipsyncStreams(None)
    box = [(0, 9, 1, 8)]
    ls.open("tiny", _frames(1), box)
    ls.feed("tiny", _audio(400))
    with pytest.raises(ValueError, match="reflect"):
        ls.close("tiny")
    ls.open("short", _frames(1), box)
    ls.feed("short", _audio(2999))
    ls.step()
    with pytest.raises(RuntimeError, match="mel columns"):              # lipsync: RuntimeError from w2l_mel_gather (T >= 16)
        ls.close("short")
    ls.open("ok", _frames(1), box)
    ls.feed("ok", _audio(3000))
    ls.close("ok")
    with pytest.raises(ValueError, match="closed"):
        ls.feed("ok", _audio(1))
    assert len(ls.drain()["ok"]) == 2                                   # mel_chunk_starts(16, 25) == [0, 0]
    with pytest.raises(ValueError, match="outside"):
        ls.open("bad", _frames(1), [(0, 13, 1, 8)])
    ls.open("dup", _frames(1), box)
    with pytest.raises(ValueError, match="already open"):
        ls.open("dup", _frames(1), box)


def test_cli_surface():
    from wav2lip_amd import streaming
    a = streaming.build_parser().parse_args(["--checkpoint_path", "c", "--face", "f0", "--audio", "a0", "--face", "f1", "--audio", "a1"])
    assert (a.face, a.audio, a.chunk_ms, a.outdir, a.precision, a.wav2lip_batch_size) == (["f0", "f1"], ["a0", "a1"], 40., "results", "fp32", 128)
    assert (a.pads, a.box, a.static, a.fps) == ([0, 10, 0, 0], [-1, -1, -1, -1], False, 25.)
