"""Host side of live streams (wav2lip_amd/streaming.py `open_live`, face_detection/live.py): the streamed finish of
`face_detect` against `many.host_boxes` of the whole video for EVERY cut of it into ticks, and `LipsyncStreams` with the device
stubbed at its three seams (`BatchRunner`, `DeviceMel`, `DeviceBoxes`): the rows of any interleaving of `feed` and `feed_frames`
are `multiclip.rows_inference` of the whole inputs, no row runs before its frame's box is final, one box launch per tick, a frame
without a face ends its stream only, the argument errors and the command line."""
import ctypes

import numpy as np
import pytest

from test_streaming_cpu import StubMel, StubRunner, _audio

FH, FW = 40, 50
PADS = [(0, 10, 0, 0), (3, 10, 5, 7), (-2, -10, -4, -3)]


# ---------------------------------------------------------------- stream_boxes_host
def _compositions(n):
    """every way to write n as an ordered sum of positive parts"""
    if n == 0:
        yield []
        return
    for first in range(1, n + 1):
        for rest in _compositions(n - first):
            yield [first] + rest


def _run_cut(live, rects, cut, close_on_empty, H, W, pads, T):
    """the ticks of `cut` (frame counts, zeros allowed) through stream_boxes_host; the close comes with the last tick, or on an
    empty tick of its own"""
    state, pos, out, counts = None, 0, [], []
    ticks = list(cut) + ([0] if close_on_empty else [])
    for k, c in enumerate(ticks):
        closed = k == len(ticks) - 1
        seen = pos
        boxes, state = live.stream_boxes_host(state, rects[pos:pos + c], closed, H, W, pads, T)
        pos += c
        assert state[0] == pos and len(state[1]) == min(pos, max(T, 1))          # the carry: never more than max(T, 1) raw rects
        assert state[1] == [tuple(r) for r in rects[pos - len(state[1]):pos]]
        assert len(boxes) == live.new_final_count(seen, c, closed, T)
        counts.append(len(boxes))
        out.append(boxes)
    assert sum(counts) == len(rects)
    return np.concatenate(out) if out else np.zeros((0, 4), np.int64)


@pytest.mark.parametrize("T", [0, 1, 2, 5])
def test_every_cut_of_a_short_video_gives_host_boxes_of_the_whole(T):
    from wav2lip_amd.face_detection import live, many
    rng = np.random.default_rng(40 + T)
    cuts = 0
    for pads in PADS:
        for n in range(1, 10):
            rects = [tuple(int(v) for v in r) for r in rng.integers(0, 71, (n, 4))]   # beyond the 40 x 50 frame: both clips act
            want = many.host_boxes(rects, FH, FW, pads, T)
            for cut in _compositions(n):
                for lead, close_on_empty in ((False, False), (True, False), (False, True)):
                    got = _run_cut(live, rects, ([0] if lead else []) + cut, close_on_empty, FH, FW, pads, T)
                    assert np.array_equal(got, want), (T, pads, n, cut, lead, close_on_empty)
                    cuts += 1
    assert cuts == 3 * 3 * sum(2 ** (n - 1) for n in range(1, 10))


@pytest.mark.parametrize("n", [70, 200])
@pytest.mark.parametrize("T", [5, 64])
def test_random_cuts_of_a_long_video_give_host_boxes_of_the_whole(n, T):
    from wav2lip_amd.face_detection import live, many
    rng = np.random.default_rng(n + T)
    rects = [tuple(int(v) for v in r) for r in rng.integers(0, 71, (n, 4))]
    for pads in PADS:
        want = many.host_boxes(rects, FH, FW, pads, T)
        for trial in range(12):
            cut, pos = [], 0
            while pos < n:
                c = min(int(rng.choice([0, 1, 1, 2, 3, 7, 16, 63, 64, 65, 100])), n - pos)
                cut.append(c)
                pos += c
            got = _run_cut(live, rects, cut, trial % 2 == 1, FH, FW, pads, T)
            assert np.array_equal(got, want), (n, T, pads, cut)


def test_new_final_count_is_the_lag_of_the_window():
    from wav2lip_amd.face_detection import live
    assert [live.new_final_count(0, k, False, 5) for k in range(7)] == [0, 0, 0, 0, 0, 1, 2]     # box i needs frame i + 4
    assert live.new_final_count(6, 1, False, 5) == 1 and live.new_final_count(6, 0, True, 5) == 4
    assert live.new_final_count(3, 0, True, 5) == 3 and live.new_final_count(0, 0, True, 5) == 0
    assert [live.new_final_count(s, 3, False, T) for s in (0, 9) for T in (0, 1)] == [3, 3, 3, 3]
    assert live.final_range(10, 4, False, 5) == (6, 10) and live.final_range(10, 4, True, 5) == (6, 14)


# ---------------------------------------------------------------- LipsyncStreams with the device stubbed
def _rect_of(frame):
    return tuple(int(v) for v in (frame[0, 1, 0], frame[0, 1, 1], frame[0, 1, 2], frame[0, 2, 0]))


def _video(n, seed, tag, no_face=()):
    """n frames of 40 x 50; pixel (0,0) names the frame, (0,1) and (0,2) carry the rect the stub detector "finds" and its flag"""
    rng = np.random.default_rng(seed)
    f = np.zeros((n, FH, FW, 3), np.uint8)
    for k in range(n):
        f[k, 0, 0] = (tag, k % 256, k // 256)
        f[k, 0, 1] = (rng.integers(0, 21), rng.integers(0, 16), rng.integers(30, 71))
        f[k, 0, 2] = (rng.integers(25, 71), 1 if k in no_face else 0, 0)
    return f


class StubBoxes:
    """DeviceBoxes on the host: the rect of a frame is written in the frame, the finish is `stream_boxes_host` per carry slot.
    Checks that a slot's `seen` continues where it stopped."""
    instances = []

    def __init__(self, device, detector, pads, T, batch_size):
        self.pads, self.T, self.state, self.launches, self.n_slots = pads, T, {}, [], 0
        StubBoxes.instances.append(self)

    def reserve(self, n_slots):
        self.n_slots = max(self.n_slots, n_slots)

    def launch(self, items):
        from wav2lip_amd.face_detection import live
        chunks, results = [], []
        assert len({it[3] for it in items}) == len(items)                       # a slot is named once per launch
        for fresh, H, W, slot, seen, closed in items:
            assert 0 <= slot < self.n_slots and all(f.shape == (H, W, 3) for f in fresh)
            state = self.state.get(slot) if seen else None
            assert seen == (state[0] if state else 0)
            chunks.append([(len(fresh), np.stack(fresh))] if fresh else [])
            flagged = [i for i, f in enumerate(fresh) if f[0, 2, 1]]
            if flagged:
                results.append((np.zeros((0, 4), np.int32), (1, seen + flagged[0])))
                continue
            boxes, self.state[slot] = live.stream_boxes_host(state, [_rect_of(f) for f in fresh], closed, H, W, self.pads, self.T)
            results.append((boxes.astype(np.int32), (0, 0)))
        self.launches.append(len(items))
        return dict(chunks=chunks, results=results)

    @staticmethod
    def collect(ticket):
        return ticket["results"]


class LiveStubMel(StubMel):
    """StubMel without its bound of 16 carried columns: the rows of a live stream may wait for their frames, and a window that
    rolls over meanwhile takes every column they will read along"""

    def carry(self, new, old, first, count):
        assert 0 < count < new.shape[1] and not np.isnan(old[:, first:first + count]).any()
        new[:, :count] = old[:, first:first + count]


@pytest.fixture
def stub(monkeypatch):
    from wav2lip_amd import streaming
    StubMel.instances, StubRunner.instances, StubBoxes.instances = [], [], []
    monkeypatch.setattr(streaming, "BatchRunner", StubRunner)
    monkeypatch.setattr(streaming, "DeviceMel", LiveStubMel)
    monkeypatch.setattr(streaming, "DeviceBoxes", StubBoxes)
    return streaming


def _want_rows(spec, T, pads):
    from wav2lip_amd import multiclip
    from wav2lip_amd.face_detection import many
    boxes = many.host_boxes([_rect_of(f) for f in spec["video"]], FH, FW, pads, T)
    rows = multiclip.rows_inference(1 + spec["n"] // 200, len(spec["video"]), boxes, spec["fps"])
    return rows if spec["cycle"] else rows[:min(len(rows), len(spec["video"]))]


def _run_live(stub, specs, seed, T=5, pads=(0, 10, 0, 0), batch_size=8, mel_window=1024, flush=True):
    """a seeded interleaving of audio feeds, frame feeds, closes and steps over all streams; every launch is checked against the
    boxes that are final at that moment.  Returns (stream object, delivered frames, launched batches, sink events)."""
    rng = np.random.default_rng(seed)
    launched, events, out = [], [], {k: [] for k in specs}
    states = {}

    def on_batch(rows):
        for key, row in rows:
            st = states[key]
            fi = row % st.n_frames if st.video_done else row
            assert fi < len(st.boxes), "row %d of %r launched before its frame's box was final" % (row, key)
        launched.append(rows)

    def sink(key, frame):
        events.append((key, frame is None))
        if frame is not None:
            out[key].append(frame)

    ls = stub.LipsyncStreams(None, batch_size=batch_size, on_batch=on_batch, sink=sink, mel_window=mel_window, detector=object(),
                             pads=pads, smooth_T=T)
    for k, s in specs.items():
        ls.open_live(k, fps=s["fps"], cycle=s["cycle"])
        states[k] = ls._streams[k]
    apos, vpos = dict.fromkeys(specs, 0), dict.fromkeys(specs, 0)
    x = {k: _audio(s["n"]) for k, s in specs.items()}
    ticks = 0
    while True:
        todo = [(k, kind) for k, s in specs.items() if k in ls._streams
                for kind, left in (("a", s["n"] - apos[k]), ("v", len(s["video"]) - vpos[k] + (not states[k].video_closed))) if left > 0]
        if not todo:
            break
        k, kind = todo[int(rng.integers(len(todo)))]
        s = specs[k]
        if kind == "a":
            c = min(int(rng.choice([0, 1, 200, 640, 641, 1500, 3333])), s["n"] - apos[k])
            ls.feed(k, x[k][apos[k]:apos[k] + c])
            apos[k] += c
            if apos[k] == s["n"]:
                ls.close(k)
        elif vpos[k] == len(s["video"]):
            ls.close_video(k)
        else:
            c = min(int(rng.choice([0, 1, 1, 2, 3, 7])), len(s["video"]) - vpos[k])
            ls.feed_frames(k, list(s["video"][vpos[k]:vpos[k] + c]))
            vpos[k] += c
        if rng.integers(3) == 0:
            before = ls.box_launches
            ls.step(flush=flush)
            ticks += 1
            assert ls.box_launches - before <= 1                                # one box launch per tick, whatever the streams
    ls.drain()
    assert not ls._streams and ls.box_launches == len(StubBoxes.instances[-1].launches) > 0
    return ls, out, launched, events


@pytest.mark.parametrize("fps", [25., 30.])
@pytest.mark.parametrize("T", [5, 0])
def test_rows_of_any_interleaving_are_rows_inference_of_the_whole_inputs(stub, fps, T):
    n = 16000 * 2 + 199                                   # 51 rows at 25 fps, 61 at 30
    rows = len(_want_rows(dict(video=_video(3, 0, 0), n=n, fps=fps, cycle=True), T, (0, 10, 0, 0)))
    specs = {
        "short": dict(video=_video(7, 1, 1), n=n, fps=fps, cycle=True),            # video shorter than audio: the rows cycle
        "equal": dict(video=_video(rows, 2, 2), n=n, fps=fps, cycle=True),
        "long": dict(video=_video(rows + 9, 3, 3), n=n, fps=fps, cycle=True),      # longer: the frames behind the audio are unused
        "prefix": dict(video=_video(11, 4, 4), n=n, fps=fps, cycle=False),         # cycle=False: the rows end with the video
        "one": dict(video=_video(1, 5, 5), n=n, fps=fps, cycle=True),
    }
    for seed, window in ((0, 1024), (1, 64), (2, 1024)):
        ls, out, launched, events = _run_live(stub, specs, seed=int(fps) + 10 * seed + T, T=T, mel_window=window)
        rec = {k: [] for k in specs}
        for batch, _ in StubRunner.instances[-1].batches:
            for key, _, box, cols in batch:
                rec[key].append((box, cols))
        for k, s in specs.items():
            want = _want_rows(s, T, (0, 10, 0, 0))
            assert len(out[k]) == len(rec[k]) == len(want) > 0, (k, len(out[k]), len(want))
            for f, (box, cols), (fi, wbox, start) in zip(out[k], rec[k], want):
                assert tuple(f[0, 0]) == (s["video"][0][0, 0, 0], fi % 256, fi // 256) and box == wbox
                assert (cols == np.arange(start, start + 16)).all()
            assert [e for e in events if e[0] == k] == [(k, False)] * len(want) + [(k, True)]
            assert [r for b in launched for kk, r in dict.fromkeys(b) if kk == k] == list(range(len(want)))
        assert not ls.errors and ls.device_bytes() == 0 and len(out["prefix"]) == 11 and len(out["short"]) == rows


def test_the_batch_sequence_repeats_for_a_repeated_call_sequence(stub):
    specs = {k: dict(video=_video(9 + 4 * k, k, k), n=20000 + 1000 * k, fps=25., cycle=bool(k % 2)) for k in range(4)}
    first = _run_live(stub, specs, seed=7, flush=False)
    again = _run_live(stub, specs, seed=7, flush=False)
    assert first[2] == again[2] and first[3] == again[3] and len(first[2]) > 3
    assert StubBoxes.instances[-1].launches == StubBoxes.instances[-2].launches
    assert any(len({k for k, _ in b}) > 1 for b in first[2])                     # live rows of several streams share a batch


def test_a_frame_without_a_face_ends_its_stream_only(stub):
    from wav2lip_amd.face_detection import many
    specs = {
        "a": dict(video=_video(12, 1, 1), n=16000, fps=25., cycle=True),
        "bad": dict(video=_video(30, 2, 2, no_face=(17, 20)), n=16000 * 2, fps=25., cycle=True),
        "c": dict(video=_video(8, 3, 3), n=16000, fps=25., cycle=True),
    }
    ls, out, launched, events = _run_live(stub, specs, seed=3)
    assert ls.errors == {"bad": many.NO_FACE}
    for k in ("a", "c"):
        want = _want_rows(specs[k], 5, (0, 10, 0, 0))
        assert len(out[k]) == len(want) and [tuple(f[0, 0])[1] for f in out[k]] == [fi for fi, _, _ in want]
    # the rows delivered are a prefix of the stream's rows: frames before the tick of frame 17 whose boxes were final
    n_bad = len(out["bad"])
    assert n_bad <= 17 - 4 and [tuple(f[0, 0])[1] for f in out["bad"]] == list(range(n_bad))
    assert [e for e in events if e[0] == "bad"] == [("bad", False)] * n_bad + [("bad", True)]
    with pytest.raises(KeyError):
        ls.feed_frames("bad", [specs["bad"]["video"][0]])


def test_cycle_false_releases_the_frames_it_has_delivered(stub):
    """a long cycle=False stream in small ticks: the chunks resident on the "device" stay a few ticks' worth"""
    n_frames = 400
    video = _video(n_frames, 9, 9)
    x = _audio(640 * n_frames + 3200)
    ls = stub.LipsyncStreams(None, batch_size=8, detector=object(), mel_window=64)
    ls.open_live("s", cycle=False)
    held = []
    for t in range(n_frames):
        ls.feed("s", x[t * 640:(t + 1) * 640])
        ls.feed_frames("s", [video[t]])
        ls.step(flush=True)
        held.append(ls.device_bytes("s") - 80 * 64 * 4 * (ls._streams["s"].window is not None))
    assert max(held) <= 12 * FH * FW * 3 and max(held[300:]) <= max(held[:200])
    ls.feed("s", x[640 * n_frames:])
    ls.close_video("s")
    ls.close("s")
    assert len(ls.drain()["s"]) == n_frames and not ls._streams


def test_argument_errors_name_the_stream(stub):
    ls = stub.LipsyncStreams(None)
    with pytest.raises(ValueError, match="'cam'.*detector"):
        ls.open_live("cam")
    for kw in (dict(smooth_T=65), dict(smooth_T=-1), dict(pads=(0, 10, 0)), dict(face_det_batch_size=0)):
        with pytest.raises(ValueError):
            stub.LipsyncStreams(None, detector=object(), **kw)
    ls = stub.LipsyncStreams(None, detector=object())
    ls.open_live("cam")
    with pytest.raises(ValueError, match="already open"):
        ls.open_live("cam")
    video = _video(3, 1, 1)
    ls.feed_frames("cam", [video[0]])
    ls.feed_frames("cam", video[1])                                             # one [H,W,3] array is one frame
    with pytest.raises(ValueError, match="'cam'.*shape"):
        ls.feed_frames("cam", [np.zeros((FH, FW + 1, 3), np.uint8)])
    with pytest.raises(ValueError, match="'cam'.*uint8"):
        ls.feed_frames("cam", [np.zeros((FH, FW, 3), np.float32)])
    ls.close_video("cam")
    with pytest.raises(ValueError, match="'cam'.*closed"):
        ls.feed_frames("cam", [video[2]])
    with pytest.raises(ValueError, match="'cam'.*closed"):
        ls.close_video("cam")
    ls.open_live("empty")
    with pytest.raises(ValueError, match="'empty'.*no frames"):
        ls.close_video("empty")
    ls.feed_frames("empty", [video[0]])                                         # it stays open: frames may still come
    ls.close_video("empty")
    ls.open("file", [video[0]], [(0, 30, 0, 40)])
    with pytest.raises(ValueError, match="'file'"):
        ls.feed_frames("file", [video[0]])
    with pytest.raises(KeyError):
        ls.feed_frames("nobody", [video[0]])


def test_cli_surface():
    from wav2lip_amd import streaming
    argv = ["--checkpoint_path", "c", "--face", "f0", "--audio", "a0"]
    assert streaming.build_parser().parse_args(argv).live_video is False
    assert streaming.build_parser().parse_args(argv + ["--live_video"]).live_video is True


def _bf16_backbone_launches(N, H, W):
    """(layer, family, tile, split-K) of every bf16 backbone convolution of S3FD at batch N (w2l_convb_resolve_geom: the function
    of the shape the launcher calls before it launches; no device)"""
    import importlib
    from wav2lip_amd import _lib
    s3fd = importlib.import_module("wav2lip_amd.face_detection.s3fd")
    lib, out = _lib.load(), []
    for item in s3fd.BACKBONE:
        if item == "pool":
            H, W = H // 2, W // 2
        elif not isinstance(item, str):
            name, cin, cout, k, stride, pad = item
            geom = _lib.ConvGeom(0, cin, cout, k, k, stride, stride, pad, pad, 0, 0, _lib.ACT_RELU)
            fam, tile, ks, flops = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
            assert lib.w2l_convb_resolve_geom(ctypes.byref(geom), N, H, W, 0, ctypes.byref(fam), ctypes.byref(tile), ctypes.byref(ks),
                                              ctypes.byref(flops)) == 0
            out.append((name, fam.value, tile.value, ks.value))
            H, W = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return out


def test_the_bf16_detector_sums_in_another_order_at_another_batch_size():
    """Why the contract of a live stream names `face_detect` IN WHOLE BATCHES of face_det_batch_size: a live tick always detects
    in whole batches (the last padded), `face_detect` ends a video in a ragged one, and the bf16 detector's launches are a
    function of the batch size - at 128 x 144 a batch of 7 runs conv3_1 .. conv5_3 with other split-K factors than a batch of 8,
    at 160 x 160 conv2_1 and conv2_2 with another tile.  Another split-K is another summation order; after bf16 rounding of every
    layer's output that can move a rect's truncated coordinate.  A batch of 8 is the same function whatever frames fill it."""
    at7, at8 = _bf16_backbone_launches(7, 128, 144), _bf16_backbone_launches(8, 128, 144)
    moved = {a[0]: (a[3], b[3]) for a, b in zip(at7, at8) if a != b}
    assert {"conv3_1", "conv4_1", "conv5_1"} <= set(moved) and all(x != y for x, y in moved.values()), moved
    assert _bf16_backbone_launches(7, 160, 160) != _bf16_backbone_launches(8, 160, 160)
    assert _bf16_backbone_launches(8, 128, 144) == at8
