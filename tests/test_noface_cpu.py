"""Host side of the opt-in pass-through for frames without a face (`no_face_hold`): the numpy model of
tests/_noface_cases.py against `get_smoothened_boxes` where every frame is detected, the product's two host statements
(`many.host_boxes_runs`, `live.stream_boxes_runs_host`) against the model on the seeded clips and every cut, `face_detect` with a
stub detector, the packer and the streams with their device sides stubbed, the argument checks and the three parsers."""
import types

import numpy as np
import pytest

import _noface_cases as cases
from _noface_cases import FH, FW
from test_multiclip_cpu import StubRunner as PackStubRunner
from test_streaming_cpu import StubRunner, _audio, _frames
from test_streaming_live_cpu import LiveStubMel, _compositions, _rect_of, _video


# ---------------------------------------------------------------- the rule on the host
def test_with_every_frame_detected_the_rule_is_get_smoothened_boxes_on_the_padded_rects():
    from wav2lip_amd import inference
    from wav2lip_amd.face_detection import many
    rng = np.random.default_rng(1)
    for n in (1, 2, 4, 5, 6, 9, 70):
        rects = cases.clip_rects(np.ones(n, bool), rng)
        for pads in cases.PADS:
            top, bottom, left, right = pads
            padded = np.array([[max(0, r[1] - top), min(FH, r[3] + bottom), max(0, r[0] - left), min(FW, r[2] + right)] for r in rects])
            for T in (0, 1, 2, 5, 8, 64):
                want = inference.get_smoothened_boxes(padded.copy(), T) if T else padded
                for G in (0, 3):
                    boxes, valid = cases.model(rects, FH, FW, pads, T, G)
                    assert np.array_equal(boxes, want) and valid.all()
                    got, got_valid = many.host_boxes_runs(rects, FH, FW, pads, T, G)
                    assert np.array_equal(got, many.host_boxes(rects, FH, FW, pads, T)) and np.array_equal(got, want) and got_valid.all()


@pytest.mark.parametrize("T", cases.WINDOWS)
def test_host_boxes_runs_is_the_model_on_the_seeded_clips(T):
    from wav2lip_amd.face_detection import many
    for G in cases.HOLDS:
        for name, clip in cases.all_clips(T, G, seed=100 * T + G):
            pads = cases.PADS[len(name) % 2]
            want, want_valid = cases.model(clip, FH, FW, pads, T, G)
            got, got_valid = many.host_boxes_runs(clip, FH, FW, pads, T, G)
            assert np.array_equal(got, want) and np.array_equal(got_valid, want_valid), (T, G, name)
            assert got.dtype == np.int64 and got_valid.dtype == bool and not got[~got_valid].any()


def _ticks(live, clip, cut, close_on_empty, pads, T, G):
    """the ticks of `cut` through the product's tick form, each checked against the model's; returns the concatenation"""
    state, pos, boxes, valid = None, 0, [], []
    ticks = list(cut) + ([0] if close_on_empty or not cut else [])
    for t, c in enumerate(ticks):
        closed = t == len(ticks) - 1
        b, v, state = live.stream_boxes_runs_host(state, clip[pos:pos + c], closed, FH, FW, pads, T, G)
        want, want_valid, (rows, dist) = cases.model_tick(clip[:pos + c], pos, closed, FH, FW, pads, T, G)
        assert np.array_equal(b, want) and np.array_equal(v, want_valid), (T, G, cut, t)
        got_rows, got_dist = live.runs_carry_words(state)
        assert np.array_equal(got_rows, rows) and got_dist == dist and state[0] == pos + c
        assert len(b) == live.new_final_count(pos, c, closed, max(T, 1))
        boxes.append(b)
        valid.append(v)
        pos += c
    return np.concatenate(boxes), np.concatenate(valid)


def test_every_cut_of_short_clips_gives_the_model_of_the_whole():
    from wav2lip_amd.face_detection import live
    rng = np.random.default_rng(2)
    for n in range(0, 8):
        for trial in range(3):
            clip = cases.clip_rects(rng.random(n) < (0.4, 0.7, 0.9)[trial], rng)
            for T, G in ((0, 0), (1, 1), (2, 0), (3, 1), (5, 2), (5, 0), (8, 100)):
                want, want_valid = cases.model(clip, FH, FW, (0, 10, 0, 0), T, G)
                for cut in _compositions(n):
                    for close_on_empty in (False, True):
                        got, got_valid = _ticks(live, clip, cut, close_on_empty, (0, 10, 0, 0), T, G)
                        assert np.array_equal(got, want) and np.array_equal(got_valid, want_valid), (clip, T, G, cut)


@pytest.mark.parametrize("T", cases.WINDOWS)
def test_the_tick_form_is_the_model_on_the_seeded_clips_cut_six_ways(T):
    from wav2lip_amd.face_detection import live
    rng = np.random.default_rng(T)
    for G in cases.HOLDS:
        for name, clip in cases.stream_clips(T, G, seed=3 + 100 * T + G):
            want, want_valid = cases.model(clip, FH, FW, cases.PADS[1], T, G)
            done = set()
            for kind in ("whole", "1", "T-1", "T", "seeded", "seeded, closed empty"):
                cut = cases.cuts(kind, len(clip), T, rng)
                if tuple(cut) in done or len(cut) > 140:
                    continue                       # a model run per tick: the long clips go frame by frame in the device test only
                done.add(tuple(cut))
                got, got_valid = _ticks(live, clip, cut[:-1] if cut[-1] == 0 and len(cut) > 1 else cut, cut[-1] == 0 and len(cut) > 1,
                                        cases.PADS[1], T, G)
                assert np.array_equal(got, want) and np.array_equal(got_valid, want_valid), (T, G, name, kind)


# ---------------------------------------------------------------- face_detect on the host path
class StubDetector:
    """get_detections_for_batch reads the rect from the frame (tests/test_streaming_live_cpu.py `_video`); a flagged frame has none"""
    precision, det_scale = "f32", 1

    def get_detections_for_batch(self, images):
        return [None if f[0, 2, 1] else _rect_of(f) for f in images]


@pytest.mark.parametrize("G", [0, 2])
def test_face_detect_applies_the_rule_and_keeps_the_references_error_without_the_keyword(G):
    from wav2lip_amd import inference
    video = _video(20, 5, 1, no_face=(0, 7, 8, 12, 19))
    rects = [None if f[0, 2, 1] else _rect_of(f) for f in video]
    for nosmooth, T in ((False, 5), (True, 0)):
        det = inference.face_detect(list(video), detector=StubDetector(), pads=[0, 10, 0, 0], nosmooth=nosmooth, batch_size=8, no_face_hold=G)
        want, valid = cases.model(rects, FH, FW, (0, 10, 0, 0), T, G)
        assert len(det) == 20 and not valid[0] and valid[1] and (valid[7] == (G > 0)) and (valid[8] == (G > 1))
        for (face, coords), w, v, f in zip(det, want, valid, video):
            if not v:
                assert face is None and coords is None
            else:
                assert tuple(coords) == tuple(w) and np.array_equal(face, f[w[0]:w[1], w[2]:w[3]])
    with pytest.raises(ValueError, match="Face not detected"):
        inference.face_detect(list(video), detector=StubDetector(), pads=[0, 10, 0, 0], nosmooth=False, batch_size=8)
    with pytest.raises(ValueError, match="Face not detected"):                   # a single (static) frame without a face
        inference.face_detect([video[7]], detector=StubDetector(), pads=[0, 10, 0, 0], nosmooth=False, batch_size=8, no_face_hold=G)


# ---------------------------------------------------------------- the packer
@pytest.fixture
def pack(monkeypatch):
    from wav2lip_amd import multiclip
    PackStubRunner.instances = []
    monkeypatch.setattr(multiclip, "BatchRunner", PackStubRunner)
    return multiclip


def _gap_job(multiclip, key, gaps, n_rows, resident=False):
    frames = np.zeros((n_rows, 12, 10, 3), np.uint8)
    for k in range(n_rows):
        frames[k, 0, 0] = (key, k, 0)
    boxes = [None if k in gaps else (1, 9, 2, 8) for k in range(n_rows)]
    rows = multiclip.rows_filelist(16 + int((n_rows - 1) * 3.2), n_rows, boxes)
    assert [r[1] is None for r in rows] == [k in gaps for k in range(n_rows)]
    if resident:
        import torch
        frames = torch.from_numpy(frames)
    return multiclip.ClipJob(key, frames, types.SimpleNamespace(shape=(80, 16 + int((n_rows - 1) * 3.2))), rows)


def test_rows_keep_a_missing_box_and_lipsync_many_delivers_those_frames_in_row_order(pack):
    rows = pack.rows_inference(100, 3, [(1, 9, 2, 8), None, (0, 4, 0, 4)], 25.)
    assert [r[1] for r in rows[:4]] == [(1, 9, 2, 8), None, (0, 4, 0, 4), (1, 9, 2, 8)] and len(rows) > 4
    # job 1 has gaps at both ends and inside, job 2 consists of gap rows only and lies between two others, job 4 is resident
    jobs = [_gap_job(pack, 1, {0, 4, 5, 10}, 11), _gap_job(pack, 2, set(range(6)), 6), _gap_job(pack, 3, {2}, 9),
            _gap_job(pack, 4, {0, 1}, 3, resident=True), _gap_job(pack, 5, set(range(2)), 2)]
    for bs, depth in ((4, 2), (3, 1), (64, 2)):
        events = []
        pack.lipsync_many(None, iter(jobs), batch_size=bs, depth=depth,
                          sink=lambda key, f: events.append((key, None if f is None else tuple(int(v) for v in f[0, 0][:2]))))
        want = []
        for key, n in ((1, 11), (2, 6), (3, 9), (4, 3), (5, 2)):
            want += [(key, (key, k)) for k in range(n)] + [(key, None)]
        assert events == want
        r = PackStubRunner.instances[-1]
        flat = [(k, fi) for b in r.batches for k, fi, box, _ in b]
        assert all(box is not None for b in r.batches for _, _, box, _ in b)      # a gap row takes no batch row
        assert flat == [(1, k) for k in range(11) if k not in {0, 4, 5, 10}] + [(3, k) for k in range(9) if k != 2] + [(4, 2)]
        assert [len(b) for b in r.batches][:-1] == [bs] * (len(r.batches) - 1)    # and the batches stay full
    got = pack.lipsync_many(None, [_gap_job(pack, 7, {0, 1, 2}, 3)], batch_size=4)  # only gap rows: no batch at all
    assert [tuple(f[0, 0][:2]) for f in got[7]] == [(7, 0), (7, 1), (7, 2)] and PackStubRunner.instances[-1].batches == []
    with pytest.raises(ValueError, match="job 9"):                                # a box that IS there is still validated
        bad = _gap_job(pack, 9, {0}, 3)
        pack.lipsync_many(None, [bad._replace(rows=[(0, None, 0), (1, (1, 90, 2, 8), 3)])], batch_size=4)


# ---------------------------------------------------------------- the streams
class HoldStubBoxes:
    """DeviceBoxes on the host with a hold: the rect of a frame is written in the frame, the finish is the product's tick form per
    carry slot (checked against the model above)"""
    instances = []

    def __init__(self, device, detector, pads, T, batch_size, hold=None):
        assert hold is not None
        self.pads, self.T, self.hold, self.state, self.launches = pads, T, hold, {}, []
        HoldStubBoxes.instances.append(self)

    def reserve(self, n_slots):
        pass

    def launch(self, items):
        from wav2lip_amd.face_detection import live
        chunks, results = [], []
        for fresh, H, W, slot, seen, closed in items:
            state = self.state.get(slot) if seen else None
            assert seen == (state[0] if state else 0)
            chunks.append([(len(fresh), np.stack(fresh))] if fresh else [])
            rects = [None if f[0, 2, 1] else _rect_of(f) for f in fresh]
            boxes, valid, self.state[slot] = live.stream_boxes_runs_host(state, rects, closed, H, W, self.pads, self.T, self.hold)
            results.append((boxes.astype(np.int32), (0, 0), valid.astype(np.int32)))
        self.launches.append(len(items))
        return dict(chunks=chunks, results=results)

    @staticmethod
    def collect(ticket):
        return ticket["results"]


@pytest.fixture
def stub(monkeypatch):
    from wav2lip_amd import streaming
    LiveStubMel.instances, StubRunner.instances, HoldStubBoxes.instances = [], [], []
    monkeypatch.setattr(streaming, "BatchRunner", StubRunner)
    monkeypatch.setattr(streaming, "DeviceMel", LiveStubMel)
    monkeypatch.setattr(streaming, "DeviceBoxes", HoldStubBoxes)
    return streaming


def _run_streams(stub, G, per_tick, batch_size=8, flush=False):
    """three live streams (one clean, one with single misses, one that starts and ends without a face and has a long miss) and a
    stream opened with its frames and None among its boxes, fed `per_tick` frames and 640 * per_tick samples per tick"""
    from wav2lip_amd import multiclip
    n = 16000 * 2
    videos = {"clean": _video(40, 1, 1), "blink": _video(33, 2, 2, no_face=(7, 20, 21)),
              "turns": _video(48, 3, 3, no_face=(0, 1, 2) + tuple(range(10, 25)) + (46, 47))}
    fixed = _frames(5, shape=(FH, FW), tag=9)
    fixed_boxes = [(1, 9, 2, 8), None, (2, 10, 2, 8), None, None]
    launched, events, out = [], [], {k: [] for k in list(videos) + ["fixed"]}

    def sink(key, frame):
        events.append((key, frame is None))
        if frame is not None:
            out[key].append(frame)

    ls = stub.LipsyncStreams(None, batch_size=batch_size, on_batch=launched.append, sink=sink, detector=object(), pads=(0, 10, 0, 0),
                             smooth_T=5, no_face_hold=G)
    ls.open("fixed", fixed, fixed_boxes)
    for k in videos:
        ls.open_live(k)
    x = _audio(n)
    ticks = (n + 640 * per_tick - 1) // (640 * per_tick)
    for t in range(ticks):
        for k in out:
            ls.feed(k, x[t * 640 * per_tick:(t + 1) * 640 * per_tick])
            if t == ticks - 1:
                ls.close(k)
            if k in videos and t * per_tick < len(videos[k]):
                ls.feed_frames(k, list(videos[k][t * per_tick:(t + 1) * per_tick]))
                if (t + 1) * per_tick >= len(videos[k]):
                    ls.close_video(k)
        ls.step(flush=flush)
    ls.drain()
    assert not ls._streams and ls.errors == {}
    want = {}
    for k, v in videos.items():
        rects = [None if f[0, 2, 1] else _rect_of(f) for f in v]
        boxes, valid = cases.model(rects, FH, FW, (0, 10, 0, 0), 5, G)
        want[k] = multiclip.rows_inference(1 + n // 200, len(v), [tuple(b) if ok else None for b, ok in zip(boxes, valid)], 25.)
    want["fixed"] = multiclip.rows_inference(1 + n // 200, 5, fixed_boxes, 25.)
    frames = dict(videos, fixed=fixed)
    return ls, out, launched, events, want, frames


@pytest.mark.parametrize("G,per_tick", [(0, 1), (0, 3), (2, 1), (2, 7), (20, 3)])
def test_streams_go_on_over_frames_without_a_face_and_deliver_them_unchanged_in_order(stub, G, per_tick):
    ls, out, launched, events, want, frames = _run_streams(stub, G, per_tick)
    rec = {k: [] for k in out}
    for batch, _ in StubRunner.instances[-1].batches:
        for key, _, box, _ in batch:                      # (a live row's frame index is relative to its chunk)
            assert box is not None
            rec[key].append(box)
    for k, rows in want.items():
        assert len(out[k]) == len(rows) > 0 and [e for e in events if e[0] == k] == [(k, False)] * len(rows) + [(k, True)]
        for f, (fi, box, _) in zip(out[k], rows):
            assert np.array_equal(f, frames[k][fi])                               # gap rows: the input frame's bytes
        assert rec[k] == [box for _, box, _ in rows if box is not None]           # only the boxed rows ran, with the rule's boxes
        boxed = [i for i, r in enumerate(rows) if r[1] is not None]
        assert [r for b in launched for kk, r in dict.fromkeys(b) if kk == k] == boxed      # on_batch sees boxed rows only
    assert any(r[1] is None for r in want["turns"]) and any(r[1] is None for r in want["fixed"])
    if G == 20:
        assert all(r[1] is not None for r in want["blink"])                       # the hold covers a blink
    assert HoldStubBoxes.instances[-1].hold == G


def test_the_batch_sequence_repeats_and_only_boxed_rows_fill_batches(stub):
    first = _run_streams(stub, 1, 3)
    again = _run_streams(stub, 1, 3)
    assert first[2] == again[2] and first[3] == again[3] and len(first[2]) > 3
    sizes = [pad for _, pad in StubRunner.instances[-1].batches]
    assert set(sizes) <= {8}                                                      # bucketing counts boxed rows: full batches of 8
    assert all(len(dict.fromkeys(b)) <= 8 for b in first[2])


def test_without_the_keyword_a_missing_box_is_refused_at_open():
    from wav2lip_amd import streaming
    ls = streaming.LipsyncStreams(None)
    with pytest.raises(ValueError, match="no_face_hold"):
        ls.open("k", _frames(2, shape=(FH, FW)), [(1, 9, 2, 8), None])


# ---------------------------------------------------------------- arguments and command lines
@pytest.mark.parametrize("bad", [-1, 251, 2.0, "3", True])
def test_a_hold_that_is_no_integer_in_range_is_a_value_error_before_any_device_work(bad):
    from wav2lip_amd import inference, multiclip, streaming
    from wav2lip_amd.face_detection import many

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("the detector was used")

    with pytest.raises(ValueError, match="no_face_hold"):
        many.check_hold(bad)
    with pytest.raises(ValueError, match="no_face_hold"):
        inference.face_detect([np.zeros((FH, FW, 3), np.uint8)], detector=Untouched(), pads=[0, 0, 0, 0], nosmooth=True, batch_size=1,
                              no_face_hold=bad)
    with pytest.raises(ValueError, match="no_face_hold"):
        next(many.detect_many(Untouched(), [many.DetectJob(0, [np.zeros((FH, FW, 3), np.uint8)])], no_face_hold=bad))
    with pytest.raises(ValueError, match="no_face_hold"):
        streaming.LipsyncStreams(None, no_face_hold=bad)
    assert multiclip is not None


def test_the_accepted_holds():
    from wav2lip_amd.face_detection import many
    assert [many.check_hold(g) for g in (None, 0, 1, 250, np.int32(7))] == [None, 0, 1, 250, 7]
    assert many.MAX_HOLD == 250 and isinstance(many.check_hold(np.int64(3)), int)


def test_the_flag_is_absent_by_default_on_the_three_commands_and_takes_0_to_250(capsys):
    from wav2lip_amd import gen_videos_from_filelist, inference, streaming
    base = {
        "inference": (inference.build_cli_parser(), ["--checkpoint_path", "c", "--face", "f", "--audio", "a"]),
        "streaming": (streaming.build_parser(), ["--checkpoint_path", "c", "--face", "f", "--audio", "a"]),
        "filelist": (gen_videos_from_filelist.build_main_parser(), ["--filelist", "l", "--results_dir", "r", "--data_root", "d",
                                                                     "--checkpoint_path", "c"]),
    }
    for name, (p, argv) in base.items():
        assert p.parse_args(argv).no_face_hold is None, name
        assert [p.parse_args(argv + ["--no_face_hold", g]).no_face_hold for g in ("0", "4", "250")] == [0, 4, 250]
        for bad in ("-1", "251", "x", "1.5"):
            with pytest.raises(SystemExit):
                p.parse_args(argv + ["--no_face_hold", bad])
        # independent of the other additions
        extra = ["--precision", "bf16", "--face_det_precision", "bf16", "--face_det_scale", "2", "--blend_feather", "4", "--no_face_hold", "2"]
        a = p.parse_args(argv + extra + (["--packed_face_det"] if name == "filelist" else []))
        assert (a.no_face_hold, a.precision, a.face_det_scale, a.blend_feather) == (2, "bf16", 2, 4)
    capsys.readouterr()
    # the reference's surfaces stay the reference's
    assert not hasattr(inference.build_parser().parse_args(base["inference"][1]), "no_face_hold")
    assert not hasattr(gen_videos_from_filelist.cli_parser.parse_args(base["filelist"][1]), "no_face_hold")
    assert inference.args.no_face_hold is None
    assert inference._hold_kw(None) == {} and inference._hold_kw(3) == {"no_face_hold": 3}


def test_a_sharded_inference_run_refuses_the_flag_up_front(monkeypatch, tmp_path):
    from wav2lip_amd import inference, sharding
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sharding, "init_from_env", lambda *a, **k: pytest.fail("the process group was initialised"))
    with pytest.raises(ValueError, match="--no_face_hold runs on one GPU"):
        inference.main(["--checkpoint_path", "c", "--face", str(tmp_path / "f.avi"), "--audio", "a.wav", "--no_face_hold", "0"])
