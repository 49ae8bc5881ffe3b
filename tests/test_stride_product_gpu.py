"""Key-frame face detection (`det_stride`) through the product on the device, with synthetic weights on the seeded
filelist clips: a clean clip, c4 (its frame 7 has no face and is no key frame at N = 2 or 3), a copy of c4 whose key frame 6 is
grey too - a missed key - and the last two joined end to end.  `detect_many(det_stride=N)` and `face_detect(det_stride=N)` against
the numpy model of tests/_stride_cases.py applied to the detector's own rects of the key frames, followed by the existing finish
models; the number of detector batches; the inference command.  With N = 1 or the keyword absent everything is what it was."""
import numpy as np
import pytest
import torch

import _noface_cases as noface
import _span_cases as spans_model
import _stride_cases as cases
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu

PADS = (0, 10, 0, 0)
DET_BATCH = 8
SCENE = 0.3
NEW = "w2l_face_rects_expand_segments"
NO_FACE = 'Face not detected! Ensure the video contains a face in all the frames.'
STRIDES = (2, 3)


@pytest.fixture(scope="module")
def env(cuda):
    """the detector, the clips and - computed once - the detector's rects of every frame of every clip"""
    from wav2lip_amd import face_detection, inference
    det = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device=str(cuda),
                                       state_dict=synth.s3fd_state_dict())
    src = synth.filelist_clips()
    grey = src["c4"][0].copy()
    grey[6] = src["c4"][0][7]                     # the clip's grey frame: key frame 6 has no face either
    clips = {"c1": src["c1"][0][:20], "c4": src["c4"][0], "kg": grey, "joined": np.concatenate([grey, src["c1"][0][:20]])}
    rects = {k: inference._detect_rects(list(f), det, DET_BATCH) for k, f in clips.items()}
    assert [i for i, r in enumerate(rects["c4"]) if r is None] == [7] and [i for i, r in enumerate(rects["kg"]) if r is None] == [6, 7]
    assert None not in rects["c1"] and rects["joined"] == rects["kg"] + rects["c1"]
    return dict(det=det, clips=clips, rects=rects, pcm=src["c4"][1])


def _expand(key_rects, n, N):
    """the model's expansion of one segment: [rect or None per key frame] -> [rect or None per frame]"""
    flags = np.array([r is not None for r in key_rects], np.int64)
    arr = np.array([r if r is not None else (0, 0, 0, 0) for r in key_rects], np.int64).reshape(-1, 4)
    return cases.filled_rects(*cases.model(arr, flags, n, N))


def _filled(rects, shots, N):
    """the per-frame rects a clip has at stride N, from the detector's per-frame rects: the key frames of every shot, expanded"""
    out = []
    for a, b in shots:
        out += _expand([rects[a + int(i)] for i in cases.key_positions(b - a, N)], b - a, N)
    return out


def _tracked(det, frames, shots, N, track="largest"):
    """`_filled` under a track: the existing single-clip track over the key frames of every shot alone, expanded"""
    from wav2lip_amd import inference
    from wav2lip_amd.face_detection.track import check_track
    out = []
    for a, b in shots:
        keys = [frames[a + int(i)] for i in cases.key_positions(b - a, N)]
        out += _expand(inference._track_rects(keys, det, DET_BATCH, check_track(track)), b - a, N)
    return out


def _strict(filled, shots, H, W, T=5):
    """today's strict finish per shot: the boxes, or None when a frame has no face"""
    if any(r is None for r in filled):
        return None
    return np.concatenate([noface.model(filled[a:b], H, W, PADS, T, 0)[0] for a, b in shots])


def _held(filled, shots, H, W, G, T=5):
    out = []
    for a, b in shots:
        boxes, valid = noface.model(filled[a:b], H, W, PADS, T, G)
        out += [tuple(int(v) for v in g) if ok else None for g, ok in zip(boxes, valid)]
    return out


def _spanned(filled, shots, H, W, spans, T=5):
    """(boxes per frame or None, [(a, b)]): the span model and then the run model, shot by shot"""
    boxes, kept = [], []
    for a, b in shots:
        flags = np.array([r is not None for r in filled[a:b]], np.int64)
        arr = np.array([r if r is not None else (0, 0, 0, 0) for r in filled[a:b]], np.int64).reshape(-1, 4)
        rects_out, flags_out, rows, status = spans_model.model(arr, flags, *spans)
        got, valid = noface.model(spans_model.filled_rects(rects_out, flags_out), H, W, PADS, T, 0)
        boxes += [tuple(int(v) for v in g) if ok else None for g, ok in zip(got, valid)]
        kept += [(a + int(f), a + int(f + L)) for f, L, _, _ in rows[:status[1]]]
    return boxes, kept


def _tuples(boxes):
    return [b if b is None else tuple(int(v) for v in b) for b in boxes]


def _forms(cuda, clips, names):
    """the three ways a group comes in: host lists, device tensors, and every clip alone on the host path"""
    from wav2lip_amd import face_detection
    return (([face_detection.DetectJob(k, list(clips[k])) for k in names], {}),
            ([face_detection.DetectJob(k, torch.from_numpy(clips[k]).to(cuda)) for k in names], {}),
            ([face_detection.DetectJob(k, list(clips[k])) for k in names], dict(max_group_bytes=1)))


def _spy(monkeypatch):
    from wav2lip_amd import _lib
    lib, calls = _lib.load(), []
    fn = getattr(lib, NEW)
    monkeypatch.setattr(lib, NEW, lambda *a: calls.append(a) or fn(*a))
    return calls


# ---------------------------------------------------------------- detection
@pytest.mark.parametrize("N", STRIDES)
def test_detect_many_and_face_detect_give_the_model_on_the_rects_of_the_key_frames(cuda, env, monkeypatch, N):
    from wav2lip_amd import face_detection, inference
    from wav2lip_amd.face_detection import many
    det, clips = env["det"], env["clips"]
    names = ["c1", "c4", "kg"]
    H, W = clips["c1"].shape[1:3]
    filled = {k: _filled(env["rects"][k], [(0, 20)], N) for k in names}
    # c4's frame without a face is no key frame: it takes an interpolated rect; a missed key leaves 2N - 1 frames without one
    assert None not in filled["c1"] and None not in filled["c4"]
    assert [i for i, r in enumerate(filled["kg"]) if r is None] == list(range(6 - N + 1, 6 + N))
    want = {k: _strict(filled[k], [(0, 20)], H, W) for k in names}
    calls = _spy(monkeypatch)
    for jobs, kw in _forms(cuda, clips, names):
        del calls[:]
        out = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, det_stride=N, **kw))
        assert [k for k, _, _ in out] == names
        for k, boxes, error in out:
            if want[k] is None:
                assert boxes is None and error == NO_FACE, (k, kw)
            else:
                assert error is None and boxes.dtype == np.int64 and np.array_equal(boxes, want[k]), (k, kw)
        assert len(calls) == (0 if kw else 1)              # one launch for the group; the host path fills on the host
    for k in names:
        if want[k] is None:
            with pytest.raises(ValueError, match="Face not detected"):
                inference.face_detect(list(clips[k]), detector=det, pads=list(PADS), nosmooth=False, batch_size=DET_BATCH, det_stride=N)
            continue
        got = inference.face_detect(list(clips[k]), detector=det, pads=list(PADS), nosmooth=False, batch_size=DET_BATCH, det_stride=N)
        assert np.array_equal(np.array([c for _, c in got]), want[k]), k
        for (face, c), f in zip(got, clips[k]):
            assert np.array_equal(face, f[c[0]:c[1], c[2]:c[3]])
    # another window and none: the finish is today's on the expanded rects
    for T in (0, 3):
        (_, boxes, _), = face_detection.detect_many(det, [face_detection.DetectJob("c4", list(clips["c4"]))], pads=PADS, T=T,
                                                    batch_size=DET_BATCH, det_stride=N)
        assert np.array_equal(boxes, _strict(filled["c4"], [(0, 20)], H, W, T)), T
    # one frame, two frames and an empty clip
    jobs = [face_detection.DetectJob("one", list(clips["c1"][:1])), face_detection.DetectJob("none", []),
            face_detection.DetectJob("two", list(clips["c1"][:2]))]
    (_, one, e1), (_, none, e0), (_, two, e2) = face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, det_stride=N)
    assert (e1, e0, e2) == (None,) * 3 and none.shape == (0, 4)
    assert np.array_equal(one, noface.model(env["rects"]["c1"][:1], H, W, PADS, 5, 0)[0])
    assert np.array_equal(two, noface.model(env["rects"]["c1"][:2], H, W, PADS, 5, 0)[0])


@pytest.mark.parametrize("N", STRIDES)
def test_with_no_face_hold_the_last_rect_is_held_over_the_frames_a_missed_key_leaves(cuda, env, N):
    from wav2lip_amd import face_detection, inference
    from wav2lip_amd.face_detection import many
    det, clips = env["det"], env["clips"]
    names = ["c1", "kg"]
    H, W = clips["c1"].shape[1:3]
    for G in (1, 2 * N - 1):
        want = {k: _held(_filled(env["rects"][k], [(0, 20)], N), [(0, 20)], H, W, G) for k in names}
        assert (None in want["kg"]) == (G < 2 * N - 1) and None not in want["c1"]
        for jobs, kw in _forms(cuda, clips, names):
            out = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, no_face_hold=G, det_stride=N, **kw))
            for k, boxes, error in out:
                assert error is None and type(boxes) is many.RunBoxes and _tuples(boxes) == want[k], (k, G, kw)
        got = inference.face_detect(list(clips["kg"]), detector=det, pads=list(PADS), nosmooth=False, batch_size=DET_BATCH, no_face_hold=G,
                                    det_stride=N)
        assert _tuples([c for _, c in got]) == want["kg"], G


@pytest.mark.parametrize("N", STRIDES)
def test_with_face_track_the_track_steps_from_key_frame_to_key_frame(cuda, env, N):
    from wav2lip_amd import face_detection, inference
    det, clips = env["det"], env["clips"]
    names = ["c1", "kg"]
    H, W = clips["c1"].shape[1:3]
    filled = {k: _tracked(det, clips[k], [(0, 20)], N) for k in names}
    want = {k: _held(filled[k], [(0, 20)], H, W, 1) for k in names}
    for jobs, kw in _forms(cuda, clips, names):
        out = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, no_face_hold=1, face_track="largest",
                                              det_stride=N, **kw))
        for k, boxes, error in out:
            assert error is None and _tuples(boxes) == want[k], (k, kw)
        (_, boxes, error), _ = face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, face_track="largest", det_stride=N,
                                                          **kw)
        assert error is None and np.array_equal(boxes, _strict(filled["c1"], [(0, 20)], H, W)), kw
    got = inference.face_detect(list(clips["c1"]), detector=det, pads=list(PADS), nosmooth=False, batch_size=DET_BATCH, face_track="largest",
                                det_stride=N)
    assert np.array_equal(np.array([c for _, c in got]), _strict(filled["c1"], [(0, 20)], H, W))


@pytest.mark.parametrize("N", STRIDES)
def test_with_track_spans_a_missed_key_is_bridged_iff_the_bridge_reaches_over_it(cuda, env, N):
    from wav2lip_amd import face_detection
    from wav2lip_amd.face_detection import many
    det, clips = env["det"], env["clips"]
    names = ["c1", "kg"]
    H, W = clips["c1"].shape[1:3]
    for bridge in (2 * N - 1, 2 * N - 2):
        spans = face_detection.TrackSpans(bridge, 4, 0)
        for track in (None, "largest"):
            if track is not None and bridge != 2 * N - 1:
                continue
            tkw = {} if track is None else {"face_track": track}
            filled = {k: _filled(env["rects"][k], [(0, 20)], N) if track is None else _tracked(det, clips[k], [(0, 20)], N) for k in names}
            want = {k: _spanned(filled[k], [(0, 20)], H, W, spans) for k in names}
            assert want["kg"][1] == ([(0, 20)] if bridge == 2 * N - 1 else [(0, 6 - N + 1), (6 + N, 20)]) and want["c1"][1] == [(0, 20)]
            for jobs, kw in _forms(cuda, clips, names):
                out = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, track_spans=spans, det_stride=N,
                                                      **tkw, **kw))
                for k, boxes, error in out:
                    assert error is None and isinstance(boxes, many.SpanBoxes) and boxes.spans == want[k][1], (k, bridge, kw)
                    assert _tuples(boxes) == want[k][0], (k, bridge, kw)


@pytest.mark.parametrize("N", STRIDES)
def test_with_scene_cuts_the_keys_are_per_shot_of_two_clips_joined_end_to_end(cuda, env, N):
    from wav2lip_amd import face_detection, inference
    from wav2lip_amd.face_detection.scene import SceneCuts
    det, frames = env["det"], env["clips"]["joined"]
    H, W = frames.shape[1:3]
    _, shots = inference._shot_rects(list(frames), det, DET_BATCH, None, SceneCuts(SCENE))
    assert shots == [(0, 6), (6, 8), (8, 40)]                                   # a change to or from grey is a cut (the join is none at 0.3)
    filled = _filled(env["rects"]["joined"], shots, N)
    assert filled[5] is not None and filled[8] is not None                      # the last frame of a shot and the first of the next are keys
    spans = face_detection.TrackSpans(1, 4, 0)
    want_held, want_spans = _held(filled, shots, H, W, 1), _spanned(_tracked(det, frames, shots, N), shots, H, W, spans)
    for job, kw in ((face_detection.DetectJob("j", list(frames)), {}), (face_detection.DetectJob("j", torch.from_numpy(frames).to(cuda)), {}),
                    (face_detection.DetectJob("j", list(frames)), dict(max_group_bytes=1))):
        jobs = [face_detection.DetectJob("c1", list(env["clips"]["c1"])), job]
        (_, first, _), (key, boxes, error) = face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, no_face_hold=1,
                                                                        scene_cuts=SCENE, det_stride=N, **kw)
        assert key == "j" and error is None and _tuples(boxes) == want_held, kw
        assert first.valid.all()
        _, (key, boxes, error) = face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, track_spans=spans,
                                                            scene_cuts=SCENE, face_track="largest", det_stride=N, **kw)
        assert error is None and boxes.spans == want_spans[1] and _tuples(boxes) == want_spans[0], kw
        _, (key, boxes, error) = face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, scene_cuts=SCENE, det_stride=N,
                                                            **kw)
        assert boxes is None and error == NO_FACE, kw                            # strict: the grey shot has no face
    got = inference.face_detect(list(frames), detector=det, pads=list(PADS), nosmooth=False, batch_size=DET_BATCH, no_face_hold=1,
                                scene_cuts=SCENE, det_stride=N)
    assert _tuples([c for _, c in got]) == want_held


@pytest.mark.parametrize("N", STRIDES)
def test_with_all_faces_the_tracks_tolerate_the_missed_keys_the_span_rule_bridges(cuda, env, N):
    from wav2lip_amd import face_detection
    from wav2lip_amd.face_detection.faces import FaceSpans, host_all_tracks
    from wav2lip_amd.face_detection.track import iou_q8
    det, clips = env["det"], env["clips"]
    names = ["c1", "kg"]
    H, W = clips["c1"].shape[1:3]
    faces = face_detection.AllFaces(2, 4, 0.25)
    keys = cases.key_positions(20, N).tolist()
    cands = {k: det.get_candidates_for_batch(np.array([clips[k][i] for i in keys]), faces.cands) for k in names}
    for bridge in (2 * N - 1, 2 * N - 2):
        spans = face_detection.TrackSpans(bridge, 4, 0)
        L = max(0, (bridge + 1) // N - 1)
        assert L == (1 if bridge == 2 * N - 1 else 0)
        want = {}
        for k in names:
            tracks = []
            for t, key_rects in enumerate(host_all_tracks(cands[k], faces.max_faces, iou_q8(faces.min_iou), L)):
                boxes, kept = _spanned(_expand(key_rects, 20, N), [(0, 20)], H, W, spans)
                tracks += [(t, a, b, np.array(boxes[a:b], np.int64)) for a, b in kept]
            want[k] = sorted(tracks, key=lambda s: (s[1], s[0]))
        assert (0, 0, 20) in [w[:3] for w in want["c1"]]
        assert [w[1:3] for w in want["kg"] if w[0] == 0] == ([(0, 20)] if bridge == 2 * N - 1 else [(0, 6 - N + 1), (6 + N, 20)])
        for jobs, kw in _forms(cuda, clips, names):
            out = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, track_spans=spans, all_faces=faces,
                                                  det_stride=N, **kw))
            for k, res, error in out:
                assert error is None and isinstance(res, FaceSpans) and len(res) == 20, (k, kw)
                assert [(t.slot, t.a, t.b) for t in res.tracks] == [w[:3] for w in want[k]], (k, bridge, kw)
                for t, w in zip(res.tracks, want[k]):
                    assert np.array_equal(t.boxes, w[3]), (k, bridge, kw)


def test_stride_1_and_the_keyword_absent_give_todays_bytes_without_the_new_launch(cuda, env, monkeypatch):
    from wav2lip_amd import face_detection, inference
    from wav2lip_amd.face_detection import many
    det, clips = env["det"], env["clips"]
    names = ["c1", "c4", "kg"]
    H, W = clips["c1"].shape[1:3]
    calls = _spy(monkeypatch)
    jobs = [face_detection.DetectJob(k, list(clips[k])) for k in names]
    for kw in ({}, dict(no_face_hold=1), dict(face_track="largest", no_face_hold=0), dict(track_spans=face_detection.TrackSpans(1, 4, 0))):
        absent = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, **kw))
        for value in (1, None):
            one = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, det_stride=value, **kw))
            for (k, a, ea), (_, b, eb) in zip(absent, one):
                assert ea == eb and type(a) is type(b), (k, kw)
                if a is not None:
                    a, b = (a, b) if isinstance(a, np.ndarray) else (a.boxes, b.boxes)
                    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (k, kw)
    assert absent[0][1].spans == [(0, 20)]
    plain = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH))
    assert np.array_equal(plain[0][1], noface.model(env["rects"]["c1"], H, W, PADS, 5, 0)[0]) and plain[1][1:] == (None, NO_FACE)
    got = inference.face_detect(list(clips["c1"]), detector=det, pads=list(PADS), nosmooth=False, batch_size=DET_BATCH, det_stride=1)
    assert np.array_equal(np.array([c for _, c in got]), plain[0][1])
    assert calls == []


@pytest.mark.parametrize("N", STRIDES)
def test_the_detector_sees_the_batches_of_the_key_frames_only(cuda, env, monkeypatch, N):
    from wav2lip_amd import face_detection
    det, clips = env["det"], env["clips"]
    names = ["c1", "c4", "kg"]
    seen, fn = [], det.rects_for_rows
    monkeypatch.setattr(det, "rects_for_rows", lambda frames, B, *a: seen.append(B) or fn(frames, B, *a))
    jobs = [face_detection.DetectJob(k, torch.from_numpy(clips[k]).to(cuda)) for k in names]
    list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH))
    frames = sum(len(clips[k]) for k in names)
    assert seen == [DET_BATCH] * -(-frames // DET_BATCH)
    del seen[:]
    list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, det_stride=N))
    keys = sum(cases.n_keys(len(clips[k]), N) for k in names)
    assert keys < frames and seen == [DET_BATCH] * -(-keys // DET_BATCH)


# ---------------------------------------------------------------- the launches of a group
HIST, CUTS, TRACK, ALL, SPAN = "w2l_frame_hist_rows", "w2l_scene_cuts", "w2l_face_track_segments", "w2l_face_tracks_all_segments", \
    "w2l_face_spans_segments"
SEGMENTS, RUNS = "w2l_face_boxes_segments", "w2l_face_boxes_runs"
# option combination -> the library entries of one group in launch order (the module text of face_detection/many.py), at stride 1
# and at stride 2: there the one expand launch sits between the track, if any, and what reads the full arenas
LAUNCHES = {
    "default": ([SEGMENTS], [NEW, SEGMENTS]),
    "hold": ([RUNS], [NEW, RUNS]),
    "track": ([TRACK, SEGMENTS], [TRACK, NEW, SEGMENTS]),
    "scene": ([HIST, CUTS, SEGMENTS], [HIST, CUTS, NEW, SEGMENTS]),
    "track+scene": ([HIST, CUTS, TRACK, SEGMENTS], [HIST, CUTS, TRACK, NEW, SEGMENTS]),
    "spans": ([SPAN, RUNS], [NEW, SPAN, RUNS]),
    "spans+all_faces": ([ALL, SPAN, RUNS], [ALL, NEW, SPAN, RUNS]),
}


def test_every_option_keeps_its_launch_sequence(cuda, env, monkeypatch):
    """one group of three host clips under every option combination, at stride 1 and 2: the library entries in the order of
    LAUNCHES, every detector batch before the finish, and exactly one `.cpu()` - read at the library and at torch, not at the
    Python that sits between them"""
    from wav2lip_amd import _lib, face_detection
    det, clips = env["det"], env["clips"]
    options = {
        "default": {},
        "hold": dict(no_face_hold=1),
        "track": dict(face_track="largest"),
        "scene": dict(scene_cuts=SCENE),
        "track+scene": dict(face_track="largest", scene_cuts=SCENE),
        "spans": dict(track_spans=face_detection.TrackSpans(1, 4, 0)),
        "spans+all_faces": dict(track_spans=face_detection.TrackSpans(1, 4, 0), all_faces=face_detection.AllFaces(2, 4, 0.25)),
    }
    assert list(options) == list(LAUNCHES)
    lib, log, copies = _lib.load(), [], []

    def spied(name, fn):
        return lambda *a, **k: log.append(name) or fn(*a, **k)

    for name in (HIST, CUTS, TRACK, ALL, NEW, SPAN, SEGMENTS, RUNS):
        monkeypatch.setattr(lib, name, spied(name, getattr(lib, name)))
    for name in ("rects_for_rows", "cands_for_rows"):
        monkeypatch.setattr(det, name, spied("batch", getattr(det, name)))
    to_host = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: copies.append(1) or to_host(t, *a, **k))
    jobs = [face_detection.DetectJob(k, list(clips[k])) for k in ("c1", "c4", "kg")]
    for which, kw in options.items():
        for N, want in zip((None, 2), LAUNCHES[which]):
            del log[:], copies[:]
            out = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, det_stride=N, **kw))
            assert [k for k, _, _ in out] == ["c1", "c4", "kg"]
            assert [e for e in log if e != "batch"] == want, (which, N)
            assert len(copies) == 1, (which, N)                # the group's one copy back
            assert log.index(want[-1]) > len(log) - 1 - log[::-1].index("batch")       # every batch is queued before the finish
            if "scene" in which and N is None:                 # the cut flags cross while the detector runs
                assert log.index(CUTS) < log.index("batch") < log.index(want[-1]), which


# ---------------------------------------------------------------- the command
def test_the_inference_command_writes_a_video_whose_boxes_are_the_models(cuda, env, tmp_path, monkeypatch):
    from scipy.io import wavfile
    from wav2lip_amd import container, inference, models
    from wav2lip_amd.face_detection import api
    tmp = str(tmp_path)
    torch.save(synth.s3fd_state_dict(), tmp + "/s3fd.pth")
    monkeypatch.setattr(api, "DEFAULT_WEIGHTS", tmp + "/s3fd.pth")
    monkeypatch.setattr(inference, "args", inference.args)        # main() replaces the module-level args
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    frames = env["clips"]["c4"]
    H, W = frames.shape[1:3]
    container.write_avi(tmp + "/c4.avi", frames, 25)
    wavfile.write(tmp + "/a.wav", 16000, env["pcm"][:, 0])
    sd = synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.Wav2Lip().state_dict().items()}, seed=0)
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}, "optimizer": None, "global_step": 7, "global_epoch": 1},
               tmp + "/ckpt.pth")
    argv = ["--checkpoint_path", tmp + "/ckpt.pth", "--face", tmp + "/c4.avi", "--audio", tmp + "/a.wav", "--wav2lip_batch_size", "8",
            "--face_det_batch_size", str(DET_BATCH)]
    with pytest.raises(ValueError, match="Face not detected"):                 # every frame is looked at: frame 7 has no face
        inference.main(argv + ["--outfile", tmp + "/none.avi"])
    returned, fn = [], inference.face_detect
    monkeypatch.setattr(inference, "face_detect", lambda *a, **k: returned.append((k, fn(*a, **k))) or returned[-1][1])
    out = inference.main(argv + ["--outfile", tmp + "/s2.avi", "--face_det_stride", "2"])
    got = container.read_avi(tmp + "/s2.avi")["frames"]
    assert len(got) == len(out) >= 18 and np.array_equal(got, np.stack(out))
    assert all(not np.array_equal(got[i], frames[i % 20]) for i in range(len(got)))          # frame 7 is pasted too: its box is interpolated
    (kw, det), = returned
    assert kw["det_stride"] == 2
    n = len(det)                                           # the command cuts the clip to its mel chunks first (inference.py:244): 19 frames
    assert n == len(out) == 19
    assert np.array_equal(np.array([c for _, c in det]), _strict(_filled(env["rects"]["c4"][:n], [(0, n)], 2), [(0, n)], H, W))
    boxed = inference.main(argv + ["--outfile", tmp + "/box.avi", "--face_det_stride", "2", "--box", "10", "100", "20", "120"])
    assert len(returned) == 1 and len(boxed) == len(out)                       # --box: no detection, the flag is irrelevant
