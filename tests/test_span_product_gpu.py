"""The face spans of finished clips (`track_spans`) through the product on the device, with synthetic weights on the
seeded filelist clips: c4 with frames 0, 3, 4, 7, 18 and 19 grey - under bridge 1 and min_len 4 a dropped span [1, 3), a span
[5, 18) bridged over frame 7 and a trailing miss - a clean clip, and the two joined end to end.  `detect_many(track_spans=...)`
against the numpy models of tests/_span_cases.py and tests/_noface_cases.py on the detector's own rects; the real-video scoring
command on AVIs against `lse_like(..., first=a)` per span.  With the keyword absent everything is what it was."""
import contextlib
import io

import numpy as np
import pytest
import torch

import _noface_cases as noface
import _span_cases as cases
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu

PADS = (0, 10, 0, 0)
DET_BATCH = 8
GREY = (0, 3, 4, 7, 18, 19)
B, M = 1, 4
SCENE = 0.3


@pytest.fixture(scope="module")
def env(cuda):
    """the detector, the clips and - computed once - the detector's rects of every clip"""
    from wav2lip_amd import face_detection, inference
    det = face_detection.FaceAlignment(face_detection.LandmarksType._2D, flip_input=False, device=str(cuda),
                                       state_dict=synth.s3fd_state_dict())
    src = synth.filelist_clips()
    grey = src["c4"][0].copy()
    for k in GREY:
        grey[k] = src["c4"][0][7]                 # the clip's grey frame
    clips = {"c4g": grey, "c1": src["c1"][0][:20], "joined": np.concatenate([grey, src["c1"][0][:20]])}
    rects = {k: inference._detect_rects(list(f), det, DET_BATCH) for k, f in clips.items()}
    assert [i for i, r in enumerate(rects["c4g"]) if r is None] == list(GREY) and None not in rects["c1"]
    return dict(det=det, clips=clips, rects=rects, src=src)


def _want(rects, shots, H, W, spans, T=5):
    """(boxes per frame or None, [(a, b)]) of a clip from its rects: the span model and then the run model, shot by shot"""
    boxes, kept = [], []
    for a, b in shots:
        flags = np.array([r is not None for r in rects[a:b]], np.int64)
        arr = np.array([r if r is not None else (0, 0, 0, 0) for r in rects[a:b]], np.int64).reshape(-1, 4)
        rects_out, flags_out, rows, status = cases.model(arr, flags, *spans)
        got, valid = noface.model(cases.filled_rects(rects_out, flags_out), H, W, PADS, T, 0)
        boxes += [tuple(int(v) for v in g) if ok else None for g, ok in zip(got, valid)]
        kept += [(a + int(f), a + int(f + L)) for f, L, _, _ in rows[:status[1]]]
    return boxes, kept


def _got(boxes):
    return [b if b is None else tuple(int(v) for v in b) for b in boxes]


# ---------------------------------------------------------------- detection
@pytest.mark.parametrize("track", [None, "largest"])
def test_detect_many_gives_the_models_on_the_detectors_rects(cuda, env, track):
    from wav2lip_amd import face_detection, inference
    from wav2lip_amd.face_detection import many
    from wav2lip_amd.face_detection.track import check_track
    det, clips = env["det"], env["clips"]
    names = ["c4g", "c1", "joined"]
    spans = face_detection.TrackSpans(B, M, 0)
    tkw = {} if track is None else {"face_track": track}
    rects = env["rects"] if track is None else {k: inference._track_rects(list(clips[k]), det, DET_BATCH, check_track(track)) for k in names}
    want = {k: _want(rects[k], [(0, len(clips[k]))], clips[k].shape[1], clips[k].shape[2], spans) for k in names}
    if track is None:                                      # a dropped span, a bridged span and a trailing miss; then the second clip
        assert want["c4g"][1] == [(5, 18)] and want["c1"][1] == [(0, 20)] and want["joined"][1] == [(5, 18), (20, 40)]
        assert [b is None for b in want["c4g"][0]] == [not 5 <= i < 18 for i in range(20)]
    for jobs, kw in (([face_detection.DetectJob(k, list(clips[k])) for k in names], {}),
                     ([face_detection.DetectJob(k, torch.from_numpy(clips[k]).to(cuda)) for k in names], {}),
                     ([face_detection.DetectJob(k, list(clips[k])) for k in names], dict(max_group_bytes=1))):
        out = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, track_spans=spans, **tkw, **kw))
        assert [k for k, _, _ in out] == names and all(e is None for _, _, e in out)
        for k, boxes, _ in out:
            assert isinstance(boxes, many.SpanBoxes) and len(boxes) == len(clips[k]) and boxes.boxes.dtype == np.int64
            assert boxes.spans == want[k][1], (k, kw)
            assert _got(boxes) == want[k][0], (k, kw)
            assert not boxes.boxes[~boxes.valid].any()
    # other parameters: no bridge keeps [5, 7) and [8, 18) apart; a large min_size drops everything
    for p in ((0, 2, 0), (25, 1, 0), (1, 4, 32767)):
        w = _want(rects["c4g"], [(0, 20)], 128, 144, p, T=0)
        (_, boxes, _), = face_detection.detect_many(det, [face_detection.DetectJob("c4g", list(clips["c4g"]))], pads=PADS, T=0,
                                                    batch_size=DET_BATCH, track_spans=face_detection.TrackSpans(*p), **tkw)
        assert boxes.spans == w[1] and _got(boxes) == w[0], p


@pytest.mark.parametrize("track", [None, "largest"])
def test_with_scene_cuts_the_rule_runs_per_shot_of_two_clips_joined_end_to_end(cuda, env, track):
    from wav2lip_amd import face_detection, inference
    from wav2lip_amd.face_detection.scene import SceneCuts
    from wav2lip_amd.face_detection.track import check_track
    det, frames = env["det"], env["clips"]["joined"]
    spans = face_detection.TrackSpans(B, M, 0)
    rects, shots = inference._shot_rects(list(frames), det, DET_BATCH, check_track(track), SceneCuts(SCENE))
    assert (20, 40) in shots and len(shots) > 2                                   # the join is a cut, and so is every grey frame
    want = _want(rects, shots, frames.shape[1], frames.shape[2], spans)
    assert want[1] == [(8, 18), (20, 40)]                                         # frame 7 is a shot of its own: no bridge across a cut
    tkw = {} if track is None else {"face_track": track}
    for job, kw in ((face_detection.DetectJob("j", list(frames)), {}), (face_detection.DetectJob("j", torch.from_numpy(frames).to(cuda)), {}),
                    (face_detection.DetectJob("j", list(frames)), dict(max_group_bytes=1))):
        jobs = [face_detection.DetectJob("c1", list(env["clips"]["c1"])), job]
        (_, first, _), (key, boxes, error) = face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=DET_BATCH, track_spans=spans,
                                                                        scene_cuts=SCENE, **tkw, **kw)
        assert key == "j" and error is None and boxes.spans == want[1] and _got(boxes) == want[0], kw
        assert first.spans == [(0, 20)] and first.valid.all()


def test_with_the_keyword_absent_the_results_are_what_they_were(cuda, env, monkeypatch):
    from wav2lip_amd import _lib, face_detection
    from wav2lip_amd.face_detection import many
    lib, calls = _lib.load(), []
    fn = lib.w2l_face_spans_segments
    monkeypatch.setattr(lib, "w2l_face_spans_segments", lambda *a: calls.append(a) or fn(*a))
    names = ["c1", "c4g"]
    jobs = [face_detection.DetectJob(k, list(env["clips"][k])) for k in names]
    out = list(face_detection.detect_many(env["det"], jobs, pads=PADS, T=5, batch_size=DET_BATCH))
    assert out[0][2] is None and isinstance(out[0][1], np.ndarray) and out[1][1:] == (None, many.NO_FACE)
    assert np.array_equal(out[0][1], noface.model(env["rects"]["c1"], 128, 144, PADS, 5, 0)[0])
    held = list(face_detection.detect_many(env["det"], jobs, pads=PADS, T=5, batch_size=DET_BATCH, no_face_hold=1))
    for (k, boxes, e) in held:
        want, valid = noface.model(env["rects"][k], 128, 144, PADS, 5, 1)
        assert e is None and type(boxes) is many.RunBoxes and np.array_equal(boxes.boxes, want) and np.array_equal(boxes.valid, valid)
    assert calls == []
    list(face_detection.detect_many(env["det"], jobs, pads=PADS, T=5, batch_size=DET_BATCH, track_spans=face_detection.TrackSpans(B, M, 0)))
    assert len(calls) == 1                                                        # one launch for the group
    with pytest.raises(ValueError, match="two answers"):
        list(face_detection.detect_many(env["det"], jobs, no_face_hold=1, track_spans=face_detection.TrackSpans()))


# ---------------------------------------------------------------- the command
def _sync_state_dict():
    from wav2lip_amd import models
    return synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.SyncNet_color().state_dict().items()}, seed=2)


def test_the_command_prints_one_line_per_kept_span_and_each_agrees_with_lse_like_on_that_span(cuda, env, tmp_path):
    """the bars are those of tests/test_score_many_gpu.py::test_lse_many_agrees_with_lse_like_per_clip for `lse_many` against
    `lse_like`: equal window counts, lse_d and lse_c within 1e-3, the offset equal unless the two smallest mean distances lie
    within 2e-3 of each other"""
    from wav2lip_amd import audio, calculate_scores_real_videos as rv, container, evaluation, face_detection, models
    from wav2lip_amd.calculate_scores import face_crops
    from wav2lip_amd.gen_videos_from_filelist import _load_audio
    tmp = str(tmp_path)
    src, clips = env["src"], env["clips"]
    grey = src["c4"][0][7]
    short = np.stack([grey] * 20)
    short[1:5] = src["c4"][0][1:5]                         # one span of 4 frames: kept, and too short for one 5-frame window
    none = np.stack([grey] * 20)
    none[9:11] = src["c4"][0][9:11]                        # one span of 2 frames: dropped
    videos = {"a_joined": clips["joined"], "b_short": short, "c_none": none, "d_clean": clips["c1"]}
    for name, frames in videos.items():
        container.write_avi("%s/%s.avi" % (tmp, name), frames, 25, audio=src["c1"][1], audio_sr=16000)
    (tmp_path / "notes.txt").write_text("not a clip")
    torch.save({"state_dict": {"module." + k: v for k, v in _sync_state_dict().items()}, "optimizer": None, "global_step": 1,
                "global_epoch": 0}, tmp + "/sync.pth")
    argv = ["--checkpoint_path", tmp + "/sync.pth", "--min_track", str(M), "--num_failed_det", str(B)]
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        scored = rv.main(argv + ["--data_root", tmp, "--scores_file", tmp + "/all_scores.txt"], state_dict=synth.s3fd_state_dict())
    lines = out.getvalue().splitlines()
    assert [r["key"] for r in scored] == ["a_joined.avi#0", "a_joined.avi#1", "d_clean.avi#0"]
    assert lines == [str(r["lse_d"]) + " " + str(r["lse_c"]) for r in scored] and all(len(ln.split()) == 2 for ln in lines)
    assert open(tmp + "/all_scores.txt").read().splitlines() == lines
    said = err.getvalue()
    assert "c_none.avi: skipped: no face span" in said and "b_short.avi#0: skipped: too short" in said
    assert "a_joined" not in said and "d_clean" not in said
    # every result against lse_like on that span's crops, placed at the span's first frame
    S = models.SyncNet_color()
    S.load_state_dict(_sync_state_dict())
    S = S.to(cuda).eval()
    det_jobs = [face_detection.DetectJob(k, list(videos[k])) for k in ("a_joined", "d_clean")]
    boxes = {k: b for k, b, _ in face_detection.detect_many(env["det"], det_jobs, pads=(0, 0, 0, 0), T=5, batch_size=DET_BATCH,
                                                            track_spans=face_detection.TrackSpans(B, M, 0))}
    assert boxes["a_joined"].spans == [(5, 18), (20, 40)] and boxes["d_clean"].spans == [(0, 20)]
    results, jobs, worst = iter(scored), [], 0.
    for k in ("a_joined", "d_clean"):
        wav, _, _ = _load_audio("%s/%s.avi" % (tmp, k), tmp)
        mel = audio.melspectrogram_device(wav, cuda)
        for a, b in boxes[k].spans:
            crops = face_crops(videos[k][a:b], boxes[k].boxes[a:b], cuda)
            ref, got = evaluation.lse_like(S, crops, mel, first=a), next(results)
            assert got["n"] == ref["n"] == len(evaluation.sync_rows(b - a, mel.shape[1], 25., first=a)) > 0
            two = np.sort(ref["mdist"])[:2]
            assert got["offset"] == ref["offset"] or two[1] - two[0] <= 2e-3
            err_ = max(abs(got["lse_d"] - ref["lse_d"]), abs(got["lse_c"] - ref["lse_c"]))
            worst = max(worst, err_)
            print("%s [%d, %d): lse_d %.6f / %.6f, lse_c %.6f / %.6f" % (k, a, b, got["lse_d"], ref["lse_d"], got["lse_c"], ref["lse_c"]))
            assert err_ <= 1e-3, (k, a, b, err_)
            if a:                                          # the offset matters: the same crops at frame 0 read other mel columns
                assert not np.array_equal(evaluation.lse_like(S, crops, mel)["mdist"], ref["mdist"])
            jobs.append((k, crops, mel, a))
    print("the command vs lse_like: largest difference of lse_d / lse_c %.3e" % worst)
    # a job with first = 0 gives the bytes of one without the field
    three = evaluation.lse_many(S, [evaluation.ScoreJob(*j[:3]) for j in jobs], batch_size=20)
    four = evaluation.lse_many(S, [evaluation.ScoreJob(j[0], j[1], j[2], first=0) for j in jobs], batch_size=20)
    assert len(three) == len(four) == 3
    for x, y in zip(three, four):
        assert (x["n"], x["offset"]) == (y["n"], y["offset"]) and x["mdist"].tobytes() == y["mdist"].tobytes()
        assert np.float32(x["lse_d"]).tobytes() == np.float32(y["lse_d"]).tobytes() and np.float32(x["lse_c"]).tobytes() == np.float32(y["lse_c"]).tobytes()
    # the command's own jobs again through lse_many: the bytes it printed
    again = evaluation.lse_many(S, [evaluation.ScoreJob(*j) for j in jobs], batch_size=20)
    assert [str(r["lse_d"]) + " " + str(r["lse_c"]) for r in again] == lines
    # one video, one box for every frame: the video is one span, no detector
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        one = rv.main(argv + ["--videofile", tmp + "/b_short.avi", "--box", "10", "106", "16", "112"])
    assert [r["key"] for r in one] == ["b_short.avi#0"] and one[0]["n"] == 16 and len(out.getvalue().splitlines()) == 1
    with pytest.raises(SystemExit):
        rv.main(argv)
