"""Every face of a shot through the front ends: `face_detection.detect_many(all_faces=...)` and the real-video scoring
command with `--all_faces`, against the model of tests/_faces_cases.py followed by the span model and today's finish, per slot.
The detector's box table is prescribed per frame through `FaceAlignment._candidates`, as tests/test_track_product_gpu.py does (its
`World`), so the real gate, NMS, w2l_s3fd_top_rects, w2l_face_tracks_all_segments, span and finish launches run on small frames
without a network."""
import contextlib
import io

import numpy as np
import pytest
import torch

import _faces_cases as fc
import _noface_cases as noface
import _span_cases as sc
import _track_cases as tc
from test_track_product_gpu import FACES, WIDE, World, count_reads, detector, jitter, swapping_clip

pytestmark = pytest.mark.gpu

PADS = (0, 10, 0, 0)
NEW = "w2l_face_tracks_all_segments"


def spy(monkeypatch):
    from wav2lip_amd import _lib
    lib, calls = _lib.load(), []
    for name in ("w2l_s3fd_top_rects", "w2l_s3fd_first_rect", "w2l_face_track_segments", NEW, "w2l_face_spans_segments", "w2l_face_boxes_runs"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _name=name: calls.append(_name) or _fn(*a))
    return calls


def expected(world, ids, faces, spans, H, W, shots=None, pads=PADS, T=5):
    """([(slot, a, b, boxes, detected)] by (a, slot), dropped, whether a frame is left to the host) of a clip of these frames"""
    per = [world.candidates(fid, faces.cands) for fid in ids]
    frames = [fc.found(*c) if c else fc.NO_FACE for c, _ in per]
    out, dropped = [], 0
    for lo, hi in shots or [(0, len(ids))]:
        rects, flags, (_, d, _), _ = fc.model_faces(*fc.pack(frames[lo:hi], faces.cands), faces.max_faces, spans.bridge,
                                                    int(faces.min_iou * 256))
        dropped += d
        for t in range(faces.max_faces):
            r2, f2, rows, (code, count) = sc.model(rects[t], flags[t], *spans)
            boxes, valid = noface.model(sc.filled_rects(r2, f2), H, W, pads, T, 0)
            out += [(t, lo + a, lo + a + n, boxes[a:a + n], det) for a, n, det, _ in rows[:count].tolist()]
    return sorted(out, key=lambda s: (s[1], s[0])), dropped, any(f == tc.HOST for _, f in per)


def same(res, want, dropped, n):
    from wav2lip_amd.face_detection.faces import FaceSpans
    assert isinstance(res, FaceSpans) and len(res) == n and res.dropped == dropped
    assert [(t.slot, t.a, t.b, t.detected) for t in res.tracks] == [w[:3] + (w[4],) for w in want]
    for t, w in zip(res.tracks, want):
        assert t.boxes.dtype == np.int64 and np.array_equal(t.boxes, w[3])


def clips_of(world):
    """ids per clip: two faces that swap score rank; three that do; one that leaves for more than L frames and returns; the same
    for exactly L frames; a clip without a face; one frame"""
    a_only = {i: [(jitter(FACES["a"], i % 3), 0.9)] for i in range(3, 8)}
    return {"two": swapping_clip(world, 12), "three": swapping_clip(world, 11, faces=("c", "a", "b")),
            "leaves": swapping_clip(world, 14, extra=a_only), "returns": swapping_clip(world, 12, extra={i: a_only[i] for i in (3, 4)}),
            "none": swapping_clip(world, 5, gaps=range(5)), "one": swapping_clip(world, 1)}


SETTINGS = [((2, 4, 0.25), (2, 3, 0)), ((4, 4, 0.25), (0, 1, 0)), ((1, 2, 0.5), (2, 2, 10))]


@pytest.mark.parametrize("faces,spans", SETTINGS)
def test_detect_many_follows_every_face(cuda, monkeypatch, faces, spans):
    from wav2lip_amd import face_detection
    faces, spans = face_detection.AllFaces(*faces), face_detection.TrackSpans(*spans)
    world = World()
    clips = clips_of(world)
    det = detector(cuda, world)
    H, W = 48, 64
    want = {k: expected(world, ids, faces, spans, H, W) for k, ids in clips.items()}
    assert not any(w[2] for w in want.values())
    if faces.max_faces == 2 and spans.bridge == 2:
        # two faces: two tracks over the whole clip, each on its own side; the third face of "three" finds no slot; the face that
        # leaves for 5 > L frames comes back as a track of its own, the one that leaves for 2 = L frames is bridged
        assert [w[:3] for w in want["two"][0]] == [(0, 0, 12), (1, 0, 12)] and want["three"][1] == 11
        assert [w[:3] for w in want["leaves"][0]] == [(0, 0, 14), (1, 0, 3), (1, 8, 14)]
        assert [(w[:3], w[4]) for w in want["returns"][0]] == [((0, 0, 12), 12), ((1, 0, 12), 10)]
        assert want["none"][0] == [] and want["one"][0] == []
    calls, reads = spy(monkeypatch), count_reads(monkeypatch)
    for form, kw in (("host", {}), ("device", {}), ("alone", dict(max_group_bytes=1))):
        jobs = [face_detection.DetectJob(k, torch.from_numpy(world.frames(ids, H, W)).to(cuda) if form == "device" else
                                         list(world.frames(ids, H, W))) for k, ids in clips.items()]
        jobs.append(face_detection.DetectJob("empty", []))
        del calls[:], reads[:]
        got = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=4, track_spans=spans, all_faces=faces, **kw))
        assert [k for k, _, _ in got] == list(clips) + ["empty"] and all(e is None for _, _, e in got)
        for (k, res, _), ids in zip(got, list(clips.values()) + [[]]):
            same(res, *(want[k][:2] if ids else ([], 0)), len(ids))
        if form == "alone":
            assert NEW not in calls and "w2l_face_spans_segments" not in calls
        else:                                               # one group: its batches, the three launches, ONE copy back
            assert calls == ["w2l_s3fd_top_rects"] * 14 + [NEW, "w2l_face_spans_segments", "w2l_face_boxes_runs"]
            assert reads == ["cpu"]


def test_a_clip_with_a_frame_left_to_the_host_takes_the_host_path(cuda, monkeypatch):
    from wav2lip_amd import face_detection
    faces, spans = face_detection.AllFaces(2, 4, 0.25), face_detection.TrackSpans(1, 2, 0)
    world = World()
    wide = [(WIDE, 0.95), (jitter(FACES["b"], 1), 0.7)]
    clips = {"clean": swapping_clip(world, 6), "wide": swapping_clip(world, 9, extra={3: wide}),
             "wide_first": swapping_clip(world, 5, extra={0: wide})}
    det = detector(cuda, world)
    calls = spy(monkeypatch)
    jobs = [face_detection.DetectJob(k, list(world.frames(ids))) for k, ids in clips.items()]
    got = list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=4, track_spans=spans, all_faces=faces))
    assert calls.count(NEW) == 1 and [k for k, _, _ in got] == list(clips)
    hosts = 0
    for (k, res, error), ids in zip(got, clips.values()):
        want, dropped, host = expected(world, ids, faces, spans, 48, 64)
        hosts += host
        assert error is None
        same(res, want, dropped, len(ids))
    assert hosts == 2 and got[1][1].dropped == 1            # the wide rect of frame 3 is a candidate on the host, beyond the two slots


def test_with_scene_cuts_no_track_crosses_the_cut(cuda, monkeypatch):
    from wav2lip_amd import face_detection
    from wav2lip_amd.face_detection.scene import SceneCuts
    faces, spans = face_detection.AllFaces(2, 4, 0.25), face_detection.TrackSpans(2, 3, 0)
    world = World()
    first, second = swapping_clip(world, 9), swapping_clip(world, 8, faces=("b", "a"))
    ids = first + second
    frames = world.frames(ids)
    frames[len(first):, 2:] = 200                           # another picture: the join is a cut
    other = swapping_clip(world, 6)                         # before the detector takes its copy of the tables
    det = detector(cuda, world)
    shots = [(0, 9), (9, 17)]
    want, dropped, _ = expected(world, ids, faces, spans, 48, 64, shots)
    whole, _, _ = expected(world, ids, faces, spans, 48, 64)
    assert [w[:3] for w in whole] == [(0, 0, 17), (1, 0, 17)]                           # without the cut the faces run through
    assert [w[:3] for w in want] == [(0, 0, 9), (1, 0, 9), (0, 9, 17), (1, 9, 17)]
    calls, reads = spy(monkeypatch), count_reads(monkeypatch)
    for kw in ({}, dict(max_group_bytes=1)):
        jobs = [face_detection.DetectJob("other", list(world.frames(other))), face_detection.DetectJob("joined", list(frames))]
        del calls[:], reads[:]
        (_, res0, _), (_, res, error) = face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=4, track_spans=spans,
                                                                   all_faces=faces, scene_cuts=SceneCuts(0.3), **kw)
        assert error is None
        same(res, want, dropped, len(ids))
        same(res0, *expected(world, other, faces, spans, 48, 64)[:2], len(other))
        assert not any(t.a < 9 < t.b for t in res.tracks)
        if not kw:                                          # the cut flags' small copy, then the group's ONE copy back
            assert calls.count(NEW) == 1 and len(reads) == 1


def test_without_the_keyword_the_new_kernel_is_never_launched(cuda, monkeypatch):
    from wav2lip_amd import face_detection
    world = World()
    ids = swapping_clip(world, 10)
    det = detector(cuda, world)
    calls = spy(monkeypatch)
    jobs = [face_detection.DetectJob("k", list(world.frames(ids)))]
    for kw in ({}, dict(track_spans=face_detection.TrackSpans(1, 2, 0)), dict(face_track="left"), dict(no_face_hold=1),
               dict(track_spans=face_detection.TrackSpans(1, 2, 0), face_track="score", scene_cuts=0.3), dict(max_group_bytes=1)):
        list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=4, **kw))
    assert NEW not in calls and "w2l_s3fd_top_rects" in calls and "w2l_s3fd_first_rect" in calls
    list(face_detection.detect_many(det, jobs, pads=PADS, T=5, batch_size=4, track_spans=face_detection.TrackSpans(1, 2, 0),
                                    all_faces=face_detection.AllFaces()))
    assert calls.count(NEW) == 1


# ---------------------------------------------------------------- the command
def _sync_state_dict():
    from wav2lip_amd import models
    from wav2lip_amd import synthetic as synth
    return synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.SyncNet_color().state_dict().items()}, seed=2)


def test_the_command_prints_one_line_per_face_track(cuda, monkeypatch, tmp_path):
    """two prescribed faces in a small AVI: two lines, each the score of that track's crops placed at its first frame.  The bars
    against `lse_like` are those of tests/test_score_many_gpu.py for `lse_many` against `lse_like` (lse_d and lse_c within 1e-3);
    against `lse_many` on the same jobs the lines are equal.  Without --all_faces the command prints what it prints today."""
    from wav2lip_amd import audio, calculate_scores_real_videos as rv, container, evaluation, face_detection, models
    from wav2lip_amd import synthetic as synth
    from wav2lip_amd.calculate_scores import face_crops
    from wav2lip_amd.gen_videos_from_filelist import _load_audio
    tmp = str(tmp_path)
    world = World()
    ids = swapping_clip(world, 20, faces=("a", "b", "c"))
    frames = world.frames(ids)
    frames[:, 2:] = np.random.default_rng(0).integers(0, 256, frames[:, 2:].shape, dtype=np.uint8)      # something to score
    wav = synth.filelist_clips()["c1"][1]
    container.write_avi(tmp + "/two.avi", frames, 25, audio=wav, audio_sr=16000)
    torch.save({"state_dict": {"module." + k: v for k, v in _sync_state_dict().items()}, "optimizer": None, "global_step": 1,
                "global_epoch": 0}, tmp + "/sync.pth")
    prescribed = detector(cuda, world)
    monkeypatch.setattr(face_detection.FaceAlignment, "_candidates",
                        lambda self, images, rows=None, resolve=True: type(prescribed)._candidates(prescribed, images, rows, resolve))
    calls = spy(monkeypatch)
    argv = ["--checkpoint_path", tmp + "/sync.pth", "--videofile", tmp + "/two.avi", "--min_track", "4", "--num_failed_det", "1"]

    def run(extra):
        out, err = io.StringIO(), io.StringIO()
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            scored = rv.main(argv + extra, state_dict=synth.s3fd_state_dict())
        return scored, out.getvalue().splitlines(), err.getvalue()

    scored, lines, said = run(["--all_faces", "--max_faces", "2"])
    assert calls.count(NEW) == 1
    assert [r["key"] for r in scored] == ["two.avi#0", "two.avi#1"]
    assert lines == [str(r["lse_d"]) + " " + str(r["lse_c"]) for r in scored]
    assert said.count("more than 2 faces: 20 candidates not followed") == 1 and "two.avi" in said
    S = models.SyncNet_color()
    S.load_state_dict(_sync_state_dict())
    S = S.to(cuda).eval()
    faces, spans = face_detection.AllFaces(2), face_detection.TrackSpans(1, 4, 0)
    want, dropped, _ = expected(world, ids, faces, spans, 48, 64, pads=(0, 0, 0, 0))
    assert [w[:3] for w in want] == [(0, 0, 20), (1, 0, 20)] and dropped == 20
    mel = audio.melspectrogram_device(_load_audio(tmp + "/two.avi", tmp)[0], cuda)
    jobs = []
    for (t, a, b, boxes, _), got in zip(want, scored):
        crops = face_crops(frames[a:b], boxes, cuda)
        ref = evaluation.lse_like(S, crops, mel, first=a)
        assert got["n"] == ref["n"] > 0
        print("track %d [%d, %d): lse_d %.6f / %.6f, lse_c %.6f / %.6f" % (t, a, b, got["lse_d"], ref["lse_d"], got["lse_c"], ref["lse_c"]))
        assert max(abs(got["lse_d"] - ref["lse_d"]), abs(got["lse_c"] - ref["lse_c"])) <= 1e-3
        jobs.append(evaluation.ScoreJob("two.avi#%d" % t, crops, mel, a))
    assert lines[0] != lines[1]
    again = evaluation.lse_many(S, jobs, batch_size=20)
    assert [str(r["lse_d"]) + " " + str(r["lse_c"]) for r in again] == lines
    # no free slot is no news with enough of them
    scored3, lines3, said3 = run(["--all_faces"])
    assert len(lines3) == 3 == len(scored3) and "faces" not in said3
    # without the flag: one face per shot, through the launches of before
    del calls[:]
    scored1, lines1, said1 = run([])
    assert NEW not in calls and [r["key"] for r in scored1] == ["two.avi#0"] and "faces" not in said1
    (_, boxes, _), = face_detection.detect_many(prescribed, [face_detection.DetectJob("two", list(frames))], pads=(0, 0, 0, 0), T=5,
                                                batch_size=rv.FACE_DET_BATCH_SIZE, track_spans=spans)
    assert boxes.spans == [(0, 20)]
    one = evaluation.lse_many(S, [evaluation.ScoreJob("k", face_crops(frames, boxes.boxes, cuda), mel, 0)], batch_size=20)
    assert lines1 == [str(one[0]["lse_d"]) + " " + str(one[0]["lse_c"])]
    # the module's own look at a video: `slot a b detected` per kept track
    from wav2lip_amd.face_detection import faces as faces_module
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = faces_module.main([tmp + "/two.avi", "--max_faces", "2", "--min_track", "4", "--num_failed_det", "1"],
                               state_dict=synth.s3fd_state_dict())
    assert rc == 0 and out.getvalue().splitlines() == ["0 0 20 20", "1 0 20 20"]
    assert "more than 2 faces: 20 candidates not followed" in err.getvalue()
