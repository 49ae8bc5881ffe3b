"""Host side of the face spans of finished clips (`track_spans`): the numpy model of tests/_span_cases.py against
its brute-force form, the product's host statement (`spans.host_spans`) against the model, the rule's degenerate case against
`many.boxed_runs`, the frame offset of a scoring job, the copy-back layout, `detect_many`'s host path with a stub detector, the
argument checks and the parser of the new command."""
import numpy as np
import pytest
import torch

import _noface_cases as noface
import _span_cases as cases
from test_noface_cpu import StubDetector
from test_streaming_live_cpu import _rect_of, _video

GROUPS = cases.groups()


def _as_list(rects, flags):
    return [tuple(int(v) for v in r) if f == 1 else None for r, f in zip(rects, flags)]


def test_the_case_list_holds_what_it_promises():
    names = [name for _, group in GROUPS for name, _, _ in group]
    assert len(names) > 300 and {B for (B, _, _), _ in GROUPS} >= set(cases.BRIDGES)
    for n in cases.LENGTHS:
        assert any(name.startswith("%d " % n) for name in names)
    kept, dropped, bridged, host = 0, 0, 0, 0
    for (B, M, S), group in GROUPS:
        for name, rects, flags in group:
            _, flags_out, spans, status = cases.model(rects, flags, B, M, S)
            if status[0] == 2:
                host += 1
                continue
            kept += status[1]
            dropped += len(list(noface_runs(cases.model(rects, flags, B, 1, 0)[1]))) - status[1]
            bridged += int((flags_out == 1).sum() - ((flags == 1) & (flags_out == 1)).sum())
    assert kept > 1000 and dropped > 100 and bridged > 1000 and host == len(cases.BRIDGES)


def noface_runs(flags):
    edges = np.flatnonzero(np.diff(np.concatenate(([0], np.asarray(flags, np.int8), [0]))))
    return zip(edges[::2].tolist(), edges[1::2].tolist())


def test_the_model_equals_its_brute_force_form_on_every_case():
    for (B, M, S), group in GROUPS:
        for name, rects, flags in group:
            a, b = cases.model(rects, flags, B, M, S), cases.brute(rects, flags, B, M, S)
            assert a[3] == b[3], (B, M, S, name)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (B, M, S, name)
            assert (a[2] is None and b[2] is None) or np.array_equal(a[2], b[2]), (B, M, S, name)


def test_what_the_decisive_cases_decide():
    by = {(p, name): (rects, flags) for p, group in GROUPS for name, rects, flags in group}

    def status(p, name):
        return cases.model(*by[p, name], *p)[3]

    for B in cases.BRIDGES:
        assert status((B, 1, 0), "miss of B") == (0, 1) and status((B, 1, 0), "miss of B+1") == (0, 2)
        assert status((B, 1, 0), "miss across a chunk") == ((0, 1) if B >= 3 else (0, 2))
        assert status((B, 1, 0), "detections at 0 and 251") == ((0, 1) if B == 250 else (0, 2))
        assert status((B, 1, 0), "detections at 0 and 252") == (0, 2)
        assert status((B, 1, 0), "a flag-2 row") == (2, 13)
    r, f, spans, st = cases.model(*by[(250, 1, 0), "coordinates up to 2^31 - 1"], 250, 1, 0)
    assert st == (0, 1) and spans[0].tolist() == [0, 252, 2, 0] and f.all() and r.max() == cases.BIG
    assert r[1].tolist() == [(0 * 250 + (cases.BIG - 7) * 1) // 251, (5 * 250) // 251, cases.BIG, (250 * (cases.BIG - 2) + cases.BIG) // 251]
    assert [status((2, M, 0), "spans of 7, 7, 8 and 70 rows, M %d" % M)[1] for M in (7, 8, 9, 70, 71)] == [4, 2, 1, 1, 0]
    assert [status((0, 1, S), "mean width 11, S %d" % S)[1] for S in (10, 11, 12)] == [1, 1, 0]
    assert [status((0, 1, S), "mean height 11, S %d" % S)[1] for S in (10, 11, 12)] == [1, 1, 0]
    assert [status((0, 1, S), "mean width 10.5, S %d" % S)[1] for S in (10, 11, 12)] == [1, 0, 0]
    assert [status((0, 1, S), "bridged mean, S %d" % S)[1] for S in (10, 11, 12)] == [2, 1, 1]
    assert status((1, 1, 11), "bridged mean 11 with B 1") == (0, 1) and status((1, 1, 12), "bridged mean 11 with B 1, S 12") == (0, 0)


def test_host_spans_equals_the_model():
    from wav2lip_amd.face_detection import spans
    for (B, M, S), group in GROUPS:
        for name, rects, flags in group:
            rects_out, flags_out, rows, status = cases.model(rects, flags, B, M, S)
            if status[0] == 2:
                continue                                   # a row the device leaves to the host has a rect or None there
            filled, kept = spans.host_spans(_as_list(rects, flags), B, M, S)
            assert filled == cases.filled_rects(rects_out, flags_out), (B, M, S, name)
            assert kept == [(int(a), int(a + L)) for a, L, _, _ in rows[:status[1]]], (B, M, S, name)
    assert spans.host_spans([], 25, 100, 0) == ([], [])
    shots = [(0, 3), (3, 4), (4, 9)]
    rects = [(1, 2, 30, 40), None, (3, 4, 50, 60), (5, 6, 7, 8), (1, 1, 2, 2), None, None, (9, 9, 12, 12), None]
    filled, kept = spans.host_spans_shots(rects, shots, spans.TrackSpans(2, 1, 0))
    assert kept == [(0, 3), (3, 4), (4, 8)] and filled[1] == (2, 3, 40, 50) and filled[5] == (3, 3, 5, 5) and filled[8] is None
    assert spans.host_spans_shots(rects, shots, spans.TrackSpans(1, 2, 0))[1] == [(0, 3)]


def test_without_bridge_and_thresholds_the_rule_is_boxed_runs_of_the_detections():
    from wav2lip_amd.face_detection import many
    for (B, M, S), group in GROUPS:
        for name, rects, flags in group:
            if (flags > 1).any():
                continue
            rects_out, flags_out, rows, status = cases.model(rects, flags, 0, 1, 0)
            assert np.array_equal(flags_out, flags) and np.array_equal(rects_out, np.where(flags[:, None] == 1, rects, 0)), name
            runs = list(many.boxed_runs(flags == 1))
            assert status == (0, len(runs)) and [(a, a + L) for a, L, _, _ in rows[:len(runs)].tolist()] == runs, name
            assert all(nd == L for _, L, nd, _ in rows[:len(runs)].tolist()) and not rows[len(runs):].any()


# ---------------------------------------------------------------- the frame offset of a scoring job
def test_sync_rows_places_a_span_at_the_mel_columns_of_its_own_frames():
    from wav2lip_amd import evaluation
    for fps in (25., 30., 23.976):
        for T, Tm in ((5, 16), (9, 40), (40, 200), (100, 1000)):
            assert evaluation.sync_rows(T, Tm, fps, first=0) == evaluation.sync_rows(T, Tm, fps) == evaluation.sync_rows(T, Tm, fps, 0)
            for a in (1, 7, 100, 290):
                want = []
                for v in range(0, T - 5 + 1):
                    s = int(80. * ((a + v) / float(fps)))
                    if s + 16 > Tm:
                        break
                    want.append((v, s))
                assert evaluation.sync_rows(T, Tm, fps, first=a) == want, (fps, T, Tm, a)
    assert evaluation.sync_rows(40, 200, 25., first=10)[:3] == [(0, 32), (1, 35), (2, 38)]
    assert evaluation.sync_rows(40, 200, 25., first=60) == []                                   # the mel ends before the span
    job = evaluation.ScoreJob("k", "faces", "mel")
    assert job.first == 0 and tuple(job[:3]) == ("k", "faces", "mel") and evaluation.ScoreJob("k", 1, 2, 9).first == 9
    assert evaluation.ScoreJob._fields[:3] == ("key", "faces", "mel")
    mel = torch.arange(80 * 60, dtype=torch.float32).reshape(80, 60)
    frames = torch.zeros((12, 96, 96, 3), dtype=torch.uint8)
    for a in (0, 3):
        faces, mels = evaluation.sync_windows(frames, mel, 25., first=a)
        rows = evaluation.sync_rows(12, 60, 25., first=a)
        assert len(faces) == len(rows) == 8 and all(torch.equal(m[0], mel[:, s:s + 16]) for m, (_, s) in zip(mels, rows))
    assert torch.equal(evaluation.sync_windows(frames, mel, 25.)[1], evaluation.sync_windows(frames, mel, 25., first=0)[1])


# ---------------------------------------------------------------- the copy-back buffer
@pytest.mark.parametrize("n_seg", [1, 3])
@pytest.mark.parametrize("n_boxes", [0, 1, 5, 6])
@pytest.mark.parametrize("track", [False, True])
def test_box_out_with_spans_keeps_the_first_parts_and_aligns_the_span_rows(track, n_boxes, n_seg):
    from wav2lip_amd.face_detection.many import BoxOut
    plain, out = BoxOut(n_boxes, n_seg, True, track, "cpu"), BoxOut(n_boxes, n_seg, True, track, "cpu", spans=True)
    assert plain.span_rows is None and plain.span_status is None
    for name in ("boxes", "valid", "status", "track_status"):
        a, b = getattr(plain, name), getattr(out, name)
        assert a.storage_offset() == b.storage_offset() and a.numel() == b.numel()
    assert out.span_rows.numel() == 4 * n_boxes and out.span_status.numel() == 2 * n_seg
    assert out.span_rows.storage_offset() % 4 == 0 and 0 <= out.span_rows.storage_offset() - plain.buffer.numel() < 4
    assert out.span_status.storage_offset() == out.span_rows.storage_offset() + 4 * n_boxes
    assert out.buffer.numel() == out.span_status.storage_offset() + 2 * n_seg
    out.buffer.zero_()
    out.span_rows.copy_(torch.arange(4 * n_boxes, dtype=torch.int32) + 100)
    out.span_status.copy_(torch.arange(2 * n_seg, dtype=torch.int32) + 900)
    rows, status = out.split_spans(out.buffer.numpy())
    assert rows.shape == (n_boxes, 4) and rows.reshape(-1).tolist() == [100 + i for i in range(4 * n_boxes)]
    assert status.shape == (n_seg, 2) and status.reshape(-1).tolist() == [900 + i for i in range(2 * n_seg)]
    assert not out.split(out.buffer.numpy())[0].any()


# ---------------------------------------------------------------- detect_many
def test_track_spans_and_no_face_hold_together_are_refused_and_the_values_are_checked():
    from wav2lip_amd.face_detection import TrackSpans, detect_many, spans
    with pytest.raises(ValueError, match="two answers to the same question"):
        list(detect_many(StubDetector(), [], no_face_hold=0, track_spans=TrackSpans()))
    assert list(detect_many(StubDetector(), [], track_spans=TrackSpans())) == []
    assert TrackSpans() == (25, 100, 0) and spans.check_spans(None) is None and spans.check_spans((3, 4, 5)) == TrackSpans(3, 4, 5)
    assert spans.check_spans(TrackSpans(np.int64(250), 1 << 30, 32767)) == (250, 1 << 30, 32767)
    for bad in (TrackSpans(-1), TrackSpans(251), TrackSpans(0, 0), TrackSpans(0, (1 << 30) + 1), TrackSpans(0, 1, -1), TrackSpans(0, 1, 32768),
                TrackSpans(1.5), TrackSpans(True), TrackSpans(0, "4"), 7, (1, 2, 3, 4)):
        with pytest.raises(ValueError, match="track_spans"):
            spans.check_spans(bad)
        with pytest.raises(ValueError, match="track_spans"):
            list(detect_many(StubDetector(), [], track_spans=bad))


@pytest.mark.parametrize("T", [0, 5])
def test_detect_many_runs_the_rule_on_the_host_for_a_clip_above_the_group_limit(T):
    """`max_group_bytes=1` sends every clip through the host path: the stub detector's rects, `host_spans`, and every kept span
    finished as a run - against the two models"""
    from wav2lip_amd.face_detection import DetectJob, TrackSpans, detect_many, many
    no_face = (0, 3, 4, 9, 10, 11, 12, 16, 29)
    video = _video(30, 5, 1, no_face=no_face)
    rects = [None if f[0, 2, 1] else _rect_of(f) for f in video]
    flags = np.array([r is not None for r in rects], np.int64)
    arr = np.array([r if r is not None else (0, 0, 0, 0) for r in rects], np.int64)
    pads = (0, 10, 0, 0)
    for B, M, S in ((1, 4, 0), (2, 4, 0), (0, 1, 0), (4, 1, 0), (1, 4, 60), (25, 100, 0)):
        rects_out, flags_out, rows, status = cases.model(arr, flags, B, M, S)
        want, want_valid = noface.model(cases.filled_rects(rects_out, flags_out), noface.FH, noface.FW, pads, T, 0)
        (key, got, err), = detect_many(StubDetector(), [DetectJob("v", list(video))], pads=pads, T=T, batch_size=8, max_group_bytes=1,
                                       track_spans=TrackSpans(B, M, S))
        assert key == "v" and err is None and isinstance(got, many.SpanBoxes) and isinstance(got, many.RunBoxes)
        assert got.spans == [(int(a), int(a + L)) for a, L, _, _ in rows[:status[1]]], (B, M, S)
        assert np.array_equal(got.boxes, want) and np.array_equal(got.valid, want_valid), (B, M, S)
        assert [b is None for b in got] == [not v for v in want_valid]
    # (1, 4, 0): [1, 3) is dropped, [5, 9) is kept, the misses of two and four rows are not bridged, [13, 29) is bridged over row 16,
    # row 29 trails
    assert cases.model(arr, flags, 1, 4, 0)[2][:2].tolist() == [[5, 4, 4, 0], [13, 16, 15, 0]] and cases.model(arr, flags, 1, 4, 0)[3] == (0, 2)
    empty, = detect_many(StubDetector(), [DetectJob("e", [])], track_spans=TrackSpans())
    assert empty[0] == "e" and isinstance(empty[1], many.SpanBoxes) and len(empty[1]) == 0 and empty[1].spans == [] and empty[2] is None


# ---------------------------------------------------------------- the command's parser
def test_parser_has_the_reference_flags_and_defaults():
    """calculate_scores_real_videos.py:10-16; --checkpoint_path in place of --initial_model"""
    from wav2lip_amd import calculate_scores_real_videos as rv
    a = rv.parser.parse_args(["--checkpoint_path", "c.pth"])
    assert (a.batch_size, a.vshift, a.data_dir, a.videofile, a.reference) == (20, 15, "data/work", "", "")
    assert sorted(vars(a)) == ["batch_size", "checkpoint_path", "data_dir", "reference", "videofile", "vshift"]
    b = rv.parser.parse_args(["--checkpoint_path", "c", "--vshift", "7", "--batch_size", "4", "--videofile", "v.avi", "--data_dir", "d",
                              "--reference", "r"])
    assert (b.batch_size, b.vshift, b.data_dir, b.videofile, b.reference) == (4, 7, "d", "v.avi", "r")
    assert isinstance(b.vshift, int) and isinstance(b.batch_size, int)
    with pytest.raises(SystemExit):
        rv.parser.parse_args([])
    a = rv.cli_parser.parse_args(["--checkpoint_path", "c", "--videofile", "v.avi"])
    assert (a.min_track, a.num_failed_det, a.min_face_size) == (100, 25, 0) and a.data_root is None and a.scores_file is None
    assert a.box is None and a.fps == 25. and a.face_det_precision == "fp32" and a.precision == "fp32" and a.face_det_scale == 1
    assert a.scene_cuts is None and a.face_track is None
    a = rv.cli_parser.parse_args(["--checkpoint_path", "c", "--data_root", "d", "--min_track", "4", "--num_failed_det", "2",
                                  "--min_face_size", "30", "--scene_cuts", "0.3", "--face_track", "largest", "--face_track_reseed", "2",
                                  "--box", "1", "90", "2", "80", "--fps", "30", "--scores_file", "all_scores.txt"])
    assert (a.min_track, a.num_failed_det, a.min_face_size, a.scene_cuts, a.face_track, a.face_track_reseed) == (4, 2, 30, 0.3, "largest", 2)
    assert a.box == [1, 90, 2, 80] and a.fps == 30. and a.scores_file == "all_scores.txt" and a.data_root == "d"
    from wav2lip_amd.face_detection.spans import spans_from_args
    assert spans_from_args(a) == (2, 4, 30)
    for bad in (["--min_track", "0"], ["--num_failed_det", "251"], ["--num_failed_det", "-1"], ["--min_face_size", "32768"],
                ["--min_track", "x"]):
        with pytest.raises(SystemExit):
            rv.cli_parser.parse_args(["--checkpoint_path", "c", "--videofile", "v.avi"] + bad)
