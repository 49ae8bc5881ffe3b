"""Every face of a shot on the host: the product's statement of the rule (face_detection/faces.py) against the model
written from the rule (tests/_faces_cases.py), the three consequences the documents promise, the parameter check and the parsers at
their range ends, the expanded segment table, `detect_many`'s host path on a stub detector, and the new entry of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import _faces_cases as fc
import _noface_cases as noface
import _span_cases as sc
import _track_cases as tc
from conftest import ROOT

ARGV = ["--checkpoint_path", "c", "--videofile", "v.avi"]


def per_frame(frames, K):
    """what the host path sees of `frames`: the candidate list of every frame (no frame is left to anyone else there)"""
    cands, ncand, cflags = fc.pack(frames, K)
    out = []
    for i in range(len(frames)):
        m = min(max(int(ncand[i]), 0), K) if cflags[i] == fc.FOUND else 0
        out.append([tuple(int(v) for v in c) for c in cands[i, :m]])
    return out


def as_arrays(slots):
    """`host_all_tracks`' lists in the model's format"""
    F, n = len(slots), len(slots[0]) if slots else 0
    rects, flags = np.zeros((F, n, 4), np.int64), np.zeros((F, n), np.int64)
    for t, rows in enumerate(slots):
        for i, r in enumerate(rows):
            if r is not None:
                assert type(r) is tuple and all(type(v) is int for v in r)
                rects[t, i], flags[t, i] = r, 1
    return rects, flags


def check_host(frames, F, K, L, q):
    from wav2lip_amd.face_detection.faces import host_all_tracks
    frames = [fr for fr in frames if fr[1] != fc.HOST]
    stats = {}
    got = host_all_tracks(per_frame(frames, K), F, q, L, stats)
    assert len(got) == F and all(len(rows) == len(frames) for rows in got)
    want_r, want_f, want_s, ev = fc.model_faces(*fc.pack(frames, K), F, L, q)
    rects, flags = as_arrays(got) if frames else (want_r, want_f)
    assert np.array_equal(flags, want_f) and np.array_equal(rects, want_r)
    assert (stats["started"], stats["dropped"], stats["peak"]) == want_s
    return ev


@pytest.mark.parametrize("name", list(fc.CASES))
def test_host_all_tracks_is_the_model_on_a_hand_made_case(name):
    F, K, L, q, frames, must, counts = fc.CASES[name]
    ev = check_host(frames, F, K, L, q)
    if not any(fr[1] == fc.HOST for fr in frames):
        assert must <= set().union(*ev)


def test_host_all_tracks_is_the_model_on_random_segments():
    seen = set()
    for F, K, L, q, segments in fc.random_cases():
        for seg in segments:
            for ev in check_host(seg, F, K, L, q):
                seen |= ev
    assert seen == {"match", "tie_slot", "tie_cand", "miss", "freed", "seed", "reseed", "drop"}


def test_the_model_tells_best_pair_first_from_slot_order():
    F, K, L, q, frames, _, _ = fc.CASES["crossing"]
    assert fc.model_faces(*fc.pack(frames, K), F, L, q)[0][:, 1].tolist() == [list(fc.Y), list(fc.X)]
    assert fc.model_faces(*fc.pack(frames, K), F, L, q, slot_order=True)[0][:, 1].tolist() == [list(fc.X), list(fc.Y)]


# ---------------------------------------------------------------- the three consequences
@pytest.mark.parametrize("K,L,q", [(1, 0, 64), (3, 1, 1), (16, 25, 256), (8, 250, 64), (8, 0, 64)])
def test_one_slot_is_the_single_track_with_pick_score(K, L, q):
    from wav2lip_amd.face_detection.faces import host_all_tracks
    from wav2lip_amd.face_detection.track import FaceTrack, host_track
    rng = np.random.default_rng([K, L, q])
    for n in fc.LENGTHS:
        frames = fc.random_case(rng, n, K)
        arenas = fc.pack(frames, K)
        rects, flags, _, _ = fc.model_faces(*arenas, 1, L, q)
        clip = [(list(c[:K]), f) for c, f, *_ in frames]
        want_r, want_f, _, _ = tc.model_track(clip, "score", L, q)
        assert np.array_equal(rects[0], want_r) and np.array_equal(flags[0], want_f)
        plain = per_frame([fr for fr in frames if fr[1] != fc.HOST], K)
        assert host_all_tracks(plain, 1, q, L)[0] == host_track(plain, FaceTrack("score", K, L, q / 256))[0]


def test_at_most_one_candidate_and_no_tolerance_is_the_untracked_sequence():
    from wav2lip_amd.face_detection.faces import host_all_tracks
    rng = np.random.default_rng(3)
    for F in fc.FS:
        frames = [fc.found(tuple(int(v) for v in np.sort(rng.integers(0, 60, 4))[[0, 1, 2, 3]])) if rng.random() < 0.7 else fc.NO_FACE
                  for _ in range(40)]
        rects, flags, (started, dropped, peak), _ = fc.model_faces(*fc.pack(frames, 4), F, 0, 64)
        assert flags[0].tolist() == [int(f == fc.FOUND) for _, f in frames] and not flags[1:].any() and dropped == 0 and peak == 1
        assert [tuple(r) for r, f in zip(rects[0].tolist(), flags[0]) if f] == [c[0] for c, f in frames if f == fc.FOUND]
        got = host_all_tracks(per_frame(frames, 4), F, 64, 0)
        assert got[0] == [c[0] if c else None for c, _ in frames] and all(r is None for rows in got[1:] for r in rows)


@pytest.mark.parametrize("L", [0, 1, 5, 25])
def test_two_tracks_in_one_slot_and_the_span_rule(L):
    """Where a slot starts a track after another one, at least L rows of flag 0 lie between the two - exactly L when the slot is
    seeded again in the very frame it was freed (step 5), L + 1 or more otherwise - so the span rule with bridge < L begins a new
    span at every seed.  It is not L + 1 for every reuse: the same-frame seed, which the rule and the F = 1 equality with
    w2l_face_track_segments demand, makes it L, and with bridge = L the span rule bridges exactly that case (the
    slot-reuse limit): pinned here as it is."""
    rng = np.random.default_rng(L)
    reused = same_frame = 0
    for F, K in ((1, 3), (2, 4), (4, 8)):
        frames = fc.random_case(rng, 400, K, hi=60, p_host=0.0, p_none=0.45)
        seeds = []
        rects, flags, _, ev = fc.model_faces(*fc.pack(frames, K), F, L, 64, seeds=seeds)
        for t in range(F):
            mine = [i for s, i in seeds if s == t]
            gaps = {i: i - np.flatnonzero(flags[t, :i])[-1] - 1 for i in mine[1:]}
            for i, gap in gaps.items():
                assert gap >= L and (gap > L or "reseed" in ev[i])
            reused += len(gaps)
            same_frame += sum(gap == L for gap in gaps.values())
            for bridge in {0, L // 2, L}:
                _, _, rows, (code, count) = sc.model(rects[t], flags[t], bridge, 1, 0)
                starts = {a for a, _, _, _ in rows[:count].tolist()}
                assert code == 0 and {i for i in mine if i not in gaps or gaps[i] > bridge} <= starts
                assert not {i for i, gap in gaps.items() if gap <= bridge} & starts
    assert reused > 10 and same_frame > 0


def test_a_slot_seeded_in_the_frame_it_is_freed_lies_L_rows_after_its_last_track():
    """the rule itself: the slot that lost its track did missed > L in this frame, and step 5 seeds it in the same frame"""
    A, FAR = fc.A, fc.FAR
    for L in (0, 1, 4):
        frames = [fc.found(A)] + [fc.NO_FACE] * L + [fc.found(FAR)] + [fc.found(FAR)]
        rects, flags, (started, _, _), _ = fc.model_faces(*fc.pack(frames, 2), 1, L, 64)
        assert flags[0].tolist() == [1] + [0] * L + [1, 1] and started == 2
        two = fc.model_faces(*fc.pack(frames, 2), 2, L, 64)      # a free slot is lower only if it is: slot 0 is freed and taken again
        assert two[1][0].tolist() == [1] + [0] * L + [1, 1] and not two[1][1].any()


# ---------------------------------------------------------------- the parameter check and the parsers
def test_check_faces_at_every_range_end():
    from wav2lip_amd.face_detection import AllFaces
    from wav2lip_amd.face_detection.faces import check_faces, faces_kw
    assert check_faces(None) is None and faces_kw(None) == {}
    assert check_faces(AllFaces()) == AllFaces(4, 8, 0.25) == check_faces((4, 8, 0.25))
    assert faces_kw(AllFaces(2)) == {"all_faces": AllFaces(2, 8, 0.25)}
    for ok in (AllFaces(1, 1, 1 / 256), AllFaces(16, 16, 1.0), AllFaces(np.int64(3), np.int32(2), np.float32(0.5)), AllFaces(4, 8, 1)):
        got = check_faces(ok)
        assert type(got.max_faces) is int and type(got.cands) is int and type(got.min_iou) is float
    for bad in (AllFaces(0), AllFaces(17), AllFaces(4, 0), AllFaces(4, 17), AllFaces(4, 8, 0.0), AllFaces(4, 8, 0.0039), AllFaces(4, 8, 1.01),
                AllFaces(4, 8, float("nan")), AllFaces(True), AllFaces(4, False), AllFaces(4, 8, True), AllFaces(2.0), AllFaces(4, "8"),
                AllFaces(4, 8, "x"), 4, "all", (1, 2, 3, 4)):
        with pytest.raises(ValueError, match="all_faces"):
            check_faces(bad)


def test_the_command_line(capsys):
    from wav2lip_amd import calculate_scores_real_videos as rv
    from wav2lip_amd.face_detection import AllFaces
    from wav2lip_amd.face_detection.faces import faces_from_args
    p = rv.build_cli_parser()
    assert faces_from_args(p.parse_args(ARGV)) is None and faces_from_args(object()) is None
    assert p.parse_args(ARGV).all_faces is False and p.parse_args(ARGV).max_faces is None
    assert faces_from_args(p.parse_args(ARGV + ["--all_faces"])) == AllFaces(4, 8, 0.25)
    full = ["--all_faces", "--max_faces", "16", "--face_track_cands", "1", "--face_track_iou", "1.0"]
    assert faces_from_args(p.parse_args(ARGV + full)) == AllFaces(16, 1, 1.0)
    assert faces_from_args(p.parse_args(ARGV + ["--all_faces", "--max_faces", "1", "--face_track_iou", "0.00390625"])) == AllFaces(1, 8, 1 / 256)
    for bad in ("0", "17", "x", "2.5"):
        with pytest.raises(SystemExit):
            p.parse_args(ARGV + ["--all_faces", "--max_faces", bad])
    with pytest.raises(ValueError, match="needs --all_faces"):
        faces_from_args(p.parse_args(ARGV + ["--max_faces", "2"]))
    with pytest.raises(ValueError, match="give one of them"):
        faces_from_args(p.parse_args(ARGV + ["--all_faces", "--face_track", "left"]))
    with pytest.raises(ValueError, match="--num_failed_det"):
        faces_from_args(p.parse_args(ARGV + ["--all_faces", "--face_track_reseed", "2"]))
    # the reference's parser does not take the flags
    with pytest.raises(SystemExit):
        rv.build_parser().parse_args(ARGV + ["--all_faces"])
    capsys.readouterr()


def test_the_command_refuses_the_conflicts_before_any_device_work(monkeypatch, capsys):
    from wav2lip_amd import calculate_scores_real_videos as rv
    import torch
    monkeypatch.setattr(torch.cuda, "current_device", lambda: pytest.fail("the device was touched"))
    for extra, text in ((["--face_track", "score"], "give one of them"), (["--box", "0", "4", "0", "4"], "--box")):
        with pytest.raises(SystemExit):
            rv.main(ARGV + ["--all_faces"] + extra)
        assert text in capsys.readouterr().err


def test_detect_many_refuses_the_combinations_up_front():
    from wav2lip_amd.face_detection import AllFaces, TrackSpans, detect_many

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("the detector was used")

    for kw, text in ((dict(), "needs track_spans"), (dict(track_spans=TrackSpans(), face_track="score"), "face_track"),
                     (dict(no_face_hold=2), "no_face_hold"), (dict(track_spans=TrackSpans(), all_faces=AllFaces(0)), "max_faces")):
        with pytest.raises(ValueError, match=text):
            list(detect_many(Untouched(), [], **{"all_faces": AllFaces(), **kw}))


# ---------------------------------------------------------------- the expanded table
def test_the_expanded_segment_table():
    from wav2lip_amd.face_detection.faces import expand_segments
    segs = [(0, 5, 40, 50), (5, 0, 40, 50), (5, 7, 40, 50)]
    wide = expand_segments(segs, 3, 12)
    assert len(wide) == 9
    for t in range(3):
        for k, (row0, n, H, W) in enumerate(segs):
            assert wide[t * 3 + k] == (t * 12 + row0, n, H, W)
    assert expand_segments(segs, 1, 12) == segs and expand_segments([], 4, 0) == []


# ---------------------------------------------------------------- detect_many's host path
class Stub:
    """a detector whose frames name their candidates: pixel (0, 0, 0) is an index into `tables`"""
    device = "cpu"

    def __init__(self, tables):
        self.tables, self.calls = tables, []

    def get_candidates_for_batch(self, images, K):
        self.calls.append((len(images), K))
        return [list(self.tables[int(f[0, 0, 0])][:K]) for f in images]

    def __getattr__(self, name):
        raise AssertionError("the host path used detector.%s" % name)


def expected_tracks(cands, F, K, q, spans, H, W, pads, T):
    """the model of the rule, the span model per slot, the finish model per slot -> [(slot, a, b, boxes, detected)] by (a, slot)"""
    frames = [fc.found(*c[:K]) if c else fc.NO_FACE for c in cands]
    rects, flags, (_, dropped, _), _ = fc.model_faces(*fc.pack(frames, K), F, spans[0], q)
    out = []
    for t in range(F):
        r2, f2, rows, (code, count) = sc.model(rects[t], flags[t], *spans)
        boxes, valid = noface.model(sc.filled_rects(r2, f2), H, W, pads, T, 0)
        for a, n, det, _ in rows[:count].tolist():
            assert valid[a:a + n].all()
            out.append((t, a, a + n, boxes[a:a + n], det))
    return sorted(out, key=lambda s: (s[1], s[0])), dropped


def test_detect_many_host_path_on_a_stub_detector():
    from wav2lip_amd.face_detection import AllFaces, DetectJob, TrackSpans, detect_many
    from wav2lip_amd.face_detection.faces import FaceSpans
    a, b, c = (4, 6, 20, 26), (30, 8, 48, 30), (50, 30, 62, 44)
    tables = [[], [a, b], [b, a], [a], [b, a, c], [c, b, a]]
    clips = {"swap": [1, 2] * 6, "leaves": [1, 2, 1, 3, 3, 3, 3, 3, 2, 1, 2, 1], "third": [1, 4, 5, 4, 5, 4, 1, 2], "none": [0] * 5,
             "gaps": [0, 1, 0, 0, 2, 1, 0, 0, 0, 1, 2, 1, 0]}
    H, W, pads, T = 48, 64, (0, 10, 0, 0), 5
    for faces, spans in ((AllFaces(2, 8, 0.25), TrackSpans(2, 3, 0)), (AllFaces(4, 2, 0.25), TrackSpans(0, 1, 0)),
                         (AllFaces(1, 8, 0.5), TrackSpans(3, 2, 10))):
        det = Stub(tables)
        jobs = []
        for key, ids in clips.items():
            frames = np.zeros((len(ids), H, W, 3), np.uint8)
            frames[:, 0, 0, 0] = ids
            jobs.append(DetectJob(key, list(frames)))
        jobs.append(DetectJob("empty", []))
        got = list(detect_many(det, jobs, pads=pads, T=T, batch_size=4, max_group_bytes=1, track_spans=spans, all_faces=faces))
        assert [k for k, _, _ in got] == list(clips) + ["empty"] and all(e is None for _, _, e in got)
        assert all(K == faces.cands for _, K in det.calls)
        total = 0
        for (key, res, _), ids in zip(got, list(clips.values()) + [[]]):
            assert isinstance(res, FaceSpans) and len(res) == len(ids)
            want, dropped = expected_tracks([tables[i] for i in ids], faces.max_faces, faces.cands, int(faces.min_iou * 256), spans, H, W,
                                            pads, T) if ids else ([], 0)
            assert res.dropped == dropped, key
            assert [(t.slot, t.a, t.b, t.detected) for t in res.tracks] == [(s, lo, hi, det_) for s, lo, hi, _, det_ in want], key
            for t, (_, lo, hi, boxes, _) in zip(res.tracks, want):
                assert t.boxes.shape == (hi - lo, 4) and np.issubdtype(t.boxes.dtype, np.integer) and np.array_equal(t.boxes, boxes)
            total += len(res.tracks)
        assert total >= 3
    # the two faces of "swap" are two tracks over the whole clip, and the third face of "third" is dropped with F = 2
    det = Stub(tables)
    spans = TrackSpans(2, 3, 0)
    (_, swap, _), (_, third, _) = detect_many(det, [DetectJob(k, list(np.full((len(clips[k]), H, W, 3), 0, np.uint8) + np.array(
        clips[k], np.uint8)[:, None, None, None])) for k in ("swap", "third")], pads=pads, T=T, batch_size=4, max_group_bytes=1,
        track_spans=spans, all_faces=AllFaces(2))
    assert [(t.slot, t.a, t.b) for t in swap.tracks] == [(0, 0, 12), (1, 0, 12)] and swap.dropped == 0
    assert all(t.boxes[:, 2].max() < 25 for t in swap.tracks if t.slot == 0) and third.dropped == 5


# ---------------------------------------------------------------- the C ABI
def test_the_entry_is_bound_with_the_arguments_the_header_declares():
    from wav2lip_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "w2l_hip.h")).read(), flags=re.S)
    args = re.search(r"int w2l_face_tracks_all_segments\(([^)]*)\);", header).group(1).split(",")
    assert len(args) == 14 and [a.split()[-1].lstrip("*") for a in args] == [
        "stream", "n_seg", "segs", "cands", "ncand", "cflags", "n_rows", "K", "F", "L", "q", "rects_out", "flags_out", "status"]
    want = [ctypes.c_void_p if "*" in a else ctypes.c_int for a in args]
    assert _lib.SIGNATURES["w2l_face_tracks_all_segments"] == (ctypes.c_int, want)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "w2l_face_tracks_all_segments")
    kernel_file = open(os.path.join(ROOT, "wav2lip_amd", "csrc", "detect.hip")).read()
    assert re.search(r"^//   w2l_face_tracks_all_segments ", kernel_file, flags=re.M)
    from wav2lip_amd.face_detection import faces
    assert (faces.MAX_FACES, faces.AllFaces._field_defaults) == (16, {"max_faces": 4, "cands": 8, "min_iou": 0.25})


def test_the_launcher_refuses_what_is_out_of_range_without_a_device():
    from wav2lip_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int32 * 256)()
    p = ctypes.addressof(buf)
    base = p + (-p % 16)

    def go(n_seg=1, segs=base, cands=base, n_rows=4, K=8, F=4, L=0, q=64, rects=base, flags=base, status=base):
        return lib.w2l_face_tracks_all_segments(None, n_seg, segs, cands, base, base, n_rows, K, F, L, q, rects, flags, status)

    for kw in (dict(K=0), dict(K=17), dict(F=0), dict(F=17), dict(L=-1), dict(L=251), dict(q=0), dict(q=257), dict(n_seg=0), dict(n_rows=-1),
               dict(segs=None), dict(cands=None), dict(rects=None), dict(flags=None), dict(status=None), dict(segs=base + 4),
               dict(cands=base + 8), dict(rects=base + 4), dict(F=16, n_rows=1 << 25), dict(F=1, n_rows=1 << 29)):
        assert go(**kw) != 0 and b"face_tracks_all_segments" in lib.w2l_last_error(), kw
