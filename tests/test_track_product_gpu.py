"""Tracked face selection through the front ends: `inference.face_detect`, `face_detection.detect_many` and the
live streams' `streaming.DeviceBoxes`, each with `face_track=...`, against the model of tests/_track_cases.py followed by today's
finish.  The detector's box table is prescribed per frame through `FaceAlignment._candidates` (the frame's first pixel names its
table), so the real gate, NMS, w2l_s3fd_top_rects, w2l_face_track_segments and box finishes run on small frames without a
network."""
import numpy as np
import pytest
import torch

import _track_cases as tc

pytestmark = pytest.mark.gpu

PADS = (0, 10, 0, 0)
FACES = {"a": (4, 6, 20, 26), "b": (30, 8, 48, 30), "c": (50, 30, 62, 44)}      # apart: the NMS keeps every one of them
WIDE = (10.0, 10.0, 40000.0, 30.0)               # a coordinate above 32767: the device leaves the frame to the host


class World:
    """box tables by frame id (0..255), and frames that name them: pixel (0,0) holds the id in all three channels, pixel (0,1) is 0"""
    P = 4

    def __init__(self):
        self.tables = np.zeros((256, self.P, 5), np.float32)
        self.tables[:, :, :4] = (1, 1, 2, 2)
        self.tables[:, :, 4] = 0.01                          # below the gate
        self.n = 0

    def add(self, rows):
        """rows: [(rect, score)], at most P; scores distinct, so the keep order is the score order"""
        assert self.n < 256 and len(rows) <= self.P and len({s for _, s in rows}) == len(rows)
        for k, (rect, score) in enumerate(rows):
            self.tables[self.n, k] = tuple(rect) + (score,)
        self.n += 1
        return self.n - 1

    def frames(self, ids, H=48, W=64):
        out = np.zeros((len(ids), H, W, 3), np.uint8)
        out[:, 2:, :, :] = 90                               # something to crop
        for i, fid in enumerate(ids):
            out[i, 0, 0] = fid
        return out

    def candidates(self, fid, K):
        """what the detector path must find for the frame: the rows above the gate in score order through the model; a frame the
        device flags goes through Python's int() without the bound, as the host rule does"""
        t = self.tables[fid]
        keep = np.array(sorted(range(self.P), key=lambda r: -t[r, 4]), np.int32)
        n = int((t[:, 4] > 0.05).sum())
        cands, flag = tc.model_top_rects(t, keep, n, K)
        if flag == tc.HOST:
            cands = [tuple(int(v) for v in np.maximum(t[r, :4], 0)) for r in keep[:n] if t[r, 4] > 0.5][:K]
        return cands, flag

    def rects(self, ids, track):
        """(rect or None per frame, whether a frame was left to the host) for a clip of these frames under `track`"""
        from wav2lip_amd.face_detection.track import iou_q8
        per = [self.candidates(fid, track.cands) for fid in ids]
        host = any(f == tc.HOST for _, f in per)
        frames = [(c, tc.FOUND if c else tc.NONE) for c, _ in per]
        r, f, _, _ = tc.model_track(frames, track.pick, track.reseed, iou_q8(track.min_iou))
        return [tuple(int(v) for v in x) if y == tc.FOUND else None for x, y in zip(r, f)], host


def detector(cuda, world):
    from wav2lip_amd import face_detection
    from wav2lip_amd._lib import check, current_stream, load
    from wav2lip_amd.face_detection.s3fd import nms_batch

    class Prescribed(face_detection.FaceAlignment):
        def __init__(self):
            self.device, self.precision, self.det_scale = str(cuda), "f32", 1
            self.tables = torch.from_numpy(world.tables).to(cuda)
            self.batches = []

        def _candidates(self, images, rows=None, resolve=True):
            if rows is None:
                ids = torch.tensor([int(f[0, 0, 0]) for f in images], dtype=torch.long, device=cuda)
            else:                                            # a device address table: the pixels through the detector's own pack kernel
                B, H, W = rows
                y = torch.empty((B, H, W, 4), dtype=torch.float32, device=cuda)
                check(load().w2l_s3fd_pack_rows(current_stream(), B, H, W, images.data_ptr(), y.data_ptr(), 4), "s3fd_pack_rows")
                ids = (y[:, 0, 0, 0] - y[:, 0, 1, 0]).round().long()
            self.batches.append(len(ids))
            table = self.tables.index_select(0, ids).contiguous()
            keep, counts = nms_batch(table, 0.05, 0.3, host_overflow=resolve and rows is None)      # rows: nothing is read back
            return table, keep, counts

    return Prescribed()


def jitter(rect, d):
    return (rect[0] + d, rect[1], rect[2] + d, rect[3] + (d % 2))


def swapping_clip(world, n, faces=("a", "b"), gaps=(), extra=None):
    """frame ids of a clip in which the named faces drift and swap score order every other frame; `gaps`: frames with no face at all;
    `extra`: {frame: rows} to put other tables in"""
    ids = []
    for i in range(n):
        if extra and i in extra:
            ids.append(world.add(extra[i]))
            continue
        if i in gaps:
            ids.append(world.add([]))
            continue
        rows = [(jitter(FACES[f], i % 3), 0.9 - 0.1 * ((k + i) % len(faces)) - 0.001 * i) for k, f in enumerate(faces)]
        ids.append(world.add(rows + [((0, 0, 5, 5), 0.3)]))      # and a box the 0.5 threshold drops
    return ids


def finish(rects, H, W, T, hold):
    """today's finish of `face_detect` on rects: the coords per frame (None for a gap frame), or the ValueError's text"""
    from wav2lip_amd.face_detection import many
    if hold is None:
        if any(r is None for r in rects):
            return many.NO_FACE
        return [tuple(int(v) for v in b) for b in many.host_boxes(rects, H, W, PADS, T)]
    if len(rects) == 1 and rects[0] is None:
        return many.NO_FACE
    boxes, valid = many.host_boxes_runs(rects, H, W, PADS, T, hold)
    return [tuple(int(v) for v in b) if ok else None for b, ok in zip(boxes, valid)]


def run_face_detect(det, frames, track, hold, nosmooth=False, batch_size=4):
    from wav2lip_amd import inference
    kw = {} if hold is None else {"no_face_hold": hold}
    try:
        out = inference.face_detect(list(frames), detector=det, pads=list(PADS), nosmooth=nosmooth, batch_size=batch_size,
                                    face_track=track, **kw)
    except ValueError as e:
        return str(e)
    for (face, coords), f in zip(out, frames):
        assert (face is None) == (coords is None)
        if coords is not None:
            y1, y2, x1, x2 = coords
            assert np.array_equal(face, f[y1:y2, x1:x2])
    return [None if c is None else tuple(int(v) for v in c) for _, c in out]


def count_reads(monkeypatch):
    """counts the calls that bring device data to the host: Tensor.cpu / item / tolist / nonzero on a device tensor"""
    seen = []
    for name in ("cpu", "item", "tolist", "nonzero"):
        orig = getattr(torch.Tensor, name)

        def wrapped(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                seen.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, wrapped)
    return seen


def spy_kernels(monkeypatch):
    from wav2lip_amd import _lib
    lib, calls = _lib.load(), []
    for name in ("w2l_s3fd_top_rects", "w2l_face_track_segments", "w2l_s3fd_first_rect"):
        fn = getattr(lib, name)

        def wrapped(*a, _fn=fn, _name=name):
            calls.append(_name)
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapped)
    return calls


TRACKS = [("score", 8, 0, 0.25), ("right", 8, 0, 0.25), ("left", 2, 2, 0.5), ("largest", 3, 1, 0.1)]


# ---------------------------------------------------------------- face_detect
@pytest.mark.parametrize("track", TRACKS)
@pytest.mark.parametrize("hold", [None, 2])
def test_face_detect_equals_the_model_followed_by_todays_finish(cuda, monkeypatch, track, hold):
    from wav2lip_amd.face_detection.track import FaceTrack
    track = FaceTrack(*track)
    world = World()
    clips = {"swap": swapping_clip(world, 10), "three": swapping_clip(world, 7, faces=("c", "a", "b")),
             "gaps": swapping_clip(world, 11, gaps=(0, 4, 5, 6, 10)), "one": swapping_clip(world, 1),
             "enter": swapping_clip(world, 9, extra={i: [(jitter(FACES["c"], i), 0.8)] for i in (0, 1, 2, 6)})}
    det = detector(cuda, world)
    reads = count_reads(monkeypatch)
    for name, ids in clips.items():
        frames = world.frames(ids)
        rects, host = world.rects(ids, track)
        assert not host
        for nosmooth in (False, True):
            del reads[:], det.batches[:]
            got = run_face_detect(det, frames, track, hold, nosmooth)
            assert got == finish(rects, 48, 64, 0 if nosmooth else 5, hold), (name, nosmooth)
            assert reads == ["cpu"] and det.batches == [4] * (len(ids) // 4) + [len(ids) % 4] * (len(ids) % 4 > 0)      # ONE copy back
    # the defining case: untracked, the rect jumps between the two heads; tracked, it stays on one
    ids = clips["swap"]
    untracked = [world.candidates(fid, 1)[0][0] for fid in ids]
    tracked, _ = world.rects(ids, track)
    assert len({r[0] < 25 for r in untracked}) == 2 and len({r[0] < 25 for r in tracked}) == 1      # face a lies left of x = 25
    assert run_face_detect(det, world.frames(ids), None, None, True) == finish(untracked, 48, 64, 0, None)
    if track.reseed == 0:
        assert isinstance(finish(world.rects(clips["gaps"], track)[0], 48, 64, 5, None), str)      # strict: still the reference's error


def test_a_clip_with_a_frame_left_to_the_host_takes_the_host_path(cuda, monkeypatch):
    from wav2lip_amd.face_detection.track import FaceTrack
    world = World()
    wide = {3: [(WIDE, 0.95), (jitter(FACES["b"], 1), 0.7)]}
    clips = {"wide": swapping_clip(world, 9, extra=wide), "wide_first": swapping_clip(world, 5, extra={0: wide[3]}),
             "wide_gap": swapping_clip(world, 8, gaps=(1, 2), extra={5: wide[3]})}
    det = detector(cuda, world)
    calls, took_wide = spy_kernels(monkeypatch), set()
    for name, ids in clips.items():
        for track, hold in ((FaceTrack("right"), None), (FaceTrack("score", 4, 1, 0.25), 3), (FaceTrack("left", 1), 0)):
            rects, host = world.rects(ids, track)
            assert host
            if any(r is not None and r[2] == 40000 for r in rects):
                took_wide.add((name, track.pick))
            del calls[:]
            assert run_face_detect(det, world.frames(ids), track, hold) == finish(rects, 48, 64, 5, hold), (name, track)
            # the device pass (which flags the frame), then the per-batch host pass: no second track launch
            n_batches = (len(ids) + 3) // 4
            assert calls == ["w2l_s3fd_top_rects"] * n_batches + ["w2l_face_track_segments"] + ["w2l_s3fd_top_rects"] * n_batches
    assert ("wide_first", "score") in took_wide and ("wide", "right") not in took_wide     # the host's rect is used, and followed past
    # a coordinate int() refuses raises what it raises there
    ids = swapping_clip(world, 4, extra={2: [((3.0, float("nan"), 9.0, 9.0), 0.9)]})
    with pytest.raises(ValueError):
        from wav2lip_amd import inference
        inference.face_detect(list(world.frames(ids)), detector=det, pads=list(PADS), nosmooth=False, batch_size=4, face_track="score")


def test_without_the_keyword_neither_new_kernel_is_launched(cuda, monkeypatch):
    world = World()
    ids = swapping_clip(world, 10)
    det = detector(cuda, world)
    calls = spy_kernels(monkeypatch)
    untracked = [world.candidates(fid, 1)[0][0] for fid in ids]
    assert run_face_detect(det, world.frames(ids), None, None) == finish(untracked, 48, 64, 5, None)
    assert calls == ["w2l_s3fd_first_rect"] * 3
    del calls[:]
    run_face_detect(det, world.frames(ids), "score", None)
    assert calls == ["w2l_s3fd_top_rects"] * 3 + ["w2l_face_track_segments"]
    # K = 1 is the untracked rule, through the new kernels
    from wav2lip_amd.face_detection.track import FaceTrack
    for pick in tc.PICKS:
        assert run_face_detect(det, world.frames(ids), FaceTrack(pick, 1), None) == finish(untracked, 48, 64, 5, None)


def test_get_candidates_for_batch(cuda):
    world = World()
    ids = swapping_clip(world, 6, faces=("b", "c", "a"), gaps=(2,), extra={4: [(WIDE, 0.95), (FACES["a"], 0.6)]})
    det = detector(cuda, world)
    for K in (1, 2, 16):
        got = det.get_candidates_for_batch(world.frames(ids), K)
        assert got == [world.candidates(fid, K)[0] for fid in ids]
        assert all(type(v) is int for c in got for r in c for v in r)
        assert [c[0] if c else None for c in got] == det.get_detections_for_batch(world.frames(ids))
    assert got[2] == [] and got[4][0][2] == 40000 and len(got[0]) == 3


# ---------------------------------------------------------------- detect_many
def many_jobs(world):
    """clips of two shapes and ragged lengths, one without any face, one that starts without one, one as a device tensor"""
    spec = [("k0", 10, (48, 64), {}), ("k1", 1, (48, 64), {}), ("none", 5, (48, 64), dict(gaps=range(5))), ("k3", 7, (40, 56), {}),
            ("late", 9, (40, 56), dict(gaps=(0, 1, 5))), ("three", 6, (48, 64), dict(faces=("c", "b", "a"))), ("empty", 0, (48, 64), {})]
    out = []
    for key, n, (H, W), kw in spec:
        faces = kw.pop("faces", ("a", "b"))
        if (H, W) == (40, 56):                               # the faces that fit the smaller frame
            faces = ("a", "b")
        ids = swapping_clip(world, n, faces=faces, **kw)
        out.append((key, ids, H, W))
    return out


@pytest.mark.parametrize("track,hold,T", [(("score", 8, 0, 0.25), None, 5), (("right", 8, 0, 0.25), None, 0), (("left", 3, 2, 0.25), 2, 5),
                                          (("largest", 8, 1, 0.5), 0, 3)])
def test_detect_many_equals_face_detect_per_job(cuda, monkeypatch, track, hold, T):
    from wav2lip_amd import face_detection
    from wav2lip_amd.face_detection import many
    from wav2lip_amd.face_detection.track import FaceTrack
    track = FaceTrack(*track)
    world = World()
    spec = many_jobs(world)
    det = detector(cuda, world)
    jobs = []
    for k, (key, ids, H, W) in enumerate(spec):
        frames = world.frames(ids, H, W)
        jobs.append(face_detection.DetectJob(key, torch.from_numpy(frames).to(cuda) if k == 3 else list(frames)))
    calls, reads = spy_kernels(monkeypatch), count_reads(monkeypatch)
    kw = {} if hold is None else {"no_face_hold": hold}
    got = list(face_detection.detect_many(det, jobs, pads=PADS, T=T, batch_size=4, face_track=track, **kw))
    # three groups (the shape changes twice), each: its batches of candidates, ONE track launch, and ONE copy back
    assert calls.count("w2l_face_track_segments") == 3 == len(reads) and set(reads) == {"cpu"}
    assert "w2l_s3fd_first_rect" not in calls and calls.count("w2l_s3fd_top_rects") == 4 + 4 + 2
    assert [key for key, _, _ in got] == [key for key, _, _, _ in spec]
    errors = 0
    for (key, boxes, error), (_, ids, H, W) in zip(got, spec):
        rects, host = world.rects(ids, track)
        want = finish(rects, H, W, T, hold) if ids else []
        assert not host
        if isinstance(want, str):
            assert boxes is None and error == want == many.NO_FACE, key
            errors += 1
            continue
        assert error is None and len(boxes) == len(ids), key
        assert [None if b is None else tuple(int(v) for v in b) for b in boxes] == want, key
        if T == 5 and ids:                                   # and per-job face_detect says the same
            assert run_face_detect(det, world.frames(ids, H, W), track, hold) == want, key
    assert errors == (2 if hold is None else 0)              # "none" and "late" in the strict mode: the error text stays an error text
    # without the keyword the launches are what they were
    del calls[:]
    list(face_detection.detect_many(det, jobs[:2], pads=PADS, T=T, batch_size=4, **kw))
    assert calls == ["w2l_s3fd_first_rect"] * 3


def test_detect_many_sends_a_clip_with_a_host_frame_through_face_detect_with_the_track(cuda):
    from wav2lip_amd import face_detection
    from wav2lip_amd.face_detection.track import FaceTrack
    world = World()
    wide = [(WIDE, 0.95), (jitter(FACES["b"], 1), 0.7)]
    spec = [("k0", swapping_clip(world, 6)), ("wide", swapping_clip(world, 7, extra={2: wide})), ("k2", swapping_clip(world, 3))]
    det = detector(cuda, world)
    for track, hold, T in ((FaceTrack("score"), None, 5), (FaceTrack("right", 4, 1), 1, 5), (FaceTrack("score", 2), None, 2)):
        kw = {} if hold is None else {"no_face_hold": hold}
        jobs = [face_detection.DetectJob(key, list(world.frames(ids))) for key, ids in spec]
        got = list(face_detection.detect_many(det, jobs, pads=PADS, T=T, batch_size=4, face_track=track, **kw))
        for (key, boxes, error), (_, ids) in zip(got, spec):
            rects, host = world.rects(ids, track)
            assert host == (key == "wide") and error is None
            assert [None if b is None else tuple(int(v) for v in b) for b in boxes] == finish(rects, 48, 64, T, hold), (key, track)


# ---------------------------------------------------------------- live streams
@pytest.mark.parametrize("track,hold", [(("score", 8, 0, 0.25), None), (("right", 2, 0, 0.25), None), (("left", 8, 3, 0.25), 3),
                                        (("largest", 3, 1, 0.25), 0)])
def test_streams_fed_in_uneven_pieces_equal_face_detect_on_the_finished_video(cuda, monkeypatch, track, hold):
    from wav2lip_amd import streaming
    from wav2lip_amd.face_detection.track import FaceTrack
    track = FaceTrack(*track)
    world = World()
    gaps = {} if hold is None else dict(gaps=(0, 6, 7, 8, 9, 10, 20))
    videos = {0: (swapping_clip(world, 23, **gaps), 48, 64), 1: (swapping_clip(world, 17, faces=("b", "a")), 40, 56),
              5: (swapping_clip(world, 9, faces=("c", "a", "b")), 48, 64)}
    pieces = {0: [3, 1, 0, 5, 2, 12], 1: [1, 1, 8, 0, 7], 5: [9]}
    det = detector(cuda, world)
    boxes = streaming.DeviceBoxes(cuda, det, PADS, 5, 4, **({} if hold is None else {"hold": hold}), track=track)
    boxes.reserve(6)
    calls = spy_kernels(monkeypatch)
    got, seen, ticks = {s: [] for s in videos}, dict.fromkeys(videos, 0), 0
    while any(pieces.values()):
        items, order = [], []
        for s, (ids, H, W) in videos.items():
            if not pieces[s]:
                continue
            n = pieces[s].pop(0)
            fresh = list(world.frames(ids[seen[s]:seen[s] + n], H, W))
            items.append((fresh, H, W, s, seen[s], not pieces[s]))
            order.append(s)
            seen[s] += n
        del calls[:]
        res = boxes.collect(boxes.launch(items))
        assert calls.count("w2l_face_track_segments") == 1 and "w2l_s3fd_first_rect" not in calls      # one launch per tick, for all
        ticks += 1
        for s, r in zip(order, res):
            assert r[1] == (0, 0), (s, r[1])
            if hold is None:
                got[s] += [tuple(int(v) for v in b) for b in r[0]]
            else:
                got[s] += [tuple(int(v) for v in b) if ok else None for b, ok in zip(r[0], r[2])]
    assert ticks == 6
    for s, (ids, H, W) in videos.items():
        rects, host = world.rects(ids, track)
        want = finish(rects, H, W, 5, hold)
        assert not host and got[s] == want, s
        assert run_face_detect(det, world.frames(ids, H, W), track, hold) == want
    # slots 2..4 of the state table were never named
    assert not boxes.track_state[[2, 3, 4]].any().item() and boxes.track_state[0].cpu().tolist()[4] in (0, 1)


def test_a_stream_whose_slot_is_used_again_starts_fresh(cuda):
    from wav2lip_amd import streaming
    from wav2lip_amd.face_detection.track import FaceTrack
    track = FaceTrack("left")
    world = World()
    first, second = swapping_clip(world, 6, faces=("a", "b")), swapping_clip(world, 6, faces=("c", "b"))
    det = detector(cuda, world)
    boxes = streaming.DeviceBoxes(cuda, det, PADS, 0, 4, track=track)
    out = []
    for ids in (first, second):                              # the same slot, seen = 0 again: the first video's face is forgotten
        res = boxes.collect(boxes.launch([(list(world.frames(ids)), 48, 64, 0, 0, True)]))
        out.append([tuple(int(v) for v in b) for b in res[0][0]])
    for ids, got in zip((first, second), out):
        assert got == finish(world.rects(ids, track)[0], 48, 64, 0, None)
    assert out[1][0][2] >= 30                                # x1 of face b, the leftmost of the second video
