"""Scene-cut detection through the front ends: `inference.face_detect` and `face_detection.detect_many` with
`scene_cuts=...`, against the composed model of tests/_scene_cases.py.  The detector's box table is prescribed per frame through
`FaceAlignment._candidates` as tests/test_track_product_gpu.py prescribes it (the frame's first pixel names its table), so the real
signature and cut kernels, the gate, NMS, rect kernels, track and box finishes run on small frames without a network.  A shot is a
run of constant frames: dark for one shot, bright for the next."""
import numpy as np
import pytest
import torch

import _scene_cases as sc
import _track_cases as tc

pytestmark = pytest.mark.gpu

PADS = (0, 10, 0, 0)
H, W = 48, 64
DARK, BRIGHT = 30, 220
THRESH = 0.3
FACES = {"a": (4, 6, 20, 26), "b": (30, 8, 48, 30)}            # apart: the NMS keeps both
WIDE = (10.0, 10.0, 40000.0, 30.0)                              # a coordinate above 32767: the device leaves the frame to the host
MODES = {"strict": (None, None), "hold": (2, None), "track": (None, ("left", 4, 0, 0.25)), "hold+track": (2, ("left", 4, 1, 0.25))}


class World:
    """box tables by frame id (0..255), and frames that name them: a constant frame whose pixel (0,0) holds the id in all three
    channels and whose pixel (0,1) is 0 - two pixels of 3072, far below any threshold"""
    P = 4

    def __init__(self):
        self.tables = np.zeros((256, self.P, 5), np.float32)
        self.tables[:, :, :4] = (1, 1, 2, 2)
        self.tables[:, :, 4] = 0.01                          # below the gate
        self.n = 0

    def add(self, rows):
        assert self.n < 256 and len(rows) <= self.P and len({s for _, s in rows}) == len(rows)
        for k, (rect, score) in enumerate(rows):
            self.tables[self.n, k] = tuple(rect) + (score,)
        self.n += 1
        return self.n - 1

    def clip(self, spec):
        """spec: [(level, rows)] per frame -> (ids, frames uint8 [n,H,W,3])"""
        ids = [self.add(rows) for _, rows in spec]
        frames = np.empty((len(spec), H, W, 3), np.uint8)
        for i, (level, _) in enumerate(spec):
            frames[i] = level
            frames[i, 0, 0] = ids[i]
            frames[i, 0, 1] = 0
        return ids, frames

    def candidates(self, fid, K):
        t = self.tables[fid]
        keep = np.array(sorted(range(self.P), key=lambda r: -t[r, 4]), np.int32)
        n = int((t[:, 4] > 0.05).sum())
        cands, flag = tc.model_top_rects(t, keep, n, K)
        if flag == tc.HOST:                                  # the host rule: Python's int() without the bound
            cands = [tuple(int(v) for v in np.maximum(t[r, :4], 0)) for r in keep[:n] if t[r, 4] > 0.5][:K]
        return cands, flag

    def rects(self, ids, shots, track):
        """a rect or None per frame: the detector's first candidate, or under `track` the model's track per shot"""
        from wav2lip_amd.face_detection.track import iou_q8
        K = 1 if track is None else track.cands
        per = [self.candidates(fid, K)[0] for fid in ids]
        if track is None:
            return [c[0] if c else None for c in per]
        return sc.track_shots([(c, tc.FOUND if c else tc.NONE) for c in per], shots, track.pick, track.reseed, iou_q8(track.min_iou))


def detector(cuda, world):
    from wav2lip_amd import face_detection
    from wav2lip_amd._lib import check, current_stream, load
    from wav2lip_amd.face_detection.s3fd import nms_batch

    class Prescribed(face_detection.FaceAlignment):
        def __init__(self):
            self.device, self.precision, self.det_scale = str(cuda), "f32", 1
            self.tables = torch.from_numpy(world.tables).to(cuda)

        def _candidates(self, images, rows=None, resolve=True):
            if rows is not None:                             # a device address table: the pixels through the detector's own pack kernel
                B, Hr, Wr = rows
                y = torch.empty((B, Hr, Wr, 4), dtype=torch.float32, device=cuda)
                check(load().w2l_s3fd_pack_rows(current_stream(), B, Hr, Wr, images.data_ptr(), y.data_ptr(), 4), "s3fd_pack_rows")
                ids = (y[:, 0, 0, 0] - y[:, 0, 1, 0]).round().long()
            elif isinstance(images, torch.Tensor):           # the batch `face_detect` uploads once under scene_cuts
                ids = images[:, 0, 0, 0].long()
            else:
                ids = torch.tensor([int(f[0, 0, 0]) for f in images], dtype=torch.long, device=cuda)
            table = self.tables.index_select(0, ids).contiguous()
            keep, counts = nms_batch(table, 0.05, 0.3, host_overflow=resolve and rows is None)
            return table, keep, counts

    return Prescribed()


def jitter(rect, d):
    return (rect[0] + d, rect[1], rect[2] + d, rect[3] + (d % 2))


def two_faces(i, first="a"):
    """both faces, drifting; `first` has the better score on even frames and the other on odd ones, so the untracked rect jumps"""
    order = ("a", "b") if first == "a" else ("b", "a")
    return [(jitter(FACES[f], i % 3), 0.9 - 0.1 * ((k + i) % 2) - 0.001 * i) for k, f in enumerate(order)]


def shot(level, n, gaps=(), first="a"):
    return [(level, [] if i in gaps else two_faces(i, first)) for i in range(n)]


def model_shots(frames):
    cuts, _ = sc.cut_flags(sc.signatures(frames), H, W, sc.q_of(THRESH))
    return sc.shots(len(frames), cuts)


def mode_args(mode):
    from wav2lip_amd.face_detection.track import FaceTrack
    hold, track = MODES[mode]
    return hold, None if track is None else FaceTrack(*track)


def run_face_detect(det, frames, hold, track, scene=THRESH, nosmooth=False, batch_size=4):
    from wav2lip_amd import inference
    kw = dict({} if hold is None else {"no_face_hold": hold}, **({} if track is None else {"face_track": track}),
              **({} if scene is None else {"scene_cuts": scene}))
    try:
        out = inference.face_detect(list(frames), detector=det, pads=list(PADS), nosmooth=nosmooth, batch_size=batch_size, **kw)
    except ValueError as e:
        return str(e)
    for (face, coords), f in zip(out, frames):
        assert (face is None) == (coords is None)
        if coords is not None:
            y1, y2, x1, x2 = coords
            assert np.array_equal(face, f[y1:y2, x1:x2])
    return [None if c is None else tuple(int(v) for v in c) for _, c in out]


def run_detect_many(det, clips, hold, track, scene=THRESH, T=5, **more):
    """clips: {key: frames} -> {key: list of tuples / None, or the error's text}"""
    from wav2lip_amd import face_detection
    kw = dict({} if hold is None else {"no_face_hold": hold}, **({} if track is None else {"face_track": track}),
              **({} if scene is None else {"scene_cuts": scene}), **more)
    jobs = [face_detection.DetectJob(key, list(frames)) for key, frames in clips.items()]
    out = {}
    for key, boxes, error in face_detection.detect_many(det, jobs, pads=PADS, T=T, batch_size=4, **kw):
        out[key] = error if boxes is None else [None if b is None else tuple(int(v) for v in b) for b in boxes]
    assert list(out) == list(clips)
    return out


def spy_kernels(monkeypatch):
    from wav2lip_amd import _lib
    lib, calls = _lib.load(), []
    for name in ("w2l_frame_hist_rows", "w2l_scene_cuts", "w2l_s3fd_first_rect", "w2l_s3fd_top_rects", "w2l_face_track_segments",
                 "w2l_face_boxes_segments", "w2l_face_boxes_runs"):
        fn = getattr(lib, name)

        def wrapped(*a, _fn=fn, _name=name):
            calls.append(_name)
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapped)
    return calls


def consequence_clips(world, hold):
    """the clips of consequences (a) to (c): one without a cut, one with a cut at every frame, A, B, and A followed by B; under a
    hold A and B hold frames without a face, B's first frame among them"""
    gaps = hold is not None
    a = shot(DARK, 6, gaps=(2,) if gaps else ())
    b = shot(BRIGHT, 7, gaps=(0, 3, 4, 5) if gaps else (), first="b")
    every = [(DARK if i % 2 == 0 else BRIGHT, two_faces(i)) for i in range(5)]
    spec = {"plain": shot(DARK, 9, gaps=(4,) if gaps else ()), "every": every, "A": a, "B": b, "AB": a + b}
    return {key: world.clip(s) for key, s in spec.items()}


def expected(world, clips, hold, track, T):
    want = {}
    for key, (ids, frames) in clips.items():
        shots = model_shots(frames)
        want[key] = sc.finish_shots(world.rects(ids, shots, track), shots, H, W, PADS, T, hold)
    assert len(model_shots(clips["plain"][1])) == 1 and len(model_shots(clips["every"][1])) == 5
    assert model_shots(clips["AB"][1]) == [(0, 6), (6, 13)]
    return want


# ---------------------------------------------------------------- consequences (a) to (c)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_face_detect_consequences(cuda, mode):
    hold, track = mode_args(mode)
    world = World()
    clips = consequence_clips(world, hold)
    det = detector(cuda, world)
    for nosmooth in (False, True):
        want = expected(world, clips, hold, track, 0 if nosmooth else 5)
        got = {key: run_face_detect(det, frames, hold, track, nosmooth=nosmooth) for key, (_, frames) in clips.items()}
        assert got == want, nosmooth
        assert got["plain"] == run_face_detect(det, clips["plain"][1], hold, track, scene=None, nosmooth=nosmooth)       # (a)
        assert got["every"] == run_face_detect(det, clips["every"][1], hold, track, nosmooth=True)                       # (b)
        assert got["AB"] == got["A"] + got["B"]                                                                          # (c)
        for key in ("A", "B"):                                                       # each alone holds no cut
            assert got[key] == run_face_detect(det, clips[key][1], hold, track, scene=None, nosmooth=nosmooth)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_detect_many_consequences(cuda, monkeypatch, mode):
    hold, track = mode_args(mode)
    world = World()
    clips = consequence_clips(world, hold)
    det = detector(cuda, world)
    frames = {key: f for key, (_, f) in clips.items()}
    calls = spy_kernels(monkeypatch)
    for T in (5, 0):
        want = expected(world, clips, hold, track, T)
        del calls[:]
        got = run_detect_many(det, frames, hold, track, T=T)
        assert got == want, T
        # one group: one signature and one cut launch, the batches, at most one track launch and ONE finish launch
        finish = "w2l_face_boxes_segments" if hold is None else "w2l_face_boxes_runs"
        assert calls[:2] == ["w2l_frame_hist_rows", "w2l_scene_cuts"] and calls.count(finish) == 1
        assert calls.count("w2l_face_track_segments") == (track is not None)
        assert calls.count("w2l_frame_hist_rows") == calls.count("w2l_scene_cuts") == 1
        off = run_detect_many(det, frames, hold, track, scene=None, T=T)
        assert got["plain"] == off["plain"] and got["A"] == off["A"] and got["B"] == off["B"]                            # (a)
        assert got["every"] == run_detect_many(det, {"every": frames["every"]}, hold, track, T=0)["every"]               # (b)
        assert got["AB"] == got["A"] + got["B"]                                                                          # (c)
        if T == 5:
            for key in frames:                                                       # and per-job face_detect says the same
                assert run_face_detect(det, frames[key], hold, track) == got[key], key


def test_without_the_keyword_the_launches_are_what_they_were(cuda, monkeypatch):
    world = World()
    ids, frames = world.clip(shot(DARK, 5) + shot(BRIGHT, 5, first="b"))
    det = detector(cuda, world)
    calls = spy_kernels(monkeypatch)
    run_face_detect(det, frames, None, None, scene=None)
    assert calls == ["w2l_s3fd_first_rect"] * 3
    del calls[:]
    run_detect_many(det, {"k": frames}, None, None, scene=None)
    assert calls == ["w2l_s3fd_first_rect"] * 3 + ["w2l_face_boxes_segments"]
    del calls[:]
    run_detect_many(det, {"k": frames}, 2, "left", scene=None)
    assert calls == ["w2l_s3fd_top_rects"] * 3 + ["w2l_face_track_segments", "w2l_face_boxes_runs"]
    del calls[:]
    run_face_detect(det, frames, None, None)
    assert calls == ["w2l_frame_hist_rows", "w2l_s3fd_first_rect"] * 3 + ["w2l_scene_cuts"]
    del calls[:]
    run_face_detect(det, frames, None, "left")
    assert calls == ["w2l_frame_hist_rows", "w2l_s3fd_top_rects"] * 3 + ["w2l_scene_cuts", "w2l_face_track_segments"]


# ---------------------------------------------------------------- further cases
def test_the_hold_does_not_cross_the_cut(cuda):
    world = World()
    ids, frames = world.clip(shot(DARK, 4) + shot(BRIGHT, 4, gaps=(0, 1), first="b"))
    det = detector(cuda, world)
    for run in (lambda **kw: run_face_detect(det, frames, 3, None, **kw), lambda **kw: run_detect_many(det, {"k": frames}, 3, None, **kw)["k"]):
        on, off = run(), run(scene=None)
        assert on[4] is None and on[5] is None and on[6] is not None                 # gaps at the start of the second shot
        assert off[4] is not None and off[5] is not None                             # held across, without the option
        shots = model_shots(frames)
        assert on == sc.finish_shots(world.rects(ids, shots, None), shots, H, W, PADS, 5, 3)


def test_the_track_reseeds_left_at_the_cut(cuda):
    from wav2lip_amd.face_detection.track import FaceTrack
    world = World()
    # the first shot holds face b alone, so the track sits on the RIGHT face when the cut comes; the second shot holds both
    first = [(DARK, [(jitter(FACES["b"], i % 3), 0.9 - 0.001 * i)]) for i in range(4)]
    ids, frames = world.clip(first + shot(BRIGHT, 4, first="b"))
    det = detector(cuda, world)
    track = FaceTrack("left", 4, 0, 0.25)
    for run in (lambda **kw: run_face_detect(det, frames, None, track, nosmooth=True, **kw),
                lambda **kw: run_detect_many(det, {"k": frames}, None, track, T=0, **kw)["k"]):
        on, off = run(), run(scene=None)
        assert all(box[2] >= 30 for box in off)                                      # x1 of face b: followed through the cut
        assert all(box[2] >= 30 for box in on[:4]) and all(box[2] < 25 for box in on[4:])      # seeded again, on the left face
        shots = model_shots(frames)
        assert shots == [(0, 4), (4, 8)] and on == sc.finish_shots(world.rects(ids, shots, track), shots, H, W, PADS, 0, None)


def test_a_faceless_frame_in_the_second_shot_is_still_the_clips_error(cuda):
    world = World()
    ids, frames = world.clip(shot(DARK, 5) + shot(BRIGHT, 5, gaps=(2,)))
    det = detector(cuda, world)
    assert run_face_detect(det, frames, None, None) == sc.NO_FACE
    assert run_detect_many(det, {"k": frames, "ok": frames[:5]}, None, None) == {
        "k": sc.NO_FACE, "ok": sc.finish_shots(world.rects(ids[:5], [(0, 5)], None), [(0, 5)], H, W, PADS, 5, None)}


@pytest.mark.parametrize("mode,T", [("strict", 5), ("strict", 3), ("hold+track", 5), ("track", 0)])
def test_a_large_clip_and_a_host_clip_give_the_packed_result_through_the_per_clip_path(cuda, monkeypatch, mode, T):
    hold, track = mode_args(mode)
    gaps = (1,) if hold is not None else ()
    world = World()
    wide = shot(DARK, 3) + [(DARK, [(WIDE, 0.95), (jitter(FACES["b"], 1), 0.7)])] + shot(BRIGHT, 4, gaps=gaps, first="b")
    spec = {"small": shot(DARK, 3) + shot(BRIGHT, 3, first="b"), "large": shot(DARK, 5, gaps=gaps) + shot(BRIGHT, 6) + shot(DARK, 2),
            "wide": wide, "tail": shot(BRIGHT, 2) + shot(DARK, 4, first="b")}
    clips = {key: world.clip(s) for key, s in spec.items()}
    det = detector(cuda, world)
    frames = {key: f for key, (_, f) in clips.items()}
    want = {}
    for key, (ids, f) in clips.items():
        shots = model_shots(f)
        want[key] = sc.finish_shots(world.rects(ids, shots, track), shots, H, W, PADS, T, hold)
    assert len(model_shots(frames["large"])) == 3 and world.candidates(clips["wide"][0][3], 4)[1] == tc.HOST
    calls = spy_kernels(monkeypatch)
    packed = run_detect_many(det, {k: frames[k] for k in ("small", "large", "tail")}, hold, track, T=T)
    assert calls.count("w2l_frame_hist_rows") == 1                                   # one group
    del calls[:]
    got = run_detect_many(det, frames, hold, track, T=T, max_group_bytes=8 * H * W * 3)      # "large" (13 frames) goes alone
    assert got == want and all(got[k] == packed[k] for k in packed)
    assert calls.count("w2l_frame_hist_rows") > 3                                    # groups, and batch by batch in the clips alone


def test_a_group_of_three_clips_with_0_1_and_3_cuts(cuda, monkeypatch):
    world = World()
    spec = {"none": shot(DARK, 6), "one": shot(BRIGHT, 3) + shot(DARK, 4, gaps=(1,), first="b"),
            "three": shot(DARK, 2) + shot(BRIGHT, 5, first="b") + shot(DARK, 1) + shot(BRIGHT, 3)}
    clips = {key: world.clip(s) for key, s in spec.items()}
    det = detector(cuda, world)
    frames = {key: f for key, (_, f) in clips.items()}
    assert [len(model_shots(frames[k])) - 1 for k in spec] == [0, 1, 3]
    calls = spy_kernels(monkeypatch)
    from wav2lip_amd.face_detection import many
    seen = []
    orig = many._finish_segments
    monkeypatch.setattr(many, "_finish_segments", lambda n_seg, *a: (seen.append(n_seg), orig(n_seg, *a))[1])
    got = run_detect_many(det, frames, None, None)
    assert calls.count("w2l_face_boxes_segments") == 1 and seen == [7]               # one finish launch over the 1 + 2 + 4 shots
    assert calls.count("w2l_frame_hist_rows") == calls.count("w2l_scene_cuts") == 1 and calls.count("w2l_s3fd_first_rect") == 6
    want = {}
    for key, (ids, f) in clips.items():
        shots = model_shots(f)
        want[key] = sc.finish_shots(world.rects(ids, shots, None), shots, H, W, PADS, 5, None)
    assert got == want and got["one"] == sc.NO_FACE and isinstance(got["none"], list) and isinstance(got["three"], list)
    # the same group under a hold: the faceless frame is a gap of its own shot, every clip has boxes
    got = run_detect_many(det, frames, 1, None)
    for key, (ids, f) in clips.items():
        shots = model_shots(f)
        assert got[key] == sc.finish_shots(world.rects(ids, shots, None), shots, H, W, PADS, 5, 1), key
    assert got["one"][4] is not None and got["one"][3] is not None
