"""Scene-cut detection on the host: the product's statements of the rule (face_detection/scene.py) against the model
written from the rule (tests/_scene_cases.py), the consequences the documents promise on prescribed rects, the parameter check
and the flag parsers at their range ends, and the two new entries of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import _scene_cases as sc
import _track_cases as tc
from conftest import ROOT

PARSER_ARGV = {
    "inference": ["--checkpoint_path", "c", "--face", "f", "--audio", "a"],
    "filelist": ["--filelist", "l", "--results_dir", "r", "--data_root", "d", "--checkpoint_path", "c"],
}
PADS = (0, 10, 0, 0)
H, W = 40, 50
DARK, BRIGHT = (10, 20, 30), (200, 210, 220)


def parsers():
    from wav2lip_amd import gen_videos_from_filelist, inference
    return {"inference": inference.build_cli_parser(), "filelist": gen_videos_from_filelist.build_main_parser()}


# ---------------------------------------------------------------- the host statements against the model
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (5, 7), (16, 16), (17, 23)])
def test_host_signatures_equal_the_model(shape):
    from wav2lip_amd.face_detection.scene import host_signatures
    rng = np.random.default_rng(5)
    frames = np.stack([sc.content(kind, *shape, rng) for kind in sc.CONTENTS])
    got = host_signatures(frames)
    assert got.dtype == np.uint32 and got.shape == (len(sc.CONTENTS), 96)
    assert (got.astype(np.int64) == sc.signatures(frames)).all()
    assert (got.reshape(-1, 3, 32).sum(axis=2) == shape[0] * shape[1]).all()
    assert (host_signatures(list(frames)) == got).all() and host_signatures(np.zeros((0, 4, 4, 3), np.uint8)).shape == (0, 96)
    with pytest.raises(ValueError):
        host_signatures(frames.astype(np.int32))


def test_host_cut_flags_equal_the_model_at_both_ends_of_q():
    from wav2lip_amd.face_detection.scene import host_cut_flags
    rng = np.random.default_rng(6)
    base, near = sc.sig_with_distance(16, 16, 6)
    _, far = sc.sig_with_distance(16, 16, 1530)
    _, farther = sc.sig_with_distance(16, 16, 1532)
    kinds = np.stack([base, near, far, farther])
    for q in (1, 2, 128, 255):
        for n in (0, 1, 2, 9, 70):
            sig = kinds[rng.integers(0, 4, n)].reshape(n, 96)
            cuts, dist = host_cut_flags(sig, 16, 16, q)
            want_c, want_d = sc.cut_flags(sig, 16, 16, q)
            assert cuts.tolist() == want_c.tolist() and dist.tolist() == want_d.tolist()
    # the bound itself is no cut, one count more is, at both ends of q
    for q in (1, 255):
        a, at = sc.sig_with_distance(16, 16, 6 * q)
        more = at.copy()
        more[5] += 1
        assert host_cut_flags(np.stack([a, at]), 16, 16, q)[0].tolist() == [0, 0]
        assert host_cut_flags(np.stack([a, more]), 16, 16, q)[0].tolist() == [0, 1]
        assert host_cut_flags(np.stack([more, a]), 16, 16, q)[0].tolist() == [0, 1]      # frame 0 never, whatever it holds
    for bad in (0, 256, True, 1.0):
        with pytest.raises(ValueError):
            host_cut_flags(np.stack([a, at]), 16, 16, bad)
    with pytest.raises(ValueError):
        host_cut_flags(np.stack([a, at]), 1 << 15, 10923, 1)                             # 6 H W >= 2^31


def test_split_shots_edge_cases():
    from wav2lip_amd.face_detection.scene import split_shots
    assert split_shots(0, []) == [] == sc.shots(0, [])
    assert split_shots(1, [0]) == [(0, 1)] and split_shots(1, [1]) == [(0, 1)]           # frame 0's flag is not looked at
    assert split_shots(4, [0, 0, 0, 1]) == [(0, 3), (3, 4)]                              # a cut on the last frame
    assert split_shots(4, [1, 1, 1, 1]) == [(0, 1), (1, 2), (2, 3), (3, 4)]              # all cuts
    assert split_shots(5, [0, 0, 0, 0, 0]) == [(0, 5)]
    rng = np.random.default_rng(1)
    for n in (2, 7, 40):
        cuts = (rng.random(n) < 0.3).astype(np.int32)
        got = split_shots(n, cuts)
        assert got == sc.shots(n, cuts) and got[0][0] == 0 and got[-1][1] == n
        assert all(a < b for a, b in got) and all(x[1] == y[0] for x, y in zip(got, got[1:]))


def test_distances_are_the_normalised_d_per_frame():
    from wav2lip_amd.face_detection.scene import distances
    frames = np.stack([sc.flat_frame(H, W, DARK)] * 2 + [sc.flat_frame(H, W, BRIGHT)] * 2)
    frames[1, 0, 0] = (255, 255, 255)                                                    # one pixel moves: 6 of 6 H W
    d = distances(frames)
    assert d.dtype == np.float64 and d.tolist() == [0.0, 6 / (6 * H * W), 1.0, 0.0]
    assert distances(np.zeros((0, H, W, 3), np.uint8)).shape == (0,)


def test_the_modules_command_prints_distances_and_cut_frames_of_an_avi(tmp_path, capsys):
    from wav2lip_amd.container import write_avi
    from wav2lip_amd.face_detection import scene
    frames = np.stack([sc.flat_frame(H, W, DARK)] * 2 + [sc.flat_frame(H, W, BRIGHT)] * 3 + [sc.flat_frame(H, W, DARK)])
    path = str(tmp_path / "clip.avi")
    write_avi(path, frames, 25)
    assert scene.main([path, "--host", "--scene_cuts", "0.3"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert [line.split()[1] for line in out[:6]] == ["0.000000", "0.000000", "1.000000", "0.000000", "0.000000", "1.000000"]
    assert [line.endswith("cut") for line in out[:6]] == [False, False, True, False, False, True]
    assert out[6] == "cuts at frames: 2 5"
    assert scene.main([path, "--host"]) == 0 and "cut" not in capsys.readouterr().out


# ---------------------------------------------------------------- the parameter and the command line
def test_check_scene_at_the_ends_of_the_range():
    from wav2lip_amd.face_detection.scene import SceneCuts, check_scene, scene_kw, scene_q8
    assert check_scene(None) is None and scene_kw(None) == {}
    assert check_scene(1 / 256) == SceneCuts(1 / 256) and scene_q8(1 / 256) == 1
    top = np.nextafter(1.0, 0.0)
    assert check_scene(top) == SceneCuts(top) and scene_q8(top) == 255
    assert check_scene(SceneCuts(0.3)) == SceneCuts(0.3) and scene_q8(0.3) == 76
    assert check_scene(np.float32(0.5)) == SceneCuts(0.5) and type(check_scene(np.float32(0.5)).thresh) is float
    assert scene_kw(0.3) == {"scene_cuts": SceneCuts(0.3)}
    for bad in (np.nextafter(1 / 256, 0.0), 1.0, 0.0, -0.3, 2, float("nan"), float("inf"), "0.3", True, False, (0.3,), [0.3],
                SceneCuts("0.3"), SceneCuts(True), SceneCuts(1.0), b"x", object()):
        with pytest.raises(ValueError):
            check_scene(bad)


@pytest.mark.parametrize("name", sorted(PARSER_ARGV))
def test_the_flag_on_the_command_lines(name, capsys):
    from wav2lip_amd import inference
    from wav2lip_amd.face_detection.scene import SceneCuts
    p = parsers()[name]
    a = p.parse_args(PARSER_ARGV[name])
    assert a.scene_cuts is None and "scene_cuts" not in inference.detect_kw_from_args(a)   # a lone absent flag: no keyword
    a = p.parse_args(PARSER_ARGV[name] + ["--scene_cuts", "0.3"])
    assert inference.detect_kw_from_args(a) == {"scene_cuts": SceneCuts(0.3)}
    a = p.parse_args(PARSER_ARGV[name] + ["--scene_cuts", "0.25", "--no_face_hold", "3", "--face_track", "left"])
    kw = inference.detect_kw_from_args(a)
    assert kw["scene_cuts"] == SceneCuts(0.25) and kw["no_face_hold"] == 3 and kw["face_track"].pick == "left"
    for bad in ("1", "0", "0.003", "-0.5", "nan", "x", ""):
        with pytest.raises(SystemExit):
            p.parse_args(PARSER_ARGV[name] + ["--scene_cuts", bad])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        p.parse_args(PARSER_ARGV[name] + ["--scene_cuts"])                               # the value is required
    assert "Not the reference's output" in " ".join(p.format_help().split())


def test_the_live_path_and_the_other_commands_do_not_take_the_flag():
    from wav2lip_amd import inference, streaming
    p = streaming.build_parser()
    with pytest.raises(SystemExit):
        p.parse_args(["--checkpoint_path", "c", "--face", "f", "--audio", "a", "--scene_cuts", "0.3"])
    a = p.parse_args(["--checkpoint_path", "c", "--face", "f", "--audio", "a"])
    assert "scene_cuts" not in inference.detect_kw_from_args(a)


def test_a_wrong_value_is_refused_before_any_device_work():
    from wav2lip_amd import face_detection, inference

    class NoDevice:
        device = "cuda"

        def __getattr__(self, name):
            raise AssertionError("the detector was touched: %s" % name)

    frames = [sc.flat_frame(H, W, DARK)] * 3
    for bad in (1.0, "0.3", True, 0.0):
        with pytest.raises(ValueError, match="scene_cuts"):
            inference.face_detect(frames, detector=NoDevice(), pads=[0, 10, 0, 0], nosmooth=False, batch_size=4, scene_cuts=bad)
        with pytest.raises(ValueError, match="scene_cuts"):
            list(face_detection.detect_many(NoDevice(), [face_detection.DetectJob("k", frames)], scene_cuts=bad))

    class Ranks:
        dist, world, rank = object(), 2, 0

    with pytest.raises(ValueError, match="one GPU"):
        inference.face_detect(frames, detector=NoDevice(), pads=[0, 10, 0, 0], nosmooth=False, batch_size=4, ranks=Ranks(), scene_cuts=0.3)


# ---------------------------------------------------------------- consequences (a) to (c) on the host path, prescribed rects
def random_rects(rng, n, p_none=0.0):
    out = []
    for _ in range(n):
        x1, y1 = int(rng.integers(0, 30)), int(rng.integers(0, 20))
        out.append(None if rng.random() < p_none else (x1, y1, x1 + int(rng.integers(5, 30)), y1 + int(rng.integers(5, 30))))
    return out


def product_finish(rects, shots, T, hold):
    """the product's host finish as the front ends report it: a list of tuples / None, or the error's text"""
    from wav2lip_amd.face_detection.scene import host_boxes_shots
    try:
        boxes, valid = host_boxes_shots(rects, shots, H, W, PADS, T, hold)
    except ValueError as e:
        return str(e)
    return [tuple(int(v) for v in b) if ok else None for b, ok in zip(boxes, valid)]


def clip_shots(frames, thresh):
    """shots of host frames through the product's host statements, checked against the model's"""
    from wav2lip_amd.face_detection.scene import host_cut_flags, host_signatures, scene_q8, split_shots
    cuts, _ = host_cut_flags(host_signatures(np.stack(frames)), H, W, scene_q8(thresh))
    got = split_shots(len(frames), cuts)
    assert got == sc.shots(len(frames), sc.cut_flags(sc.signatures(frames), H, W, sc.q_of(thresh))[0])
    return got


MODES = [(None, False), (2, False), (None, True), (2, True)]      # strict, hold, track, hold + track


def mode_rects(rng, n, shots, hold, tracked, p_none):
    """prescribed rects of a clip for a mode: under a track they come from prescribed candidates through the product's host track
    per shot (checked against the model's)"""
    if not tracked:
        return random_rects(rng, n, p_none)
    from wav2lip_amd.face_detection.scene import host_track_shots
    from wav2lip_amd.face_detection.track import FaceTrack, iou_q8
    track = FaceTrack("left", 4, 0 if hold is None else 1, 0.25)     # strict: with L = 0 a frame with a candidate has a rect
    cands = [[r for r in random_rects(rng, int(rng.integers(1, 4)), p_none) if r is not None] for _ in range(n)]
    got = host_track_shots(cands, shots, track)
    frames = [(c, tc.FOUND if c else tc.NONE) for c in cands]
    assert got == sc.track_shots(frames, shots, track.pick, track.reseed, iou_q8(track.min_iou))
    return got


@pytest.mark.parametrize("hold,tracked", MODES)
def test_a_clip_without_a_cut_is_the_feature_switched_off(hold, tracked):
    from wav2lip_amd.face_detection import many
    rng = np.random.default_rng(21)
    for n in (1, 3, 9):
        frames = [sc.flat_frame(H, W, DARK) for _ in range(n)]
        frames[n // 2][:4] = BRIGHT                                                      # a change below the threshold
        shots = clip_shots(frames, 0.3)
        assert shots == [(0, n)]
        for T in (0, 5):
            rects = mode_rects(rng, n, shots, hold, tracked, 0.3 if hold is not None else 0.0)
            got = product_finish(rects, shots, T, hold)
            if hold is None:
                off = [tuple(int(v) for v in b) for b in many.host_boxes(rects, H, W, PADS, T)]
            else:
                boxes, valid = many.host_boxes_runs(rects, H, W, PADS, T, hold)
                off = [tuple(int(v) for v in b) if ok else None for b, ok in zip(boxes, valid)]
            assert got == off == sc.finish_shots(rects, shots, H, W, PADS, T, hold)


@pytest.mark.parametrize("hold,tracked", MODES)
def test_a_cut_at_every_frame_gives_the_unsmoothed_boxes(hold, tracked):
    rng = np.random.default_rng(22)
    n = 7
    frames = [sc.flat_frame(H, W, DARK if i % 2 == 0 else BRIGHT) for i in range(n)]
    shots = clip_shots(frames, 0.3)
    assert shots == [(i, i + 1) for i in range(n)]
    rects = mode_rects(rng, n, shots, hold, tracked, 0.0)
    smoothed, plain = product_finish(rects, shots, 5, hold), product_finish(rects, shots, 0, hold)
    assert smoothed == plain == sc.finish_shots(rects, shots, H, W, PADS, 0, hold)       # a one-frame shot's mean is itself
    assert plain == [(max(0, r[1] - PADS[0]), min(H, r[3] + PADS[1]), max(0, r[0] - PADS[2]), min(W, r[2] + PADS[3])) for r in rects]


@pytest.mark.parametrize("hold,tracked", MODES)
def test_two_clips_joined_at_a_cut_are_the_two_clips_detected_apart(hold, tracked):
    rng = np.random.default_rng(23)
    for na, nb in ((4, 6), (1, 3), (7, 2)):
        frames = [sc.flat_frame(H, W, DARK)] * na + [sc.flat_frame(H, W, BRIGHT)] * nb
        shots = clip_shots(frames, 0.3)
        assert shots == [(0, na), (na, na + nb)]
        p_none = 0.35 if hold is not None else 0.0
        rects = mode_rects(rng, na + nb, shots, hold, tracked, p_none)
        if hold is not None:
            rects[na] = None                                                             # the hold must not reach across the cut
            rects[na - 1] = rects[na - 1] or (3, 4, 20, 30)
        for T in (0, 5):
            joined = product_finish(rects, shots, T, hold)
            apart = product_finish(rects[:na], [(0, na)], T, hold) + product_finish(rects[na:], [(0, nb)], T, hold)
            assert joined == apart == sc.finish_shots(rects, shots, H, W, PADS, T, hold)
            if hold is not None:
                assert joined[na] is None and joined[na - 1] is not None
                assert product_finish(rects, [(0, na + nb)], T, hold)[na] is not None    # without the cut the rect is held across


def test_in_the_strict_mode_a_faceless_frame_in_any_shot_is_the_clips_error():
    from wav2lip_amd.face_detection import many
    rects = [(1, 2, 20, 30)] * 4 + [None] + [(5, 6, 25, 35)] * 2
    assert product_finish(rects, [(0, 3), (3, 7)], 5, None) == many.NO_FACE == sc.finish_shots(rects, [(0, 3), (3, 7)], H, W, PADS, 5, None)
    assert many.NO_FACE == sc.NO_FACE


def test_shot_statuses_fold_into_the_clips():
    from wav2lip_amd.face_detection.many import _fold_shot_status
    shot_status = np.array([[0, 0], [1, 2], [0, 0], [1, 0], [2, 1], [1, 1], [0, 0]], np.int32)
    folded = _fold_shot_status(shot_status, [[(0, 4)], [(0, 3), (3, 5)], [(0, 2), (2, 6), (6, 7)], [(0, 9)]])
    assert folded.tolist() == [[0, 0], [1, 2], [2, 3], [0, 0]]          # code 2 wins over code 1; the row is the clip's frame


# ---------------------------------------------------------------- structure and ABI of the two entries
def test_the_two_entries_are_declared_bound_and_exported():
    from wav2lip_amd import _lib
    text = open(os.path.join(ROOT, "include", "w2l_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+w2l_frame_hist_rows\(void\*\s*stream,\s*int B,\s*int H,\s*int W,\s*const uint64_t\*\s*frames,\s*uint32_t\*\s*sig\)", plain)
    assert re.search(r"int\s+w2l_scene_cuts\(void\*\s*stream,\s*int n_seg,\s*const w2l_box_segment\*\s*segs,\s*const uint32_t\*\s*sig,\s*int n_rows,"
                     r"\s*int q,\s*int32_t\*\s*cuts,\s*int32_t\*\s*dist,\s*int32_t\*\s*status\)", plain)
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["w2l_frame_hist_rows"] == (i, [vp, i, i, i, vp, vp])
    assert _lib.SIGNATURES["w2l_scene_cuts"] == (i, [vp, i, vp, vp, i, i, vp, vp, vp])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "w2l_frame_hist_rows") and hasattr(lib, "w2l_scene_cuts")
    assert _lib.BOX_SEGMENT.itemsize == 16                              # the cut kernel reads the finish's table
    assert "scene.hip" in open(os.path.join(ROOT, "wav2lip_amd", "csrc", "Makefile")).read()


def test_host_refusals_need_no_device():
    """the argument checks come before any launch: a NULL pointer is refused with the library loaded on a machine without a GPU"""
    from wav2lip_amd import _lib
    lib = _lib.load()
    assert lib.w2l_frame_hist_rows(None, 1, 4, 4, None, None) != 0 and b"frame_hist_rows" in lib.w2l_last_error()
    assert lib.w2l_scene_cuts(None, 1, None, None, 0, 1, None, None, None) != 0 and b"scene_cuts" in lib.w2l_last_error()
