"""Tracked face selection on the host: the product's statement of the rule (face_detection/track.py: host_top_rects,
host_track) against the model written from the rule (tests/_track_cases.py), the consequences the documents promise, the
parameter checks and flag parsers at their range ends, and the new struct and entries of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import _track_cases as tc
from conftest import ROOT

PARSER_ARGV = {
    "inference": ["--checkpoint_path", "c", "--face", "f", "--audio", "a"],
    "streaming": ["--checkpoint_path", "c", "--face", "f", "--audio", "a"],
    "filelist": ["--filelist", "l", "--results_dir", "r", "--data_root", "d", "--checkpoint_path", "c"],
}


def parsers():
    from wav2lip_amd import gen_videos_from_filelist, inference, streaming
    return {"inference": inference.build_cli_parser(), "streaming": streaming.build_parser(),
            "filelist": gen_videos_from_filelist.build_main_parser()}


def random_table(rng, P, n_keep, frac_pass=0.5):
    xy = rng.normal(60, 50, (P, 2))
    wh = rng.uniform(0, 80, (P, 2))
    sc = np.where(rng.random(P) < frac_pass, rng.uniform(0.5, 1.0, P), rng.uniform(0.0, 0.5, P))
    sc[rng.integers(0, P)] = 0.5                                    # exactly one half does not pass
    table = np.concatenate([xy, xy + wh, sc[:, None]], axis=1).astype(np.float32)
    keep = np.zeros(P, np.int32)
    keep[:n_keep] = rng.permutation(P)[:n_keep]
    return table, keep


# ---------------------------------------------------------------- the product's host statement against the model
@pytest.mark.parametrize("scale", [None, (np.float32(1.5), np.float32(4.0 / 3.0))])
def test_host_top_rects_equals_the_model_on_random_tables(scale):
    from wav2lip_amd.face_detection.track import host_top_rects
    rng = np.random.default_rng(11)
    seen_counts = set()
    for case in range(200):
        P = int(rng.integers(1, 60))
        n = int(rng.integers(0, P + 1))
        K = int(rng.integers(1, 17))
        table, keep = random_table(rng, P, n, frac_pass=rng.choice([0.0, 0.2, 0.9]))
        want, flag = tc.model_top_rects(table, keep, n, K, *(scale or (1.0, 1.0)))
        got = host_top_rects(table, keep, n, K, scale)
        assert flag != tc.HOST and got == want, case
        assert all(type(v) is int for r in got for v in r) and len(got) <= K
        seen_counts.add(min(len(got), 3) if len(got) < K else "K")
    assert seen_counts >= {0, 1, 3, "K"}


def test_host_top_rects_where_the_device_would_flag_the_frame():
    """int() decides on the host: NaN and inf raise, a coordinate above 32767 converts (no limit there), a keep entry outside the
    table is an IndexError up to the K-th passing row and not looked at after it"""
    from wav2lip_amd.face_detection.track import host_top_rects
    rows = np.array([[1, 2, 3, 4, 0.9], [5, 6, 40000.5, 8, 0.8], [9, 9, 9, 9, 0.7]], np.float32)
    keep = np.arange(3, dtype=np.int32)
    assert host_top_rects(rows, keep, 3, 8) == [(1, 2, 3, 4), (5, 6, 40000, 8), (9, 9, 9, 9)]
    assert tc.model_top_rects(rows, keep, 3, 8)[1] == tc.HOST and tc.model_top_rects(rows, keep, 3, 1) == ([(1, 2, 3, 4)], tc.FOUND)
    for bad, err in ((np.nan, ValueError), (np.inf, OverflowError)):
        rows[1, 2] = bad
        with pytest.raises(err):
            host_top_rects(rows, keep, 3, 8)
        assert host_top_rects(rows, keep, 3, 1) == [(1, 2, 3, 4)]          # not looked at
    rows[1, 2] = -np.inf
    assert host_top_rects(rows, keep, 3, 2)[1] == (5, 6, 0, 8)
    keep = np.array([0, 7, 2], np.int32)
    with pytest.raises(IndexError):
        host_top_rects(rows, keep, 3, 2)
    assert host_top_rects(rows, keep, 3, 1) == [(1, 2, 3, 4)]
    assert tc.model_top_rects(rows, keep, 3, 2)[1] == tc.HOST and tc.model_top_rects(rows, keep, 3, 1)[1] == tc.FOUND


def as_words(state):
    (x1, y1, x2, y2), has, missed = state
    return (x1, y1, x2, y2, has, missed, 0, 0)


@pytest.mark.parametrize("pick", tc.PICKS)
def test_host_track_equals_the_model_on_random_clips(pick):
    from wav2lip_amd.face_detection.track import FaceTrack, host_track, iou_q8
    rng = np.random.default_rng(tc.PICKS.index(pick))
    happened = set()
    for case in range(300):
        K, L = int(rng.integers(1, 17)), int(rng.choice([0, 0, 1, 3]))
        min_iou = float(rng.choice([1 / 256, 0.1, 0.25, 0.5, 1.0]))
        frames = tc.random_clip(rng, int(rng.integers(1, 41)), K)
        rects, flags, words, events = tc.model_track(frames, pick, L, iou_q8(min_iou))
        got, state = host_track([c for c, _ in frames], FaceTrack(pick, K, L, min_iou))
        assert got == [tuple(r) if f == tc.FOUND else None for r, f in zip(rects.tolist(), flags)], case
        assert as_words(state) == words, case
        happened |= set().union(*events)
    assert happened >= {"continue", "iou_tie", "miss", "lost", "reseed", "seed", "none"}
    assert pick == "score" or "seed_tie" in happened


def test_the_quantised_threshold():
    from wav2lip_amd.face_detection.track import FaceTrack, check_track, iou_q8
    assert [iou_q8(f) for f in (1 / 256, 0.25, 0.2539, 0.5, 0.999, 1.0)] == [1, 64, 64, 128, 255, 256]
    assert iou_q8(check_track("score").min_iou) == 64 and FaceTrack("left") == ("left", 8, 0, 0.25)


# ---------------------------------------------------------------- the consequences the documents state
def test_with_no_reseed_tolerance_a_frame_that_has_a_candidate_is_never_lost():
    from wav2lip_amd.face_detection.track import FaceTrack, host_track
    rng = np.random.default_rng(5)
    lost_with_tolerance = 0
    for case in range(200):
        frames = [c for c, _ in tc.random_clip(rng, 30, 4)]
        pick = tc.PICKS[case % 4]
        got, _ = host_track(frames, FaceTrack(pick, 4, 0, 0.25))
        assert [r is None for r in got] == [len(c) == 0 for c in frames], case
        got, _ = host_track(frames, FaceTrack(pick, 4, 2, 0.25))
        lost_with_tolerance += sum(r is None and len(c) > 0 for r, c in zip(got, frames))
    assert lost_with_tolerance > 0                           # the statement is about L = 0, and says something


def test_one_candidate_per_frame_or_k_of_one_gives_the_untracked_rects():
    from wav2lip_amd.face_detection.track import FaceTrack, host_track
    rng = np.random.default_rng(6)
    differs = 0
    for case in range(100):
        frames = [c for c, _ in tc.random_clip(rng, 25, 5)]
        untracked = [c[0] if c else None for c in frames]
        assert host_track([c[:1] for c in frames], FaceTrack("score", 5, 0, 0.25))[0] == untracked
        for pick in tc.PICKS:                               # with one candidate every pick seeds the same
            assert host_track([c[:1] for c in frames], FaceTrack(pick, 1, 0, float(rng.choice([0.01, 0.25, 1.0]))))[0] == untracked
        differs += host_track(frames, FaceTrack("score", 5, 0, 0.25))[0] != untracked
    assert differs > 50                                      # and with several candidates the track does choose otherwise


def test_the_track_over_any_cut_with_carried_state_equals_one_go():
    from wav2lip_amd.face_detection.track import FaceTrack, host_track
    rng = np.random.default_rng(7)
    for case in range(60):
        n = 12 if case < 20 else 200
        track = FaceTrack(tc.PICKS[case % 4], 6, int(rng.choice([0, 1, 3])), 0.25)
        frames = [c for c, _ in tc.random_clip(rng, n, 6)]
        whole, end = host_track(frames, track)
        cuts = ([[k] for k in range(0, n + 1)] if case < 20 else
                [sorted(rng.integers(0, n + 1, int(rng.integers(1, 9))).tolist()) for _ in range(4)])
        for cut in cuts:
            got, state = [], None
            for a, b in zip([0] + cut, cut + [n]):
                part, state = host_track(frames[a:b], track, state)
                got += part
            assert got == whole and state == end, (case, cut)


# ---------------------------------------------------------------- parameters and flags
def test_check_track_at_and_beyond_every_range_end():
    from wav2lip_amd.face_detection.track import FaceTrack, check_track, track_kw
    assert check_track(None) is None and track_kw(None) == {}
    assert check_track("right") == FaceTrack("right", 8, 0, 0.25) == track_kw("right")["face_track"]
    for ok in (FaceTrack("score", 1, 0, 1 / 256), FaceTrack("largest", 16, 250, 1.0), ("left", np.int32(3), np.int64(4), np.float32(0.5))):
        t = check_track(ok)
        assert t == tuple(ok) and type(t.cands) is int and type(t.reseed) is int and type(t.min_iou) is float
    for bad in ("best", "", 3, ("score", 0), ("score", 17), ("score", 8, -1), ("score", 8, 251), ("score", 8, 0, 0.0),
                ("score", 8, 0, 1 / 257), ("score", 8, 0, 1.0001), ("score", 8, 0, float("nan")), ("score", 8.0), ("score", True),
                ("score", 8, 0, "0.5"), ("score", 8, 0, 0.5, 1), ()):
        with pytest.raises(ValueError, match="face_track"):
            check_track(bad)


def test_a_bad_track_is_a_value_error_before_any_device_work():
    from wav2lip_amd import inference, streaming
    from wav2lip_amd.face_detection import many

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("the detector was used")

    frame = np.zeros((8, 8, 3), np.uint8)
    for bad in ("best", ("score", 17), ("left", 8, 251)):
        with pytest.raises(ValueError, match="face_track"):
            inference.face_detect([frame], detector=Untouched(), pads=[0, 0, 0, 0], nosmooth=True, batch_size=1, face_track=bad)
        with pytest.raises(ValueError, match="face_track"):
            next(many.detect_many(Untouched(), [many.DetectJob(0, [frame])], face_track=bad))
        with pytest.raises(ValueError, match="face_track"):
            streaming.LipsyncStreams(None, face_track=bad)


def test_the_flags_are_absent_by_default_on_the_three_commands_and_end_where_the_ranges_end(capsys):
    from wav2lip_amd import gen_videos_from_filelist, inference
    from wav2lip_amd.face_detection.track import FaceTrack, track_from_args
    for name, p in parsers().items():
        argv = PARSER_ARGV[name]
        a = p.parse_args(argv)
        assert (a.face_track, a.face_track_reseed, a.face_track_iou, a.face_track_cands) == (None,) * 4 and track_from_args(a) is None
        for pick in tc.PICKS:
            assert track_from_args(p.parse_args(argv + ["--face_track", pick])) == FaceTrack(pick, 8, 0, 0.25)
        full = ["--face_track", "largest", "--face_track_reseed", "250", "--face_track_iou", "1.0", "--face_track_cands", "16"]
        assert track_from_args(p.parse_args(argv + full)) == FaceTrack("largest", 16, 250, 1.0)
        low = ["--face_track", "left", "--face_track_reseed", "0", "--face_track_iou", "0.00390625", "--face_track_cands", "1"]
        assert track_from_args(p.parse_args(argv + low)) == FaceTrack("left", 1, 0, 1 / 256)
        for flag, values in (("--face_track", ("best", "0")), ("--face_track_reseed", ("-1", "251", "x", "1.5")),
                             ("--face_track_iou", ("0", "0.0039", "1.01", "nan", "x")), ("--face_track_cands", ("0", "17", "x", "2.5"))):
            for bad in values:
                with pytest.raises(SystemExit):
                    p.parse_args(argv + ["--face_track", "score"] * (flag != "--face_track") + [flag, bad])
        for lone in (["--face_track_reseed", "3"], ["--face_track_iou", "0.5"], ["--face_track_cands", "2"]):
            with pytest.raises(ValueError, match="needs --face_track"):
                track_from_args(p.parse_args(argv + lone))
        extra = ["--precision", "bf16", "--face_det_scale", "2", "--blend_feather", "4", "--no_face_hold", "3", "--face_track", "right",
                 "--face_track_reseed", "3"]                          # independent of the other additions; L = G is the natural pairing
        a = p.parse_args(argv + extra + (["--packed_face_det"] if name == "filelist" else []))
        assert (track_from_args(a), a.no_face_hold, a.face_det_scale) == (FaceTrack("right", 8, 3, 0.25), 3, 2)
    capsys.readouterr()
    # the reference's surfaces stay the reference's, and the commands that do not take the flags do not
    assert not hasattr(inference.build_parser().parse_args(PARSER_ARGV["inference"]), "face_track")
    assert not hasattr(gen_videos_from_filelist.cli_parser.parse_args(PARSER_ARGV["filelist"]), "face_track")
    assert inference.args.face_track is None and track_from_args(object()) is None
    assert inference._track_kw(None) == {} and inference._track_kw("left") == {"face_track": FaceTrack("left")}


def test_a_sharded_inference_run_refuses_the_flag_up_front(monkeypatch, tmp_path):
    from wav2lip_amd import inference, sharding
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sharding, "init_from_env", lambda *a, **k: pytest.fail("the process group was initialised"))
    monkeypatch.setattr(inference, "args", inference.args)        # main() replaces the module-level args
    with pytest.raises(ValueError, match="--face_track runs on one GPU"):
        inference.main(["--checkpoint_path", "c", "--face", str(tmp_path / "f.avi"), "--audio", "a.wav", "--face_track", "score"])

    class Ranks:
        dist, world, rank = object(), 2, 0

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("the detector was used")

    with pytest.raises(ValueError, match="face_track runs on one GPU"):
        inference.face_detect([np.zeros((8, 8, 3), np.uint8)], detector=Untouched(), pads=[0, 0, 0, 0], nosmooth=True, batch_size=1,
                              ranks=Ranks(), face_track="score")


def test_a_lone_companion_flag_is_refused_by_the_commands_before_any_device_work(monkeypatch, tmp_path):
    from wav2lip_amd import gen_videos_from_filelist, inference, sharding, streaming
    monkeypatch.setattr(sharding, "init_from_env", lambda *a, **k: pytest.fail("the process group was initialised"))
    monkeypatch.setattr(inference, "args", inference.args)
    with pytest.raises(ValueError, match="needs --face_track"):
        inference.main(PARSER_ARGV["inference"] + ["--face_track_cands", "2"])
    with pytest.raises(ValueError, match="needs --face_track"):
        gen_videos_from_filelist.main(PARSER_ARGV["filelist"] + ["--face_track_reseed", "2"])
    with pytest.raises(ValueError, match="needs --face_track"):
        streaming.main(PARSER_ARGV["streaming"] + ["--face_track_iou", "0.5"])


def test_lipsync_streams_hands_the_track_to_its_device_boxes(monkeypatch):
    from wav2lip_amd import streaming
    from wav2lip_amd.face_detection.track import FaceTrack
    made = []

    class Runner:
        device = "cpu"

        def __init__(self, *a, **k):
            pass

    class Boxes:
        def __init__(self, *a, **k):
            made.append(k)

    monkeypatch.setattr(streaming, "BatchRunner", Runner)
    monkeypatch.setattr(streaming, "DeviceMel", lambda dev: None)
    monkeypatch.setattr(streaming, "DeviceBoxes", Boxes)
    streaming.LipsyncStreams(None, detector=object(), face_track="right")._backend()
    streaming.LipsyncStreams(None, detector=object(), face_track=FaceTrack("left", 2, 5, 0.5), no_face_hold=5)._backend()
    streaming.LipsyncStreams(None, detector=object())._backend()
    assert made == [{"track": FaceTrack("right")}, {"hold": 5, "track": FaceTrack("left", 2, 5, 0.5)}, {}]


# ---------------------------------------------------------------- the C ABI: the new struct and the two entries
def test_the_track_segment_struct_is_mirrored_once_and_asserted_in_the_kernel_file():
    from test_struct_mirrors_cpu import HEADER, stated_table, typedef_layout
    from wav2lip_amd import _lib, streaming
    from wav2lip_amd.face_detection import many, track
    fields, size = typedef_layout("w2l_track_segment")
    assert size == 16 == ctypes.sizeof(_lib.TrackSegment) == _lib.TRACK_SEGMENT.itemsize
    names = [f for f, _, _, _ in fields]
    assert names == ["row0", "n", "slot", "seen"] == [f for f, _ in _lib.TrackSegment._fields_] == list(_lib.TRACK_SEGMENT.names)
    for field, ctype, length, off in fields:
        assert (ctype, length) == ("int32_t", 0) and getattr(_lib.TrackSegment, field).offset == _lib.TRACK_SEGMENT.fields[field][1] == off
    assert "w2l_track_segment, 16 bytes, the table 16-byte aligned" in HEADER and stated_table("w2l_track_segment", 16) == []
    assert np.dtype(_lib.TrackSegment) == _lib.TRACK_SEGMENT
    for module in (many, track, streaming):                          # the modules import the name instead of spelling it
        assert module.TRACK_SEGMENT is _lib.TRACK_SEGMENT
    kernel_file = open(os.path.join(ROOT, "wav2lip_amd", "csrc", "detect.hip")).read()
    assert "static_assert(sizeof(TrackSeg) == 16 && sizeof(w2l_track_segment) == 16" in kernel_file
    for sym in ("w2l_s3fd_top_rects", "w2l_face_track_segments"):
        assert re.search(r"^//   %s " % sym, kernel_file, flags=re.M), sym      # the file's header list names it


def test_the_two_entries_are_bound_with_the_arguments_the_header_declares():
    from wav2lip_amd import _lib
    from wav2lip_amd.face_detection import track
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "w2l_hip.h")).read(), flags=re.S)
    kinds = {"void*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float}
    for sym in ("w2l_s3fd_top_rects", "w2l_face_track_segments"):
        args = re.search(r"int %s\(([^)]*)\);" % sym, header).group(1).split(",")
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in args]
        assert _lib.SIGNATURES[sym] == (ctypes.c_int, want), sym
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "w2l_s3fd_top_rects") and hasattr(lib, "w2l_face_track_segments")
    assert track.PICKS == tc.PICKS == ("score", "largest", "left", "right")
    assert (track.MAX_CANDS, track.MAX_RESEED, track.STATE_INTS) == (16, 250, 8)
    assert track.FRESH == ((0, 0, 0, 0), 0, 0) and as_words(track.FRESH) == tc.FRESH


def test_the_launchers_refuse_what_is_out_of_range_without_a_device():
    """W2L_REQUIRE runs before anything is launched: K, pick, L and q beyond their ends, a NULL pointer, a misaligned table"""
    from wav2lip_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int32 * 256)()
    p = ctypes.addressof(buf)
    base = p + (-p % 16)

    def top(K=8, sx=1.0, sy=1.0, B=1, P=4, table=base):
        return lib.w2l_s3fd_top_rects(None, B, P, table, base, base, 0.5, sx, sy, K, base, base, base)

    for kw in (dict(K=0), dict(K=17), dict(sx=0.0), dict(sy=float("inf")), dict(sx=float("nan")), dict(B=0), dict(P=0), dict(table=None),
               dict(B=1 << 15, P=1 << 15)):
        assert top(**kw) != 0 and lib.w2l_last_error(), kw

    def trk(n_seg=1, segs=base, K=8, pick=0, L=0, q=64, state=None, n_slots=0, n_rows=4, rects=base, cands=base):
        return lib.w2l_face_track_segments(None, n_seg, segs, cands, base, base, n_rows, K, pick, L, q, state, n_slots, rects, base, base)

    for kw in (dict(K=0), dict(K=17), dict(pick=-1), dict(pick=4), dict(L=-1), dict(L=251), dict(q=0), dict(q=257), dict(n_seg=0),
               dict(n_rows=-1), dict(n_slots=1), dict(n_slots=-1), dict(segs=None), dict(segs=base + 4), dict(rects=base + 8),
               dict(cands=base + 4)):
        assert trk(**kw) != 0 and lib.w2l_last_error(), kw
    assert b"face_track_segments" in lib.w2l_last_error()
