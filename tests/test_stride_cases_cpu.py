"""The key-frame rule on the host (wav2lip_amd/face_detection/stride.py) against hand-written values, the numpy
model of tests/_stride_cases.py and the span rule it borrows its formula from; the argument checks; the flag on the five commands."""
import numpy as np
import pytest

import _stride_cases as cases

GROUPS = cases.groups()


def test_hand_written_cases():
    from wav2lip_amd.face_detection.stride import host_stride_fill, key_frames
    assert key_frames(1, 4) == [0] and key_frames(2, 4) == [0, 1] and key_frames(5, 4) == [0, 4] and key_frames(6, 4) == [0, 4, 5]
    assert key_frames(9, 4) == [0, 4, 8] and key_frames(10, 4) == [0, 4, 8, 9] and key_frames(0, 4) == [] and key_frames(3, 1) == [0, 1, 2]
    a, b = (0, 10, 40, 50), (8, 2, 44, 57)
    # the interval of 4 divides x1 and x2; y1 falls (10 -> 2: 8, 6, 4) and y2 rises by 7 / 4 (floor: 51, 53, 55)
    assert host_stride_fill([a, b], 5, 4) == [a, (2, 8, 41, 51), (4, 6, 42, 53), (6, 4, 43, 55), b]
    # differences the interval does not divide, rising and falling: 1 -> 0 and 3 -> 0 over 2 frames are floor(1 / 2), floor(3 / 2)
    assert host_stride_fill([(1, 3, 0, 0), (0, 0, 1, 3)], 3, 2) == [(1, 3, 0, 0), (0, 1, 0, 1), (0, 0, 1, 3)]
    # floor, not truncation: a rect that begins left of the frame has a negative numerator, -3 / 2 -> -2 and -1 / 2 -> -1
    assert host_stride_fill([(-3, -1, 5, 5), (0, 0, 5, 6)], 3, 2) == [(-3, -1, 5, 5), (-2, -1, 5, 5), (0, 0, 5, 6)]
    # the last interval is shorter: 7 frames at stride 4 have the keys 0, 4, 6
    c = (16, 0, 50, 63)
    assert host_stride_fill([a, b, c], 7, 4) == [a, (2, 8, 41, 51), (4, 6, 42, 53), (6, 4, 43, 55), b, (12, 1, 47, 60), c]
    # a missed key leaves the frames on both sides of it without a rect: 2N - 1 = 7 frames
    assert host_stride_fill([a, None, c, c], 10, 4) == [a] + [None] * 7 + [c, c]
    assert host_stride_fill([None, b, c], 7, 4) == [None] * 4 + [b, (12, 1, 47, 60), c]
    assert host_stride_fill([a, b, None], 7, 4)[4:] == [b, None, None]
    assert host_stride_fill([None], 1, 4) == [None] and host_stride_fill([a], 1, 4) == [a] and host_stride_fill([], 0, 4) == []
    with pytest.raises(ValueError, match="key rects"):
        host_stride_fill([a, b], 7, 4)


def test_key_frames_against_the_closed_form():
    from wav2lip_amd.face_detection.stride import key_frames
    for N in range(1, 33):
        for n in list(range(1, 4 * N + 3)) + [1100]:
            keys = key_frames(n, N)
            assert keys == cases.key_positions(n, N).tolist() and len(keys) == (n - 1 + N - 1) // N + 1
            assert keys == sorted(set(list(range(0, n, N)) + [n - 1]))


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=["N%d" % N for N, _ in GROUPS])
def test_host_stride_fill_is_the_model_and_the_span_rule_with_a_bridge_of_n_minus_1(g):
    from wav2lip_amd.face_detection.spans import host_spans
    from wav2lip_amd.face_detection.stride import host_stride_fill, key_frames
    N, group = GROUPS[g]
    checked = 0
    for name, n, key_rects, key_flags in group:
        if (key_flags == 2).any():
            continue
        keys = cases.key_list(key_rects, key_flags)
        got = host_stride_fill(keys, n, N)
        assert got == cases.filled_rects(*cases.model(key_rects, key_flags, n, N)), name
        # the frames between the keys as misses: the span rule with bridge N - 1 joins exactly neighbouring keys that were both found
        expanded = [None] * n
        for pos, r in zip(key_frames(n, N), keys):
            expanded[pos] = r
        assert got == host_spans(expanded, bridge=N - 1, min_len=1, min_size=0)[0], name
        checked += 1
    assert checked > 30


def test_stride_1_is_the_identity():
    from wav2lip_amd.face_detection.stride import host_stride_fill, key_frames, stride_kw
    rects = [(1, 2, 3, 4), None, (5, 6, 7, 8), None, None, (9, 9, 9, 9)]
    assert key_frames(6, 1) == list(range(6)) and host_stride_fill(rects, 6, 1) == rects
    assert stride_kw(1) == {} and stride_kw(None) == {} and stride_kw(2) == {"det_stride": 2}


def test_the_argument_checks():
    import argparse
    from wav2lip_amd.face_detection.stride import MAX_STRIDE, check_stride, stride_arg
    assert MAX_STRIDE == 32 and check_stride(None) == 1 and check_stride(1) == 1 and check_stride(32) == 32
    assert check_stride(np.int64(5)) == 5 and type(check_stride(np.int64(5))) is int
    for bad in (0, -1, 33, True, 2.0, "2", (2,)):
        with pytest.raises(ValueError, match="det_stride"):
            check_stride(bad)
    assert stride_arg("1") == 1 and stride_arg("32") == 32
    for bad in ("0", "33", "-2", "x", "2.5", ""):
        with pytest.raises(argparse.ArgumentTypeError):
            stride_arg(bad)


def test_a_bad_stride_is_a_value_error_before_any_device_work():
    from wav2lip_amd import inference
    from wav2lip_amd.face_detection import many

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("the detector was used")

    frame = np.zeros((8, 8, 3), np.uint8)
    for bad in (0, 33, True, "2"):
        with pytest.raises(ValueError, match="det_stride"):
            inference.face_detect([frame], detector=Untouched(), pads=[0, 0, 0, 0], nosmooth=True, batch_size=1, det_stride=bad)
        with pytest.raises(ValueError, match="det_stride"):
            next(many.detect_many(Untouched(), [many.DetectJob(0, [frame])], det_stride=bad))


def test_a_sharded_run_refuses_the_option_up_front(monkeypatch, tmp_path):
    from wav2lip_amd import inference, sharding
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sharding, "init_from_env", lambda *a, **k: pytest.fail("the process group was initialised"))
    monkeypatch.setattr(inference, "args", inference.args)        # main() replaces the module-level args
    with pytest.raises(ValueError, match="--face_det_stride runs on one GPU"):
        inference.main(["--checkpoint_path", "c", "--face", str(tmp_path / "f.avi"), "--audio", "a.wav", "--face_det_stride", "2"])

    class Ranks:
        dist, world, rank = object(), 2, 0

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError("the detector was used")

    with pytest.raises(ValueError, match="runs on one GPU: a frame is interpolated from key frames of other shards"):
        inference.face_detect([np.zeros((8, 8, 3), np.uint8)], detector=Untouched(), pads=[0, 0, 0, 0], nosmooth=True, batch_size=1,
                              ranks=Ranks(), det_stride=2)


def _parsers():
    from wav2lip_amd import calculate_scores, calculate_scores_real_videos, gen_videos_from_filelist, inference, real_videos_inference
    return {"inference": (inference.cli_parser, ["--checkpoint_path", "c", "--face", "f", "--audio", "a"]),
            "filelist": (gen_videos_from_filelist.build_main_parser(),
                         ["--filelist", "l", "--results_dir", "r", "--data_root", "d", "--checkpoint_path", "c"]),
            "real_videos": (real_videos_inference.main_parser, ["--mode", "dubbed", "--results_dir", "r", "--data_root", "d",
                                                                "--checkpoint_path", "c"]),
            "scores": (calculate_scores.cli_parser, ["--data_root", "d", "--checkpoint_path", "c"]),
            "scores_real_videos": (calculate_scores_real_videos.cli_parser, ["--data_root", "d", "--checkpoint_path", "c"])}


def test_the_flag_is_on_the_five_commands_with_default_1(capsys):
    from wav2lip_amd import gen_videos_from_filelist, inference, preprocess, streaming
    from wav2lip_amd.face_detection.stride import stride_from_args
    parsers = _parsers()
    assert len(parsers) == 5
    for name, (p, argv) in parsers.items():
        a = p.parse_args(argv)
        assert a.face_det_stride == 1 and stride_from_args(a) == {}, name
        for N in (1, 2, 32):
            a = p.parse_args(argv + ["--face_det_stride", str(N)])
            assert a.face_det_stride == N and stride_from_args(a) == ({} if N == 1 else {"det_stride": N}), name
        for bad in ("0", "33", "x", "1.5"):
            with pytest.raises(SystemExit):
                p.parse_args(argv + ["--face_det_stride", bad])
        a = p.parse_args(argv + ["--face_det_stride", "3", "--face_det_scale", "2", "--face_det_precision", "bf16"])     # independent
        assert (a.face_det_stride, a.face_det_scale, a.face_det_precision) == (3, 2, "bf16"), name
    capsys.readouterr()
    a = parsers["filelist"][0].parse_args(parsers["filelist"][1] + ["--face_det_stride", "4", "--packed_face_det", "--scene_cuts", "0.4"])
    assert inference.detect_kw_from_args(a)["det_stride"] == 4
    assert "det_stride" not in inference.detect_kw_from_args(parsers["inference"][0].parse_args(parsers["inference"][1]))
    # the reference's surfaces stay the reference's; the live path and preprocess have no such option
    assert not hasattr(inference.build_parser().parse_args(parsers["inference"][1]), "face_det_stride")
    assert not hasattr(gen_videos_from_filelist.cli_parser.parse_args(parsers["filelist"][1]), "face_det_stride")
    for p in (streaming.build_parser(), preprocess.build_main_parser()):
        assert "--face_det_stride" not in p.format_help()
    assert stride_from_args(object()) == {} and inference.args.face_det_stride == 1
