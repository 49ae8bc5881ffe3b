"""The numpy model of the feathered, mouth-region paste (tests/_blend_cases.py) on its own, the division the kernels use, and
the host side of the option: `inference.check_blend`, `_blend_kw`, the four command lines and `lipsync`'s host-paste case.

The float64 bound.  BLEND_BOUND = 1.5 grey levels, strict, between the model and alpha*bilinear_f64 + (1-alpha)*o with
alpha = a/D.  The model is x = alpha*p + (1-alpha)*o rounded once, half up: at most 0.5 from x.  x differs from the float64
blend by alpha*(p - bilinear_f64), and |p - bilinear_f64| < BOUND = 1.0 (tests/_frame_cases.py, held by
tests/test_frame_cases_cpu.py), alpha <= 1: below 1.0.  Together below 1.5."""
import functools

import numpy as np
import pytest

import _blend_cases as BC
import _frame_cases as FC

FRAMES = (FC.FRAME_ODD, FC.FRAME_EVEN)


@functools.lru_cache(maxsize=None)
def _frame_inputs(frame):
    """(source frame, [(id, box, prediction)]) of one frame shape, read-only"""
    H, W = frame
    src = FC.image("random", H, W, seed=7)
    src.setflags(write=False)
    return src, [(name, box, FC.image(FC.IMAGE_KINDS[b % 3], FC.PASTE_S, FC.PASTE_S, seed=30 + b))
                 for b, (name, box) in enumerate(FC.paste_boxes(H, W))]


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
def test_no_feather_and_no_top_is_the_plain_paste(frame):
    src, cases = _frame_inputs(frame)
    for name, box, pred in cases:
        got, want = BC.blend_model(src, pred, box, 0, 0), FC.compose_model(src, pred, box)
        assert np.array_equal(got, want), FC.diff_message("identity %s %s" % (name, box), got, want)


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
def test_weights_fill_the_centre_and_mirror_left_to_right(frame):
    """max(a) == D for every box (Fe is per box: a small box still reaches full weight), a == 0 exactly in the rows above t0, and
    the weights are the same read from the right"""
    for name, (y1, y2, x1, x2) in FC.paste_boxes(*frame):
        h, w = y2 - y1, x2 - x1
        for F in (0,) + BC.MODEL_FEATHERS:
            for T in BC.MODEL_TOPS:
                a, D = BC.weights(h, w, F, T)
                t0, Fe = BC.effective_feather(h, w, F, T)
                case = (name, h, w, F, T)
                assert a.shape == (h, w) and int(a.max()) == D == (Fe + 1) ** 2, case
                assert 0 <= Fe <= F and 0 <= t0 < h, case
                assert not a[:t0].any() and a[t0:].min() >= 1, case
                assert np.array_equal(a, a[:, ::-1]), case
                assert np.array_equal(a[t0:], a[t0:][::-1]), case          # and top to bottom within the blended rows


@pytest.mark.parametrize("T", BC.MODEL_TOPS)
@pytest.mark.parametrize("F", BC.MODEL_FEATHERS)
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%dx%d" % f)
def test_model_stays_within_the_bound_of_the_float64_blend(frame, F, T):
    src, cases = _frame_inputs(frame)
    worst = 0.0
    for name, box, pred in cases:
        got = BC.blend_model(src, pred, box, F, T)
        d = np.abs(got.astype(np.float64) - BC.blend_f64(src, pred, box, F, T))
        y1, y2, x1, x2 = box
        outside = d.copy()
        outside[y1:y2, x1:x2] = 0
        assert not outside.any(), (name, box)
        t0 = BC.effective_feather(y2 - y1, x2 - x1, F, T)[0]
        assert np.array_equal(got[y1:y1 + t0, x1:x2], src[y1:y1 + t0, x1:x2]), (name, box)     # above t0: the frame itself
        worst = max(worst, float(d.max()))
        assert d.max() < BC.BLEND_BOUND, "%s box %s F=%d T=%d: %.4f from the float64 blend" % (name, box, F, T, d.max())
    print("frame %dx%d F=%d T=%d: worst %.4f grey levels" % (frame[0], frame[1], F, T, worst))


def test_numerators_fit_32_bits_and_the_reciprocal_divides_exactly():
    """every numerator a*p + (D-a)*o + D/2 lies in [0, 255*D + D/2] <= 4225*255 + 2112 < 2^31; for every D = (Fe+1)^2 > 1 the
    kernels' quotient (n * ceil(2^32/D)) >> 32 equals n // D on ALL of that range, the multiplier fits 32 bits and the product
    64.  D == 1 has no band (a is 0 or D there, checked above): the kernels never divide by it"""
    assert BC.MAX_NUMERATOR == 4225 * 255 + 2112 < 2 ** 31
    for Fe in range(BC.MAX_FEATHER + 1):
        D = (Fe + 1) ** 2
        top = 255 * D + D // 2
        assert top <= BC.MAX_NUMERATOR
        # the extreme numerators are reached: a = D - 1, p = o = 255 and a = 1, p = o = 0
        assert (D - 1) * 255 + 1 * 255 + D // 2 == top
        if D == 1:
            a, _ = BC.weights(5, 5, 0, 0)
            assert set(np.unique(a)) == {1}
            continue
        m = BC.reciprocal(D)
        assert m == -(-2 ** 32 // D) and m < 2 ** 32 and top * m < 2 ** 64
        n = np.arange(top + 1, dtype=np.uint64)
        q = BC.divide_by_reciprocal(n, D)
        bad = np.flatnonzero(q != n // np.uint64(D))
        assert bad.size == 0, "D = %d: %d numerators divide wrongly, first %d" % (D, bad.size, int(bad[0]))


def test_check_blend_accepts_and_rejects():
    from wav2lip_amd import inference
    cb = inference.check_blend
    assert cb(None) is None and cb((0, 0.0)) is None and cb((0, 0)) is None and cb([0, 0.003]) is None     # int(0.003 * 256) == 0
    assert cb((3, 0.5)) == (3, 0.5) and cb((0, 0.5)) == (0, 0.5) and cb((64, 0.0)) == (64, 0.0) and cb([1, 0]) == (1, 0.0)
    assert cb((np.int64(8), np.float32(0.25))) == (8, 0.25)
    assert cb(cb((3, 0.5))) == (3, 0.5)                                       # what it returns passes again, unchanged
    assert inference.blend_top_q8(0.5) == 128 and inference.blend_top_q8(0.0) == 0 and inference.blend_top_q8(0.999999) == 255
    assert isinstance(cb((np.int64(8), 0.25))[0], int)
    for bad in ((-1, 0.0), (65, 0.0), (3, 1.0), (3, -0.1), (3, float("nan")), (3.0, 0.5), ("3", 0.5), (3, "0.5"), (True, 0.5),
                (3, None), (3,), (3, 0.5, 1), 3, "ab"):
        with pytest.raises(ValueError, match="blend"):
            cb(bad)


def test_blend_kw_is_empty_for_the_plain_paste():
    from wav2lip_amd import inference
    assert inference._blend_kw(None) == {}
    assert inference._blend_kw((0, 0.0)) == {}
    assert inference._blend_kw((4, 0.5)) == {"blend": (4, 0.5)}
    with pytest.raises(ValueError, match="blend"):
        inference._blend_kw((65, 0.0))


def _parsers():
    from wav2lip_amd import gen_videos_from_filelist, inference, real_videos_inference, streaming
    return {
        "inference": (inference.cli_parser, ["--checkpoint_path", "c", "--face", "f.png", "--audio", "a.wav"]),
        "gen_videos_from_filelist": (gen_videos_from_filelist.main_parser,
                                     ["--filelist", "f", "--results_dir", "r", "--data_root", "d", "--checkpoint_path", "c"]),
        "real_videos_inference": (real_videos_inference.main_parser,
                                  ["--mode", "tts", "--results_dir", "r", "--data_root", "d", "--checkpoint_path", "c"]),
        "streaming": (streaming.build_parser(), ["--checkpoint_path", "c", "--face", "f", "--audio", "a"]),
    }


@pytest.mark.parametrize("command", ["inference", "gen_videos_from_filelist", "real_videos_inference", "streaming"])
def test_the_four_command_lines_take_the_two_flags(command, capsys):
    from wav2lip_amd import inference
    parser, base = _parsers()[command]
    a = parser.parse_args(base)
    assert (a.blend_feather, a.blend_top) == (0, 0.0) and inference.blend_from_args(a) is None
    a = parser.parse_args(base + ["--blend_feather", "4", "--blend_top", "0.5"])
    assert (a.blend_feather, a.blend_top) == (4, 0.5) and inference.blend_from_args(a) == (4, 0.5)
    a = parser.parse_args(base + ["--blend_feather", "64", "--blend_top", "0.99"])
    assert inference.blend_from_args(a) == (64, 0.99)
    assert inference.blend_from_args(parser.parse_args(base + ["--blend_top", "0.5"])) == (0, 0.5)
    for bad in (["--blend_feather", "65"], ["--blend_feather", "-1"], ["--blend_feather", "2.5"], ["--blend_feather", "x"],
                ["--blend_top", "1.0"], ["--blend_top", "-0.1"], ["--blend_top", "nan"], ["--blend_top", "half"]):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)
    capsys.readouterr()
    assert "--blend_feather" in parser.format_help() and "--blend_top" in parser.format_help()


def test_the_reference_surfaces_do_not_have_the_flags():
    from wav2lip_amd import gen_videos_from_filelist, inference, real_videos_inference
    for p in (inference.parser, gen_videos_from_filelist.parser, gen_videos_from_filelist.cli_parser, real_videos_inference.parser,
              real_videos_inference.cli_parser):
        assert not any(o.startswith("--blend") for act in p._actions for o in act.option_strings)
    # a namespace from such a parser means: no blend
    a = gen_videos_from_filelist.cli_parser.parse_args(["--filelist", "f", "--results_dir", "r", "--data_root", "d", "--checkpoint_path", "c"])
    assert inference.blend_from_args(a) is None


def test_a_bad_flag_value_stops_main_before_any_device_work(monkeypatch, tmp_path):
    """`--blend_feather 65` is a parse error in every command; nothing of the run starts (no file is looked at, no process group,
    no runner)"""
    from wav2lip_amd import gen_videos_from_filelist, inference, real_videos_inference, sharding, streaming

    def forbidden(*a, **k):
        raise AssertionError("device work was started")

    monkeypatch.setattr(sharding, "init_from_env", forbidden)
    monkeypatch.setattr(inference, "PipelinedRunner", forbidden)
    monkeypatch.setattr(inference, "load_model", forbidden)
    monkeypatch.setattr(inference, "read_frames", forbidden)
    for main, base in ((inference.main, _parsers()["inference"][1]), (gen_videos_from_filelist.main, _parsers()["gen_videos_from_filelist"][1]),
                       (real_videos_inference.main, _parsers()["real_videos_inference"][1]), (streaming.main, _parsers()["streaming"][1])):
        for bad in (["--blend_feather", "65"], ["--blend_top", "1.5"]):
            with pytest.raises(SystemExit):
                main(base + bad)


def test_lipsync_refuses_a_blend_in_the_host_paste_case(monkeypatch):
    """without a box, or with frames of several shapes, `lipsync` pastes on the host: a blend there raises and names the option,
    before the spectrogram and before a runner exists"""
    from wav2lip_amd import audio, inference
    built = []

    class Runner:
        def __init__(self, *a, **k):
            built.append((a, k))
            raise AssertionError("a runner was built")

    def no_mel(*a, **k):
        raise AssertionError("the spectrogram was computed")

    monkeypatch.setattr(inference, "PipelinedRunner", Runner)
    monkeypatch.setattr(audio, "melspectrogram_device", no_mel)
    frames = [np.zeros((96, 96, 3), np.uint8)] * 3
    wav = np.zeros(16000, np.float32)
    with pytest.raises(ValueError, match="blend"):
        inference.lipsync(object(), frames, wav, blend=(3, 0.5))                           # no box: pre-sized faces, host paste
    with pytest.raises(ValueError, match="blend"):
        inference.lipsync(object(), frames + [np.zeros((100, 96, 3), np.uint8)], wav, box=(0, 96, 0, 96), blend=(3, 0.5))
    with pytest.raises(ValueError, match="blend"):
        inference.lipsync(object(), frames, wav, box=(0, 96, 0, 96), blend=(65, 0.5))     # a bad pair, in the device case
    assert not built
