"""Colour matching on the CPU: the numpy model of tests/_color_cases.py against the float64 transfer and against what each
constructed case is for (asserted on the model's intermediate values, not only on its output), the spelling and the flags of the
four commands, and the shared arithmetic of csrc/color_match_core.h as a host program under the host sanitizers."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _color_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = sorted(CC.MODES)


# ---------------------------------------------------------------- the model against float64
def _in_play(pred, ref, mode):
    """(|model - float64| where neither side clamps, the mask of those pixels)"""
    out, info = CC.model(pred, ref, mode)
    f = CC.transfer_f64(pred, ref, mode)
    quot = np.stack([ch["quot"] for ch in info], axis=2)
    mask = (quot >= 0) & (quot <= 255) & (f >= 0.0) & (f <= 255.0)
    assert np.array_equal(out[mask], quot[mask])
    return np.abs(out.astype(np.float64) - f), mask


def test_model_stays_within_the_bound_of_the_float64_transfer_on_random_cases():
    cases = CC.random_cases()
    assert {S for S, _, _ in cases} == {2, 6, 96}
    worst, used, total = 0.0, 0, 0
    for S, pred, ref in cases:
        for mode in MODES:
            err, mask = _in_play(pred, ref, mode)
            used += int(mask.sum())
            total += mask.size
            if mask.any():
                worst = max(worst, float(err[mask].max()))
    print("worst deviation %.4f grey levels, %d of %d pixels in play" % (worst, used, total))
    assert worst <= CC.COLOR_BOUND
    assert used >= 0.9 * total                      # the exclusion of clamped pixels leaves the comparison its substance
    assert used < total                             # ... and some of the random cases do clamp


@pytest.mark.parametrize("mode", MODES)
def test_constructed_cases_stay_within_the_bound_too(mode):
    for S, group in CC.case_groups()[:3]:
        for name, (pred, ref) in group.items():
            err, mask = _in_play(pred, ref, mode)
            assert not mask.any() or err[mask].max() <= CC.COLOR_BOUND, (S, name, err[mask].max())


# ---------------------------------------------------------------- identity
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [2, 6, 96])
def test_equal_upper_halves_leave_the_prediction_unchanged(S, mode):
    r = np.random.default_rng(20 + S)
    ref = r.integers(0, 256, (S, S, 3), dtype=np.uint8)
    pred = ref.copy()
    pred[S // 2:] = r.integers(0, 256, (S // 2, S, 3), dtype=np.uint8)
    out, info = CC.model(pred, ref, mode)
    assert np.array_equal(out, pred) and not np.array_equal(pred, ref)
    assert all(ch["g"] == 256 for ch in info)
    flat = np.full((S, S, 3), 77, dtype=np.uint8)                       # a flat pair too (Vp == Vo == 0)
    assert np.array_equal(CC.model(flat, flat, mode)[0], flat)


@pytest.mark.parametrize("mode", MODES)
def test_the_lower_half_of_the_reference_does_not_matter(mode):
    pred, ref = CC.constructed_cases(6)["noise"]
    other = ref.copy()
    other[3:] = 255 - other[3:]
    assert np.array_equal(CC.model(pred, ref, mode)[0], CC.model(pred, other, mode)[0])


# ---------------------------------------------------------------- what each constructed case is for
def _info(S, name, mode):
    pred, ref = CC.constructed_cases(S)[name]
    return CC.model(pred, ref, mode)


@pytest.mark.parametrize("S", [CC.PRODUCT_S, CC.SMALL_S, 2])
def test_constructed_cases_have_the_properties_they_are_named_for(S):
    for name in CC.constructed_cases(S):
        assert all(ch["g"] == 256 and ch["root"] is None for ch in _info(S, name, "mean")[1]), name
    _, info = _info(S, "flat_pred", "full")
    assert all(ch["Vp"] == 0 and ch["Vo"] > 0 and ch["g"] == 256 for ch in info)
    _, info = _info(S, "flat_ref", "full")
    assert all(ch["Vo"] == 0 and ch["Vp"] > 0 and ch["root"] == 0 and ch["g"] == 128 for ch in info)
    _, info = _info(S, "ratio_high", "full")
    assert all(ch["root"] > 512 and ch["g"] == 512 for ch in info)
    _, info = _info(S, "ratio_exactly_half", "full")
    assert all((ch["Vo"] << 16) // ch["Vp"] == 128 * 128 and ch["root"] == 128 == ch["g"] for ch in info)
    _, info = _info(S, "ratio_exactly_two", "full")
    assert all((ch["Vo"] << 16) // ch["Vp"] == 512 * 512 and ch["root"] == 512 == ch["g"] for ch in info)
    _, info = _info(S, "three_gains", "full")
    assert [ch["g"] for ch in info] == [192, 256, 384] and [ch["root"] for ch in info] == [192, 256, 384]
    out, info = _info(S, "identity", "full")
    assert np.array_equal(out, CC.constructed_cases(S)["identity"][0])
    _, info = _info(S, "noise", "full")
    assert len({ch["g"] for ch in info}) >= 2 or S == 2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [CC.PRODUCT_S, CC.SMALL_S, 2])
def test_the_saturating_case_leaves_0_to_255_on_both_sides(S, mode):
    """quotients below 0 and above 255 before the clamp, 0 and 255 after it; and a negative numerator that is no multiple of the
    divisor, less than one divisor below zero: truncation toward zero would make its quotient 0 where the floor is -1 (both clamp
    to 0 in the output, which is why the property is asserted here, on the quotient)"""
    out, info = _info(S, "saturate", mode)
    quot = np.stack([ch["quot"] for ch in info], axis=2)
    assert quot.min() < 0 and quot.max() > 255
    assert out[quot < 0].max() == 0 and out[quot > 255].min() == 255
    assert any(((ch["num"] < 0) & (ch["num"] % ch["den"] != 0)).any() for ch in info)
    assert (info[0]["quot"] < 0).any() and (info[1]["quot"] > 255).any()
    if mode == "full":
        assert info[2]["g"] == 512 and (info[2]["quot"] < 0).any() and (info[2]["quot"] > 255).any()


def test_floor_and_truncation_differ_on_a_numerator_just_below_zero():
    """S = 2 (N = 2, divisor 512, mean mode: the numerator is 256*(2x - Sp) + 256*So + 256), worked by hand: a numerator of -256
    has the floor quotient -1 where truncation toward zero gives 0"""
    pred = np.zeros((2, 2, 3), np.uint8)
    ref = np.zeros((2, 2, 3), np.uint8)
    pred[0, :, 0] = (1, 2)          # Sp = 3
    ref[0, :, 0] = (0, 0)           # So = 0
    pred[1, :, 0] = (1, 0)          # x = 1: 256*(2 - 3) + 0 + 256 = 0 -> 0; x = 0: 256*(0 - 3) + 256 = -512 -> -1
    pred[0, :, 1] = (1, 1)          # Sp = 2
    ref[0, :, 1] = (0, 1)           # So = 1
    pred[1, :, 1] = (0, 0)          # x = 0: 256*(0 - 2) + 256 + 256 = 0 -> 0
    pred[0, :, 2] = (2, 1)          # Sp = 3
    ref[0, :, 2] = (1, 0)           # So = 1
    pred[1, :, 2] = (1, 0)          # x = 1: -256 + 256 + 256 = 256 -> 0; x = 0: -768 + 512 = -256 -> floor -1, truncation 0
    out, info = CC.model(pred, ref, "mean")
    assert info[0]["num"][1].tolist() == [0, -512] and info[0]["quot"][1].tolist() == [0, -1]
    assert info[2]["num"][1].tolist() == [256, -256] and info[2]["quot"][1].tolist() == [0, -1]
    assert int(-256 / 512) == 0                                         # what truncation would give
    assert out[1, :, 2].tolist() == [0, 0]


def test_the_largest_sums_and_numerators():
    cases = CC.largest_sums_cases()
    for mode in MODES:
        out, info = CC.model(*cases["all_255"], mode)
        assert np.array_equal(out, cases["all_255"][0])
        for ch in info:
            assert ch["Sp"] == ch["So"] == 32768 * 255 and ch["Qp"] == 32768 * 65025 < 1 << 32
            assert ch["Vp"] == 0 and 32768 * ch["Qp"] > 1 << 45 and ch["g"] == 256
            assert int(ch["num"].max()) == 256 * 255 * 32768 + 128 * 32768
        out, info = CC.model(*cases["wide"], mode)
        for ch in info:
            assert int(ch["num"].max()) > (1 << 31) - 1                  # the numerator leaves int32
            assert ch["g"] == (512 if mode == "full" else 256)
            assert mode == "mean" or ((ch["Vo"] << 16) >> 59 and ch["root"] > 512)      # the shifted variance needs 60 bits


def test_the_s2_group_is_two_pixels_of_statistics():
    for name, (pred, ref) in CC.constructed_cases(2).items():
        assert pred.shape == ref.shape == (2, 2, 3)
        out, info = CC.model(pred, ref, "full")
        assert all(ch["den"] == 512 for ch in info)


def test_case_groups_cover_the_sizes():
    groups = CC.case_groups()
    assert [S for S, _ in groups] == [96, 6, 2, 256]
    assert ((6 // 2) * 6) % 4 != 0                                          # the ragged upper half
    for S, group in groups:
        pred, ref = CC.stack(group)
        assert pred.shape == ref.shape == (len(group), S, S, 3)
        for mode in MODES:
            want = CC.model_rows(pred, ref, mode)
            assert len({want[k].tobytes() for k in range(len(group))}) == len(group)     # rows with different results


# ---------------------------------------------------------------- the spelling and the flags
def test_check_color_match_accepts_and_rejects():
    from wav2lip_amd import inference
    cc = inference.check_color_match
    assert cc(None) is None and cc("mean") == "mean" and cc("full") == "full"
    assert inference.COLOR_MATCH_MODES == CC.MODES
    for bad in ("", "Mean", "histogram", "off", 1, 2, True, False, 0, ("mean",), ["full"], b"mean", 0.5):
        with pytest.raises(ValueError, match="'mean' or 'full'"):
            cc(bad)
    assert inference._color_kw(None) == {} and inference._color_kw("full") == {"color_match": "full"}
    with pytest.raises(ValueError, match="color_match"):
        inference._color_kw("both")


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
def test_the_four_command_lines_take_the_flag(command, capsys):
    from wav2lip_amd import inference
    parser, base = _parsers()[command]
    a = parser.parse_args(base)
    assert a.color_match is None and inference.color_match_from_args(a) is None          # off by default
    for mode in MODES:
        a = parser.parse_args(base + ["--color_match", mode])
        assert a.color_match == mode and inference.color_match_from_args(a) == mode
    a = parser.parse_args(base + ["--color_match", "full", "--blend_feather", "4", "--blend_top", "0.5"])     # independent
    assert inference.color_match_from_args(a) == "full" and inference.blend_from_args(a) == (4, 0.5)
    for bad in (["--color_match", "histogram"], ["--color_match", "1"], ["--color_match", ""], ["--color_match"]):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)
    capsys.readouterr()
    assert "--color_match" in parser.format_help()


def test_the_reference_surfaces_do_not_have_the_flag():
    from wav2lip_amd import gen_videos_from_filelist, inference, real_videos_inference
    for p in (inference.parser, gen_videos_from_filelist.parser, gen_videos_from_filelist.cli_parser, real_videos_inference.parser,
              real_videos_inference.cli_parser):
        assert not any(o.startswith("--color") for act in p._actions for o in act.option_strings)
    a = gen_videos_from_filelist.cli_parser.parse_args(["--filelist", "f", "--results_dir", "r", "--data_root", "d", "--checkpoint_path", "c"])
    assert inference.color_match_from_args(a) is None


def test_a_bad_flag_value_stops_main_before_any_device_work(monkeypatch):
    from wav2lip_amd import gen_videos_from_filelist, inference, real_videos_inference, sharding, streaming

    def forbidden(*a, **k):
        raise AssertionError("device work was started")

    monkeypatch.setattr(sharding, "init_from_env", forbidden)
    monkeypatch.setattr(inference, "PipelinedRunner", forbidden)
    monkeypatch.setattr(inference, "load_model", forbidden)
    monkeypatch.setattr(inference, "read_frames", forbidden)
    for main, base in ((inference.main, _parsers()["inference"][1]), (gen_videos_from_filelist.main, _parsers()["gen_videos_from_filelist"][1]),
                       (real_videos_inference.main, _parsers()["real_videos_inference"][1]), (streaming.main, _parsers()["streaming"][1])):
        with pytest.raises(SystemExit):
            main(base + ["--color_match", "histogram"])


def test_the_carriers_refuse_a_bad_value_before_any_device_work(monkeypatch):
    """`lipsync`, `lipsync_many` and `LipsyncStreams` name the option before a spectrogram or a runner exists; the runners check
    it themselves"""
    from wav2lip_amd import audio, inference, multiclip, streaming

    def forbidden(*a, **k):
        raise AssertionError("device work was started")

    monkeypatch.setattr(inference, "PipelinedRunner", forbidden)
    monkeypatch.setattr(multiclip, "BatchRunner", forbidden)
    monkeypatch.setattr(audio, "melspectrogram_device", forbidden)
    frames = [np.zeros((96, 96, 3), np.uint8)] * 3
    with pytest.raises(ValueError, match="color_match"):
        inference.lipsync(object(), frames, np.zeros(16000, np.float32), color_match="both")
    with pytest.raises(ValueError, match="color_match"):
        multiclip.lipsync_many(object(), iter(()), color_match="both")
    with pytest.raises(ValueError, match="color_match"):
        streaming.LipsyncStreams(object(), color_match=2)
    assert streaming.LipsyncStreams(object(), color_match="mean").color_match == "mean"
    assert streaming.LipsyncStreams(object()).color_match is None


# ---------------------------------------------------------------- the shared arithmetic, on the CPU
def test_the_shared_arithmetic_under_the_host_sanitizers():
    """tools/color_match_host_check.py builds tools/color_match_host.cpp (a stand-alone program around csrc/color_match_core.h;
    nothing is loaded into Python, nothing touches a GPU) with -fsanitize=address,undefined and runs it over every case of the
    list in both modes, out of place and in place: the bytes and the gains equal the model's; a report of either sanitizer ends
    the program with a failure"""
    n = 2 * sum(len(group) for _, group in CC.case_groups())
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "color_match_host_check.py")], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "%d of %d cases equal, 0 failures" % (n, n) in run.stdout
    assert "runtime error" not in run.stdout and "AddressSanitizer" not in run.stdout
