"""`--face_det_precision` on the inference command line (a documented addition, not one of the reference's flags): fp32 by
default, bf16 on request, anything else is a parse error; independent of the generator's `--precision`.  Runs without a GPU."""
import pytest

from wav2lip_amd import inference

BASE = ["--checkpoint_path", "ckpt.pth", "--face", "face.png", "--audio", "a.wav"]


def test_face_det_precision_defaults_to_fp32():
    a = inference.parse_args(BASE)
    assert a.face_det_precision == "fp32"
    assert inference.CLI_PRECISION[a.face_det_precision] == "f32"


def test_face_det_precision_bf16_is_accepted():
    a = inference.parse_args(BASE + ["--face_det_precision", "bf16"])
    assert a.face_det_precision == "bf16"
    assert inference.CLI_PRECISION[a.face_det_precision] == "bf16"


@pytest.mark.parametrize("bad", ["fp16", "f32", "BF16", "fp8", ""])
def test_bad_face_det_precision_is_a_parse_error(bad, capsys):
    with pytest.raises(SystemExit) as e:
        inference.parse_args(BASE + ["--face_det_precision", bad])
    assert e.value.code == 2
    assert "--face_det_precision" in capsys.readouterr().err


@pytest.mark.parametrize("gen,det", [("fp32", "bf16"), ("bf16", "fp32"), ("bf16", "bf16"), ("fp32", "fp32")])
def test_the_two_precision_flags_are_independent(gen, det):
    a = inference.parse_args(BASE + ["--precision", gen, "--face_det_precision", det])
    assert (a.precision, a.face_det_precision) == (gen, det)
    assert inference.parse_args(BASE + ["--face_det_precision", det]).precision == "fp32"
    assert inference.parse_args(BASE + ["--precision", gen]).face_det_precision == "fp32"


def test_reference_parser_is_unchanged():
    """`inference.parser` keeps the reference's surface: neither precision flag is on it"""
    opts = {o for act in inference.parser._actions for o in act.option_strings}
    assert "--face_det_precision" not in opts and "--precision" not in opts
    with pytest.raises(SystemExit):
        inference.parser.parse_args(BASE + ["--face_det_precision", "bf16"])
    assert "--face_det_precision" in {o for act in inference.cli_parser._actions for o in act.option_strings}


def test_face_detect_rejects_a_bad_precision_before_touching_the_device():
    with pytest.raises(ValueError):
        inference.face_detect([], detector=object(), precision="fp16")
