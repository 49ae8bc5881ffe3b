"""`--precision` on the inference command line (a documented addition, not one of the reference's flags): fp32 by default,
bf16 on request, anything else is a parse error.  Runs without a GPU."""
import pytest

from wav2lip_amd import inference

BASE = ["--checkpoint_path", "ckpt.pth", "--face", "face.png", "--audio", "a.wav"]


def test_precision_defaults_to_fp32():
    a = inference.parse_args(BASE)
    assert a.precision == "fp32"
    assert inference.CLI_PRECISION[a.precision] == "f32"


def test_precision_bf16_is_accepted():
    a = inference.parse_args(BASE + ["--precision", "bf16"])
    assert a.precision == "bf16"
    assert inference.CLI_PRECISION[a.precision] == "bf16"


@pytest.mark.parametrize("bad", ["fp16", "f32", "BF16", "fp8", ""])
def test_bad_precision_is_a_parse_error(bad, capsys):
    with pytest.raises(SystemExit) as e:
        inference.parse_args(BASE + ["--precision", bad])
    assert e.value.code == 2
    assert "--precision" in capsys.readouterr().err


def test_reference_flags_are_unchanged():
    """the flag adds one option; every reference flag keeps its default"""
    a = inference.parse_args(BASE)
    assert (a.wav2lip_batch_size, a.face_det_batch_size, a.resize_factor, a.pads, a.box) == (128, 16, 1, [0, 10, 0, 0], [-1, -1, -1, -1])


def test_precision_checker_rejects_other_values():
    from wav2lip_amd.models.wav2lip import check_precision
    assert check_precision("f32") == "f32" and check_precision("bf16") == "bf16"
    for bad in ("fp32", "fp16", None, 16):
        with pytest.raises(ValueError):
            check_precision(bad)
