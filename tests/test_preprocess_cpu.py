"""The command-line surface of wav2lip_amd.preprocess against the reference's preprocess.py (flags, types, defaults, required),
the `--ngpu` / launch check, discovery and output naming - everything that needs no device."""
import argparse
import os

import pytest

from wav2lip_amd import preprocess

# preprocess.py:21-26 of the reference: (flag, type, default, required)
REFERENCE_FLAGS = [("--ngpu", int, 1, False), ("--batch_size", int, 32, False), ("--data_root", None, None, True),
                   ("--preprocessed_root", None, None, True)]


def _actions(parser):
    return {a.option_strings[0]: a for a in parser._actions if a.option_strings and not isinstance(a, argparse._HelpAction)}


def test_reference_flags_keep_their_names_types_defaults_and_requiredness():
    acts = _actions(preprocess.parser)
    for flag, typ, default, required in REFERENCE_FLAGS:
        a = acts[flag]
        assert (a.type, a.default, a.required) == (typ, default, required), flag
    assert set(acts) == {f for f, _, _, _ in REFERENCE_FLAGS} | {"--face_det_precision"}


def test_face_det_precision_is_fp32_by_default_and_takes_bf16():
    a = preprocess.parser.parse_args(["--data_root", "d", "--preprocessed_root", "p"])
    assert (a.ngpu, a.batch_size, a.face_det_precision) == (1, 32, "fp32")
    b = preprocess.parser.parse_args(["--data_root", "d", "--preprocessed_root", "p", "--face_det_precision", "bf16"])
    assert b.face_det_precision == "bf16"
    with pytest.raises(SystemExit):
        preprocess.parser.parse_args(["--data_root", "d", "--preprocessed_root", "p", "--face_det_precision", "fp16"])


@pytest.mark.parametrize("ngpu,world", [(1, 1), (1, 4), (4, 4), (8, 8)])
def test_ngpu_one_or_the_world_size_is_accepted(ngpu, world):
    preprocess.check_world(ngpu, world)


@pytest.mark.parametrize("ngpu,world", [(2, 1), (4, 2), (0, 1)])
def test_other_ngpu_names_the_launch_command(ngpu, world):
    with pytest.raises(ValueError) as e:
        preprocess.check_world(ngpu, world)
    msg = str(e.value)
    assert "python -m torch.distributed.run --nproc-per-node %d -m wav2lip_amd.preprocess" % ngpu in msg


def test_main_checks_ngpu_before_touching_a_device(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "1")
    args = preprocess.parser.parse_args(["--data_root", str(tmp_path), "--preprocessed_root", str(tmp_path / "o"), "--ngpu", "2"])
    with pytest.raises(ValueError, match="torch.distributed.run"):
        preprocess.main(args)


def test_discovery_takes_mp4_and_avi_one_directory_down(tmp_path):
    for rel in ("a/1.mp4", "a/2.avi", "b/3.avi", "b/4.wav", "5.avi", "c/d/6.avi"):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    got = [os.path.relpath(f, str(tmp_path)) for f in preprocess.list_videos(str(tmp_path))]
    assert got == ["a/1.mp4", "a/2.avi", "b/3.avi"]


def test_output_directory_is_the_references(tmp_path):
    args = argparse.Namespace(preprocessed_root="out")
    assert preprocess._out_dir("root/spk/00017.avi", args) == os.path.join("out", "spk", "00017")
    assert preprocess._out_dir("root/spk/clip.v2.avi", args) == os.path.join("out", "spk", "clip")


def test_an_mp4_is_refused_with_the_reason(tmp_path):
    v = tmp_path / "spk" / "1.mp4"
    v.parent.mkdir()
    v.write_bytes(b"\x00" * 16)
    args = argparse.Namespace(preprocessed_root=str(tmp_path / "out"), batch_size=4, face_det_precision="fp32")
    with pytest.raises(ValueError, match="AVI"):
        preprocess.process_audio_file(str(v), args)
    assert not (tmp_path / "out").exists()


def test_audio_is_written_unchanged_as_a_wav(tmp_path):
    import wave

    import numpy as np
    from wav2lip_amd import container
    pcm = np.arange(-300, 300, dtype=np.int16).reshape(-1, 2)
    frames = np.zeros((3, 8, 8, 3), np.uint8)
    v = tmp_path / "spk" / "7.avi"
    v.parent.mkdir()
    container.write_avi(str(v), frames, 25, audio=pcm, audio_sr=22050)
    args = argparse.Namespace(preprocessed_root=str(tmp_path / "out"))
    preprocess.process_audio_file(str(v), args)
    with wave.open(str(tmp_path / "out" / "spk" / "7" / "audio.wav")) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (2, 2, 22050)
        got = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, 2)
    assert np.array_equal(got, pcm)
