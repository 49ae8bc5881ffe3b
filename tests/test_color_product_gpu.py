"""Colour matching through the product: `Wav2LipRunner.run_batch` / `run_frames`, `multiclip.lipsync_many`,
`streaming.LipsyncStreams` against `inference.lipsync`, the host paste of `lipsync`, and the command-line switch of
`inference.main`.  Synthetic weights, the smallest clips that do the job; every expectation is the numpy model of
tests/_color_cases.py (and of tests/_blend_cases.py for the paste), byte for byte.

A run with the option and a run without it launch the same generator plan on the same inputs, so their predictions are the same
bytes.  Where a test has no prediction in hand it uses a 96x96 box: crop and paste are then copies, the box of the default run's
output IS the prediction and the box of the input frame IS the crop the generator was given."""
import os

import numpy as np
import pytest
import torch

import _blend_cases as BC
import _color_cases as CC
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu
N_SAMPLES = 7000          # 36 mel columns: 7 full windows at 25 fps and the re-anchored tail, 8 rows = one batch of 8
diff = BC.FC.diff_message


def _state_dict():
    from wav2lip_amd import models
    return synth.synthetic_state_dict({k: tuple(v.shape) for k, v in models.Wav2Lip().state_dict().items()}, seed=0)


@pytest.fixture(scope="module")
def model(cuda):
    from wav2lip_amd import models
    m = models.Wav2Lip()
    m.load_state_dict(_state_dict())
    return m.to(cuda).eval()


@pytest.fixture(scope="module")
def clip():
    r = np.random.default_rng(61)
    return r.integers(0, 256, (12, 120, 150, 3), dtype=np.uint8)


def _matched_box(frame, plain, box, mode):
    """`plain` (the default run's output frame) with its 96x96 box matched to the same box of the input frame"""
    y1, y2, x1, x2 = box
    assert (y2 - y1, x2 - x1) == (96, 96)
    want = plain.copy()
    want[y1:y2, x1:x2] = CC.model(plain[y1:y2, x1:x2], frame[y1:y2, x1:x2], mode)[0]
    return want


@pytest.mark.parametrize("mode", sorted(CC.MODES))
def test_run_batch_matches_the_plain_prediction_to_the_faces(cuda, model, mode):
    from wav2lip_amd import inference
    n = 5
    faces = synth.face_crops_u8(n, seed=4)
    mels = torch.from_numpy(synth.mel_windows(n, seed=4)).to(cuda)
    faces_dev = torch.from_numpy(faces).to(cuda)
    plain = inference.Wav2LipRunner(model, batch_size=n).run_batch(faces_dev, mel_windows=mels).cpu().numpy()
    off = inference.Wav2LipRunner(model, batch_size=n, color_match=None)
    assert off.color_match is None
    assert np.array_equal(off.run_batch(faces_dev, mel_windows=mels).cpu().numpy(), plain)
    runner = inference.Wav2LipRunner(model, batch_size=n, color_match=mode)
    assert runner.color_match == mode
    got = runner.run_batch(faces_dev, mel_windows=mels).cpu().numpy()
    want = CC.model_rows(plain, faces, mode)
    assert np.array_equal(got, want), diff("run_batch %s" % mode, got, want)
    assert not np.array_equal(got, plain)
    slot = torch.zeros((n + 2, 96, 96, 3), dtype=torch.uint8, device=cuda)          # the `out=` form: a send slot's view
    assert runner.run_batch(faces_dev, mel_windows=mels, out=slot[1:n + 1]) is not None
    slot = slot.cpu().numpy()
    assert np.array_equal(slot[1:n + 1], want) and not slot[0].any() and not slot[n + 1].any()
    assert np.array_equal(faces_dev.cpu().numpy(), faces)                            # the faces are not written


def test_run_frames_pastes_and_blends_the_matched_prediction(cuda, model, clip):
    """four rows with four boxes (general, 96x96 copy, 2x area, one at the frame's corner): the output is the paste's oracle (and,
    with blend=(3, 0.5), the blend's model) applied to the model of the prediction `run_batch` gives for the faces the crop
    kernel cuts"""
    from wav2lip_amd import _lib, inference
    from wav2lip_amd._lib import check, current_stream, ptr
    idx = [0, 5, 11, 3]
    boxes = [(10, 100, 20, 130), (3, 99, 5, 101), (20, 68, 100, 148), (30, 120, 60, 150)]
    n = len(idx)
    frames = torch.from_numpy(clip).to(cuda)
    mels = torch.from_numpy(synth.mel_windows(n, seed=3)).to(cuda)
    faces = torch.empty((n, 96, 96, 3), dtype=torch.uint8, device=cuda)
    # both tables stay alive in names until the launch has run: a temporary's block goes back to the allocator at once
    idx_dev = torch.tensor(idx, dtype=torch.int32, device=cuda)
    boxes_dev = torch.tensor(boxes, dtype=torch.int32, device=cuda)
    check(_lib.load().w2l_crop_resize_u8(current_stream(), n, ptr(frames), 120, 150, ptr(idx_dev), ptr(boxes_dev), 96, ptr(faces)), "crop")
    torch.cuda.synchronize()
    pred = inference.Wav2LipRunner(model, batch_size=n).run_batch(faces, mel_windows=mels).cpu().numpy()
    matched = CC.model_rows(pred, faces.cpu().numpy(), "full")
    plain = inference.Wav2LipRunner(model, batch_size=n).run_frames(frames, idx, boxes, mel_windows=mels).cpu().numpy()
    for blend, (F, T) in ((None, (0, 0)), ((3, 0.5), (3, 128))):
        runner = inference.Wav2LipRunner(model, batch_size=n, blend=blend, color_match="full")
        got = runner.run_frames(frames, idx, boxes, mel_windows=mels).cpu().numpy()
        assert got.shape == plain.shape == (n, 120, 150, 3)
        for k in range(n):
            want = BC.blend_model(clip[idx[k]], matched[k], boxes[k], F, T)          # F = T = 0: the plain paste
            assert np.array_equal(got[k], want), diff("run_frames blend %s row %d box %s" % (blend, k, boxes[k]), got[k], want)
            assert not np.array_equal(got[k], plain[k])
    assert torch.equal(frames.cpu(), torch.from_numpy(clip))                        # the input frames are not written


def test_lipsync_many_matches_every_row_of_two_clips_of_different_shapes(cuda, model):
    from wav2lip_amd import audio, multiclip
    r = np.random.default_rng(62)
    spec = {"a": (list(r.integers(0, 256, (3, 120, 150, 3), dtype=np.uint8)), (10, 106, 20, 116), 4000),
            "b": (list(r.integers(0, 256, (5, 97, 131, 3), dtype=np.uint8)), (1, 97, 35, 131), 5000)}
    rows = {}

    def jobs():
        for i, (k, (frames, box, ns)) in enumerate(spec.items()):
            mel = audio.melspectrogram_device(synth.noise_wav(ns, seed=70 + i), cuda)
            rows[k] = multiclip.rows_inference(mel.shape[1], len(frames), [box] * len(frames))
            yield multiclip.ClipJob(k, frames, mel, rows[k])

    plain = multiclip.lipsync_many(model, jobs(), batch_size=8)
    got = multiclip.lipsync_many(model, jobs(), batch_size=8, color_match="full")
    assert [len(rows[k]) for k in spec] == [3, 5]                                # one batch of 8 rows, two frame shapes
    for k, (frames, box, _) in spec.items():
        assert len(got[k]) == len(plain[k]) == len(rows[k])
        for i, (fi, _, _) in enumerate(rows[k]):
            want = _matched_box(frames[fi], plain[k][i], box, "full")
            assert np.array_equal(got[k][i], want), diff("clip %s row %d" % (k, i), got[k][i], want)
            assert not np.array_equal(got[k][i], plain[k][i])


def test_a_stream_equals_lipsync_on_the_whole_audio(cuda, model, clip):
    """one stream, its audio fed in ragged chunks; its 8 rows leave as one batch of 8, the batch `lipsync` runs: the same plan on
    the same faces and windows, so the frames are the same bytes (a general box: crop and paste resize)"""
    from wav2lip_amd import inference, streaming
    frames, box = list(clip[:5]), (10, 100, 20, 130)
    wav = synth.noise_wav(N_SAMPLES, seed=80)
    ref = inference.lipsync(model, frames, wav, batch_size=8, box=box, color_match="mean")
    plain = inference.lipsync(model, frames, wav, batch_size=8, box=box)
    ls = streaming.LipsyncStreams(model, batch_size=8, color_match="mean", mel_window=64)
    assert ls.color_match == "mean"
    ls.open("s", frames, [box] * len(frames))
    for lo in range(0, N_SAMPLES, 1777):
        ls.feed("s", wav[lo:lo + 1777])
        ls.step()
    ls.close("s")
    got = ls.drain()["s"]
    assert len(got) == len(ref) == len(plain) == 8
    for i, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(a, b), diff("streamed frame %d against lipsync" % i, a, b)
        assert not np.array_equal(b, plain[i])


@pytest.mark.parametrize("mode", sorted(CC.MODES))
def test_the_host_paste_of_lipsync_gets_the_matched_prediction(cuda, model, mode):
    """pre-sized 96x96 faces and no box: `lipsync` pastes on the host what `run_batch` returns, so every output frame is the
    model of the default run's frame and the input frame"""
    from wav2lip_amd import inference
    frames = list(synth.face_crops_u8(3, seed=9))
    wav = synth.noise_wav(N_SAMPLES, seed=81)
    plain = inference.lipsync(model, frames, wav, batch_size=8)
    got = inference.lipsync(model, frames, wav, batch_size=8, color_match=mode)
    assert len(got) == len(plain) == 8
    for i in range(8):
        want = CC.model(plain[i], frames[i % 3], mode)[0]
        assert np.array_equal(got[i], want), diff("frame %d" % i, got[i], want)
        assert not np.array_equal(got[i], plain[i])


def test_the_command_line_switch(cuda, tmp_path):
    """`--color_match mean` on a clip of three frames with a 96x96 `--box`: against the same command without the flag, every
    frame is the model applied to the default run's box and the input frame's; outside the box nothing differs"""
    from scipy.io import wavfile
    from wav2lip_amd import container, inference
    tmp = str(tmp_path)
    video = np.random.default_rng(63).integers(0, 256, (3, 120, 150, 3), dtype=np.uint8)
    container.write_avi(os.path.join(tmp, "face.avi"), video, 25)
    wav = synth.noise_wav(N_SAMPLES, seed=82) * np.float32(0.5)
    wavfile.write(os.path.join(tmp, "audio.wav"), 16000, np.clip(np.round(wav * 32768.0), -32768, 32767).astype(np.int16))
    torch.save({"state_dict": {"module." + k: v for k, v in _state_dict().items()}, "optimizer": None, "global_step": 7, "global_epoch": 1},
               os.path.join(tmp, "ckpt.pth"))
    box = (12, 108, 30, 126)
    common = ["--checkpoint_path", os.path.join(tmp, "ckpt.pth"), "--face", os.path.join(tmp, "face.avi"), "--audio",
              os.path.join(tmp, "audio.wav"), "--box"] + [str(v) for v in box] + ["--wav2lip_batch_size", "8"]
    plain = np.stack(inference.main(common + ["--outfile", os.path.join(tmp, "a.avi")]))
    assert inference.args.color_match is None
    got = np.stack(inference.main(common + ["--outfile", os.path.join(tmp, "b.avi"), "--color_match", "mean"]))
    assert inference.args.color_match == "mean"
    assert got.shape == plain.shape and len(got) >= 3 and got.shape[1:] == (120, 150, 3)
    for i in range(len(got)):
        want = _matched_box(video[i % 3], plain[i], box, "mean")
        assert np.array_equal(got[i], want), diff("frame %d" % i, got[i], want)
        assert not np.array_equal(got[i], plain[i])
    back = container.read_avi(os.path.join(tmp, "b.avi"))["frames"]
    assert np.array_equal(np.stack(list(back)), got)                             # what was written is what was returned
    assert np.array_equal(container.read_avi(os.path.join(tmp, "face.avi"))["frames"], video)       # the input is not written
