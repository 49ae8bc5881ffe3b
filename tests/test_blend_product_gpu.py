"""The feathered, mouth-region paste through the product: `Wav2LipRunner.run_frames`, `multiclip.lipsync_many`,
`streaming.LipsyncStreams` against `inference.lipsync`, and the command-line switch of `inference.main`.  Synthetic weights, the
smallest clips that do the job; every expectation is the numpy model of tests/_blend_cases.py, byte for byte.

A run with the blend and a run without it launch the same generator plan on the same inputs, so their predictions are the same
bytes: where a test has no prediction in hand, it takes the resized prediction from the box of the default run's output (the
plain paste, which tests/test_frame_kernels_gpu.py pins to the oracle) and blends that."""
import os

import numpy as np
import pytest
import torch

import _blend_cases as BC
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu
BLEND = (3, 0.5)
F, T = 3, 128
N_SAMPLES = 7000          # 36 mel columns: 7 full windows at 25 fps and the re-anchored tail, 8 rows = one batch of 8


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
    r = np.random.default_rng(31)
    return r.integers(0, 256, (12, 120, 150, 3), dtype=np.uint8)


def test_the_fraction_of_the_tests_is_the_top_q8_of_the_model():
    from wav2lip_amd import inference
    assert inference.check_blend(BLEND) == BLEND and (BLEND[0], inference.blend_top_q8(BLEND[1])) == (F, T)


def test_run_frames_blends_the_prediction_of_run_batch(cuda, model, clip):
    """four rows with four boxes (general, 96x96 copy, 2x area, one at the frame's corner): the output is the model applied to
    the prediction `run_batch` gives for the faces the crop kernel cuts"""
    from wav2lip_amd import _lib, inference
    from wav2lip_amd._lib import check, current_stream, ptr
    idx = [0, 5, 11, 3]
    boxes = [(10, 100, 20, 130), (3, 99, 5, 101), (20, 68, 100, 148), (30, 120, 60, 150)]
    n = len(idx)
    frames = torch.from_numpy(clip).to(cuda)
    mels = torch.from_numpy(synth.mel_windows(n, seed=3)).to(cuda)
    runner = inference.Wav2LipRunner(model, batch_size=n, blend=BLEND)
    assert runner.blend == BLEND
    got = runner.run_frames(frames, idx, boxes, mel_windows=mels).cpu().numpy()
    faces = torch.empty((n, 96, 96, 3), dtype=torch.uint8, device=cuda)
    # both tables stay alive in names until the launch has run: a temporary's block goes back to the allocator at once
    idx_dev = torch.tensor(idx, dtype=torch.int32, device=cuda)
    boxes_dev = torch.tensor(boxes, dtype=torch.int32, device=cuda)
    check(_lib.load().w2l_crop_resize_u8(current_stream(), n, ptr(frames), 120, 150, ptr(idx_dev), ptr(boxes_dev), 96, ptr(faces)), "crop")
    torch.cuda.synchronize()
    pred = runner.run_batch(faces, mel_windows=mels).cpu().numpy()
    plain = inference.Wav2LipRunner(model, batch_size=n).run_frames(frames, idx, boxes, mel_windows=mels).cpu().numpy()
    assert got.shape == plain.shape == (n, 120, 150, 3)
    for k in range(n):
        want = BC.blend_model(clip[idx[k]], pred[k], boxes[k], F, T)
        assert np.array_equal(got[k], want), BC.FC.diff_message("run_frames row %d box %s" % (k, boxes[k]), got[k], want)
        assert not np.array_equal(got[k], plain[k])
    assert torch.equal(frames.cpu(), torch.from_numpy(clip))                    # the input frames are not written


def test_lipsync_many_blends_every_row_of_two_clips_of_different_shapes(cuda, model):
    from wav2lip_amd import audio, multiclip
    r = np.random.default_rng(32)
    spec = {"a": (list(r.integers(0, 256, (3, 120, 150, 3), dtype=np.uint8)), (10, 100, 20, 130), 4000),
            "b": (list(r.integers(0, 256, (5, 97, 131, 3), dtype=np.uint8)), (1, 96, 5, 60), 5000)}
    rows = {}

    def jobs():
        for i, (k, (frames, box, ns)) in enumerate(spec.items()):
            mel = audio.melspectrogram_device(synth.noise_wav(ns, seed=40 + i), cuda)
            rows[k] = multiclip.rows_inference(mel.shape[1], len(frames), [box] * len(frames))
            yield multiclip.ClipJob(k, frames, mel, rows[k])

    plain = multiclip.lipsync_many(model, jobs(), batch_size=8)
    got = multiclip.lipsync_many(model, jobs(), batch_size=8, blend=BLEND)
    assert [len(rows[k]) for k in spec] == [3, 5]                                # one batch of 8 rows, two frame shapes
    for k, (frames, box, _) in spec.items():
        y1, y2, x1, x2 = box
        assert len(got[k]) == len(plain[k]) == len(rows[k])
        for i, (fi, _, _) in enumerate(rows[k]):
            want = BC.blend_resized(frames[fi], plain[k][i][y1:y2, x1:x2], box, F, T)
            assert np.array_equal(got[k][i], want), BC.FC.diff_message("clip %s row %d" % (k, i), got[k][i], want)
            assert not np.array_equal(got[k][i], plain[k][i])


def test_a_stream_equals_lipsync_on_the_whole_audio(cuda, model, clip):
    """one stream, its audio fed in ragged chunks; its 8 rows leave as one batch of 8, the batch `lipsync` runs: the same plan on
    the same faces and windows, so the frames are the same bytes, and they are the model applied to the default run"""
    from wav2lip_amd import inference, streaming
    frames, box = list(clip[:5]), (10, 100, 20, 130)
    wav = synth.noise_wav(N_SAMPLES, seed=50)
    ref = inference.lipsync(model, frames, wav, batch_size=8, box=box, blend=BLEND)
    plain = inference.lipsync(model, frames, wav, batch_size=8, box=box)
    ls = streaming.LipsyncStreams(model, batch_size=8, blend=BLEND, mel_window=64)
    assert ls.blend == BLEND
    ls.open("s", frames, [box] * len(frames))
    for lo in range(0, N_SAMPLES, 1777):
        ls.feed("s", wav[lo:lo + 1777])
        ls.step()
    ls.close("s")
    got = ls.drain()["s"]
    assert len(got) == len(ref) == len(plain) == 8
    y1, y2, x1, x2 = box
    for i, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(a, b), BC.FC.diff_message("streamed frame %d against lipsync" % i, a, b)
        want = BC.blend_resized(frames[i % len(frames)], plain[i][y1:y2, x1:x2], box, F, T)
        assert np.array_equal(b, want), BC.FC.diff_message("lipsync frame %d against the model" % i, b, want)


def test_lipsync_with_a_blend_takes_the_device_paste_for_a_96x96_box(cuda, model, clip):
    """a 96x96 box goes through the host paste by default; with a blend it takes the device branch, and the result is the model
    applied to the default run's output"""
    from wav2lip_amd import inference
    frames, box = list(clip[:3]), (12, 108, 30, 126)
    wav = synth.noise_wav(N_SAMPLES, seed=51)
    plain = inference.lipsync(model, frames, wav, batch_size=8, box=box)
    got = inference.lipsync(model, frames, wav, batch_size=8, box=box, blend=BLEND)
    assert len(got) == len(plain) == 8
    for i in range(8):
        want = BC.blend_resized(frames[i % 3], plain[i][12:108, 30:126], box, F, T)
        assert np.array_equal(got[i], want), BC.FC.diff_message("frame %d" % i, got[i], want)


def test_the_command_line_switch(cuda, tmp_path):
    """`--blend_feather 4 --blend_top 0.5` with a `--box`: against the default run the frames differ inside the box and are
    byte-equal outside it; in the box rows above t0 they are the INPUT frame (the default run has generated pixels there); all of
    it is the model applied to the default run's box"""
    from PIL import Image
    from scipy.io import wavfile
    from wav2lip_amd import inference
    tmp = str(tmp_path)
    face = np.random.default_rng(33).integers(0, 256, (120, 150, 3), dtype=np.uint8)
    Image.fromarray(np.ascontiguousarray(face[:, :, ::-1])).save(os.path.join(tmp, "face.png"))
    wav = synth.noise_wav(N_SAMPLES, seed=52) * np.float32(0.5)
    wavfile.write(os.path.join(tmp, "audio.wav"), 16000, np.clip(np.round(wav * 32768.0), -32768, 32767).astype(np.int16))
    torch.save({"state_dict": {"module." + k: v for k, v in _state_dict().items()}, "optimizer": None, "global_step": 7, "global_epoch": 1},
               os.path.join(tmp, "ckpt.pth"))
    box = (10, 100, 20, 130)
    common = ["--checkpoint_path", os.path.join(tmp, "ckpt.pth"), "--face", os.path.join(tmp, "face.png"), "--audio",
              os.path.join(tmp, "audio.wav"), "--box"] + [str(v) for v in box] + ["--wav2lip_batch_size", "8"]
    plain = np.stack(inference.main(common + ["--outfile", os.path.join(tmp, "a.avi")]))
    got = np.stack(inference.main(common + ["--outfile", os.path.join(tmp, "b.avi"), "--blend_feather", "4", "--blend_top", "0.5"]))
    assert (inference.args.blend_feather, inference.args.blend_top) == (4, 0.5)
    assert got.shape == plain.shape == (8, 120, 150, 3)
    y1, y2, x1, x2 = box
    t0 = ((y2 - y1) * 128) >> 8
    assert t0 == 45
    for i in range(len(got)):
        assert not np.array_equal(got[i][y1:y2, x1:x2], plain[i][y1:y2, x1:x2])
        outside_got, outside_plain = got[i].copy(), plain[i].copy()
        outside_got[y1:y2, x1:x2] = 0
        outside_plain[y1:y2, x1:x2] = 0
        assert np.array_equal(outside_got, outside_plain)
        assert np.array_equal(got[i][y1:y1 + t0, x1:x2], face[y1:y1 + t0, x1:x2])
        assert not np.array_equal(plain[i][y1:y1 + t0, x1:x2], face[y1:y1 + t0, x1:x2])
        want = BC.blend_resized(face, plain[i][y1:y2, x1:x2], box, 4, 128)
        assert np.array_equal(got[i], want), BC.FC.diff_message("frame %d" % i, got[i], want)
    from wav2lip_amd import container
    back = container.read_avi(os.path.join(tmp, "b.avi"))["frames"]
    assert np.array_equal(np.stack(list(back)), got)                             # what was written is what was returned
