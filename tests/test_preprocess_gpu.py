"""python -m wav2lip_amd.preprocess on the device against the executed reference (tests/golden/golden_preprocess_v1.npz, written by
make_golden_preprocess.py from the reference's own process_video_file + FaceAlignment on CPU): the same clips as BI_RGB / PCM16
AVIs, the same batch size, the same crops under the same names, the audio tracks, an .mp4 that is reported and skipped, the round
trip into data.ClipStore, the bf16 detector, and two ranks on one GPU."""
import io
import os
import socket
import sys
import wave
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wav2lip_amd import synthetic as synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_preprocess_v1.npz"))


def jpeg_bytes(crop_bgr):
    """PIL's quality-95 4:2:0 encoding (cv2.imwrite's defaults) of a BGR crop"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(crop_bgr[:, :, ::-1])).save(buf, format="JPEG", quality=95, subsampling=2)
    return buf.getvalue()


def write_tree(root):
    """data/<dir>/<clip>.avi for every synthetic clip, plus an .mp4 nothing here can decode"""
    from wav2lip_amd import container
    for d, name, frames, pcm, sr in synth.preprocess_clips():
        os.makedirs(os.path.join(root, d), exist_ok=True)
        container.write_avi(os.path.join(root, d, name + ".avi"), frames, 25, audio=pcm, audio_sr=sr or 16000)
    with open(os.path.join(root, "spk1", "00099.mp4"), "wb") as f:
        f.write(b"\x00\x00\x00\x18ftypmp42" + bytes(64))


def files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def run(data, out, precision="fp32", batch_size=4, backend="nccl"):
    from wav2lip_amd import preprocess
    args = preprocess.parser.parse_args(["--data_root", data, "--preprocessed_root", out, "--batch_size", str(batch_size),
                                         "--face_det_precision", precision])
    preprocess.main(args, state_dict=synth.s3fd_state_dict(), backend=backend)


class Recorder:
    """wraps FaceAlignment.get_detections_for_batch: the rects of every real frame, in call order"""

    def __init__(self, monkeypatch):
        from wav2lip_amd import face_detection
        self.rects = []
        orig = face_detection.FaceAlignment.get_detections_for_batch

        def wrapped(fa, images):
            out = orig(fa, images)
            self.rects.append(out)
            return out
        monkeypatch.setattr(face_detection.FaceAlignment, "get_detections_for_batch", wrapped)


@pytest.fixture(scope="module")
def fp32_run(tmp_path_factory, gold):
    mp = pytest.MonkeyPatch()
    mp.delenv("WORLD_SIZE", raising=False)
    tmp = tmp_path_factory.mktemp("pre")
    data, out = str(tmp / "data"), str(tmp / "out")
    write_tree(data)
    rec = Recorder(mp)
    import contextlib
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        run(data, out, batch_size=int(gold["batch_size"]))
    mp.undo()
    return dict(data=data, out=out, rects=rec.rects, stderr=err.getvalue(), tmp=tmp)


def test_the_written_files_are_the_references(cuda, gold, fp32_run):
    want = sorted(str(p) for p in gold["paths"]) + sorted(os.path.join(d, n, "audio.wav")
                                                          for d, n, _, pcm, _ in synth.preprocess_clips() if pcm is not None)
    assert files_under(fp32_run["out"]) == sorted(want)


def test_every_jpeg_is_the_quality_95_encoding_of_the_reference_crop(cuda, gold, fp32_run):
    frames = {(d, n): fr for d, n, fr, _, _ in synth.preprocess_clips()}
    for p, shape, crc, (x1, y1, x2, y2) in zip(gold["paths"], gold["shapes"], gold["crc32"], gold["rects"]):
        d, n, f = str(p).split("/")
        crop = frames[(d, n)][int(f.split(".")[0])][y1:y2, x1:x2]
        assert crop.shape == tuple(shape) and zlib.crc32(np.ascontiguousarray(crop).tobytes()) == int(crc), p
        with open(os.path.join(fp32_run["out"], str(p)), "rb") as fh:
            assert fh.read() == jpeg_bytes(crop), p


def test_audio_wav_holds_the_tracks_samples_rate_and_channels(cuda, fp32_run):
    for d, n, _, pcm, sr in synth.preprocess_clips():
        p = os.path.join(fp32_run["out"], d, n, "audio.wav")
        if pcm is None:
            assert not os.path.exists(p)
            continue
        with wave.open(p) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (pcm.shape[1], 2, sr)
            got = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, pcm.shape[1])
        assert np.array_equal(got, pcm)


def test_an_mp4_is_reported_and_the_other_clips_complete(cuda, fp32_run):
    assert "00099.mp4" in fp32_run["stderr"] and "Traceback" in fp32_run["stderr"] and "AVI" in fp32_run["stderr"]
    assert not os.path.exists(os.path.join(fp32_run["out"], "spk1", "00099"))


def test_round_trip_into_the_clip_store(cuda, gold, fp32_run):
    """ClipStore.from_directory over the output (a filelist of the 16 kHz clips) = add_clip of the same crops and tracks"""
    from PIL import Image
    from wav2lip_amd import data
    tmp = fp32_run["tmp"]
    lists = tmp / "filelists"
    lists.mkdir(exist_ok=True)
    clips = [(d, n, fr, pcm) for d, n, fr, pcm, sr in synth.preprocess_clips() if pcm is not None and sr == 16000]
    (lists / "train.txt").write_text("".join("%s/%s\n" % (d, n) for d, n, _, _ in clips))
    store = data.ClipStore.from_directory(fp32_run["out"], "train", cuda, filelist_dir=str(lists))
    ref = data.ClipStore(cuda)
    for d, n, fr, pcm in clips:
        ids, crops = [], []
        for p, (x1, y1, x2, y2) in zip(gold["paths"], gold["rects"]):
            if str(p).startswith("%s/%s/" % (d, n)):
                i = int(str(p).split("/")[2].split(".")[0])
                ids.append(i)
                crops.append(np.asarray(Image.open(io.BytesIO(jpeg_bytes(fr[i][y1:y2, x1:x2]))).convert("RGB"))[:, :, ::-1])
        order = np.argsort(ids)
        ref.add_clip([crops[k] for k in order], [ids[k] for k in order], pcm[:, 0].astype(np.float32) / np.float32(32768.0))
    assert store.frame_ids == ref.frame_ids and len(store) == len(clips)
    assert torch.equal(store.frames(), ref.frames())
    assert torch.equal(store.mels._bank(), ref.mels._bank())


def fp32_margins(cuda, batch_size):
    """per frame of the run, in its batch order (sorted clips, padded batches): how far, in logits, the fp32 detector's best box
    leads every box of its table that lies more than 2 px away from it"""
    from wav2lip_amd import face_detection
    fa = face_detection.FaceAlignment(face_detection.LandmarksType._2D, device=cuda, state_dict=synth.s3fd_state_dict())
    out = []
    for _, _, fr, _, _ in sorted(synth.preprocess_clips(), key=lambda c: (c[0], c[1])):
        for lo in range(0, len(fr), batch_size):
            fb = fr[lo:lo + batch_size]
            fb = np.concatenate([fb, np.repeat(fb[-1:], batch_size - len(fb), axis=0)])
            with torch.no_grad():
                t = fa._candidates(fb)[0].double().cpu().numpy()
            for k in range(batch_size):
                s = t[k, :, 4]
                top = int(np.argmax(s))
                far = np.abs(t[k, :, :4] - t[k, top, :4]).max(axis=1) > 2
                logit = lambda p: np.log(p) - np.log1p(-p)        # noqa: E731
                out.append(float(logit(s[top]) - logit(s[far].max())))
    return out


def test_bf16_detector_writes_the_same_frames_with_rects_within_2px(cuda, gold, fp32_run, tmp_path, monkeypatch):
    """The frames with a detection are the same set.  The rects agree within 2 px wherever the fp32 choice is one bf16 rounding
    cannot change: the seeded detector is not a trained one, and on some frames two boxes tens of pixels apart score within a few
    hundredths of a logit of each other (one suppresses the other in NMS), where the reference's argmax itself is a coin toss;
    bf16 moves the winning logit by less than 0.1 on these frames, so a lead of 0.25 is decided."""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    rec = Recorder(monkeypatch)
    run(fp32_run["data"], str(tmp_path / "out"), precision="bf16")
    a = [r for batch in fp32_run["rects"] for r in batch]
    b = [r for batch in rec.rects for r in batch]
    assert len(a) == len(b) > 0
    assert [r is None for r in a] == [r is None for r in b]
    margins = fp32_margins(cuda, int(gold["batch_size"]))
    assert len(margins) == len(a)
    checked = 0
    for ra, rb, m in zip(a, b, margins):
        if ra is not None and m >= 0.25:
            assert max(abs(x - y) for x, y in zip(ra, rb)) <= 2, (ra, rb, m)
            checked += 1
    assert checked >= len([r for r in a if r is not None]) // 2
    names = lambda root: [f for f in files_under(root) if f.endswith(".jpg")]   # noqa: E731
    assert names(str(tmp_path / "out")) == names(fp32_run["out"])


def test_padding_the_ragged_batch_keeps_one_detector_graph(cuda, gold, fp32_run):
    """every detection batch of the run had the full batch size (the clips' ragged tails were padded)"""
    assert {len(batch) for batch in fp32_run["rects"]} == {int(gold["batch_size"])}
    assert len(fp32_run["rects"]) == sum(-(-int(t) // int(gold["batch_size"])) for t in gold["n_frames"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, q, data, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0")
    run(data, out, backend="gloo")
    q.put(rank)


def test_two_ranks_on_one_gpu_write_what_one_process_writes(cuda, fp32_run, tmp_path):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    out = str(tmp_path / "out")
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, fp32_run["data"], out)) for r in range(2)]
    for p in procs:
        p.start()
    assert sorted(q.get(timeout=420) for _ in range(2)) == [0, 1]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert files_under(out) == files_under(fp32_run["out"])
    for f in files_under(out):
        with open(os.path.join(out, f), "rb") as a, open(os.path.join(fp32_run["out"], f), "rb") as b:
            assert a.read() == b.read(), f
