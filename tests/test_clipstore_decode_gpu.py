"""ClipStore.from_directory(decode="device"): the store a directory of `<id>.jpg` crops gives when the files' bytes are decoded on
the device is the store the host path (PIL per file) gives - frames, frame ids, rows and the mel bank - and the files the device
does not decode or refuses are handled as documented."""
import os

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_decode_cases as dc
from wav2lip_amd import synthetic as synth

pytestmark = pytest.mark.gpu

SIZES = [(96, 96), (81, 107), (64, 72), (96, 96), (131, 96)]       # already 96x96, odd, below 96, and one with a single side of 96


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """two clips of 20 frames; the filelists name them for both splits"""
    from scipy.io import wavfile
    tmp = tmp_path_factory.mktemp("clipstore_decode")
    root = tmp / "data"
    (tmp / "filelists").mkdir()
    for split in ("train", "val"):
        (tmp / "filelists" / (split + ".txt")).write_text("spk/00001 extra-column\nspk/00002\n")
    rng = np.random.default_rng(5)
    for ci, vid in enumerate(("spk/00001", "spk/00002")):
        d = root / vid
        d.mkdir(parents=True)
        for i in range(20):
            h, w = SIZES[(i + ci) % len(SIZES)]
            img = jc.image("gradient", h, w) if i % 4 == 3 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            (d / ("%d.jpg" % (i + 3 * ci))).write_bytes(dc.pil_file(img, 95, optimize=bool(i % 2)))
        wavfile.write(str(d / "audio.wav"), 16000, (synth.noise_wav(16000, seed=ci + 1) * 20000).astype(np.int16))
    return tmp, root


def load(tree, cuda, decode, root=None):
    from wav2lip_amd import data
    tmp, r = tree
    return data.ClipStore.from_directory(str(root or r), "train", cuda, filelist_dir=str(tmp / "filelists"), decode=decode)


@pytest.fixture(scope="module")
def host_store(tree, cuda):
    return load(tree, cuda, "host")


def same_mels(a, b):
    assert a.mels.offsets == b.mels.offsets and a.mels.lengths == b.mels.lengths and len(a.mels.lengths) == len(a.names)
    assert torch.equal(a.mels._bank(), b.mels._bank())


def same_stores(a, b):
    assert a.names == b.names and a.frame_ids == b.frame_ids and a.row_of == b.row_of and a.first == b.first and a.n_rows == b.n_rows
    assert a.frames().shape == (40, 96, 96, 3) and torch.equal(a.frames(), b.frames())
    same_mels(a, b)


def test_device_decode_gives_the_store_of_the_host_path(tree, cuda, host_store):
    dev = load(tree, cuda, "device")
    same_stores(dev, host_store)
    assert dev.host_decoded == 0 and host_store.host_decoded == 0
    assert dev.frame_ids[1] == list(range(3, 23))
    # the host path's frames are PIL's pixels: a 96x96 file is stored as decoded
    tmp, root = tree
    want = dc.pil_decode((root / "spk/00001" / "0.jpg").read_bytes())
    assert want.shape == (96, 96, 3) and np.array_equal(dev.frames()[dev.row_of[0][0]].cpu().numpy(), want)
    # and a batch drawn from either store is the same
    picks = [(0, 2, 9), (1, 7, 12)]
    for x, y in zip(dev.generator_batch(picks), host_store.generator_batch(picks)):
        assert torch.equal(x, y)


def test_small_batches_that_span_clips_give_the_same_store(tree, cuda, host_store, monkeypatch):
    from wav2lip_amd import data, jpeg
    monkeypatch.setattr(data.ClipStore, "DEVICE_BATCH_FILES", 7)          # 40 files: batches end inside both clips
    same_stores(load(tree, cuda, "device"), host_store)
    monkeypatch.setattr(data.ClipStore, "DEVICE_BATCH_FILES", 4096)
    monkeypatch.setattr(data.ClipStore, "DEVICE_BATCH_BYTES", 40000)      # the cap by bytes
    same_stores(load(tree, cuda, "device"), host_store)
    monkeypatch.setattr(data.ClipStore, "DEVICE_BATCH_BYTES", 64 << 20)
    monkeypatch.setattr(data.ClipStore, "DEVICE_BATCH_BLOCKS", 500)       # the cap by workspace: 81x107 is 252 blocks, two files at most
    calls = []
    real = jpeg._decode

    def spy(datas, infos, device):
        calls.append((len(datas), max(jpeg.blocks(i.H, i.W) for i in infos)))
        return real(datas, infos, device)
    monkeypatch.setattr(jpeg, "_decode", spy)
    same_stores(load(tree, cuda, "device"), host_store)
    assert sum(n for n, _ in calls) == 40 and len(calls) > 10 and all(n == 1 or n * b <= 500 for n, b in calls)


def copy_tree(tree, tmp_path):
    import shutil
    root = tmp_path / "data"
    shutil.copytree(str(tree[1]), str(root))
    return root


def test_a_progressive_file_goes_through_the_host_alone(tree, cuda, tmp_path):
    root = copy_tree(tree, tmp_path)
    p = root / "spk/00002" / "9.jpg"
    img = dc.pil_decode(p.read_bytes())
    p.write_bytes(dc.pil_file(img, 95, progressive=True))
    dev, host = load(tree, cuda, "device", root), load(tree, cuda, "host", root)
    same_stores(dev, host)
    assert dev.host_decoded == 1 and host.host_decoded == 0


def test_a_truncated_file_raises_value_error_naming_its_path(tree, cuda, tmp_path):
    root = copy_tree(tree, tmp_path)
    p = root / "spk/00001" / "13.jpg"
    d = p.read_bytes()
    p.write_bytes(d[:len(d) * 3 // 4])
    with pytest.raises(ValueError, match="13.jpg") as e:
        load(tree, cuda, "device", root)
    assert str(p) in str(e.value)
    with pytest.raises(OSError):
        load(tree, cuda, "host", root)


def test_add_clip_files_equals_add_clip(tree, cuda):
    from wav2lip_amd import data
    tmp, root = tree
    names = sorted(os.listdir(str(root / "spk/00001")), key=lambda n: (n == "audio.wav", int(n.split(".")[0]) if n != "audio.wav" else 0))[:-1]
    datas = [(root / "spk/00001" / n).read_bytes() for n in names]
    ids = [int(n.split(".")[0]) for n in names]
    wav = synth.noise_wav(16000, seed=3)
    a, b = data.ClipStore(cuda), data.ClipStore(cuda)
    assert a.add_clip_files(datas, ids, wav, name="x") == 0
    assert b.add_clip([dc.pil_decode(d) for d in datas], ids, wav, name="x") == 0
    assert a.names == b.names and a.row_of == b.row_of and torch.equal(a.frames(), b.frames())
    with pytest.raises(ValueError):
        a.add_clip_files(datas, ids[:-1], wav)
    with pytest.raises(ValueError):
        data.ClipStore.from_directory(str(root), "train", cuda, filelist_dir=str(tmp / "filelists"), decode="gpu")


def test_the_environment_variable_reaches_the_loaders(tree, cuda, tmp_path, monkeypatch):
    from wav2lip_amd import trainer
    root = copy_tree(tree, tmp_path)
    monkeypatch.chdir(tree[0])                                            # 'filelists/<split>.txt' relative to the cwd
    prog = root / "spk/00001" / "4.jpg"
    prog.write_bytes(dc.pil_file(dc.pil_decode(prog.read_bytes()), 95, progressive=True))
    monkeypatch.setenv("W2L_JPEG_DECODE", "device")
    tr, va = trainer._loaders(str(root), cuda, 2, "generator")
    assert tr.store.host_decoded == 1 and va.store.host_decoded == 1      # the device path ran: it counted the one file it passed on
    monkeypatch.setenv("W2L_JPEG_DECODE", "host")
    tr_h, _ = trainer._loaders(str(root), cuda, 2, "generator")
    assert tr_h.store.host_decoded == 0
    assert torch.equal(tr.store.frames(), tr_h.store.frames()) and torch.equal(va.store.frames(), tr_h.store.frames())
    monkeypatch.delenv("W2L_JPEG_DECODE")
    assert trainer._loaders(str(root), cuda, 2, "generator")[0].store.host_decoded == 0
    monkeypatch.setenv("W2L_JPEG_DECODE", "fast")
    with pytest.raises(ValueError, match="W2L_JPEG_DECODE"):
        trainer._loaders(str(root), cuda, 2, "generator")
