"""w2l_jpeg_encode_rows (csrc/jpeg.hip) and what is built on it, on the device.  Every expectation is the bytes PIL writes for the
same crop (`Image.save(format="JPEG", quality=q, subsampling=2)`, what `preprocess._write_jpeg` calls): whole files, header
included.  Output slots sit between guard bytes, frames lie at odd addresses, and boxes are chosen so that a kernel that padded
with frame pixels from outside the box would write other bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _jpeg_cases as jc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def launch(cuda, items, q, caps=None):
    """One w2l_jpeg_encode_rows launch.  items: [(frame uint8 [H,W,3] BGR numpy, byte misalignment of its base, (x1, y1, x2, y2))];
    a frame object named twice (at one misalignment) is stored once.  caps: {row: capacity} overrides jpeg.capacity.  Returns
    (lengths int32 [n], [file bytes or None], whole output buffer uint8 numpy, boolean mask of the bytes inside slots)."""
    from wav2lip_amd import _lib, jpeg
    from wav2lip_amd.multiclip import FRAME_ROW
    lib = _lib.load()
    n = len(items)
    place, off = {}, 0
    for f, mis, _ in items:
        if (id(f), mis) not in place:
            off = -(-off // 16) * 16 + mis
            place[(id(f), mis)] = off
            off += f.size
    host = np.zeros(off + 16, np.uint8)
    for f, mis, _ in items:
        o = place[(id(f), mis)]
        host[o:o + f.size] = f.reshape(-1)
    frames = torch.from_numpy(host).to(cuda)
    assert frames.data_ptr() % 16 == 0
    table = np.zeros(n, FRAME_ROW)
    cap = np.zeros(n, np.int32)
    offs, off, max_blocks = [], GUARD, 0
    for r, (f, mis, (x1, y1, x2, y2)) in enumerate(items):
        assert 0 <= y1 < y2 <= f.shape[0] and 0 <= x1 < x2 <= f.shape[1]
        cap[r] = jpeg.capacity(y2 - y1, x2 - x1) if caps is None or r not in caps else caps[r]
        max_blocks = max(max_blocks, jpeg.blocks(y2 - y1, x2 - x1))
        table[r] = (frames.data_ptr() + place[(id(f), mis)], 0, f.shape[0], f.shape[1], y1, y2, x1, x2, (0, 0))
        offs.append(off)
        off += int(cap[r]) + GUARD + r % 3                   # slots at every byte alignment
    out = torch.full((off,), FILL, dtype=torch.uint8, device=cuda)
    table["dst"] = out.data_ptr() + np.array(offs, dtype=np.int64)
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).to(cuda)
    cap_dev = torch.from_numpy(cap).to(cuda)
    lengths = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    ws_bytes = int(lib.w2l_jpeg_workspace_bytes(n, max_blocks))
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device=cuda)
    rc = lib.w2l_jpeg_encode_rows(_lib.current_stream(), n, _lib.ptr(table_dev), _lib.ptr(cap_dev), q, max_blocks, _lib.ptr(lengths),
                                  _lib.ptr(ws), ws_bytes)
    assert rc == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    got, buf = lengths.cpu().numpy(), out.cpu().numpy()
    inside = np.zeros(off, bool)
    files = []
    for r in range(n):
        inside[offs[r]:offs[r] + cap[r]] = True
        files.append(None if got[r] < 0 else buf[offs[r]:offs[r] + got[r]].tobytes())
    assert (buf[~inside] == FILL).all(), "bytes outside the slots were written"
    return got, files, buf, inside


def whole(img):
    return (0, 0, img.shape[1], img.shape[0])


def crop_bytes(f, box, q=95):
    x1, y1, x2, y2 = box
    return jc.pil_bytes(f[y1:y2, x1:x2], q)


# ---------------------------------------------------------------- 1. all cases
def test_every_case_equals_pil_in_one_launch_per_quality(cuda):
    by_q = {}
    for name, img, q in jc.cases():
        by_q.setdefault(q, []).append((name, img))
    assert sorted(by_q) == [30, 75, 95, 100]
    for q, part in by_q.items():
        got, files, _, _ = launch(cuda, [(img, i % 4, whole(img)) for i, (_, img) in enumerate(part)], q)
        for (name, img), n, data in zip(part, got, files):
            want = jc.expected(name, img, q)
            assert n == len(want) and data == want, name


# ---------------------------------------------------------------- 2. crops inside frames
def test_crops_inside_larger_frames_at_odd_addresses(cuda):
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    items = [(a, 1, (3, 5, 40, 42)),            # odd x1, frame base + 1
             (a, 1, whole(a)),                  # a box equal to the frame, the same frame again
             (a, 2, (77, 13, 78, 14)),          # 1x1
             (a, 3, (100, 60, 131, 97)),        # touches the right and bottom edges
             (a, 1, (0, 0, 131, 97)),
             (a, 1, (9, 7, 9 + 24, 7 + 8)),     # H = 8: the chroma plane's rows are repeated after downsampling
             (a, 1, (51, 33, 51 + 21, 33 + 19)),   # padding of 11 columns and 13 rows: noise outside the box differs from the edge
             (b, 0, (1, 1, 50, 40)),            # a second frame shape in the launch
             (b, 3, (7, 0, 56, 9)),
             (b, 3, (7, 0, 56, 9))]             # the same crop twice
    got, files, _, _ = launch(cuda, items, 95)
    for (f, _, box), n, data in zip(items, got, files):
        want = crop_bytes(f, box)
        assert n == len(want) and data == want, box
    # the boxes above are ones where looking outside the box would show: the frame's pixels there differ from the replicated edge
    f, _, (x1, y1, x2, y2) = items[6]
    assert (f[y1:y2, x2] != f[y1:y2, x2 - 1]).any() and (f[y2, x1:x2] != f[y2 - 1, x1:x2]).any()


# ---------------------------------------------------------------- 3. batch sizes
def test_batch_sizes(cuda):
    rng = np.random.default_rng(12)
    f = rng.integers(0, 256, (64, 80, 3), dtype=np.uint8)
    got, files, _, _ = launch(cuda, [(f, 0, (5, 6, 38, 31))], 95)
    assert files == [crop_bytes(f, (5, 6, 38, 31))] and got[0] == len(files[0])
    items = []
    for i in range(65):
        x1, y1 = int(rng.integers(0, 60)), int(rng.integers(0, 50))
        items.append((f, 0, (x1, y1, int(rng.integers(x1 + 1, 81)), int(rng.integers(y1 + 1, 65)))))
    got, files, _, _ = launch(cuda, items, 95)
    assert files == [crop_bytes(f, box) for _, _, box in items]
    big = jc.image("noise", 160, 160)
    got, files, _, _ = launch(cuda, [(big, 0, whole(big)), (big, 0, (159, 159, 160, 160)), (big, 0, whole(big))], 95)
    assert files == [jc.pil_bytes(big), crop_bytes(big, (159, 159, 160, 160)), jc.pil_bytes(big)]


# ---------------------------------------------------------------- 4. run to run
def test_two_runs_write_the_same_bytes(cuda):
    imgs = [jc.image(c, h, w) for c in ("noise", "checker") for (h, w) in ((160, 160), (49, 63), (17, 15))]
    items = [(img, i % 4, whole(img)) for i, img in enumerate(imgs)]
    a = launch(cuda, items, 95)
    b = launch(cuda, items, 95)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and None not in a[1]


# ---------------------------------------------------------------- 5. the capacity guard
def test_a_slot_one_byte_short_is_flagged_and_its_neighbours_are_intact(cuda):
    imgs = [jc.image("noise", h, w) for (h, w) in ((37, 53), (40, 40), (16, 33), (1, 1))]
    items = [(img, 0, whole(img)) for img in imgs]
    want = [jc.pil_bytes(img) for img in imgs]
    got, files, buf, inside = launch(cuda, items, 95, caps={1: len(want[1]) - 1, 3: len(want[3]) - 1})
    assert got.tolist() == [len(want[0]), -1, len(want[2]), -1]
    assert files[0] == want[0] and files[2] == want[2]
    # a slot that fits exactly is written
    got, files, _, _ = launch(cuda, items, 95, caps={1: len(want[1]), 3: len(want[3])})
    assert files == want
    # a capacity below the header's size, zero and negative ones
    got, files, buf, inside = launch(cuda, items, 95, caps={0: 0, 1: 624, 3: 1})
    assert got.tolist() == [-1, -1, len(want[2]), -1] and files[2] == want[2]


# ---------------------------------------------------------------- 6. refused arguments
def test_bad_arguments_are_refused_and_nothing_is_written(cuda):
    from wav2lip_amd import _lib, jpeg
    from wav2lip_amd.multiclip import FRAME_ROW
    lib = _lib.load()
    img = torch.from_numpy(jc.image("noise", 16, 16)).to(cuda)
    out = torch.full((2 * jpeg.capacity(16, 16),), FILL, dtype=torch.uint8, device=cuda)
    table = np.zeros(2, FRAME_ROW)
    table["src"], table["H"], table["W"], table["y2"], table["x2"] = img.data_ptr(), 16, 16, 16, 16
    table["dst"] = out.data_ptr() + np.arange(2) * jpeg.capacity(16, 16)
    tdev = torch.from_numpy(table.view(np.uint8).copy()).to(cuda)
    shifted = torch.zeros(2 * 48 + 16, dtype=torch.uint8, device=cuda)
    shifted[8:8 + 96] = tdev                               # the same table, 8 bytes off
    assert tdev.data_ptr() % 16 == 0 and shifted[8:].data_ptr() % 16 == 8
    cap = torch.full((2,), jpeg.capacity(16, 16), dtype=torch.int32, device=cuda)
    lengths = torch.full((2,), -7, dtype=torch.int32, device=cuda)
    nbytes = int(lib.w2l_jpeg_workspace_bytes(2, 6))
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device=cuda)
    s, p = _lib.current_stream(), _lib.ptr
    good = dict(B=2, rows=p(tdev), cap=p(cap), q=95, mb=6, lengths=p(lengths), ws=p(ws), wsb=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        return lib.w2l_jpeg_encode_rows(s, a["B"], a["rows"], a["cap"], a["q"], a["mb"], a["lengths"], a["ws"], a["wsb"])
    bad = dict(null_rows=dict(rows=None), null_cap=dict(cap=None), null_lengths=dict(lengths=None), null_ws=dict(ws=None),
               b0=dict(B=0), b_negative=dict(B=-1), b_large=dict(B=65536), misaligned_table=dict(rows=p(shifted[8:])),
               q0=dict(q=0), q101=dict(q=101), q_negative=dict(q=-5), small_ws=dict(wsb=nbytes - 1), no_ws=dict(wsb=0),
               misaligned_ws=dict(ws=C.c_void_p(ws.data_ptr() + 8)), mb0=dict(mb=0), mb_huge=dict(mb=(1 << 20) + 1))
    for name, kw in bad.items():
        assert call(**kw) != 0, name
        assert lib.w2l_last_error(), name
    torch.cuda.synchronize()
    assert (out == FILL).all() and (lengths == -7).all()
    assert lib.w2l_jpeg_workspace_bytes(0, 6) == 0 and lib.w2l_jpeg_workspace_bytes(2, 0) == 0
    assert call() == 0                                     # and the same call, well formed
    torch.cuda.synchronize()
    want = jc.pil_bytes(jc.image("noise", 16, 16))
    assert lengths.tolist() == [len(want)] * 2
    assert out[:len(want)].cpu().numpy().tobytes() == want
    # a crop with more blocks than max_blocks is flagged, not encoded
    lengths.fill_(-7)
    assert call(mb=5) == 0
    torch.cuda.synchronize()
    assert lengths.tolist() == [-1, -1]


# ---------------------------------------------------------------- 7. the public interface
def test_encode_crops_and_crop_encoder_write_what_write_jpeg_writes(cuda, tmp_path):
    from wav2lip_amd import jpeg, preprocess
    rng = np.random.default_rng(13)
    frames = rng.integers(0, 256, (5, 72, 90, 3), dtype=np.uint8)
    other = rng.integers(0, 256, (33, 47, 3), dtype=np.uint8)
    boxes = [(3, 4, 60, 70), (0, 0, 90, 72), (11, 9, 12, 10), (40, 20, 90, 72), (7, 1, 39, 33)]
    want = []
    for i, (x1, y1, x2, y2) in enumerate(boxes):
        p = str(tmp_path / ("host_%d.jpg" % i))
        preprocess._write_jpeg(p, frames[i][y1:y2, x1:x2])
        want.append(open(p, "rb").read())
    dev = torch.from_numpy(frames).to(cuda)
    assert jpeg.encode_crops(dev, boxes) == want
    assert jpeg.encode_crops(dev, boxes[::-1], frame_index=[4, 3, 2, 1, 0]) == want[::-1]
    # a list of tensors of different shapes, counted through; another quality
    got = jpeg.encode_crops([dev, torch.from_numpy(other).to(cuda)], [(1, 2, 47, 33), boxes[0]], quality=75, frame_index=[5, 0])
    assert got == [jc.pil_bytes(other[2:33, 1:47], 75), jc.pil_bytes(frames[0][4:70, 3:60], 75)]
    for bad in ((0, 0, 91, 72), (5, 5, 5, 9), (-1, 0, 4, 4), (0, 9, 4, 9)):
        with pytest.raises(ValueError):
            jpeg.encode_crops(dev, [bad])
    with pytest.raises(RuntimeError):
        jpeg.encode_crops(torch.from_numpy(frames), boxes)
    enc = jpeg.CropEncoder(preprocess.JPEG_QUALITY, max_batches=1)
    paths = [[str(tmp_path / ("dev_%d_%d.jpg" % (k, i))) for i in range(len(boxes))] for k in range(3)]
    for k in range(3):                                     # three batches: the bound makes `submit` collect the oldest
        enc.submit(dev, boxes, paths[k])
        assert len(enc.jobs) <= 1
    enc.close()
    assert not enc.jobs and not enc.writes
    for k in range(3):
        assert [open(p, "rb").read() for p in paths[k]] == want


# ---------------------------------------------------------------- 8. preprocess --jpeg device
def test_preprocess_with_device_jpeg_writes_the_same_tree(cuda, tmp_path, monkeypatch):
    from wav2lip_amd import container, preprocess
    from wav2lip_amd import synthetic as synth
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    data = str(tmp_path / "data")
    clips = synth.preprocess_clips()[:2]                   # 11 and 5 frames at batch size 4: ragged last batches
    for d, name, frames, pcm, sr in clips:
        os.makedirs(os.path.join(data, d), exist_ok=True)
        container.write_avi(os.path.join(data, d, name + ".avi"), frames, 25, audio=pcm, audio_sr=sr or 16000)

    def tree(mode):
        out = str(tmp_path / mode)
        args = preprocess.main_parser.parse_args(["--data_root", data, "--preprocessed_root", out, "--batch_size", "4", "--jpeg", mode])
        preprocess.main(args, state_dict=synth.s3fd_state_dict())
        names = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
        return {n: open(os.path.join(out, n), "rb").read() for n in names}
    host, dev = tree("host"), tree("device")
    assert sorted(dev) == sorted(host)
    for n in host:
        assert dev[n] == host[n], n
    jpgs = [n for n in host if n.endswith(".jpg")]
    total = sum(len(c[2]) for c in clips)
    assert 0 < len(jpgs) < total                           # faces were found, and a frame without one left a gap
    assert sum(n.endswith("audio.wav") for n in host) == 2
