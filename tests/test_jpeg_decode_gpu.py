"""w2l_jpeg_decode_rows (csrc/jpeg_decode.hip) and what is built on it, on the device.  Every expectation is the image PIL decodes
from the same bytes (`np.asarray(Image.open(BytesIO(d)).convert("RGB"))[:, :, ::-1]`), byte for byte.  Output images sit between
guard bytes at every byte alignment, the files' bytes lie at odd addresses, and the corrupt corpus of tests/_jpeg_decode_cases.py
(which has passed the host build of tools/jpeg_decode_host.cpp under the host sanitizers) shares its launch with valid files."""
import ctypes as C

import numpy as np
import pytest
import torch

import _jpeg_cases as jc
import _jpeg_decode_cases as dc

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


def parsed(d):
    from wav2lip_amd import _lib
    lib = _lib.load()
    info = _lib.JpegInfo()
    rc = lib.w2l_jpeg_parse(bytes(d), len(d), C.byref(info))
    return (info if rc == 0 else None), rc


def launch(cuda, items):
    """One w2l_jpeg_decode_rows launch.  items: [(file bytes, _lib.JpegInfo describing them)].  The entropy segments lie at odd
    addresses, the images between guard bytes at every byte alignment.  Returns (status int32 [n], [image uint8 [H,W,3] numpy],
    number of table sets); asserts that no byte outside the images was written."""
    from wav2lip_amd import _lib, jpeg
    lib = _lib.load()
    n = len(items)
    tb = int(lib.w2l_jpeg_table_bytes())
    sets, table = {}, np.zeros(n, jpeg.JPEG_ROW)
    src_offs, dst_offs = [], []
    soff, doff, max_blocks = 1, GUARD, 1
    for r, (d, info) in enumerate(items):
        key = C.string_at(C.addressof(info) + 20, C.sizeof(_lib.JpegInfo) - 20)
        if key not in sets:
            buf = (C.c_uint8 * tb)()
            assert lib.w2l_jpeg_build_tables(C.byref(info), buf) == 0, lib.w2l_last_error()
            sets[key] = (len(sets), bytes(buf))
        nbytes = max(0, min(info.ecs_bytes, len(d) - info.ecs_offset))
        table[r] = (0, 0, nbytes, info.H, info.W, sets[key][0])
        max_blocks = max(max_blocks, jpeg.blocks(info.H, info.W))
        soff += (soff + 1) % 2                                   # odd
        src_offs.append(soff)
        soff += nbytes
        dst_offs.append(doff)
        doff += info.H * info.W * 3 + GUARD + r % 3              # images at every byte alignment
    host = np.zeros(soff + 16, np.uint8)
    for r, (d, info) in enumerate(items):
        nb = int(table["nbytes"][r])
        host[src_offs[r]:src_offs[r] + nb] = np.frombuffer(d, np.uint8, nb, info.ecs_offset) if nb else 0
    streams = torch.from_numpy(host).to(cuda)
    out = torch.full((doff,), FILL, dtype=torch.uint8, device=cuda)
    assert streams.data_ptr() % 16 == 0
    table["src"] = streams.data_ptr() + np.array(src_offs, dtype=np.int64)
    table["dst"] = out.data_ptr() + np.array(dst_offs, dtype=np.int64)
    tdev = torch.from_numpy(table.view(np.uint8).copy()).to(cuda)
    blob = b"".join(b for _, b in sorted(sets.values()))
    tabs = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(cuda)
    status = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    ws_bytes = int(lib.w2l_jpeg_decode_workspace_bytes(n, max_blocks))
    assert ws_bytes > 0
    ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device=cuda)
    rc = lib.w2l_jpeg_decode_rows(_lib.current_stream(), n, _lib.ptr(tdev), _lib.ptr(tabs), len(sets), max_blocks, _lib.ptr(status),
                                  _lib.ptr(ws), ws_bytes)
    assert rc == 0, lib.w2l_last_error()
    torch.cuda.synchronize()
    st, buf = status.cpu().numpy(), out.cpu().numpy()
    inside = np.zeros(doff, bool)
    imgs = []
    for r, (_, info) in enumerate(items):
        sz = info.H * info.W * 3
        inside[dst_offs[r]:dst_offs[r] + sz] = True
        imgs.append(buf[dst_offs[r]:dst_offs[r] + sz].reshape(info.H, info.W, 3))
    assert (buf[~inside] == FILL).all(), "bytes outside the images were written"
    return st, imgs, len(sets)


def valid_items(names=None):
    out = []
    for name, d in dc.files():
        if names is None or names(name):
            info, rc = parsed(d)
            assert rc == 0, name
            out.append((name, d, info))
    return out


def check_valid(part, st, imgs):
    for (name, d, _), s, img in zip(part, st, imgs):
        assert s == 0, (name, s)
        assert np.array_equal(img, dc.expected(name, d)), name


# ---------------------------------------------------------------- 1. the files, one launch
def test_every_file_equals_pil_in_one_launch(cuda):
    subset = {"%s_%dx%d_q%d" % (c, h, w, q) for (h, w) in jc.SUBSET for c in jc.CONTENTS for q in (30, 75, 95, 100)}
    subset |= {"%s_%dx%d_q95" % (c, h, w) for (h, w) in ((96, 96), (160, 160)) for c in jc.CONTENTS}
    subset |= {"%s_%dx%d_q95" % (c, h, w) for (h, w) in dc.NARROW for c in ("noise", "redblue")}   # 1 to 4 columns: plain upsampling
    part = valid_items(lambda n: n[:-4] in subset)
    assert len(part) == 2 * (len(jc.SUBSET) * 5 * 4 + 2 * 5 + 2 * len(dc.NARROW))            # both table kinds
    st, imgs, nsets = launch(cuda, [(d, info) for _, d, info in part])
    assert nsets >= 3
    check_valid(part, st, imgs)


# ---------------------------------------------------------------- 2. one file, two rows
def test_two_rows_that_name_one_file_give_the_same_image(cuda):
    part = valid_items(lambda n: n in ("noise_81x107_q95_opt", "checker_37x53_q95_std"))
    part = [part[0], part[1], part[0], part[1], part[0]]
    st, imgs, nsets = launch(cuda, [(d, info) for _, d, info in part])
    check_valid(part, st, imgs)
    assert nsets == 2 and np.array_equal(imgs[0], imgs[2]) and np.array_equal(imgs[0], imgs[4]) and np.array_equal(imgs[1], imgs[3])


# ---------------------------------------------------------------- 3. batch sizes
def test_batch_sizes(cuda):
    one = valid_items(lambda n: n == "noise_17x15_q95_std")
    st, imgs, _ = launch(cuda, [(d, info) for _, d, info in one])
    check_valid(one, st, imgs)
    small = valid_items(lambda n: any(("_%dx%d_q95" % s) in n for s in ((1, 1), (3, 5), (7, 9), (16, 16), (17, 15), (24, 8), (33, 16))))
    part = (small * 2)[:129]                                             # one file above a multiple of 64: a wave with one lane
    assert len(part) == 129
    st, imgs, _ = launch(cuda, [(d, info) for _, d, info in part])
    check_valid(part, st, imgs)


# ---------------------------------------------------------------- 4. the round trip
def test_files_of_the_device_encoder_decode_to_pils_image(cuda):
    """`preprocess --jpeg device`, then training with decode="device": what the encoder wrote is decoded to what PIL decodes"""
    from wav2lip_amd import jpeg
    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, (3, 120, 150, 3), dtype=np.uint8)
    frames[1] = jc.image("gradient", 120, 150)
    boxes = [(3, 4, 99, 100), (0, 0, 150, 120), (40, 20, 131, 117)]
    files = jpeg.encode_crops(torch.from_numpy(frames).to(cuda), boxes)
    imgs = jpeg.decode_files(files, cuda)
    for d, (x1, y1, x2, y2), img in zip(files, boxes, imgs):
        assert tuple(img.shape) == (y2 - y1, x2 - x1, 3) and img.dtype == torch.uint8 and img.is_cuda
        assert np.array_equal(img.cpu().numpy(), dc.pil_decode(d))


# ---------------------------------------------------------------- 5. the corrupt corpus
def test_corrupt_rows_report_a_negative_status_and_their_neighbours_decode(cuda):
    """a corrupt file is described by the library's own parser where that accepts it (a file without EOI runs to its last byte),
    else by its source's description with the byte count cut to what is left; valid files sit between the corrupt ones"""
    valid = valid_items(lambda n: n in ("noise_37x53_q95_std", "gradient_81x107_q75_opt", "noise_96x96_q95_opt", "redblue_24x8_q30_std"))
    items, kinds = [], []
    planted = []
    for k, (name, c, src) in enumerate(dc.corrupt_corpus()):
        info, rc = parsed(c)
        if info is None:
            info, rc = parsed(src)
            assert rc == 0
        items.append((c, info))
        kinds.append(name)
        if name.endswith("_eoi_planted"):                                # the marker inside the segment the source describes
            planted.append((c, parsed(src)[0]))
        v = valid[k % len(valid)]
        items.append((v[1], v[2]))
        kinds.append(None)
    items += planted
    kinds += ["planted, source's byte count"] * len(planted)
    st, imgs, _ = launch(cuda, items)
    reasons = set()
    for k, (kind, s) in enumerate(zip(kinds, st)):
        if kind is None:
            v = valid[(k // 2) % len(valid)]
            assert s == 0 and np.array_equal(imgs[k], dc.expected(v[0], v[1])), (k, s)
        else:
            assert -5 <= s < 0, (kind, s)
            reasons.add(int(s))
    assert {-1, -2, -3, -4} <= reasons                                   # every reason of the entropy routine is met
    assert [int(s) for k, s in zip(kinds, st) if k == "planted, source's byte count"] == [-3] * 3


def test_overwrites_that_stay_decodable_give_the_references_pixels(cuda):
    """the single-byte overwrites passed over when the corpus was drawn: no decoder can refuse them, so the row reports 0 and
    the image is the strict restatement's"""
    alt = dc.altered_files()
    items = []
    for name, c, _ in alt:
        info, rc = parsed(c)
        assert rc == 0, name
        items.append((c, info))
    st, imgs, _ = launch(cuda, items)
    for (name, _, want), s, img in zip(alt, st, imgs):
        assert s == 0 and np.array_equal(img, want), (name, s)


# ---------------------------------------------------------------- 6. the public interface
def test_decode_files_and_probe(cuda):
    from wav2lip_amd import jpeg
    part = valid_items(lambda n: n in ("noise_81x107_q95_std", "noise_81x107_q95_opt", "flat_1x1_q95_std", "checker_96x96_q95_std"))
    imgs = jpeg.decode_files([d for _, d, _ in part], cuda)
    base = imgs[0].untyped_storage().data_ptr()
    for (name, d, _), img in zip(part, imgs):
        assert np.array_equal(img.cpu().numpy(), dc.expected(name, d)), name
        assert img.untyped_storage().data_ptr() == base                  # views of one buffer
        assert jpeg.probe(d) == dc.expected(name, d).shape[:2]
    corpus = dict((n, c) for n, c, _ in dc.corrupt_corpus())
    bad = corpus["noise_37x53_q95_std_cut50"]
    with pytest.raises(ValueError, match="file 1 is corrupt") as e:
        jpeg.decode_files([part[0][1], bad, part[1][1]], cuda)
    assert not isinstance(e.value, jpeg.UnsupportedJpeg)
    with pytest.raises(ValueError, match="file 0"):
        jpeg.decode_files([corpus["noise_37x53_q95_std_sparse_ac"]], cuda)
    prog = dc.pil_file(jc.image("noise", 40, 40), 95, progressive=True)
    with pytest.raises(jpeg.UnsupportedJpeg, match="progressive"):
        jpeg.probe(prog)
    with pytest.raises(jpeg.UnsupportedJpeg, match="file 1"):
        jpeg.decode_files([part[0][1], prog], cuda)
    with pytest.raises(RuntimeError):
        jpeg.decode_files([part[0][1]], "cpu")


# ---------------------------------------------------------------- 7. refused arguments
def test_bad_arguments_are_refused_and_nothing_is_written(cuda):
    from wav2lip_amd import _lib, jpeg
    lib = _lib.load()
    (name, d, info), = valid_items(lambda n: n == "noise_16x16_q95_std")
    tb = int(lib.w2l_jpeg_table_bytes())
    buf = (C.c_uint8 * tb)()
    assert lib.w2l_jpeg_build_tables(C.byref(info), buf) == 0
    tabs = torch.zeros(tb + 16, dtype=torch.uint8, device=cuda)
    tabs[:tb] = torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(cuda)
    tabs_shifted = torch.zeros(tb + 16, dtype=torch.uint8, device=cuda)
    tabs_shifted[8:8 + tb] = tabs[:tb]
    ecs = torch.from_numpy(np.frombuffer(d, np.uint8, info.ecs_bytes, info.ecs_offset).copy()).to(cuda)
    out = torch.full((2 * 16 * 16 * 3,), FILL, dtype=torch.uint8, device=cuda)
    table = np.zeros(2, jpeg.JPEG_ROW)
    table["src"], table["nbytes"], table["H"], table["W"] = ecs.data_ptr(), info.ecs_bytes, 16, 16
    table["dst"] = out.data_ptr() + np.arange(2) * 768
    tdev = torch.from_numpy(table.view(np.uint8).copy()).to(cuda)
    shifted = torch.zeros(2 * 32 + 16, dtype=torch.uint8, device=cuda)
    shifted[8:8 + 64] = tdev
    status = torch.full((2,), 7, dtype=torch.int32, device=cuda)
    nbytes = int(lib.w2l_jpeg_decode_workspace_bytes(2, 6))
    assert nbytes == 2 * 6 * 192
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device=cuda)
    s, p = _lib.current_stream(), _lib.ptr
    good = dict(B=2, rows=p(tdev), tabs=p(tabs), nt=1, mb=6, status=p(status), ws=p(ws), wsb=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        return lib.w2l_jpeg_decode_rows(s, a["B"], a["rows"], a["tabs"], a["nt"], a["mb"], a["status"], a["ws"], a["wsb"])
    bad = dict(null_rows=dict(rows=None), null_tabs=dict(tabs=None), null_status=dict(status=None), null_ws=dict(ws=None),
               b0=dict(B=0), b_negative=dict(B=-1), b_large=dict(B=65536), misaligned_rows=dict(rows=p(shifted[8:])),
               misaligned_tabs=dict(tabs=p(tabs_shifted[8:])), nt0=dict(nt=0), nt_large=dict(nt=65536), mb0=dict(mb=0),
               mb_huge=dict(mb=(1 << 20) + 1), small_ws=dict(wsb=nbytes - 1), no_ws=dict(wsb=0),
               misaligned_ws=dict(ws=C.c_void_p(ws.data_ptr() + 8)))
    for what, kw in bad.items():
        assert call(**kw) != 0, what
        assert lib.w2l_last_error(), what
    torch.cuda.synchronize()
    assert (out == FILL).all() and (status == 7).all()
    assert lib.w2l_jpeg_decode_workspace_bytes(0, 6) == 0 and lib.w2l_jpeg_decode_workspace_bytes(2, 0) == 0
    assert lib.w2l_jpeg_decode_workspace_bytes(65536, 6) == 0 and lib.w2l_jpeg_decode_workspace_bytes(2, (1 << 20) + 1) == 0
    assert call() == 0                                                    # and the same call, well formed
    torch.cuda.synchronize()
    want = dc.expected(name, d)
    assert status.tolist() == [0, 0]
    assert np.array_equal(out.cpu().numpy().reshape(2, 16, 16, 3), np.stack([want, want]))
    # rows the launch cannot take are flagged, not decoded: more blocks than max_blocks; a table index outside the launch; no bytes
    out.fill_(FILL)
    assert call(mb=5) == 0
    torch.cuda.synchronize()
    assert status.tolist() == [-5, -5] and (out == FILL).all()
    for field, value in (("table", 1), ("table", -1), ("nbytes", 0), ("H", 0), ("W", 65536)):
        t2 = table.copy()
        t2[field][1] = value
        t2dev = torch.from_numpy(t2.view(np.uint8).copy()).to(cuda)
        out.fill_(FILL)
        assert call(rows=p(t2dev)) == 0
        torch.cuda.synchronize()
        assert status.tolist() == [0, -5], field
        assert np.array_equal(out[:768].cpu().numpy().reshape(16, 16, 3), want) and (out[768:] == FILL).all()
