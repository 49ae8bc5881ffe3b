"""Motion-JPEG without a GPU: the host entry points behind restart intervals (w2l_jpeg_header_rst, w2l_jpeg_parse_rst,
w2l_jpeg_restart_segments) against PIL / libjpeg-turbo's files, the MJPG container (wav2lip_amd/container.py) field by field, and
the segment decoder's arithmetic - jd::decode_mcus, the text the device kernel is compiled from - as a stand-alone host program
under the host sanitizers (tools/jpeg_segments_host.cpp)."""
import ctypes as C
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

import _mjpeg_cases as mc
from conftest import ROOT


def lib():
    from wav2lip_amd import _lib
    return _lib.load()


def parse_rst(d):
    from wav2lip_amd import _lib
    info, ri = _lib.JpegInfo(), C.c_int32(-1)
    rc = lib().w2l_jpeg_parse_rst(d, len(d), C.byref(info), C.byref(ri))
    return rc, info, ri.value


def segments(ecs, ri, n_mcus, cap=None):
    from wav2lip_amd import jpeg
    n = -(-n_mcus // ri) if ri else 1
    out = np.zeros(n if cap is None else cap, jpeg.JPEG_SEGMENT)
    buf = (C.c_uint8 * len(ecs)).from_buffer_copy(ecs)          # exactly the scan's bytes
    return lib().w2l_jpeg_restart_segments(buf, len(ecs), ri, n_mcus, C.c_void_p(out.ctypes.data), len(out)), out


def mcus(h, w):
    return (-(-h // 16)) * (-(-w // 16))


def test_the_stuffed_case_is_in_the_input():
    """a condition on the INPUT: PIL's file of the 330x24 image has an interval that ends in a stuffed FF (FF 00 FF Dn)"""
    assert mc.has_stuffed_interval_end(mc.pil_file(mc.STUFFED, 1, 95))


@pytest.mark.parametrize("shape,rows,quality", mc.cases())
def test_header_rst_equals_pils_first_629_bytes(shape, rows, quality):
    h, w = shape
    d = mc.pil_file(shape, rows, quality)
    buf = (C.c_uint8 * 629)()
    assert lib().w2l_jpeg_header_rst(h, w, quality, rows, buf) == 0
    assert bytes(buf) == d[:629]
    assert d[609:613] == b"\xff\xdd\x00\x04" and d[163:167] == struct.pack(">HH", h, w)
    from wav2lip_amd import jpeg
    assert jpeg.header_rst(h, w, quality, rows) == d[:629] and len(d) <= jpeg.capacity_rst(h, w, rows)


def test_header_rst_and_capacity_refuse_bad_arguments():
    buf = (C.c_uint8 * 629)()
    for h, w, q, r in ((0, 1, 95, 1), (1, 65536, 95, 1), (1, 1, 0, 1), (1, 1, 101, 1), (1, 1, 95, 0)):
        assert lib().w2l_jpeg_header_rst(h, w, q, r, buf) != 0
    assert lib().w2l_jpeg_capacity_rst(16, 16, 0) == 0 and lib().w2l_jpeg_capacity_rst(0, 16, 1) == 0
    # beyond today's bound: 6 header bytes and 4 per interval
    from wav2lip_amd import jpeg
    assert jpeg.capacity_rst(150, 40, 1) == jpeg.capacity(150, 40) + 6 + 4 * 10
    assert jpeg.capacity_rst(150, 40, 2) == jpeg.capacity(150, 40) + 6 + 4 * 5


@pytest.mark.parametrize("shape,rows,quality", mc.cases())
def test_parse_rst_reports_pils_interval_and_parse_still_refuses(shape, rows, quality):
    from wav2lip_amd import _lib, jpeg
    h, w = shape
    d = mc.pil_file(shape, rows, quality)
    rc, info, ri = parse_rst(d)
    assert rc == 0 and ri == rows * (-(-w // 16)) == struct.unpack(">H", d[613:615])[0]
    assert (info.H, info.W, info.ecs_offset, info.eoi) == (h, w, 629, 1) and info.ecs_offset + info.ecs_bytes == len(d) - 2
    assert lib().w2l_jpeg_parse(d, len(d), C.byref(_lib.JpegInfo())) == -105
    with pytest.raises(jpeg.UnsupportedJpeg):
        jpeg.parse(d)
    got, r2 = jpeg.parse_frame(d)
    assert r2 == ri and (got.H, got.W) == (h, w)


def test_parse_rst_on_an_interval_in_blocks_and_on_a_plain_file():
    img = (np.random.RandomState(3).rand(40, 70, 3) * 255).astype(np.uint8)
    d = mc.pil_encode(img, restart_marker_blocks=2)
    rc, info, ri = parse_rst(d)
    assert rc == 0 and ri == 2
    plain = mc.pil_encode(img)
    rc, info2, ri = parse_rst(plain)
    from wav2lip_amd import _lib
    ref = _lib.JpegInfo()
    assert rc == 0 and ri == 0 and lib().w2l_jpeg_parse(plain, len(plain), C.byref(ref)) == 0
    assert bytes(info2) == bytes(ref)                               # the same class, the same record
    prog = io.BytesIO()
    Image.fromarray(img).save(prog, format="JPEG", progressive=True)
    assert parse_rst(prog.getvalue())[0] == -101 and parse_rst(b"\xff\xd8\xff")[0] == -100


@pytest.mark.parametrize("shape,rows,quality", mc.cases() + (((40, 70), "blocks", 95),))
def test_restart_segments_equal_a_python_scan(shape, rows, quality):
    h, w = shape
    d = mc.pil_encode(mc.image(h, w), restart_marker_blocks=2) if rows == "blocks" else mc.pil_file(shape, rows, quality)
    want, start, end = mc.scan_segments(d)
    rc, info, ri = parse_rst(d)
    assert rc == 0 and (info.ecs_offset, info.ecs_bytes) == (start, end - start)
    n, out = segments(d[start:end], ri, mcus(h, w))
    assert n == len(want) == -(-mcus(h, w) // ri)
    assert [(int(s["offset"]), int(s["nbytes"])) for s in out] == want
    assert [int(s["first_mcu"]) for s in out] == [k * ri for k in range(n)]
    assert [int(s["n_mcus"]) for s in out] == [min(ri, mcus(h, w) - k * ri) for k in range(n)]
    assert not out["row"].any() and not out["pad"].any()
    # a smaller table is not overrun, the count still comes back
    n2, out2 = segments(d[start:end], ri, mcus(h, w), cap=max(1, n - 1))
    assert n2 == n and np.array_equal(out2, out[:len(out2)])


def test_restart_segments_without_interval_is_one_segment():
    d = mc.pil_encode(mc.image(17, 33))
    want, start, end = mc.scan_segments(d)
    n, out = segments(d[start:end], 0, mcus(17, 33))
    assert n == 1 and tuple(int(out[0][k]) for k in ("offset", "nbytes", "first_mcu", "n_mcus")) == (0, end - start, 0, 6)
    rst = mc.pil_file((17, 33), 1, 95)
    _, s2, e2 = mc.scan_segments(rst)
    assert segments(rst[s2:e2], 0, mcus(17, 33))[0] == -100            # a marker where no interval was declared


def test_restart_segments_refuses_wrong_markers():
    d = mc.pil_file(*mc.BAD_SOURCE)
    segs, start, end = mc.scan_segments(d)
    ecs, ri, nm = d[start:end], 3, mcus(150, 40)
    assert segments(ecs, ri, nm)[0] == 10
    m = [o + n for o, n in segs[:-1]]                                # where the nine markers stand in the scan
    assert [ecs[i:i + 2] for i in m] == [bytes([0xFF, 0xD0 + k % 8]) for k in range(9)]       # RST7 wraps to RST0
    bad = {
        "deleted": ecs[:m[4]] + ecs[m[4] + 2:],
        "deleted last": ecs[:m[8]] + ecs[m[8] + 2:],
        "duplicated": ecs[:m[4]] + ecs[m[4]:m[4] + 2] + ecs[m[4]:],
        "wrong number": ecs[:m[4] + 1] + bytes([0xD5]) + ecs[m[4] + 2:],
        "cut inside a marker": ecs[:m[8] + 1],
        "cut inside an earlier marker": ecs[:m[2] + 1],
        "one too many": ecs + b"\xff\xd1",
        "another marker": ecs[:m[4] + 1] + bytes([0xC4]) + ecs[m[4] + 2:],
    }
    for name, e in bad.items():
        assert segments(e, ri, nm)[0] == -100 and lib().w2l_last_error().startswith(b"jpeg:"), name
    for args in ((ecs, -1, nm), (ecs, 70000, nm), (ecs, ri, 0)):
        assert segments(*args, cap=1)[0] == -100


# ---------------------------------------------------------------- the container
def avi_fields(path):
    buf = open(path, "rb").read()
    out = {"riff": struct.unpack_from("<I", buf, 4)[0] + 8 == len(buf)}
    i = buf.index(b"avih") + 8
    out["avih"] = struct.unpack_from("<14I", buf, i)
    i = buf.index(b"strh") + 8
    out["strh"] = struct.unpack_from("<4s4sIHHIIIIIIII4h", buf, i)
    i = buf.index(b"strf") + 8
    out["strf"] = struct.unpack_from("<IiiHHIIiiII", buf, i)
    movi = buf.index(b"movi")
    i = buf.index(b"idx1", movi)
    n = struct.unpack_from("<I", buf, i + 4)[0] // 16
    out["idx1"] = [struct.unpack_from("<4sIII", buf, i + 8 + 16 * k) for k in range(n)]
    # an idx1 offset counts from the 'movi' fourcc to the chunk's own header
    out["chunks"] = [buf[movi + off + 8:movi + off + 8 + size] for cc, _, off, size in out["idx1"] if cc == b"00dc"]
    out["tags"] = [buf[movi + off:movi + off + 8] for _, _, off, _ in out["idx1"]]
    return out


def test_mjpg_container_host_path_field_by_field(tmp_path):
    from wav2lip_amd import container
    r = np.random.RandomState(5)
    frames = (r.rand(5, 50, 70, 3) * 255).astype(np.uint8)
    pcm = (r.rand(3200, 1) * 2000).astype(np.int16)
    path = str(tmp_path / "m.avi")
    container.write_avi(path, frames, 25, audio=pcm, audio_sr=16000, codec="mjpg", quality=90, restart_rows=2)
    f = avi_fields(path)
    want = [mc.pil_encode(fr, 90, restart_marker_rows=2) for fr in frames]
    assert f["chunks"] == want and f["riff"]
    big, total = max(map(len, want)), sum(map(len, want))
    assert f["strh"][0] == b"vids" and f["strh"][1] == b"MJPG" and f["strh"][6:8] == (1000, 25000) and f["strh"][9] == 5
    assert f["strh"][10] == big and f["strh"][-2:] == (70, 50)
    assert f["strf"][:7] == (40, 70, 50, 1, 24, struct.unpack("<I", b"MJPG")[0], big)
    assert f["avih"][0] == 40000 and f["avih"][1] == total * 25000 // (1000 * 5) + 32000 and f["avih"][4] == 5 and f["avih"][7] == big
    assert f["avih"][8:10] == (70, 50)
    video = [e for e in f["idx1"] if e[0] == b"00dc"]
    assert len(video) == 5 and all(e[1] == 0x10 for e in f["idx1"]) and [e[3] for e in video] == list(map(len, want))
    assert f["tags"] == [e[0] + struct.pack("<I", e[3]) for e in f["idx1"]]      # every index entry points at its chunk's header
    clip = container.read_avi(path)
    assert isinstance(clip["frames"], np.ndarray) and clip["frames"].shape == frames.shape
    assert all(np.array_equal(clip["frames"][k], mc.pil_decode(want[k])) for k in range(5))
    assert np.array_equal(clip["audio"], pcm) and clip["fps"] == 25.0 and clip["audio_sr"] == 16000


def test_default_codec_is_unchanged_and_write_jpeg_checks_the_size(tmp_path):
    from wav2lip_amd import container
    frames = (np.random.RandomState(6).rand(2, 18, 22, 3) * 255).astype(np.uint8)
    raw = str(tmp_path / "r.avi")
    container.write_avi(raw, frames, 25)
    f = avi_fields(raw)
    assert f["strh"][1] == b"DIB " and f["strf"][5] == 0 and [e[0] for e in f["idx1"]] == [b"00db"] * 2
    assert np.array_equal(container.read_avi(raw)["frames"], frames)
    with container.AviWriter(str(tmp_path / "m.avi"), 25, (22, 18), codec="mjpg") as out:
        out.write_jpeg(mc.pil_encode(frames[0], restart_marker_rows=1))
        with pytest.raises(ValueError, match="22x18"):
            out.write_jpeg(mc.pil_encode(frames[0][:, :20], restart_marker_rows=1))
        with pytest.raises(ValueError):
            out.write_jpeg(b"not a jpeg")
        assert out.n_frames == 1
    with container.AviWriter(raw, 25, (22, 18)) as out:
        with pytest.raises(ValueError, match="mjpg"):
            out.write_jpeg(mc.pil_encode(frames[0]))
        out.write(frames[0])
    with pytest.raises(ValueError):
        container.AviWriter(str(tmp_path / "x.avi"), 25, (22, 18), codec="h264")


def test_read_avi_takes_a_progressive_frame_through_pil(tmp_path):
    from wav2lip_amd import container
    frames = (np.random.RandomState(7).rand(3, 33, 47, 3) * 255).astype(np.uint8)
    prog = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frames[1][:, :, ::-1])).save(prog, format="JPEG", quality=95, progressive=True)
    datas = [container.encode_jpeg_host(frames[0]), prog.getvalue(), container.encode_jpeg_host(frames[2], 95, 2)]
    path = str(tmp_path / "p.avi")
    with container.AviWriter(path, 30, (47, 33), codec="mjpg") as out:
        for d in datas:
            out.write_jpeg(d)
    got = container.read_avi(path)["frames"]
    assert all(np.array_equal(got[k], mc.pil_decode(datas[k])) for k in range(3))


# ---------------------------------------------------------------- the segment decoder's arithmetic, on the CPU
def test_segment_decoder_arithmetic_under_the_host_sanitizers(tmp_path):
    """tools/jpeg_segments_host.cpp, a stand-alone program (nothing is loaded into Python, nothing touches a GPU), built with
    -fsanitize=address,undefined: every file of the cases, the same images without restarts and an interval counted in blocks
    decode to PIL's pixels; the truncated file, the one with a flipped byte and files with damaged markers are refused; a report
    of either sanitizer ends the program with a failure"""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_segments_host")
    # the sanitizer runtimes linked INTO the program (clang's default, gcc's by flag): it runs as it is, whatever else is loaded
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [os.path.join(ROOT, "tools", "jpeg_segments_host.cpp"), "-o", exe], check=True)
    valid = {"%dx%d_r%d_q%d" % (s + (r, q)): mc.pil_file(s, r, q) for s, r, q in mc.cases()}
    valid.update({"%dx%d_plain" % s: mc.pil_encode(mc.image(*s)) for s in mc.SHAPES})
    valid["40x70_blocks2"] = mc.pil_encode(mc.image(40, 70), restart_marker_blocks=2)
    d = mc.pil_file(*mc.BAD_SOURCE)
    segs, start, _ = mc.scan_segments(d)
    m4 = start + segs[4][0] + segs[4][1]
    corrupt = {"truncated": mc.truncated(), "flipped": mc.flipped(), "deleted_marker": d[:m4] + d[m4 + 2:],
               "wrong_marker": d[:m4 + 1] + b"\xd7" + d[m4 + 2:], "cut_in_marker": d[:m4 + 1],
               "short_interval": d[:m4 - 3] + d[m4:]}
    lines = []
    for name, data in valid.items():
        jpg, npy = str(tmp_path / (name + ".jpg")), str(tmp_path / (name + ".npy"))
        open(jpg, "wb").write(data)
        np.save(npy, mc.pil_decode(data))
        lines.append("valid %s %s" % (jpg, npy))
    for name, data in corrupt.items():
        jpg = str(tmp_path / ("corrupt_" + name + ".jpg"))
        open(jpg, "wb").write(data)
        lines.append("corrupt %s -" % jpg)
    manifest = str(tmp_path / "manifest.txt")
    open(manifest, "w").write("\n".join(lines) + "\n")
    run = subprocess.run([exe, manifest], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert "%d of %d valid files equal" % (len(valid), len(valid)) in run.stdout
    assert "%d of %d corrupt files refused, 0 failures" % (len(corrupt), len(corrupt)) in run.stdout
