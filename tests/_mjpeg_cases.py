"""The images and PIL files the Motion-JPEG tests share (tests/test_mjpeg_cpu.py, tests/test_mjpeg_gpu.py): every expectation is
what PIL / libjpeg-turbo writes or decodes for the same pixels and parameters."""
import functools
import io

import numpy as np
from PIL import Image

# H x W: the smallest image; one MCU (DRI and no marker); edge replication and one marker; 9 markers (RST7 wraps to RST0); a long
# MCU row; the image whose file has an interval ending in a stuffed FF; flat colour (intervals of a few bytes)
SHAPES = ((1, 1), (16, 16), (17, 33), (150, 40), (16, 1283), (330, 24), (96, 96))
FLAT = (96, 96)
STUFFED = (330, 24)
QUALITY_50 = ((17, 33), (150, 40))                 # the two shapes that also run at quality 50


def image(h, w):
    """uint8 [h,w,3] BGR: noise, or one colour for FLAT"""
    if (h, w) == FLAT:
        return np.ascontiguousarray(np.broadcast_to(np.array([200, 40, 90], np.uint8), (h, w, 3)))
    return (np.random.RandomState(0).rand(h, w, 3) * 255).astype(np.uint8)


def pil_encode(bgr, quality=95, **kw):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, format="JPEG", quality=quality, subsampling=2, **kw)
    return buf.getvalue()


def pil_decode(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


@functools.lru_cache(maxsize=None)
def cases():
    """((h, w), restart_rows, quality) of every encoder / decoder case"""
    out = [(s, r, 95) for s in SHAPES for r in (1, 2)]
    out += [(s, r, 50) for s in QUALITY_50 for r in (1, 2)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pil_file(shape, rows, quality):
    return pil_encode(image(*shape), quality, restart_marker_rows=rows)


def has_stuffed_interval_end(data):
    """an interval ending in a stuffed FF: FF 00 FF Dn inside the file"""
    return any(data.find(bytes([0xFF, 0x00, 0xFF, 0xD0 + k])) > 0 for k in range(8))


BAD_SOURCE = ((150, 40), 1, 95)                    # 10 intervals


def truncated():
    """BAD_SOURCE's file cut in the middle of its third interval"""
    d = pil_file(*BAD_SOURCE)
    segs, start, _ = scan_segments(d)
    return d[:start + segs[2][0] + segs[2][1] // 2]


def flipped():
    """BAD_SOURCE's file with every bit of one byte in the middle of its fourth interval flipped (never to FF: the markers stay
    where they are, so the host's scan accepts the file and the interval's own decoder meets the damage)"""
    d = bytearray(pil_file(*BAD_SOURCE))
    segs, start, _ = scan_segments(bytes(d))
    i = start + segs[3][0] + segs[3][1] // 2
    while d[i] in (0x00, 0xFF) or d[i - 1] == 0xFF:
        i += 1
    d[i] ^= 0xFF
    return bytes(d)


def scan_segments(data):
    """[(offset, nbytes)] of the restart intervals of a file's scan, relative to the scan's first byte: the ten-line scan"""
    start = data.index(b"\xff\xda") + 14
    end = data.rindex(b"\xff\xd9")
    out, s, i = [], start, start
    while i < end - 1:
        if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7:
            out.append((s - start, i - s))
            s = i = i + 2
        else:
            i += 2 if data[i] == 0xFF else 1
    return out + [(s - start, end - s)], start, end
