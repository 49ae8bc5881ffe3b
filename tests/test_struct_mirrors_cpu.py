"""Every table struct of the packed paths, held together in one place: the typedef in include/w2l_hip.h is the authority, the
ctypes class in wav2lip_amd/_lib.py mirrors it, and the numpy dtype the modules fill their tables through is derived from the
class.  Each typedef is parsed out of the header and laid out under natural alignment; class and dtype must have its field names
in its order, its offsets, its element types and its size.  The sizes and offsets the header's comments state are checked too."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "w2l_hip.h")).read()
C_TYPES = {"uint64_t": (8, ctypes.c_uint64, "<u8"), "int64_t": (8, ctypes.c_int64, "<i8"), "int32_t": (4, ctypes.c_int32, "<i4"),
           "double": (8, ctypes.c_double, "<f8")}
KINDS = {"uint64": "uint64_t", "int64": "int64_t", "int32": "int32_t", "float64": "double"}      # the comment tables' words

# typedef -> (ctypes class, dtype, bytes, the modules through which the dtype is reached, the offsets spelled out by hand)
STRUCTS = {
    "w2l_frame_row": ("FrameRow", "FRAME_ROW", 48, ["multiclip"],
                      dict(src=0, dst=8, H=16, W=20, y1=24, y2=28, x1=32, x2=36, pad=40)),
    "w2l_mel_row": ("MelRow", "MEL_ROW", 16, ["multiclip"], dict(mel=0, T=8, start=12)),
    "w2l_resize_row": ("ResizeRow", "RESIZE_ROW", 32, ["real_videos_inference"], dict(src=0, dst=8, Hs=16, Ws=20, Hd=24, Wd=28)),
    "w2l_jpeg_row": ("JpegRow", "JPEG_ROW", 32, ["jpeg"], dict(src=0, dst=8, nbytes=16, H=20, W=24, table=28)),
    "w2l_jpeg_segment": ("JpegSegment", "JPEG_SEGMENT", 32, ["jpeg"], dict(row=0, offset=4, nbytes=8, first_mcu=12, n_mcus=16, pad=20)),
    "w2l_box_segment": ("BoxSegment", "BOX_SEGMENT", 16, ["face_detection.many"], dict(row0=0, n=4, H=8, W=12)),
    "w2l_box_stream_segment": ("BoxStreamSegment", "BOX_STREAM_SEGMENT", 32, ["face_detection.live"],
                               dict(row0=0, n_new=4, H=8, W=12, slot=16, seen=20, closed=24, out0=28)),
    "w2l_mel_stream": ("MelStream", "MEL_STREAM", 48, ["streaming"], dict(samples=0, first=8, total=16, window=24, held=32, cap=36, col0=40)),
    "w2l_mel_col": ("MelCol", "MEL_COL", 16, ["streaming"], dict(stream=0, rsv=4, col=8)),
    "w2l_resample_stream_entry": ("ResampleStreamEntry", "RESAMPLE_STREAM", 128, ["streaming"], dict(src=0, scale=80, src_held=96, unused=116)),
    "w2l_resample_block": ("ResampleBlock", "RESAMPLE_BLOCKS", 32, ["streaming"], dict(stream=0, count=4, t0=8, tr0=16, copy=24, unused=28)),
    "w2l_sync_row": ("SyncRow", "SYNC_ROW", 32, ["evaluation"], dict(frames=0, mel=8, T=16, start=20, pad=24)),
    "w2l_lse_segment": ("LseSegment", "LSE_SEGMENT", 8, ["evaluation"], dict(row0=0, n=4)),
}


def typedef_layout(name):
    """([(field, C type, array length or 0, offset)], size) of `typedef struct { ... } name;` under natural alignment"""
    body = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, HEADER).group(1)
    fields, off, widest = [], 0, 1
    for ctype, members in re.findall(r"(\w+)\s+([^;]+);", body):
        width = C_TYPES[ctype][0]
        widest = max(widest, width)
        for member in members.split(","):
            field, length = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", member).groups()
            off = (off + width - 1) // width * width
            fields.append((field, ctype, int(length or 0), off))
            off += width * int(length or 1)
    return fields, (off + widest - 1) // widest * widest


def stated_table(name, size):
    """[(offset, kind, first field)] of the rows `offset N type field` / `at N type field` / `byte N type field` of the comment
    that states the struct's layout (some comments give byte ranges instead: no rows)"""
    start = HEADER.index("%s, %d bytes" % (name, size))
    end = min(e for e in (HEADER.find(" bytes, ", start + len(name) + 10), HEADER.find("typedef", start)) if e >= 0)
    return [(int(off), kind, field) for off, kind, field in
            re.findall(r"\* +(?:offset|at|byte) +(\d+) +(u?int\d+|float64) +(\w+)", HEADER[start:end])]


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_class_and_dtype_have_the_layout_of_the_typedef(name):
    from wav2lip_amd import _lib
    cls_name, dt_name, size, modules, by_hand = STRUCTS[name]
    ct, dt = getattr(_lib, cls_name), getattr(_lib, dt_name)
    fields, c_size = typedef_layout(name)
    aligned = {"w2l_lse_segment": "alignment 8", "w2l_box_segment": "the table 16-byte aligned",
               "w2l_box_stream_segment": "the table 16-byte aligned"}.get(name, "alignment 16")
    assert "%s, %d bytes, %s" % (name, size, aligned) in HEADER, name
    assert c_size == size == ctypes.sizeof(ct) == dt.itemsize
    assert size % 16 == 0 or name == "w2l_lse_segment"              # consecutive rows stay 16-byte aligned
    assert [f for f, _, _, _ in fields] == [f for f, _ in ct._fields_] == list(dt.names)
    for (field, ctype, length, off), (_, c_field) in zip(fields, ct._fields_):
        _, c_elem, np_elem = C_TYPES[ctype]
        assert getattr(ct, field).offset == dt.fields[field][1] == off, (name, field)
        assert c_field is (c_elem * length if length else c_elem), (name, field)
        assert dt.fields[field][0].base.str == np_elem and dt.fields[field][0].shape == ((length,) if length else ()), (name, field)
    for field, off in by_hand.items():
        assert getattr(ct, field).offset == dt.fields[field][1] == off, (name, field)
    layout = {f: (off, ctype) for f, ctype, _, off in fields}
    for off, kind, field in stated_table(name, size):
        assert layout[field] == (off, KINDS[kind]), (name, field)
    for module in modules:                                           # the modules import the name instead of spelling it
        assert getattr(importlib.import_module("wav2lip_amd." + module), dt_name) is dt, (module, dt_name)
    assert np.dtype(ct) == dt


def test_the_comment_tables_that_list_every_field():
    """the two resample structs: the header's `at N` table names every member, in order; the row tables of multiclip and
    streaming: every field that opens a row of the `offset N` table"""
    for name, n_rows in (("w2l_resample_stream_entry", 18), ("w2l_resample_block", 6)):
        size = STRUCTS[name][2]
        m = re.search(r"%s, (\d+) bytes, alignment 16:\n((?: \*   at .*\n)+)" % name, HEADER)
        assert m and int(m.group(1)) == size
        stated = re.findall(r"at +(\d+) +(u?int\d+|float64) +(\w+)", m.group(2))
        assert len(stated) == n_rows
        assert [(f, KINDS[kind], int(off)) for off, kind, f in stated] == [(f, ctype, off) for f, ctype, _, off in typedef_layout(name)[0]]
    opened = {name: [f for _, _, f in stated_table(name, STRUCTS[name][2])] for name in STRUCTS}
    assert opened["w2l_frame_row"] == ["src", "dst", "H", "y1", "pad"] and opened["w2l_mel_row"] == ["mel", "T", "start"]
    assert opened["w2l_mel_stream"] == ["samples", "first", "total", "window", "held", "cap", "col0"]
    assert opened["w2l_mel_col"] == ["stream", "rsv", "col"]
    assert opened["w2l_resize_row"] == ["src", "dst", "Hs"] and opened["w2l_sync_row"] == ["frames", "mel", "T", "start", "pad"]
    assert "evaluation/real_videos_inference.py:51-70,239-245" in HEADER


def test_the_entry_points_that_take_the_tables_are_bound():
    from wav2lip_amd import _lib
    from wav2lip_amd.face_detection import live, many
    for sym in ("w2l_crop_resize_rows_u8", "w2l_compose_rows_u8", "w2l_mel_gather_rows", "w2l_mel_gather_rows_bf16", "w2l_mel_stream_cols",
                "w2l_s3fd_pack_rows", "w2l_s3fd_pack_rows_bf16", "w2l_face_boxes_segments", "w2l_face_boxes_stream", "w2l_resize_rows_u8",
                "w2l_jpeg_decode_rows", "w2l_jpeg_decode_rows_rst", "w2l_sync_window_rows", "w2l_lse_score_segments"):
        assert sym in _lib.SIGNATURES, sym
    assert len(_lib.SIGNATURES["w2l_face_boxes_stream"][1]) == 17
    assert _lib.SIGNATURES["w2l_resample_stream"][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert live.CARRY_ROWS == many.MAX_T == 64
