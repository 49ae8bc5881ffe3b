"""The host side of the device JPEG decoder: the numpy restatement of libjpeg's decoding rules (tests/_jpeg_decode_cases.py)
against PIL's own pixels, that the file set reaches every path of the decoder (asserted on the restatement's counters, so the set
cannot silently stop covering one), and w2l_jpeg_parse / w2l_jpeg_build_tables through ctypes: what they accept, what they refuse
and why, and that no cut of a header makes them read past the bytes they were given."""
import ctypes as C
import functools

import numpy as np
import pytest

import _jpeg_cases as jc
import _jpeg_decode_cases as dc


@functools.lru_cache(maxsize=None)
def restated():
    """{name: (restatement's image, counters, PIL's image)} of every file, once"""
    return {name: dc.decode(d) + (dc.expected(name, d),) for name, d in dc.files()}


def test_the_restatement_equals_pil_on_every_file():
    assert len(restated()) == 2 * len(jc.cases()) + 4 * len(dc.NARROW)
    bad = [name for name, (got, _, want) in restated().items() if got.shape != want.shape or not np.array_equal(got, want)]
    assert not bad, bad


def test_the_files_reach_every_path_of_the_decoder():
    cnt = [c for _, c, _ in restated().values()]
    assert sum(c["zrl"] for c in cnt) > 0
    assert sum(c["stuffed"] for c in cnt) > 0
    assert sum(c["code16"] for c in cnt) > 0
    assert sum(c["coef63"] for c in cnt) > 0
    assert max(c["dc_cat"] for c in cnt) == 11
    assert sum(c["dummy_right"] for c in cnt) > 0 and sum(c["dummy_bottom"] for c in cnt) > 0
    shapes = {img.shape[:2] for _, _, img in restated().values()}
    assert any(h % 2 for h, _ in shapes) and any(w % 2 for _, w in shapes) and (1, 1) in shapes
    # both table kinds: the optimised files carry tables of their own
    tables = {repr(jc.parse_header(d)[2]) for _, d in dc.files()}
    assert len(tables) > 100


def test_narrow_images_take_the_plain_upsampling_and_it_differs_from_the_fancy_rule():
    """libjpeg blends chroma only where the chroma plane is more than 2 samples wide: the NARROW files (1 to 4 columns, 3 rows and
    more) equal PIL under the replication rule, and would not under the other - so the files tell the two apart"""
    shapes = {img.shape[:2] for name, (_, _, img) in restated().items() if any(name.startswith("noise_%dx%d_" % s) for s in dc.NARROW)}
    assert {(16, 4), (9, 3), (5, 2)} <= shapes and {w for _, w in shapes} == {1, 2, 3, 4}
    c = np.arange(16, dtype=np.int64).reshape(8, 2) * 13 % 256
    box = dc.upsample(c, 16, 4)
    assert np.array_equal(box, c.repeat(2, 0).repeat(2, 1))
    wide = dc.upsample(np.concatenate([c, c[:, :1]], 1), 16, 6)          # three columns: blended
    assert not np.array_equal(wide[:, :4], box)


def test_overwrites_that_stay_decodable_are_kept_as_files_with_the_references_pixels():
    alt = dc.altered_files()
    assert len(alt) >= 20 and len({n for n, _, _ in alt}) == len(alt)
    for name, c, img in alt:
        assert img.dtype == np.uint8 and img.ndim == 3, name


def test_the_corpus_is_deterministic_and_every_member_differs_from_its_source():
    a = dc.corrupt_corpus()
    assert len(a) == 3 * (3 + 1 + dc.N_OVERWRITES + 1)
    assert len({name for name, _, _ in a}) == len(a)
    for name, c, d in a:
        assert c != d, name
    dc._corpus.clear()
    b = dc.corrupt_corpus()
    assert [(n, c) for n, c, _ in a] == [(n, c) for n, c, _ in b]


# ---------------------------------------------------------------- w2l_jpeg_parse
def parse(d):
    from wav2lip_amd import _lib
    lib = _lib.load()
    info = _lib.JpegInfo()
    d = bytes(d)
    rc = lib.w2l_jpeg_parse(d, len(d), C.byref(info))
    return rc, info, (lib.w2l_last_error() or b"").decode()


def test_parse_reads_what_the_python_parser_reads():
    from wav2lip_amd import jpeg
    for name, d in dc.files():
        rc, info, _ = parse(d)
        assert rc == 0, name
        hdr, dqt, dht = jc.parse_header(d)
        assert (info.H, info.W) == dc.sof(d, len(hdr)) == dc.expected(name, d).shape[:2] == jpeg.probe(d), name
        assert info.ecs_offset == len(hdr) and info.ecs_bytes == len(d) - 2 - len(hdr) and info.eoi == 1, name
        assert list(info.quant[0]) == dqt[0].tolist() and list(info.quant[1]) == dqt[1].tolist(), name
        for j, key in enumerate((0x00, 0x10, 0x01, 0x11)):
            bits, vals = dht[key]
            assert list(info.bits[j]) == bits and info.nvals[j] == len(vals) and list(info.vals[j])[:len(vals)] == vals, (name, j)


def test_parse_refuses_files_outside_the_class_each_with_its_own_reason():
    from wav2lip_amd import jpeg
    from PIL import Image
    import io
    img = jc.image("noise", 40, 56)
    gray = io.BytesIO()
    Image.fromarray(img[:, :, 0]).save(gray, format="JPEG", quality=95)
    cases = {"progressive": (dc.pil_file(img, 95, progressive=True), -101, "progressive"),
             "444": (dc.pil_file(img, 95, subsampling=0), -104, "1x1"),
             "422": (dc.pil_file(img, 95, subsampling=1), -104, "2x1"),
             "grayscale": (gray.getvalue(), -103, "1 components"),
             "restart": (dc.pil_file(img, 95, restart_marker_rows=1), -105, "restart interval")}
    texts = set()
    for name, (d, code, word) in cases.items():
        assert dc.pil_decode(d).shape[:2] == (40, 56)                 # PIL decodes every one of them
        rc, _, text = parse(d)
        assert rc == code and word in text, (name, rc, text)
        texts.add(text)
        with pytest.raises(jpeg.UnsupportedJpeg, match=word) as e:
            jpeg.probe(d)
        assert e.value.code == code
    assert len(texts) == len(cases)
    # hand-made: an Adobe APP14 segment, a 16-bit quantiser, a restart interval of 0 (accepted), a size of 0
    d = dc.pil_file(img, 95)
    adobe = bytes([0xFF, 0xEE, 0, 14]) + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 1])
    rc, _, text = parse(d[:2] + adobe + d[2:])
    assert rc == -108 and "Adobe" in text
    i = d.index(b"\xff\xdb")
    rc, _, text = parse(d[:i + 4] + bytes([0x10]) + d[i + 5:])
    assert rc == -106 and "16-bit" in text
    s = d.index(b"\xff\xda")
    assert parse(d[:s] + bytes([0xFF, 0xDD, 0, 4, 0, 0]) + d[s:])[0] == 0
    assert parse(d[:s] + bytes([0xFF, 0xDD, 0, 4, 0, 7]) + d[s:])[0] == -105
    f = d.index(b"\xff\xc0")
    assert parse(d[:f + 5] + bytes([0, 0]) + d[f + 7:])[0] == -109
    assert parse(d[:f + 7] + bytes([0, 0]) + d[f + 9:])[0] == -109
    assert parse(d[:-2] + d[s:])[0] == -107                           # a second scan behind the first
    assert parse(d + d[2:])[0] == 0                                   # bytes behind EOI are not the file's (libjpeg ignores them too)
    # component ids 'R' 'G' 'B' and no JFIF segment: libjpeg decodes such a file as RGB, so it is not the device's
    nojfif = d[:2] + d[20:]
    assert d[2:4] == b"\xff\xe0" and parse(nojfif)[0] == 0
    rgb = bytearray(nojfif)
    f2, s2 = rgb.index(b"\xff\xc0"), rgb.index(b"\xff\xda")
    for c, ch in enumerate(b"RGB"):
        rgb[f2 + 10 + 3 * c] = ch
        rgb[s2 + 5 + 2 * c] = ch
    rc, _, text = parse(bytes(rgb))
    assert rc == -111 and "RGB" in text
    assert np.abs(dc.pil_decode(bytes(rgb)).astype(int) - dc.pil_decode(nojfif)).max() > 30      # PIL does decode it as RGB
    withjfif = d[:20] + bytes(rgb[2:])
    assert parse(withjfif)[0] == 0 and np.array_equal(dc.pil_decode(withjfif), dc.pil_decode(d))    # JFIF says YCbCr
    assert parse(b"")[0] == -100 and parse(b"\x89PNG\r\n\x1a\n" + bytes(64))[0] == -100
    with pytest.raises(ValueError) as e:                              # no JPEG at all: plain ValueError, not UnsupportedJpeg
        jpeg.probe(b"\x89PNG\r\n\x1a\n" + bytes(64))
    assert not isinstance(e.value, jpeg.UnsupportedJpeg)


def test_files_cut_at_every_byte_of_the_header_are_refused_without_a_crash():
    """the copy handed to the parser ends exactly where the cut is (a bytes object of that length), and a segment length is
    never trusted beyond it"""
    for name in ("noise_37x53_q95_std", "noise_37x53_q95_opt"):
        d = dict(dc.files())[name]
        ecs = len(jc.parse_header(d)[0])
        for n in range(ecs + 1):
            rc, _, text = parse(d[:n])
            assert rc == -100 and text, (name, n, rc)
        # cut inside the scan: described (the kernel meets the end), with no EOI
        rc, info, _ = parse(d[:ecs + 10])
        assert rc == 0 and info.eoi == 0 and info.ecs_offset == ecs and info.ecs_bytes == 10
        # a segment that claims more bytes than the file has
        i = d.index(b"\xff\xc4")
        rc, _, text = parse(d[:i + 2] + b"\xff\xff" + d[i + 4:])
        assert rc == -100 and "claims" in text


def test_table_builder_refuses_what_is_no_prefix_code():
    from wav2lip_amd import _lib
    lib = _lib.load()
    assert lib.w2l_jpeg_table_bytes() == 5952
    d = dict(dc.files())["noise_37x53_q95_std"]
    out = (C.c_uint8 * 5952)()

    def build(change):
        rc, info, _ = parse(d)
        assert rc == 0
        change(info)
        return lib.w2l_jpeg_build_tables(C.byref(info), out), (lib.w2l_last_error() or b"").decode()

    assert build(lambda i: None)[0] == 0
    look = np.frombuffer(out, np.uint16, 512, 256)                   # DC luma: category 0 has the 2-bit code 00
    assert look[0] == (2 << 8) | 0 and look[127] == (2 << 8) | 0 and look[128] == (3 << 8) | 1

    def oversubscribe(i):
        i.bits[1][0] = 3                                             # three codes of one bit, for three symbols of their own
        for k, sym in enumerate((0x0B, 0x0C, 0x0D)):
            i.vals[1][i.nvals[1] + k] = sym
        i.nvals[1] += 3
    rc, text = build(oversubscribe)
    assert rc != 0 and "oversubscribe" in text

    def full_then_more(i):                                           # 2 codes of 1 bit fill the space; a third code of 2 bits
        for k in range(16):
            i.bits[0][k] = 0
        i.bits[0][0], i.bits[0][1], i.nvals[0] = 2, 1, 3
    assert build(full_then_more)[0] != 0

    def twice(i):
        i.vals[1][1] = i.vals[1][0]
    rc, text = build(twice)
    assert rc != 0 and "twice" in text

    def count(i):
        i.nvals[2] -= 1
    assert build(count)[0] != 0

    def dc12(i):
        i.vals[0][0] = 12
    assert build(dc12)[0] != 0

    def q0(i):
        i.quant[1][5] = 0
    assert build(q0)[0] != 0
