"""The host side of the device JPEG encoder: the numpy restatement of libjpeg's rules (tests/_jpeg_cases.py) and the header the
library builds, both against PIL's own bytes; the capacity bound; the `--jpeg` flag; and that the case set reaches every path of
the entropy coder (asserted on the restatement's counters, so the set cannot silently stop covering one)."""
import functools

import numpy as np
import pytest

import _jpeg_cases as jc

needs_turbo = pytest.mark.skipif(not jc.turbo(), reason="PIL is not linked against libjpeg-turbo: its bytes follow other rounding rules")


@functools.lru_cache(maxsize=None)
def restated():
    """{name: (restatement's bytes, counters, PIL's bytes, (h, w))} of every case, once"""
    return {name: jc.encode(img, q) + (jc.expected(name, img, q), img.shape[:2]) for name, img, q in jc.cases()}


@needs_turbo
def test_the_restatement_equals_pil_on_every_case():
    bad = [name for name, (got, _, want, _) in restated().items() if got != want]
    assert not bad, bad
    assert len(restated()) == len(jc.SIZES) * len(jc.CONTENTS) + len(jc.OTHER_Q) * len(jc.SUBSET) * len(jc.CONTENTS) + 1


@needs_turbo
@pytest.mark.parametrize("q", [1, 30, 50, 75, 95, 100])
def test_header_equals_pils_first_623_bytes(q):
    from wav2lip_amd import jpeg
    for h, w in ((1, 1), (37, 53), (160, 160), (300, 257)):
        want = jc.pil_bytes(jc.image("gradient", h, w), q)
        got = jpeg.header(h, w, q)
        assert len(got) == jpeg.HEADER_BYTES == 623 and got == want[:623], (h, w, q)
        assert int.from_bytes(got[163:165], "big") == h and int.from_bytes(got[165:167], "big") == w
    hdr, dqt, _ = jc.parse_header(want)
    assert len(hdr) == 623
    luma, chroma = jpeg.quant_tables(q)
    assert luma.shape == chroma.shape == (64,)
    assert np.array_equal(luma[jc.ZZ], dqt[0]) and np.array_equal(chroma[jc.ZZ], dqt[1])


def test_quant_tables_follow_the_quality_rule():
    """scale = 5000 / q below 50, else 200 - 2 q; t = clamp((base * scale + 50) / 100, 1, 255): the corners of the two tables"""
    from wav2lip_amd import jpeg
    for q in (1, 10, 49, 50, 75, 95, 100):
        scale = 5000 // q if q < 50 else 200 - 2 * q
        luma, chroma = jpeg.quant_tables(q)
        for table, first, last in ((luma, 16, 99), (chroma, 17, 99)):
            assert table[0] == min(max((first * scale + 50) // 100, 1), 255)
            assert table[63] == min(max((last * scale + 50) // 100, 1), 255)
    assert (jpeg.quant_tables(100)[0] == 1).all()


def test_header_refuses_bad_arguments():
    from wav2lip_amd import jpeg
    for h, w, q in ((0, 1, 95), (1, 0, 95), (65536, 1, 95), (1, 1, 0), (1, 1, 101)):
        with pytest.raises(RuntimeError):
            jpeg.header(h, w, q)


@needs_turbo
def test_capacity_bounds_every_case_and_is_the_documented_formula():
    from wav2lip_amd import jpeg
    for name, (_, _, want, (h, w)) in restated().items():
        assert len(want) <= jpeg.capacity(h, w), name
    for h, w in ((1, 1), (16, 16), (17, 16), (16, 17), (160, 160), (161, 1)):
        nblocks = 6 * ((h + 15) // 16) * ((w + 15) // 16)
        assert jpeg.blocks(h, w) == nblocks and jpeg.capacity(h, w) == 625 + 416 * nblocks
    # per block: 22 bits of DC (an 11-bit code + 11 bits) and 63 x 26 bits of AC (a 16-bit code + 10 bits), each byte stuffed
    assert -(-(22 + 63 * 26) // 8) * 2 == 416


def test_the_jpeg_flag_is_on_the_command_line_parser_only():
    from wav2lip_amd import preprocess
    base = ["--data_root", "d", "--preprocessed_root", "p"]
    assert preprocess.main_parser.parse_args(base).jpeg == "host"
    assert preprocess.main_parser.parse_args(base + ["--jpeg", "device"]).jpeg == "device"
    with pytest.raises(SystemExit):
        preprocess.main_parser.parse_args(base + ["--jpeg", "gpu"])
    with pytest.raises(SystemExit):
        preprocess.parser.parse_args(base + ["--jpeg", "device"])
    assert not hasattr(preprocess.parser.parse_args(base), "jpeg")


def test_encode_crops_refuses_host_tensors():
    import torch
    from wav2lip_amd import jpeg
    with pytest.raises(RuntimeError):
        jpeg.encode_crops(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), [(0, 0, 8, 8)])
    with pytest.raises(RuntimeError):
        jpeg.encode_crops(np.zeros((1, 8, 8, 3), np.uint8), [(0, 0, 8, 8)])


@needs_turbo
def test_the_case_set_reaches_every_path():
    cnt = {name: c for name, (_, c, _, _) in restated().items()}
    shape = {name: hw for name, (_, _, _, hw) in restated().items()}
    assert cnt["noise_160x160_q30"]["zrl"] >= 1                                   # a run of 16 zeros
    assert sum(c["stuffed"] for c in cnt.values()) >= 10                          # 0xFF in the stream
    assert any(c["dummy_right"] for c in cnt.values()) and any(c["dummy_bottom"] for c in cnt.values())
    assert any(c["dummy_right"] and c["dummy_bottom"] for c in cnt.values())      # a dummy whose predecessor is a dummy
    assert any(h % 16 == 8 for h, _ in shape.values())                            # chroma rows padded after downsampling
    assert any(c["eob_only"] for c in cnt.values())
    assert any(c["coef63"] for c in cnt.values())                                 # a block that ends without an EOB
    assert max(c["dc_cat"] for c in cnt.values()) >= 9
    assert max(c["ac_cat"] for c in cnt.values()) >= 10
    assert any(c["blocks"] > 256 for c in cnt.values())                           # more blocks than the entropy kernel has threads
