"""Files for the JPEG decoder's tests and a numpy restatement of what libjpeg does for `PIL.Image.open(...).convert("RGB")` on a
baseline 4:2:0 file (jdhuff.c decode_mcu, jidctint.c jpeg_idct_islow, jdsample.c h2v2_fancy_upsample, jdcolor.c ycc_rgb_convert),
with counters of the code paths a file takes.  The expectation of every test is PIL's own pixels; the restatement exists so that
the file set can be shown to reach every path (a ZRL, a stuffed byte, a 16-bit code, ...), and it is itself held to PIL in
test_jpeg_decode_cpu.py.  Test infrastructure only: nothing in the package imports it.

The restatement is STRICT where libjpeg is lenient: it refuses (raises Corrupt) a stream with bits that are no code, a zero run
past coefficient 63, a marker other than the stuffed FF 00 before the last MCU, a stream that ends early, or bytes left over behind
the last MCU.  That is the contract of w2l_jpeg_decode_rows, and it is what defines the corrupt corpus below."""
import io

import numpy as np

import _jpeg_cases as jc

ZZ = np.array(jc.ZZ)


class Corrupt(Exception):
    pass


def pil_file(bgr, q=95, **kw):
    """a JPEG file of PIL's: 4:2:0 unless `subsampling` says otherwise; optimize=True for per-file Huffman tables"""
    from PIL import Image
    b = io.BytesIO()
    kw.setdefault("subsampling", 2)
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(b, format="JPEG", quality=q, **kw)
    return b.getvalue()


def pil_decode(d):
    """the expectation: uint8 [H,W,3] BGR"""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[:, :, ::-1])


NARROW = [(16, 4), (9, 3), (5, 2), (16, 3), (16, 2), (9, 4), (3, 3), (4, 4), (3, 1), (7, 2)]   # W <= 4 with H >= 3: plain upsampling

_files = {}


def files():
    """[(name, file bytes)]: every case of _jpeg_cases.cases() with the standard Huffman tables ("_std") and with
    optimize=True ("_opt": tables of the file's own), then the NARROW sizes in both kinds; computed once per process"""
    if not _files:
        for name, img, q in jc.cases():
            _files[name + "_std"] = jc.expected(name, img, q)
            _files[name + "_opt"] = pil_file(img, q, optimize=True)
        for h, w in NARROW:                       # images of 1 to 4 columns: libjpeg replicates their chroma instead of blending it
            for c in ("noise", "redblue"):
                _files["%s_%dx%d_q95_std" % (c, h, w)] = pil_file(jc.image(c, h, w, seed=1), 95)
                _files["%s_%dx%d_q95_opt" % (c, h, w)] = pil_file(jc.image(c, h, w, seed=1), 95, optimize=True)
    return list(_files.items())


_expected = {}


def expected(name, d):
    if name not in _expected:
        _expected[name] = pil_decode(d)
    return _expected[name]


def sof(d, hdr_len):
    """(H, W) of the SOF0 segment inside the header"""
    i = 2
    while i < hdr_len:
        m, n = d[i + 1], int.from_bytes(d[i + 2:i + 4], "big")
        if m == 0xC0:
            return int.from_bytes(d[i + 5:i + 7], "big"), int.from_bytes(d[i + 7:i + 9], "big")
        i += 2 + n
    raise ValueError("no SOF0")


_lookups = {}


def lookup(bits, vals):
    """full 16-bit lookahead of a (bits, vals) table: (length [65536], symbol [65536]); length 0: no code"""
    key = (tuple(bits), tuple(vals))
    if key not in _lookups:
        ln = np.zeros(65536, np.int64)
        sy = np.zeros(65536, np.int64)
        code, k = 0, 0
        for n in range(1, 17):
            for _ in range(bits[n - 1]):
                ln[code << (16 - n):(code + 1) << (16 - n)] = n
                sy[code << (16 - n):(code + 1) << (16 - n)] = vals[k]
                code += 1
                k += 1
            code <<= 1
        _lookups[key] = (ln.tolist(), sy.tolist())
    return _lookups[key]


def entropy(ecs, H, W, dqt, dht, cnt):
    """dequantised coefficients int64 [nblocks, 64] in row-major order, blocks MCU-interleaved (Y00 Y01 Y10 Y11 Cb Cr)"""
    raw = bytes(ecs)
    real = bytearray()
    i, marker = 0, False
    while i < len(raw):
        b = raw[i]
        if b == 0xFF:
            if i + 1 < len(raw) and raw[i + 1] == 0:
                cnt["stuffed"] += 1
                i += 2
            else:
                marker = True
                break
        else:
            i += 1
        real.append(b)
    nreal = 8 * len(real)
    buf = bytes(real) + b"\0\0\0\0"
    mw, mh = -(-W // 16), -(-H // 16)
    nblocks = 6 * mw * mh
    coef = np.zeros((nblocks, 64), np.int64)
    dc = [lookup(*dht[0x00]), lookup(*dht[0x01])]
    ac = [lookup(*dht[0x10]), lookup(*dht[0x11])]
    q = [dqt[0].tolist(), dqt[1].tolist()]
    pos = 0
    pred = [0, 0, 0]

    def peek16():
        j = pos >> 3
        if j + 3 > len(buf):
            return 0
        return (((buf[j] << 16) | (buf[j + 1] << 8) | buf[j + 2]) >> (8 - (pos & 7))) & 0xFFFF

    def over():
        if pos > nreal:
            raise Corrupt("a marker in the stream" if marker else "the stream ends early")

    for blk in range(nblocks):
        k6 = blk % 6
        c, t = (0, 0) if k6 < 4 else (k6 - 3, 1)
        v = peek16()
        n = dc[t][0][v]
        if n == 0:
            raise Corrupt("no DC code")
        cnt["code16"] += n == 16
        pos += n
        s = dc[t][1][v]
        if s > 11:
            raise Corrupt("DC category %d" % s)
        cnt["dc_cat"] = max(cnt["dc_cat"], s)
        if s:
            r = peek16() >> (16 - s)
            pos += s
            pred[c] += r if r >= (1 << (s - 1)) else r - (1 << s) + 1
        coef[blk, 0] = max(-32768, min(32767, pred[c] * q[t][0]))          # the workspace holds int16
        k = 1
        aln, asy = ac[t]
        while k < 64:
            v = peek16()
            n = aln[v]
            if n == 0:
                over()
                raise Corrupt("no AC code")
            cnt["code16"] += n == 16
            pos += n
            rs = asy[v]
            run, s = rs >> 4, rs & 15
            if s:
                k += run
                if k > 63:
                    raise Corrupt("a run past coefficient 63")
                r = peek16() >> (16 - s)
                pos += s
                coef[blk, ZZ[k]] = max(-32768, min(32767, (r if r >= (1 << (s - 1)) else r - (1 << s) + 1) * q[t][k]))
                cnt["coef63"] += k == 63
            else:
                if run != 15:
                    break
                cnt["zrl"] += 1
                k += 15
                if k > 63:
                    raise Corrupt("a run past coefficient 63")
            k += 1
        over()
    if marker or nreal - pos >= 8:
        raise Corrupt("a marker or bytes left over behind the last MCU")
    return coef


def idct(b):
    """libjpeg's jpeg_idct_islow on [..., 8, 8] blocks of dequantised coefficients: columns first (descale 11), then rows (descale
    18), then the range-limit table with its & 1023 wrap; returns samples 0..255"""
    def one(d, shift):
        d = [d[..., k] for k in range(8)]
        z2, z3 = d[2], d[6]
        z1 = (z2 + z3) * 4433
        t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
        t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        r = 1 << (shift - 1)
        o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
        return np.stack([(((x + r + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)) >> shift for x in o], -1)   # 32-bit wrap-around, as the C code
    cols = one(b.astype(np.int64).swapaxes(-1, -2), 11).swapaxes(-1, -2)       # each column transformed
    v = one(cols, 18) & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896)))


def upsample(c, H, W):
    """h2v2_fancy_upsample of the REAL chroma plane c [ceil(H/2), ceil(W/2)] to [H, W]; plain 2x2 replication (h2v2_upsample)
    for a plane of one or two columns"""
    c = c.astype(np.int64)
    if c.shape[1] <= 2:                       # jinit_upsampler: fancy only where the plane is more than 2 samples wide
        return c.repeat(2, 0).repeat(2, 1)[:H, :W]
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    v = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    v[0::2] = 3 * c + up
    v[1::2] = 3 * c + down
    left = np.concatenate([v[:, :1], v[:, :-1]], 1)
    right = np.concatenate([v[:, 1:], v[:, -1:]], 1)
    o = np.empty((v.shape[0], 2 * v.shape[1]), np.int64)
    o[:, 0::2] = (3 * v + left + 8) >> 4
    o[:, 1::2] = (3 * v + right + 7) >> 4
    return o[:H, :W]


def decode(d, pixels=True):
    """(uint8 [H,W,3] BGR image or None, counters) of one file; raises Corrupt"""
    hdr, dqt, dht = jc.parse_header(d)
    H, W = sof(d, len(hdr))
    end = len(d) - 2 if d[-2:] == b"\xff\xd9" else len(d)
    cnt = dict(zrl=0, stuffed=0, code16=0, coef63=0, dc_cat=0)
    mw, mh = -(-W // 16), -(-H // 16)
    cnt["dummy_right"] = int(-(-W // 8) < 2 * mw)
    cnt["dummy_bottom"] = int(-(-H // 8) < 2 * mh)
    coef = entropy(d[len(hdr):end], H, W, dqt, dht, cnt)
    if not pixels:
        return None, cnt
    s = idct(coef.reshape(mh, mw, 6, 8, 8))
    y = s[:, :, :4].reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(16 * mh, 16 * mw)
    cb = s[:, :, 4].transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw)
    cr = s[:, :, 5].transpose(0, 2, 1, 3).reshape(8 * mh, 8 * mw)
    ch, cw = -(-H // 2), -(-W // 2)
    y = y[:H, :W]
    cb = upsample(cb[:ch, :cw], H, W) - 128
    cr = upsample(cr[:ch, :cw], H, W) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8), cnt


# ---------------------------------------------------------------- the corrupt corpus
CORPUS_SEED = 20240607
N_OVERWRITES = 20


def valid_three():
    """the three valid files the corpus is made from: small (every candidate is decoded by the restatement), two table kinds"""
    return [("noise_37x53_q95_std", pil_file(jc.image("noise", 37, 53), 95)),
            ("noise_40x40_q30_opt", pil_file(jc.image("noise", 40, 40), 30, optimize=True)),
            ("gradient_49x63_q95_std", pil_file(jc.image("gradient", 49, 63), 95))]


def sparse_ac_table(d):
    """the file with its luma AC table (DHT class 1, id 0) replaced by one of three symbols (EOB, 0/1, ZRL: codes 0, 10, 110): a
    valid table that lacks the symbols the stream uses"""
    i = 2
    while True:
        m, n = d[i + 1], int.from_bytes(d[i + 2:i + 4], "big")
        if m == 0xC4 and d[i + 4] == 0x10:
            seg = bytes([0xFF, 0xC4, 0, 2 + 17 + 3, 0x10, 1, 1, 1] + [0] * 13 + [0x00, 0x01, 0xF0])
            return d[:i] + seg + d[i + 2 + n:]
        assert m != 0xDA, "no luma AC table in its own DHT segment"
        i += 2 + n


_corpus = []
_altered = []


def corrupt_corpus():
    """[(name, file bytes, valid file it was made from)], deterministic: of each of the three valid files
      - the file cut at 25 %, at 50 % and before its last byte;
      - FF D9 planted in the middle of the entropy segment;
      - one byte of the entropy segment overwritten, 20 times: positions and values come from a generator seeded with
        (CORPUS_SEED, file index), drawn in order.  A draw that leaves a stream the restatement above still decodes - a changed
        magnitude bit, say - is a VALID file with other pixels, which no decoder can refuse, so it is no member of a corrupt corpus:
        the first 20 draws the restatement refuses are taken.  The restatement is held to PIL on every valid file and is the
        reference here, not the code under test.  The draws passed over on the way are not dropped: `altered_files()` returns
        them, and the decoder must give the restatement's pixels for each;
      - its luma AC table replaced by one that lacks the symbols the stream uses."""
    if _corpus:
        return _corpus
    for fi, (name, d) in enumerate(valid_three()):
        hdr = jc.parse_header(d)[0]
        s, e = len(hdr), len(d) - 2
        _corpus.append((name + "_cut25", d[:len(d) // 4], d))
        _corpus.append((name + "_cut50", d[:len(d) // 2], d))
        _corpus.append((name + "_cutlast", d[:-1], d))
        mid = (s + e) // 2
        _corpus.append((name + "_eoi_planted", d[:mid] + b"\xff\xd9" + d[mid + 2:], d))
        rng = np.random.default_rng([CORPUS_SEED, fi])
        kept = 0
        while kept < N_OVERWRITES:
            pos, val = int(rng.integers(s, e)), int(rng.integers(0, 256))
            if val == d[pos]:
                continue
            c = d[:pos] + bytes([val]) + d[pos + 1:]
            try:
                decode(c, pixels=False)
            except Corrupt:
                _corpus.append(("%s_byte%d_%02x" % (name, pos, val), c, d))
                kept += 1
            else:
                _altered.append(("%s_altered%d_%02x" % (name, pos, val), c))
        _corpus.append((name + "_sparse_ac", sparse_ac_table(d), d))
    for name, c, _ in _corpus:                     # every member is one the reference refuses (the cuts inside the header: cannot read)
        try:
            decode(c, pixels=False)
        except (Corrupt, IndexError, ValueError, KeyError):
            continue
        raise AssertionError("%s is no corrupt file: the restatement decodes it" % name)
    return _corpus


_altered_images = {}


def altered_files():
    """[(name, file bytes, image)]: the single-byte overwrites drawn for the corpus that leave a stream the restatement decodes
    (changed magnitude bits, codes that fall back into step before the last MCU).  No decoder can refuse them; the expectation is
    the restatement's own image (libjpeg's where the coefficients stay in the range an encoder produces; beyond it the 32-bit
    wrap-around and the int16 workspace of the library's contract, which the restatement follows)."""
    corrupt_corpus()
    for name, c in _altered:
        if name not in _altered_images:
            _altered_images[name] = decode(c)[0]
    return [(name, c, _altered_images[name]) for name, c in _altered]
