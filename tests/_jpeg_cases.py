"""Case images for the JPEG encoder and a numpy restatement of what libjpeg does for `PIL.Image.save(format="JPEG", quality=q,
subsampling=2)`, with counters of the code paths an image takes.  The expectation of every test is PIL's own bytes; the
restatement exists so that the case set can be shown to reach every path (a ZRL, a stuffed byte, dummy blocks, ...), and it is
itself held to PIL's bytes in test_jpeg_cpu.py.  Test infrastructure only: nothing in the package imports it.

The restatement takes its quantisation and Huffman tables out of the header PIL writes (it restates the pixel and entropy rules,
not the tables; `wav2lip_amd.jpeg.header` is compared with PIL's header on its own)."""
import io

import numpy as np

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
      56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

SIZES = [(1, 1), (2, 2), (3, 5), (8, 8), (7, 9), (9, 7), (16, 16), (17, 15), (15, 17), (24, 8), (8, 24), (33, 16), (16, 33), (37, 53),
         (40, 40), (49, 63), (81, 107), (96, 96), (160, 160)]
CONTENTS = ["noise", "gradient", "flat", "checker", "redblue"]
SUBSET = [(1, 1), (8, 8), (17, 15), (24, 8), (37, 53), (81, 107)]       # the sizes that also run at the other qualities
OTHER_Q = [30, 75, 100]


def image(content, h, w, seed=0):
    """uint8 [h,w,3] BGR"""
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "noise":
        return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "gradient":
        return np.stack([(yy * 3 + xx) % 256, (xx * 5) % 256, (yy * 2 + xx * 2) % 256], -1).astype(np.uint8)
    if content == "flat":
        return np.full((h, w, 3), 200, np.uint8)
    if content == "checker":
        return (((yy + xx) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    if content == "redblue":                     # saturated red / blue in 8x8 tiles: the largest chroma and DC steps
        red = ((yy // 8 + xx // 8) % 2).astype(bool)
        out = np.zeros((h, w, 3), np.uint8)
        out[..., 2] = np.where(red, 255, 0)
        out[..., 0] = np.where(red, 0, 255)
        return out
    raise ValueError(content)


def cases():
    """[(name, bgr image, quality)]: every size and content at quality 95, the subset at 30, 75 and 100, and the largest noise
    image at 30 (many zero runs)"""
    out = [("%s_%dx%d_q95" % (c, h, w), image(c, h, w), 95) for (h, w) in SIZES for c in CONTENTS]
    out += [("%s_%dx%d_q%d" % (c, h, w, q), image(c, h, w), q) for q in OTHER_Q for (h, w) in SUBSET for c in CONTENTS]
    out.append(("noise_160x160_q30", image("noise", 160, 160), 30))
    return out


def turbo():
    """PIL is linked against libjpeg-turbo (whose arithmetic the rules restate)"""
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


def pil_bytes(bgr, q=95):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(b, format="JPEG", quality=q, subsampling=2)
    return b.getvalue()


_expected = {}


def expected(name, bgr, q):
    """PIL's bytes of a case, computed once per process"""
    if name not in _expected:
        _expected[name] = pil_bytes(bgr, q)
    return _expected[name]


def parse_header(d):
    """(header bytes, {table id: quantisers in zigzag order}, {class << 4 | id: (bits, vals)}) of a JFIF file"""
    i, dqt, dht = 2, {}, {}
    while True:
        m, n = d[i + 1], int.from_bytes(d[i + 2:i + 4], "big")
        seg = d[i + 4:i + 2 + n]
        if m == 0xDB:
            dqt[seg[0] & 15] = np.array(list(seg[1:65]))
        if m == 0xC4:
            bits = list(seg[1:17])
            dht[seg[0]] = (bits, list(seg[17:17 + sum(bits)]))
        i += 2 + n
        if m == 0xDA:
            return d[:i], dqt, dht


def huff(bits, vals):
    code, k, t = 0, 0, {}
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            t[vals[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    return t


def fdct(b):
    """libjpeg's jpeg_fdct_islow on [..., 8, 8] blocks: rows first, then columns"""
    def one(d, first):
        d = [d[..., k] for k in range(8)]
        t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
        t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2

        def ds(x, n):
            return (x + (1 << (n - 1))) >> n
        o = [None] * 8
        if first:
            o[0], o[4], n = (t10 + t11) << 2, (t10 - t11) << 2, 11
        else:
            o[0], o[4], n = ds(t10 + t11, 2), ds(t10 - t11, 2), 15
        z1 = (t12 + t13) * 4433
        o[2], o[6] = ds(z1 + t13 * 6270, n), ds(z1 - t12 * 15137, n)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
        z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
        o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, n), ds(t5 + z2 + z4, n), ds(t6 + z2 + z3, n), ds(t7 + z1 + z4, n)
        return np.stack(o, -1)
    r = one(b.astype(np.int64), True)
    return one(r.swapaxes(-1, -2), False).swapaxes(-1, -2)


def encode(bgr, q=95):
    """(file bytes, counters) of the rules applied to a uint8 [H,W,3] BGR image"""
    H, W, _ = bgr.shape
    hdr, dqt, dht = parse_header(pil_bytes(bgr, q))
    b, g, r = [bgr[..., k].astype(np.int64) for k in range(3)]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16

    def pad(a):
        return np.pad(a, ((0, Hp - H), (0, Wp - W)), mode="edge")
    y, cb, cr = pad(y), pad(cb), pad(cr)

    def down(a):
        s = a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
        bias = np.tile(np.array([1, 2]), s.shape[1] // 2 + 1)[:s.shape[1]]
        return (s + bias[None, :]) >> 2
    He = H + (H & 1)                 # rows are padded to an even height BEFORE downsampling, to the MCU height AFTER it

    def fix(c):
        return np.pad(down(c[:He]), ((0, (Hp - He) // 2), (0, 0)), mode="edge")
    cb, cr = fix(cb), fix(cr)

    def blocks(a, qt):
        h, w = a.shape
        bl = (a - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
        co = fdct(bl).reshape(h // 8, w // 8, 64)
        qn = np.zeros(64, np.int64)
        qn[ZZ] = qt
        qn = qn * 8                                              # natural-order divisors
        return (np.sign(co) * ((np.abs(co) + (qn >> 1)) // qn))[..., ZZ]
    Y, CB, CR = blocks(y, dqt[0]), blocks(cb, dqt[1]), blocks(cr, dqt[1])
    hd = [huff(*dht[0x00]), huff(*dht[0x01])]
    ha = [huff(*dht[0x10]), huff(*dht[0x11])]
    cnt = dict(zrl=0, stuffed=0, dummy_right=0, dummy_bottom=0, eob_only=0, coef63=0, dc_cat=0, ac_cat=0, blocks=0)
    st = dict(acc=0, nb=0)
    out = bytearray()

    def put(code, n):
        st["acc"] = (st["acc"] << n) | code
        st["nb"] += n
        while st["nb"] >= 8:
            byte = (st["acc"] >> (st["nb"] - 8)) & 255
            out.append(byte)
            if byte == 255:
                out.append(0)
                cnt["stuffed"] += 1
            st["nb"] -= 8
        st["acc"] &= (1 << st["nb"]) - 1

    def mag(v):
        n = abs(v).bit_length()
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)

    def enc(blk, pred, tbl):
        cnt["blocks"] += 1
        n, bits = mag(int(blk[0]) - pred)
        cnt["dc_cat"] = max(cnt["dc_cat"], n)
        put(*hd[tbl][n])
        if n:
            put(bits, n)
        run = 0
        for k in range(1, 64):
            v = int(blk[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(*ha[tbl][0xF0])
                cnt["zrl"] += 1
                run -= 16
            n, bits = mag(v)
            cnt["ac_cat"] = max(cnt["ac_cat"], n)
            put(*ha[tbl][(run << 4) | n])
            put(bits, n)
            run = 0
        if run:
            put(*ha[tbl][0])
        cnt["eob_only"] += run == 63
        cnt["coef63"] += int(blk[63]) != 0
        return int(blk[0])
    p = [0, 0, 0]
    for my in range(Hp // 16):
        for mx in range(Wp // 16):
            mcu = []
            for dy in (0, 1):
                for dx in (0, 1):
                    by, bx = 2 * my + dy, 2 * mx + dx
                    if by < -(-H // 8) and bx < -(-W // 8):
                        blk = Y[by, bx]
                    else:                  # libjpeg's dummy block: AC zero, DC of the previous block of the MCU
                        blk = np.zeros(64, np.int64)
                        blk[0] = mcu[-1][0]
                        cnt["dummy_bottom" if by >= -(-H // 8) else "dummy_right"] += 1
                    mcu.append(blk)
            for blk in mcu:
                p[0] = enc(blk, p[0], 0)
            p[1] = enc(CB[my, mx], p[1], 1)
            p[2] = enc(CR[my, mx], p[2], 1)
    if st["nb"]:
        put((1 << (8 - st["nb"])) - 1, 8 - st["nb"])
    return bytes(hdr) + bytes(out) + b"\xff\xd9", cnt
