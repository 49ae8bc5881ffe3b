// Baseline JPEG decoding, the arithmetic: the per-file entropy routine and the per-block / per-pixel rules, with no HIP type in
// them, so that the same text is the device code of csrc/jpeg_decode.hip and the plain host C++ of tools/jpeg_decode_host.cpp
// (which runs it under the host sanitizers).  Every rule is libjpeg's published algorithm, restated: jdhuff.c decode_mcu (T.81
// F.2.2), jidctint.c jpeg_idct_islow, jdsample.c h2v2_fancy_upsample over the real chroma plane, jdcolor.c ycc_rgb_convert.
// Integer work only: the pixels are a function of the file's bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define W2L_JD_FN __host__ __device__ __forceinline__
#else
#define W2L_JD_FN inline
#endif

namespace w2l {
namespace jd {

// reason codes of a row (status[b]); 0: the image is complete
enum {
    kOk = 0,
    kBadCode = -1,      // bits that are no code of the table
    kRunPast63 = -2,    // a zero run that leaves the block
    kMarker = -3,       // a marker (anything but the stuffed FF 00) or bytes left over where the last MCU should end
    kEndedEarly = -4,   // the stream ended before the last MCU
    kBadRow = -5        // a size of 0 or above 65535, more blocks than max_blocks, no bytes, or a table index outside the launch
};

constexpr int kLookBits = 9;

// one Huffman table in the form the decoder reads (T.81 F.2.2.3 with a lookahead in front): look[first 9 bits] = length << 8 |
// symbol for codes of up to 9 bits, 0 otherwise; longer codes: the first length l with code <= maxcode[l] (-1: no code of that
// length), symbol vals[code + valoff[l]]
struct alignas(16) HuffLookup {
    uint16_t look[1 << kLookBits];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t vals[256];
};
// what one file's tables become: quantisers in zigzag order (as the DQT segment carries them), [0] luma, [1] chroma; Huffman
// tables DC luma, AC luma, DC chroma, AC chroma
struct alignas(16) TableSet {
    uint16_t quant[2][64];
    HuffLookup huff[4];
};
static_assert(sizeof(HuffLookup) == 1424 && sizeof(TableSet) == 5952, "the table set's layout is part of the ABI");

W2L_JD_FN int natural_of(int k) {     // zigzag position -> row-major index (T.81 figure A.6)
    constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k & 63];
}

// MCUs of 16x16 pixels in raster order, six blocks each (Y00 Y01 Y10 Y11 Cb Cr)
struct Geom {
    int mw, mh, nblocks;
    int cw, ch;                 // the real chroma plane: ceil(W / 2) x ceil(H / 2) samples
};
W2L_JD_FN bool geom_of(int H, int W, int max_blocks, Geom& g) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) return false;
    g.mw = (W + 15) >> 4;
    g.mh = (H + 15) >> 4;
    g.cw = (W + 1) >> 1;
    g.ch = (H + 1) >> 1;
    const long long n = 6ll * g.mw * g.mh;
    if (n > max_blocks) return false;
    g.nblocks = (int)n;
    return true;
}

// The bit reader.  Every read of the stream is bounded by n.  FF 00 is the byte FF; FF followed by anything else, or by nothing, is
// a marker: loading stops there for good.  Behind the last real byte the reader appends zero bits (`virt` counts them), so that a
// lookahead may run over the end; CONSUMING one of them is the error (`overrun`).
struct BitReader {
    const uint8_t* p;
    int n, pos;
    uint64_t acc;
    int nb, virt;
    bool marker;
    W2L_JD_FN void begin(const uint8_t* data, int nbytes) {
        p = data;
        n = nbytes;
        pos = 0;
        acc = 0;
        nb = 0;
        virt = 0;
        marker = false;
    }
    W2L_JD_FN void refill() {          // afterwards nb >= 57
        while (nb <= 56) {
            unsigned b = 0;
            if (!marker && pos < n) {
                b = p[pos];
                if (b == 0xFF) {
                    if (pos + 1 < n && p[pos + 1] == 0) {
                        pos += 2;
                    } else {
                        marker = true;
                        continue;
                    }
                } else {
                    ++pos;
                }
            } else {
                virt += 8;
            }
            acc = (acc << 8) | b;
            nb += 8;
        }
    }
    W2L_JD_FN unsigned peek(int k) const { return (unsigned)(acc >> (nb - k)) & ((1u << k) - 1u); }   // 1 <= k <= 16 <= nb
    W2L_JD_FN void skip(int k) { nb -= k; }
    W2L_JD_FN bool overrun() const { return nb < virt; }
    // the reason a block is refused: where bits behind the end were consumed, the end is the cause, whatever they decoded to
    W2L_JD_FN int why(int code) const { return overrun() ? (marker ? kMarker : kEndedEarly) : code; }
    // after the last MCU: every byte was loaded, and less than one byte of it (the padding) is unread
    W2L_JD_FN int finish() {
        refill();
        if (overrun()) return why(kOk);
        if (marker || pos != n || nb - virt >= 8) return kMarker;
        return kOk;
    }
};

// one symbol, or -1 where the next bits are no code of the table (T.81 F.2.2.3); needs nb >= 16
W2L_JD_FN int huff_symbol(BitReader& br, const HuffLookup& h) {
    const unsigned v = br.peek(16);
    const unsigned e = h.look[v >> (16 - kLookBits)];
    if (e) {
        br.skip((int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (code <= h.maxcode[l]) {
            br.skip(l);
            return h.vals[(code + h.valoff[l]) & 255];
        }
    }
    return -1;
}

W2L_JD_FN int extend(int r, int s) { return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r; }     // T.81 F.2.2.1, s >= 1
W2L_JD_FN int16_t to_i16(long long v) { return (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// MCUs [first_mcu, first_mcu + n_mcus) of one file from the bytes that code exactly them (jdhuff.c decode_mcu for an interleaved
// 4:2:0 scan): the whole entropy-coded segment of a file without restarts, or ONE restart interval - jdhuff.c process_restart puts
// the three DC predictions back to 0 and starts at a byte boundary, which is how this routine begins.  Dequantised coefficients in
// row-major order into coef[nblocks][64] (the file's first block, not the range's), which the caller has ZEROED - only non-zero
// values are written, each at an index < 64 of a block of the range.  Returns kOk or the reason the bytes are refused (kBadRow for
// a range outside the file); what was written until then stays.
W2L_JD_FN int decode_mcus(const uint8_t* data, int nbytes, const Geom& g, const TableSet& t, int16_t* coef, int first_mcu, int n_mcus) {
    if (nbytes < 1 || first_mcu < 0 || n_mcus < 1 || n_mcus > g.nblocks / 6 - first_mcu) return kBadRow;
    BitReader br;
    br.begin(data, nbytes);
    int pred[3] = {0, 0, 0};
    const int id_end = 6 * (first_mcu + n_mcus);
    for (int id = 6 * first_mcu; id < id_end; ++id) {
        const int k6 = id % 6;
        const int c = k6 < 4 ? 0 : k6 - 3, tq = k6 < 4 ? 0 : 1;
        const HuffLookup& hdc = t.huff[2 * tq];
        const HuffLookup& hac = t.huff[2 * tq + 1];
        const uint16_t* q = t.quant[tq];
        int16_t* blk = coef + (long long)id * 64;
        br.refill();
        int s = huff_symbol(br, hdc);
        if (s < 0 || s > 11) return br.why(kBadCode);
        if (s) {
            const int r = (int)br.peek(s);
            br.skip(s);
            pred[c] += extend(r, s);
        }
        const long long dc = (long long)pred[c] * q[0];      // |pred| < 2^20 blocks x 2^11
        if (dc) blk[0] = to_i16(dc);
        for (int k = 1; k < 64; ++k) {
            br.refill();
            const int rs = huff_symbol(br, hac);
            if (rs < 0) return br.why(kBadCode);
            const int run = rs >> 4;
            s = rs & 15;
            if (s) {
                k += run;
                if (k > 63) return br.why(kRunPast63);
                const int r = (int)br.peek(s);
                br.skip(s);
                const long long v = (long long)extend(r, s) * q[k];
                if (v) blk[natural_of(k)] = to_i16(v);
            } else {
                if (run != 15) break;          // EOB (libjpeg takes every run < 15 with size 0 as one)
                k += 15;
                if (k > 63) return br.why(kRunPast63);
            }
        }
        if (br.overrun()) return br.why(kOk);
    }
    return br.finish();
}

// The entropy-coded segment of one file without restarts: every MCU from one stream
W2L_JD_FN int decode_scan(const uint8_t* data, int nbytes, const Geom& g, const TableSet& t, int16_t* coef) {
    return decode_mcus(data, nbytes, g, t, coef, 0, g.nblocks / 6);
}

// ---- pixels

// jpeg_idct_islow, one dimension (CONST_BITS 13, PASS1_BITS 2): the column pass descales by 11, the row pass by 18.  libjpeg's
// shortcut for a column or row whose AC terms are all zero gives the same values, so there is no branch.
W2L_JD_FN void idct8(int d[8], int shift) {
    // unsigned arithmetic: the same bits as libjpeg's for every file an encoder writes, and wrap-around instead of undefined
    // behaviour for coefficients no encoder produces
    typedef uint32_t U;
    U z2 = (U)d[2], z3 = (U)d[6];
    U z1 = (z2 + z3) * 4433u;
    U tmp2 = z1 - z3 * 15137u;
    U tmp3 = z1 + z2 * 6270u;
    z2 = (U)d[0];
    z3 = (U)d[4];
    U tmp0 = (z2 + z3) * 8192u;
    U tmp1 = (z2 - z3) * 8192u;
    const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = (U)d[7];
    tmp1 = (U)d[5];
    tmp2 = (U)d[3];
    tmp3 = (U)d[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    U z4 = tmp1 + tmp3;
    const U z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u;
    tmp1 *= 16819u;
    tmp2 *= 25172u;
    tmp3 *= 12299u;
    z1 = 0u - z1 * 7373u;
    z2 = 0u - z2 * 20995u;
    z3 = z5 - z3 * 16069u;
    z4 = z5 - z4 * 3196u;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const U rnd = 1u << (shift - 1);
    d[0] = (int)(tmp10 + tmp3 + rnd) >> shift;
    d[7] = (int)(tmp10 - tmp3 + rnd) >> shift;
    d[1] = (int)(tmp11 + tmp2 + rnd) >> shift;
    d[6] = (int)(tmp11 - tmp2 + rnd) >> shift;
    d[2] = (int)(tmp12 + tmp1 + rnd) >> shift;
    d[5] = (int)(tmp12 - tmp1 + rnd) >> shift;
    d[3] = (int)(tmp13 + tmp0 + rnd) >> shift;
    d[4] = (int)(tmp13 - tmp0 + rnd) >> shift;
}

// libjpeg's range-limit table behind the IDCT (jdmaster.c prepare_range_limit_table), indexed with (v & 1023): v is the sample
// minus 128.  [0,128) -> v + 128, [128,512) -> 255, [512,896) -> 0, [896,1024) (v in [-128,0)) -> v + 128
W2L_JD_FN uint8_t range_limit(int v) {
    const int i = v & 1023;
    return (uint8_t)(i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896)));
}

// one block, both passes (columns first): coef[64] row-major -> out[64] row-major samples
W2L_JD_FN void idct_block(const int16_t* coef, uint8_t* out) {
    int ws[64];
    for (int c = 0; c < 8; ++c) {
        int d[8];
        for (int r = 0; r < 8; ++r) d[r] = coef[r * 8 + c];
        idct8(d, 11);
        for (int r = 0; r < 8; ++r) ws[r * 8 + c] = d[r];
    }
    for (int r = 0; r < 8; ++r) {
        int d[8];
        for (int c = 0; c < 8; ++c) d[c] = ws[r * 8 + c];
        idct8(d, 18);
        for (int c = 0; c < 8; ++c) out[r * 8 + c] = range_limit(d[c]);
    }
}

// where block `id` of a file lies in its sample planes: Y [16 mh][16 mw], then Cb and Cr [8 mh][8 mw] each (64 bytes per block
// in all); returns the offset of the block's first sample and its plane's pitch
W2L_JD_FN long long block_origin(const Geom& g, int id, int& pitch) {
    const int mcu = id / 6, k = id - mcu * 6;
    const int my = mcu / g.mw, mx = mcu - my * g.mw;
    const long long ysize = 256ll * g.mw * g.mh;
    if (k < 4) {
        pitch = 16 * g.mw;
        return (long long)(16 * my + 8 * (k >> 1)) * pitch + 16 * mx + 8 * (k & 1);
    }
    pitch = 8 * g.mw;
    return ysize + (k - 4) * (ysize >> 2) + (long long)(8 * my) * pitch + 8 * mx;
}

// One chroma plane at output pixel (y, x), as jdsample.c jinit_upsampler chooses: h2v2_fancy_upsample where the real plane is more
// than 2 samples wide - vertically 3 * near + far, the far row clamped to the real plane; horizontally (3 * this + left + 8) >> 4
// on even columns and (3 * this + right + 7) >> 4 on odd ones, the neighbour clamped to the real plane's first and last column -
// and plain h2v2_upsample, the sample repeated 2x2 with no blending in either direction, for an image of 1 to 4 columns
W2L_JD_FN int upsample_at(const uint8_t* plane, int pitch, const Geom& g, int y, int x) {
    const int cy = y >> 1, cx = x >> 1;
    if (g.cw <= 2) return plane[(long long)cy * pitch + cx];
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : (fy > g.ch - 1 ? g.ch - 1 : fy);
    int nx = (x & 1) ? cx + 1 : cx - 1;
    nx = nx < 0 ? 0 : (nx > g.cw - 1 ? g.cw - 1 : nx);
    const uint8_t* near = plane + (long long)cy * pitch;
    const uint8_t* far = plane + (long long)fy * pitch;
    const int cur = 3 * near[cx] + far[cx], nei = 3 * near[nx] + far[nx];
    return (3 * cur + nei + ((x & 1) ? 7 : 8)) >> 4;
}

W2L_JD_FN uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// pixel (y, x) of the image from the three sample planes of block_origin's layout, in BGR order (ycc_rgb_convert)
W2L_JD_FN void pixel_bgr(const uint8_t* planes, const Geom& g, int y, int x, uint8_t* bgr) {
    const long long ysize = 256ll * g.mw * g.mh;
    const int Y = planes[(long long)y * (16 * g.mw) + x];
    const int cb = upsample_at(planes + ysize, 8 * g.mw, g, y, x) - 128;
    const int cr = upsample_at(planes + ysize + (ysize >> 2), 8 * g.mw, g, y, x) - 128;
    bgr[0] = clamp_u8(Y + ((116130 * cb + 32768) >> 16));
    bgr[1] = clamp_u8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    bgr[2] = clamp_u8(Y + ((91881 * cr + 32768) >> 16));
}

}  // namespace jd
}  // namespace w2l
