// Baseline JPEG decoding, the host side: the marker parser and the table builder behind w2l_jpeg_parse / w2l_jpeg_build_tables.
// Plain C++ with no HIP type, shared by csrc/jpeg_decode.hip and tools/jpeg_decode_host.cpp.  Errors are a reason code plus a
// text in the caller's buffer.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../include/w2l_hip.h"
#include "jpeg_decode_core.h"

namespace w2l {
namespace jd {

struct ErrText {
    char text[160];
    int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
        return code;
    }
};

// Walks the markers of one file (T.81 B.2).  Every index is checked against n before the byte is read.  restart_interval NULL:
// the class of w2l_jpeg_parse, a DRI above 0 is refused; otherwise the class of w2l_jpeg_parse_rst: DRI's value goes there (0: none)
// and, where it is above 0, RSTn markers inside the scan are passed over (w2l_jpeg_restart_segments checks their count and order).
inline int parse(const uint8_t* d, size_t n, w2l_jpeg_info* info, ErrText& err, int* restart_interval = nullptr) {
    memset(info, 0, sizeof(*info));
    if (restart_interval) *restart_interval = 0;
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return err.fail(W2L_JPEG_MALFORMED, "jpeg: no SOI marker (not a JPEG file)");
    bool have_q[4] = {false, false, false, false}, have_h[2][4] = {{false, false, false, false}, {false, false, false, false}};
    uint8_t q[4][64], hbits[2][4][16], hvals[2][4][256];
    int hn[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    bool have_sof = false, jfif = false;
    int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    size_t i = 2;
    for (;;) {
        if (i + 2 > n) return err.fail(W2L_JPEG_MALFORMED, "jpeg: the file ends inside its header (at byte %zu)", i);
        if (d[i] != 0xFF) return err.fail(W2L_JPEG_MALFORMED, "jpeg: byte %zu is no marker", i);
        const int m = d[i + 1];
        if (m == 0xFF) {                       // a fill byte in front of a marker
            ++i;
            continue;
        }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0x00)
            return err.fail(W2L_JPEG_MALFORMED, "jpeg: marker FF %02X in the header", m);
        if (m == 0xD9) return err.fail(W2L_JPEG_MALFORMED, "jpeg: EOI before any scan");
        if (i + 4 > n) return err.fail(W2L_JPEG_MALFORMED, "jpeg: the file ends inside its header (at byte %zu)", i);
        const size_t len = ((size_t)d[i + 2] << 8) | d[i + 3];
        if (len < 2 || i + 2 + len > n)
            return err.fail(W2L_JPEG_MALFORMED, "jpeg: segment FF %02X at byte %zu claims %zu bytes, the file has %zu", m, i, len, n - i - 2);
        const uint8_t* s = d + i + 4;
        const size_t sl = len - 2;
        if (m == 0xC0) {
            if (have_sof) return err.fail(W2L_JPEG_MALFORMED, "jpeg: two SOF segments");
            if (sl < 6) return err.fail(W2L_JPEG_MALFORMED, "jpeg: short SOF0 segment");
            if (s[0] != 8) return err.fail(W2L_JPEG_PRECISION, "jpeg: %d-bit samples (8-bit only)", s[0]);
            info->H = (s[1] << 8) | s[2];
            info->W = (s[3] << 8) | s[4];
            if (info->H == 0 || info->W == 0) return err.fail(W2L_JPEG_SIZE, "jpeg: size %d x %d", info->H, info->W);
            if (s[5] != 3) return err.fail(W2L_JPEG_COMPONENTS, "jpeg: %d components (three only: no grayscale, no CMYK)", s[5]);
            if (sl != 6 + 9) return err.fail(W2L_JPEG_MALFORMED, "jpeg: SOF0 of %zu bytes for three components", sl);
            for (int c = 0; c < 3; ++c) {
                comp_id[c] = s[6 + 3 * c];
                const int hv = s[7 + 3 * c];
                if (hv != (c == 0 ? 0x22 : 0x11))
                    return err.fail(W2L_JPEG_SAMPLING, "jpeg: component %d is sampled %dx%d (4:2:0 only: 2x2, 1x1, 1x1)", c, hv >> 4, hv & 15);
                comp_tq[c] = s[8 + 3 * c];
                if (comp_tq[c] > 3) return err.fail(W2L_JPEG_TABLES, "jpeg: quantisation table id %d", comp_tq[c]);
            }
            if (comp_tq[1] != comp_tq[2]) return err.fail(W2L_JPEG_TABLES, "jpeg: Cb and Cr use different quantisation tables");
            have_sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return err.fail(W2L_JPEG_NOT_BASELINE, "jpeg: SOF%d (%s); baseline SOF0 only", m - 0xC0,
                            m == 0xC2 ? "progressive" : (m == 0xC1 ? "extended sequential" : "not baseline"));
        } else if (m == 0xCC) {
            return err.fail(W2L_JPEG_NOT_BASELINE, "jpeg: arithmetic coding conditioning (DAC)");
        } else if (m == 0xDB) {
            size_t o = 0;
            while (o < sl) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq != 0) return err.fail(W2L_JPEG_QUANT16, "jpeg: a 16-bit quantisation table (Pq = %d)", pq);
                if (tq > 3) return err.fail(W2L_JPEG_TABLES, "jpeg: quantisation table id %d", tq);
                if (o + 65 > sl) return err.fail(W2L_JPEG_MALFORMED, "jpeg: short DQT segment");
                memcpy(q[tq], s + o + 1, 64);
                have_q[tq] = true;
                o += 65;
            }
        } else if (m == 0xC4) {
            size_t o = 0;
            while (o < sl) {
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return err.fail(W2L_JPEG_TABLES, "jpeg: Huffman table class %d id %d", tc, th);
                if (o + 17 > sl) return err.fail(W2L_JPEG_MALFORMED, "jpeg: short DHT segment");
                int cnt = 0;
                for (int k = 0; k < 16; ++k) cnt += s[o + 1 + k];
                if (cnt > 256 || o + 17 + (size_t)cnt > sl) return err.fail(W2L_JPEG_MALFORMED, "jpeg: DHT names %d symbols", cnt);
                memcpy(hbits[tc][th], s + o + 1, 16);
                memset(hvals[tc][th], 0, 256);
                memcpy(hvals[tc][th], s + o + 17, (size_t)cnt);
                hn[tc][th] = cnt;
                have_h[tc][th] = true;
                o += 17 + (size_t)cnt;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return err.fail(W2L_JPEG_MALFORMED, "jpeg: DRI segment of %zu bytes", sl);
            const int ri = (s[0] << 8) | s[1];
            if (ri != 0 && !restart_interval) return err.fail(W2L_JPEG_RESTART, "jpeg: restart interval %d", ri);
            if (restart_interval) *restart_interval = ri;
        } else if (m >= 0xE0 && m <= 0xEF) {
            const bool app0 = m == 0xE0 && sl >= 5 && (memcmp(s, "JFIF", 5) == 0 || memcmp(s, "JFXX", 5) == 0);
            if (app0 && s[2] == 'I') jfif = true;
            if (!app0) {
                if (m == 0xEE && sl >= 5 && memcmp(s, "Adobe", 5) == 0)
                    return err.fail(W2L_JPEG_APPN, "jpeg: an Adobe APP14 segment (its colour transform flag is not handled)");
                return err.fail(W2L_JPEG_APPN, "jpeg: an APP%d segment that is not JFIF", m - 0xE0);
            }
        } else if (m == 0xDA) {
            if (!have_sof) return err.fail(W2L_JPEG_MALFORMED, "jpeg: SOS before SOF");
            // without a JFIF segment libjpeg guesses the colour space from the component ids: 'R' 'G' 'B' is RGB, not YCbCr
            if (!jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
                return err.fail(W2L_JPEG_COLORSPACE, "jpeg: components 'R' 'G' 'B' without a JFIF segment (an RGB file, not YCbCr)");
            if (sl < 1) return err.fail(W2L_JPEG_MALFORMED, "jpeg: short SOS segment");
            if (s[0] != 3) return err.fail(W2L_JPEG_SCANS, "jpeg: a scan of %d components (one interleaved scan of all three only)", s[0]);
            if (sl != 1 + 6 + 3) return err.fail(W2L_JPEG_MALFORMED, "jpeg: SOS of %zu bytes for three components", sl);
            int td[3], ta[3];
            for (int c = 0; c < 3; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return err.fail(W2L_JPEG_SCANS, "jpeg: the scan names its components out of order");
                td[c] = s[2 + 2 * c] >> 4;
                ta[c] = s[2 + 2 * c] & 15;
                if (td[c] > 3 || ta[c] > 3) return err.fail(W2L_JPEG_TABLES, "jpeg: Huffman table id %d / %d", td[c], ta[c]);
            }
            if (s[7] != 0 || s[8] != 63 || s[9] != 0)
                return err.fail(W2L_JPEG_SCANS, "jpeg: scan with Ss = %d, Se = %d, Ah/Al = %02X (a sequential scan has 0, 63, 00)", s[7], s[8], s[9]);
            if (td[1] != td[2] || ta[1] != ta[2]) return err.fail(W2L_JPEG_TABLES, "jpeg: Cb and Cr use different Huffman tables");
            for (int t = 0; t < 2; ++t) {
                const int c = t;                                  // component 0: luma, component 1: chroma
                if (!have_q[comp_tq[c]] || !have_h[0][td[c]] || !have_h[1][ta[c]])
                    return err.fail(W2L_JPEG_MALFORMED, "jpeg: the scan names a table the file does not define");
                memcpy(info->quant[t], q[comp_tq[c]], 64);
                memcpy(info->bits[2 * t], hbits[0][td[c]], 16);
                memcpy(info->vals[2 * t], hvals[0][td[c]], 256);
                info->nvals[2 * t] = hn[0][td[c]];
                memcpy(info->bits[2 * t + 1], hbits[1][ta[c]], 16);
                memcpy(info->vals[2 * t + 1], hvals[1][ta[c]], 256);
                info->nvals[2 * t + 1] = hn[1][ta[c]];
            }
            i += 2 + len;
            break;
        }
        // DNL, COM, JPGn and the rest carry nothing the decoder needs
        i += 2 + len;
    }
    // the entropy-coded segment: up to the first marker that is not the stuffed FF 00
    const size_t start = i;
    if (start >= n) return err.fail(W2L_JPEG_MALFORMED, "jpeg: the file ends behind its SOS header");
    if (n - start > 0x7fffffffu) return err.fail(W2L_JPEG_MALFORMED, "jpeg: a scan of more than 2^31 bytes");
    size_t end = n;
    info->eoi = 0;
    while (i < n) {
        if (d[i] != 0xFF) {
            ++i;
            continue;
        }
        if (i + 1 >= n) break;                  // a lone FF at the end of the file: no EOI, the kernel meets it
        const int m = d[i + 1];
        if (m == 0x00) {
            i += 2;
        } else if (m == 0xD9) {
            end = i;
            info->eoi = 1;
            break;
        } else if (m >= 0xD0 && m <= 0xD7) {
            if (restart_interval && *restart_interval > 0) {
                i += 2;
                continue;
            }
            return err.fail(W2L_JPEG_MALFORMED, "jpeg: restart marker RST%d in a scan without restart interval", m - 0xD0);
        } else if (m == 0xFF) {
            ++i;
        } else {
            return err.fail(W2L_JPEG_SCANS, "jpeg: marker FF %02X behind the first scan (one scan only)", m);
        }
    }
    if (end == start) return err.fail(W2L_JPEG_MALFORMED, "jpeg: an empty scan");
    info->ecs_offset = (int32_t)start;
    info->ecs_bytes = (int32_t)(end - start);
    return 0;
}

// The restart intervals of one entropy-coded segment (T.81 B.2.1, E.1.4): interval k codes MCUs [k * ri, min((k + 1) * ri, n_mcus))
// and ends in front of the marker FF D0+(k mod 8); behind the last interval there is none.  A data byte FF is always followed by
// 00, so FF D0..D7 in the bytes IS a marker and one linear pass finds them all.  Writes at most `cap` records (row = 0) and
// returns the number of intervals, ceil(n_mcus / ri), or W2L_JPEG_MALFORMED: a marker too many or too few, one out of order, or
// any other marker.  ri = 0: one record, the whole segment (RSTn markers are then refused).  Never reads ecs[n] or beyond.
inline int restart_segments(const uint8_t* ecs, size_t n, int ri, int n_mcus, w2l_jpeg_segment* out, int cap, ErrText& err) {
    if (n < 1 || n > 0x7fffffffu || ri < 0 || ri > 65535 || n_mcus < 1 || cap < 0)
        return err.fail(W2L_JPEG_MALFORMED, "jpeg: restart_segments of %zu bytes, interval %d, %d MCUs", n, ri, n_mcus);
    const int expected = ri > 0 ? (n_mcus + ri - 1) / ri : 1;
    int k = 0;
    size_t start = 0, i = 0;
    auto emit = [&](size_t end) {
        if (k < cap) {
            w2l_jpeg_segment s;
            memset(&s, 0, sizeof(s));
            s.offset = (int32_t)start;
            s.nbytes = (int32_t)(end - start);
            s.first_mcu = ri > 0 ? k * ri : 0;
            s.n_mcus = ri > 0 && (k + 1) * ri < n_mcus ? ri : n_mcus - s.first_mcu;
            out[k] = s;
        }
    };
    while (i < n) {
        if (ecs[i] != 0xFF) {
            ++i;
            continue;
        }
        if (i + 1 >= n) break;                  // a lone FF at the end: part of the last interval, whose decoder refuses it
        const int m = ecs[i + 1];
        if (m == 0x00) {
            i += 2;
            continue;
        }
        if (m < 0xD0 || m > 0xD7) return err.fail(W2L_JPEG_MALFORMED, "jpeg: marker FF %02X at byte %zu of the scan", m, i);
        if (ri == 0) return err.fail(W2L_JPEG_MALFORMED, "jpeg: restart marker RST%d in a scan without restart interval", m - 0xD0);
        if (k >= expected - 1)
            return err.fail(W2L_JPEG_MALFORMED, "jpeg: more than the %d restart markers of %d MCUs at interval %d", expected - 1, n_mcus, ri);
        if (m - 0xD0 != (k & 7))
            return err.fail(W2L_JPEG_MALFORMED, "jpeg: restart marker %d is RST%d, not RST%d", k, m - 0xD0, k & 7);
        emit(i);
        ++k;
        i += 2;
        start = i;
    }
    if (k != expected - 1)
        return err.fail(W2L_JPEG_MALFORMED, "jpeg: %d restart markers where %d MCUs at interval %d have %d", k, n_mcus, ri, expected - 1);
    emit(n);
    return expected;
}

// (bits, vals) -> the lookup form. Canonical codes of T.81 Annex C; refuses what is no prefix code.
inline int build_huff(const uint8_t bits[16], const uint8_t* vals, int nvals, bool dc, HuffLookup& h, ErrText& err) {
    memset(&h, 0, sizeof(h));
    int total = 0;
    for (int l = 0; l < 16; ++l) total += bits[l];
    if (total != nvals || total > 256 || total < 1) return err.fail(W2L_JPEG_MALFORMED, "jpeg: a Huffman table of %d codes for %d symbols", total, nvals);
    bool seen[256];
    memset(seen, 0, sizeof(seen));
    for (int k = 0; k < total; ++k) {
        if (seen[vals[k]]) return err.fail(W2L_JPEG_MALFORMED, "jpeg: Huffman symbol %02X is listed twice", vals[k]);
        seen[vals[k]] = true;
        if (dc && vals[k] > 11) return err.fail(W2L_JPEG_MALFORMED, "jpeg: DC category %d (8-bit baseline has 0..11)", vals[k]);
        h.vals[k] = vals[k];
    }
    for (int l = 0; l < 18; ++l) h.maxcode[l] = -1;
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = bits[l - 1];
        // codes of length l are code .. code + cnt - 1 and must fit l bits: otherwise the lengths oversubscribe the code space
        if (code + (unsigned)cnt > (1u << l)) return err.fail(W2L_JPEG_MALFORMED, "jpeg: Huffman code lengths oversubscribe the code space at %d bits", l);
        if (cnt) {
            h.valoff[l] = k - (int)code;
            h.maxcode[l] = (int)code + cnt - 1;
            if (l <= kLookBits) {
                for (int c = 0; c < cnt; ++c) {
                    const unsigned first = (code + (unsigned)c) << (kLookBits - l);
                    for (unsigned f = 0; f < (1u << (kLookBits - l)); ++f) h.look[first + f] = (uint16_t)((l << 8) | vals[k + c]);
                }
            }
        }
        code = (code + (unsigned)cnt) << 1;
        k += cnt;
    }
    return 0;
}

inline int build_tables(const w2l_jpeg_info* info, TableSet& t, ErrText& err) {
    memset(&t, 0, sizeof(t));
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) {
            if (info->quant[c][k] == 0) return err.fail(W2L_JPEG_MALFORMED, "jpeg: a quantiser of 0");
            t.quant[c][k] = info->quant[c][k];
        }
    for (int j = 0; j < 4; ++j) {
        if (info->nvals[j] < 0 || info->nvals[j] > 256) return err.fail(W2L_JPEG_MALFORMED, "jpeg: a Huffman table of %d symbols", info->nvals[j]);
        const int rc = build_huff(info->bits[j], info->vals[j], info->nvals[j], (j & 1) == 0, t.huff[j], err);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace jd
}  // namespace w2l
