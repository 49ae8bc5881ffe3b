// The segment form of the JPEG decoder as a stand-alone HOST program: w2l_jpeg_parse_rst's parser, w2l_jpeg_restart_segments'
// marker scan and jd::decode_mcus - the very text the device kernel jpeg_segment_decode_kernel is compiled from - applied the way
// w2l_jpeg_decode_rows_rst applies them (one call per segment, the row's reason the minimum over its segments), around a main of
// their own, so that they can run under the host sanitizers:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_segments_host.cpp -o jpeg_segments_host
//     ./jpeg_segments_host MANIFEST
//
// MANIFEST as for tools/jpeg_decode_host.cpp: `valid FILE.jpg EXPECTED.npy` (uint8 [H,W,3] BGR, must be equalled byte for byte) or
// `corrupt FILE.jpg -` (must be refused; nothing may crash).  The file, its scan and EVERY SEGMENT are copied into buffers of
// their exact sizes, so that a read past one is a sanitizer report.  tests/test_mjpeg_cpu.py writes the files and the manifest,
// builds and runs this.  Exit status 0: every line held.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../wav2lip_amd/csrc/jpeg_decode_host.h"

using namespace w2l;

static bool read_file(const std::string& path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n >= 0 && fread(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    return ok;
}

// the array of a version 1 / 2 .npy file holding uint8 [H, W, 3] in C order
static bool read_npy(const std::string& path, int& H, int& W, std::vector<uint8_t>& px) {
    std::vector<uint8_t> raw;
    if (!read_file(path, raw) || raw.size() < 12 || memcmp(raw.data(), "\x93NUMPY", 6) != 0) return false;
    const size_t hl = raw[6] == 1 ? (size_t)raw[8] | ((size_t)raw[9] << 8)
                                  : (size_t)raw[8] | ((size_t)raw[9] << 8) | ((size_t)raw[10] << 16) | ((size_t)raw[11] << 24);
    const size_t off = (raw[6] == 1 ? 10 : 12) + hl;
    if (off > raw.size()) return false;
    const std::string hdr(raw.begin() + (raw[6] == 1 ? 10 : 12), raw.begin() + off);
    if (hdr.find("'|u1'") == std::string::npos || hdr.find("'fortran_order': False") == std::string::npos) return false;
    const size_t s = hdr.find("'shape': (");
    int c = 0;
    if (s == std::string::npos || sscanf(hdr.c_str() + s + 10, "%d, %d, %d", &H, &W, &c) != 3 || c != 3) return false;
    if (raw.size() - off != (size_t)H * W * 3) return false;
    px.assign(raw.begin() + off, raw.end());
    return true;
}

// 0 and the image, or the reason (a parser / scan / builder code below -99, or the entropy routine's -1 .. -5) and its text
static int decode(const std::vector<uint8_t>& file, int& H, int& W, std::vector<uint8_t>& bgr, std::string& why, int& n_segments) {
    uint8_t* data = (uint8_t*)malloc(file.size() ? file.size() : 1);
    memcpy(data, file.data(), file.size());
    w2l_jpeg_info info;
    jd::ErrText err;
    int ri = 0;
    int rc = jd::parse(data, file.size(), &info, err, &ri);
    jd::TableSet* t = new jd::TableSet;
    if (rc == 0) rc = jd::build_tables(&info, *t, err);
    jd::Geom g;
    if (rc == 0 && !jd::geom_of(info.H, info.W, 1 << 20, g)) rc = err.fail(jd::kBadRow, "more than 2^20 blocks");
    std::vector<w2l_jpeg_segment> segs;
    uint8_t* ecs = nullptr;
    if (rc == 0) {
        H = info.H;
        W = info.W;
        ecs = (uint8_t*)malloc((size_t)info.ecs_bytes);            // the scan alone, at its exact size
        memcpy(ecs, data + info.ecs_offset, (size_t)info.ecs_bytes);
        const int n_mcus = g.nblocks / 6;
        segs.resize(ri > 0 ? (size_t)((n_mcus + ri - 1) / ri) : 1);
        const int n = jd::restart_segments(ecs, (size_t)info.ecs_bytes, ri, n_mcus, segs.data(), (int)segs.size(), err);
        if (n < 0) rc = n;
    }
    free(data);
    if (rc != 0) {
        why = err.text;
        delete t;
        free(ecs);
        return rc;
    }
    n_segments = (int)segs.size();
    int16_t* coef = (int16_t*)calloc((size_t)g.nblocks * 64, sizeof(int16_t));
    int covered = 0;
    for (const w2l_jpeg_segment& s : segs) {                         // what one lane does
        int st = jd::kBadRow;
        if (s.offset >= 0 && s.nbytes >= 1 && s.nbytes <= info.ecs_bytes - s.offset) {
            uint8_t* piece = (uint8_t*)malloc((size_t)s.nbytes);      // the segment alone, at its exact size
            memcpy(piece, ecs + s.offset, (size_t)s.nbytes);
            st = jd::decode_mcus(piece, s.nbytes, g, *t, coef, s.first_mcu, s.n_mcus);
            free(piece);
        }
        if (st == 0) covered += s.n_mcus;
        if (st < rc) rc = st;
    }
    if (rc == 0 && covered != g.nblocks / 6) rc = jd::kBadRow;
    free(ecs);
    delete t;
    if (rc != 0) {
        static const char* names[] = {"", "bits that are no code", "a run past coefficient 63", "a marker or bytes left over",
                                      "the stream ended early", "a row the launch cannot take"};
        why = names[-rc];
        free(coef);
        return rc;
    }
    uint8_t* planes = (uint8_t*)malloc((size_t)g.nblocks * 64);
    for (int id = 0; id < g.nblocks; ++id) {
        uint8_t blk[64];
        jd::idct_block(coef + (size_t)id * 64, blk);
        int pitch;
        const long long org = jd::block_origin(g, id, pitch);
        for (int r = 0; r < 8; ++r) memcpy(planes + org + (long long)r * pitch, blk + 8 * r, 8);
    }
    free(coef);
    bgr.resize((size_t)H * W * 3);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) jd::pixel_bgr(planes, g, y, x, bgr.data() + ((size_t)y * W + x) * 3);
    free(planes);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s MANIFEST\n", argv[0]);
        return 2;
    }
    FILE* mf = fopen(argv[1], "r");
    if (!mf) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    char kind[16], a[1024], b[1024];
    int n_valid = 0, n_equal = 0, n_corrupt = 0, n_refused = 0, failed = 0, segments = 0;
    while (fscanf(mf, "%15s %1023s %1023s", kind, a, b) == 3) {
        std::vector<uint8_t> file, bgr, want;
        if (!read_file(a, file)) {
            fprintf(stderr, "cannot read %s\n", a);
            return 2;
        }
        int H = 0, W = 0, ns = 0;
        std::string why;
        const int rc = decode(file, H, W, bgr, why, ns);
        segments += ns;
        if (std::string(kind) == "valid") {
            ++n_valid;
            int eh = 0, ew = 0;
            if (!read_npy(b, eh, ew, want)) {
                fprintf(stderr, "cannot read %s as uint8 [H,W,3]\n", b);
                return 2;
            }
            if (rc != 0 || eh != H || ew != W || bgr != want) {
                ++failed;
                printf("FAIL valid %s: status %d (%s), %dx%d against %dx%d\n", a, rc, why.c_str(), H, W, eh, ew);
            } else {
                ++n_equal;
            }
        } else {
            ++n_corrupt;
            if (rc >= 0) {
                ++failed;
                printf("FAIL corrupt %s: decoded with status %d\n", a, rc);
            } else {
                ++n_refused;
                printf("refused %s: %d (%s)\n", a, rc, why.c_str());
            }
        }
    }
    fclose(mf);
    printf("%d of %d valid files equal their expectation (%d segments), %d of %d corrupt files refused, %d failures\n", n_equal, n_valid,
           segments, n_refused, n_corrupt, failed);
    return failed ? 1 : 0;
}
