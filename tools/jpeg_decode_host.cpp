// The JPEG decoder's arithmetic as a stand-alone HOST program: the parser and table builder of csrc/jpeg_decode_host.h and the
// entropy / IDCT / upsampling / colour rules of csrc/jpeg_decode_core.h - the very text the device kernels are compiled from - around
// a main of their own, so that they can run under the host sanitizers:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_decode_host.cpp -o jpeg_decode_host
//     ./jpeg_decode_host MANIFEST
//
// MANIFEST: one line per file, `valid FILE.jpg EXPECTED.npy` (a uint8 [H,W,3] BGR array in NumPy's .npy format: the decoded image
// must equal it byte for byte) or `corrupt FILE.jpg -` (the parser, the table builder or the entropy routine must refuse it with
// its reason; nothing may crash).  Buffers are allocated at their exact sizes, so that a read or write past one is a sanitizer
// report.  tools/jpeg_decode_host_check.py writes the files and the manifest (PIL's pixels as the expectation), builds and runs this.
// Exit status 0: every line held.
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

// 0 and the image, or the reason (a parser / builder code below -99, or the entropy routine's -1 .. -5) and its text
static int decode(const std::vector<uint8_t>& file, int& H, int& W, std::vector<uint8_t>& bgr, std::string& why) {
    // a copy of exactly the file's size: reading file[n] is a heap overflow the sanitizer sees
    uint8_t* data = (uint8_t*)malloc(file.size() ? file.size() : 1);
    memcpy(data, file.data(), file.size());
    w2l_jpeg_info info;
    jd::ErrText err;
    int rc = jd::parse(data, file.size(), &info, err);
    jd::TableSet* t = new jd::TableSet;
    if (rc == 0) rc = jd::build_tables(&info, *t, err);
    if (rc != 0) {
        why = err.text;
        delete t;
        free(data);
        return rc;
    }
    H = info.H;
    W = info.W;
    jd::Geom g;
    if (!jd::geom_of(H, W, 1 << 20, g)) {
        why = "more than 2^20 blocks";
        delete t;
        free(data);
        return jd::kBadRow;
    }
    // the segment alone, at its exact size
    uint8_t* ecs = (uint8_t*)malloc((size_t)info.ecs_bytes);
    memcpy(ecs, data + info.ecs_offset, (size_t)info.ecs_bytes);
    free(data);
    int16_t* coef = (int16_t*)calloc((size_t)g.nblocks * 64, sizeof(int16_t));
    rc = jd::decode_scan(ecs, info.ecs_bytes, g, *t, coef);
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
    int n_valid = 0, n_equal = 0, n_corrupt = 0, failed = 0, reasons[6] = {0, 0, 0, 0, 0, 0}, host_refused = 0;
    while (fscanf(mf, "%15s %1023s %1023s", kind, a, b) == 3) {
        std::vector<uint8_t> file, bgr, want;
        if (!read_file(a, file)) {
            fprintf(stderr, "cannot read %s\n", a);
            return 2;
        }
        int H = 0, W = 0;
        std::string why;
        const int rc = decode(file, H, W, bgr, why);
        if (std::string(kind) == "valid") {
            ++n_valid;
            int eh = 0, ew = 0;
            if (!read_npy(b, eh, ew, want)) {
                fprintf(stderr, "cannot read %s as uint8 [H,W,3]\n", b);
                return 2;
            }
            if (rc != 0 || eh != H || ew != W || bgr != want) {
                ++failed;
                size_t diff = 0;
                if (rc == 0 && bgr.size() == want.size())
                    for (size_t i = 0; i < bgr.size(); ++i) diff += bgr[i] != want[i];
                printf("FAIL valid %s: status %d (%s), %dx%d against %dx%d, %zu bytes differ\n", a, rc, why.c_str(), H, W, eh, ew, diff);
            } else {
                ++n_equal;
            }
        } else {
            ++n_corrupt;
            if (rc >= 0) {
                ++failed;
                printf("FAIL corrupt %s: decoded with status %d\n", a, rc);
            } else if (rc <= -100) {
                ++host_refused;
            } else {
                ++reasons[-rc];
            }
        }
    }
    fclose(mf);
    printf("%d of %d valid files equal their expectation, %d corrupt files refused (parser/builder %d, no code %d, run past 63 %d, "
           "marker or leftover %d, ended early %d), %d failures\n",
           n_equal, n_valid, n_corrupt, host_refused, reasons[1], reasons[2], reasons[3], reasons[4], failed);
    return failed ? 1 : 0;
}
