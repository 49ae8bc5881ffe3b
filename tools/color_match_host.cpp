// The arithmetic of colour matching (wav2lip_amd/csrc/color_match_core.h, what the kernel of csrc/color_match.hip computes with)
// as a plain host program, for the host sanitizers: tools/color_match_host_check.py builds it with -fsanitize=address,undefined
// and hands it one file of cases and expectations.  Nothing here touches a GPU and nothing is loaded into Python.
//
//     color_match_host <cases.bin>
//
// The file (little endian): int32 count, then per case int32 S, int32 mode, int32 gain[3] (the model's), and three blocks of
// S*S*3 bytes: the prediction, the reference, the model's output.  Every case is computed twice, out of place and in place (the
// kernel's order: all sums first, then the transfer through a 256-entry table per channel), in buffers of exactly S*S*3 bytes,
// so that a read or write past a row is a sanitizer report.  Exit status 0: every case equals the model in both forms.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../wav2lip_amd/csrc/color_match_core.h"

using namespace w2l;

static bool read_i32(FILE* f, int32_t* v, int n) { return fread(v, sizeof(int32_t), (size_t)n, f) == (size_t)n; }

// one row, as the kernel does it: sums over the upper half, gains, one table per channel, the table applied to every byte
static void color_match_row(const uint8_t* pred, const uint8_t* ref, int S, int mode, uint8_t* out, int32_t gain[3]) {
    const uint32_t N = (uint32_t)(S / 2) * (uint32_t)S;
    cm::Sums s[3] = {};
    for (uint32_t i = 0; i < N; ++i)
        for (int c = 0; c < 3; ++c) {
            const uint32_t x = pred[3 * i + c], y = ref[3 * i + c];
            s[c].sp += x;
            s[c].so += y;
            s[c].qp += x * x;
            s[c].qo += y * y;
        }
    uint8_t lut[3][256];
    for (int c = 0; c < 3; ++c) {
        gain[c] = cm::gain_q8(mode, N, s[c]);
        for (uint32_t x = 0; x < 256; ++x) lut[c][x] = cm::transfer(gain[c], N, s[c].sp, s[c].so, x);
    }
    for (uint32_t i = 0; i < (uint32_t)S * (uint32_t)S; ++i)
        for (int c = 0; c < 3; ++c) out[3 * i + c] = lut[c][pred[3 * i + c]];
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <cases.bin>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int32_t count = 0;
    if (!read_i32(f, &count, 1) || count < 0) {
        fprintf(stderr, "bad case file\n");
        return 2;
    }
    int equal = 0, failures = 0;
    for (int k = 0; k < count; ++k) {
        int32_t head[5];
        if (!read_i32(f, head, 5) || head[0] < 2 || head[0] > cm::kMaxS || (head[0] & 1)) {
            fprintf(stderr, "case %d: bad header\n", k);
            return 2;
        }
        const int S = head[0], mode = head[1];
        const size_t bytes = (size_t)S * S * 3;
        std::vector<uint8_t> pred(bytes), ref(bytes), want(bytes), out(bytes);
        if (fread(pred.data(), 1, bytes, f) != bytes || fread(ref.data(), 1, bytes, f) != bytes || fread(want.data(), 1, bytes, f) != bytes) {
            fprintf(stderr, "case %d: short file\n", k);
            return 2;
        }
        int32_t gain[3];
        color_match_row(pred.data(), ref.data(), S, mode, out.data(), gain);
        bool ok = memcmp(out.data(), want.data(), bytes) == 0 && gain[0] == head[2] && gain[1] == head[3] && gain[2] == head[4];
        std::vector<uint8_t> in_place(pred);
        color_match_row(in_place.data(), ref.data(), S, mode, in_place.data(), gain);
        ok = ok && memcmp(in_place.data(), want.data(), bytes) == 0;
        // the table against the transfer called pixel by pixel (what the rule says), on the bytes of this case
        const uint32_t N = (uint32_t)(S / 2) * (uint32_t)S;
        for (int c = 0; c < 3 && ok; ++c) {
            uint32_t sp = 0, so = 0;
            for (uint32_t i = 0; i < N; ++i) {
                sp += pred[3 * i + c];
                so += ref[3 * i + c];
            }
            for (size_t i = 0; i < (size_t)S * S && ok; ++i) ok = cm::transfer(gain[c], N, sp, so, pred[3 * i + c]) == want[3 * i + c];
        }
        if (ok) {
            ++equal;
        } else {
            ++failures;
            printf("case %d (S %d, mode %d): differs from the model (gains %d %d %d, expected %d %d %d)\n", k, S, mode, gain[0], gain[1],
                   gain[2], head[2], head[3], head[4]);
        }
    }
    fclose(f);
    printf("%d of %d cases equal, %d failures\n", equal, count, failures);
    return failures ? 1 : 0;
}
