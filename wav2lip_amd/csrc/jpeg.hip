// Baseline JPEG encoding of face crops that already lie in device memory (the dataset step of the reference, preprocess.py:62
// `cv2.imwrite(<i>.jpg, fb[j][y1:y2, x1:x2])`: quality 95, 4:2:0, standard Huffman tables).  The files are byte-equal to what
// libjpeg(-turbo) writes for the same pixels: baseline JPEG is integer arithmetic end to end, and every rule below is libjpeg's
// (jccolor.c rgb_ycc_convert, jcsample.c h2v2_downsample + expand_right_edge, jcprepct.c pre_process_data, jfdctint.c jpeg_fdct_islow,
// jcdctmgr.c forward_DCT, jccoefct.c compress_data's dummy blocks, jchuff.c encode_one_block).
//
// Two launches per batch, whatever B is:
//   jpeg_transform_kernel  grid (ceil(max_blocks / 32), B), 8 lanes per 8x8 block: colour conversion from the BGR bytes of the
//                          frame, edge replication of THE CROP (never a frame pixel outside the box), 2x2 chroma averaging, the
//                          row pass in registers, a transpose through LDS, the column pass, the exact integer quantisation;
//                          int16 coefficients in zigzag order, MCU-interleaved (Y00 Y01 Y10 Y11 Cb Cr), into the workspace.
//   jpeg_entropy_kernel    one workgroup per row.  A thread owns a CONTIGUOUS run of blocks: it sums their code lengths, a
//                          fixed-order scan over the threads gives its bit offset, and it packs its run through one 64-bit
//                          accumulator into a staging stream - full words with plain stores, the two words it shares with its
//                          neighbours (zeroed beforehand) with an atomic OR.  Then the threads count the 0xFF bytes of their
//                          share of the staged bytes, scan the counts, and write header, stuffed stream, EOI and the length.
// DC predictions need no scan: a block's predecessor (dummy blocks included) is a fixed function of its index.
// Integer work only, so the bytes are a function of the pixels: nothing depends on the order in which threads run.
#include "w2l_common.h"

#include <string.h>

namespace w2l {

namespace {

constexpr int kHeaderBytes = 623;       // SOI .. SOS; the entropy stream starts here
constexpr int kBlockBytes = 128;        // 64 int16 coefficients
constexpr int kBlockStreamBytes = 208;  // 22 bits of DC + 63 x 26 bits of AC = 1660 bits, rounded up to whole bytes
constexpr int kThreads = 256;
constexpr int kMaxBlocksLimit = 1 << 20;   // keeps a row's bit count below 2^31

struct FrameRow {           // mirrors w2l_frame_row (include/w2l_hip.h), 48 bytes
    unsigned long long src, dst;
    int H, W, y1, y2, x1, x2;
    int pad0, pad1;
};
static_assert(sizeof(FrameRow) == 48, "w2l_frame_row is 48 bytes");

// ---- tables of the JPEG standard (ITU-T T.81): zigzag order (figure A.6), Annex K.1 quantisation, Annex K.3 Huffman
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// what the two kernels take by value
struct TransformTables {
    uint16_t div[2][64];    // 8 * quantiser, natural order: [0] luma, [1] chroma
    uint8_t zzpos[64];      // natural index -> position in zigzag order
};
struct EntropyTables {
    uint32_t dc[2][16];     // (code << 5) | length per category
    uint32_t ac[2][256];    // (code << 5) | length per (run << 4 | category) symbol; 0 where the table has no code
    uint8_t header[624];
};

// the quantisers of libjpeg's jpeg_set_quality (jcparam.c: jpeg_quality_scaling + jpeg_add_quant_table, force_baseline)
void quant_table(int quality, int which, uint8_t out[64]) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        int t = (kBaseQuant[which][i] * scale + 50) / 100;
        out[i] = (uint8_t)(t < 1 ? 1 : (t > 255 ? 255 : t));
    }
}

// canonical codes of a (bits, vals) table (T.81 Annex C): out[symbol] = (code << 5) | length
void huff_codes(const uint8_t bits[16], const uint8_t* vals, uint32_t* out, int nout) {
    for (int i = 0; i < nout; ++i) out[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = (code++ << 5) | (uint32_t)len;
        code <<= 1;
    }
}

// SOI, APP0 (JFIF 1.1, no units, 1x1), DQT luma, DQT chroma, SOF0 (Y 2x2 table 0; Cb, Cr 1x1 table 1), DHT DC0 AC0 DC1 AC1, SOS
// ri > 0: DRI (restart interval of ri MCUs) between the last DHT and SOS, where jcmarker.c write_scan_header puts it
int build_header(int h, int w, int quality, uint8_t* out, int ri = 0) {
    uint8_t* p = out;
    auto put = [&](std::initializer_list<int> v) { for (int b : v) *p++ = (uint8_t)b; };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        uint8_t q[64];
        quant_table(quality, t, q);
        put({0xFF, 0xDB, 0, 67, t});
        for (int i = 0; i < 64; ++i) *p++ = q[kZigzag[i]];
    }
    put({0xFF, 0xC0, 0, 17, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 2; ++t) {
        put({0xFF, 0xC4, 0, 19 + 12, 0x00 | t});
        for (int i = 0; i < 16; ++i) *p++ = kDcBits[t][i];
        for (int i = 0; i < 12; ++i) *p++ = kDcVals[i];
        put({0xFF, 0xC4, 0, 19 + 162, 0x10 | t});
        for (int i = 0; i < 16; ++i) *p++ = kAcBits[t][i];
        for (int i = 0; i < 162; ++i) *p++ = kAcVals[t][i];
    }
    if (ri > 0) put({0xFF, 0xDD, 0, 4, ri >> 8, ri & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return (int)(p - out);
}

size_t row_coef_bytes(int max_blocks) { return (size_t)max_blocks * kBlockBytes; }
size_t row_stage_bytes(int max_blocks) { return (size_t)max_blocks * kBlockStreamBytes + 16; }   // + the word behind the last bit
// the restart form: every interval (at most one per MCU) adds less than a byte of padding to the staged stream, and the staged
// byte offsets at which the intervals end follow it, one uint32 each
size_t row_stage_bytes_rst(int max_blocks) { return (row_stage_bytes(max_blocks) + (size_t)max_blocks / 6 + 1 + 15) & ~(size_t)15; }
size_t row_ends_bytes_rst(int max_blocks) { return (((size_t)max_blocks / 6 + 1) * 4 + 15) & ~(size_t)15; }

// ---- device side

// libjpeg's jpeg_fdct_islow, one dimension: CONST_BITS 13, PASS1_BITS 2.  The row pass scales elements 0 and 4 up by 2 bits and
// descales the others by 11; the column pass descales 0 and 4 by 2 and the others by 15.
template <bool kFirst>
__device__ __forceinline__ void fdct8(int d[8]) {
    constexpr int n = kFirst ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (kFirst) {
        d[0] = (t10 + t11) << 2;
        d[4] = (t10 - t11) << 2;
    } else {
        d[0] = (t10 + t11 + 2) >> 2;
        d[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    d[2] = (z1 + t13 * 6270 + (1 << (n - 1))) >> n;
    d[6] = (z1 - t12 * 15137 + (1 << (n - 1))) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = (a4 + z1 + z3 + (1 << (n - 1))) >> n;
    d[5] = (a5 + z2 + z4 + (1 << (n - 1))) >> n;
    d[3] = (a6 + z2 + z3 + (1 << (n - 1))) >> n;
    d[1] = (a7 + z1 + z4 + (1 << (n - 1))) >> n;
}

__device__ __forceinline__ int ycc_y(const uint8_t* p) { return (19595 * p[2] + 38470 * p[1] + 7471 * p[0] + 32768) >> 16; }
__device__ __forceinline__ int ycc_cb(const uint8_t* p) {
    return (-11059 * p[2] - 21709 * p[1] + 32768 * p[0] + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int ycc_cr(const uint8_t* p) {
    return (32768 * p[2] - 27439 * p[1] - 5329 * p[0] + (128 << 16) + 32767) >> 16;
}

// blocks of a crop: MCUs of 16x16 pixels in raster order, six blocks each
struct CropGeom {
    int h, w, mw, mh, nblocks, bh, bw;     // bh, bw: luma block rows / columns that hold pixels
};
__device__ __forceinline__ CropGeom crop_geom(const FrameRow& r) {
    CropGeom g;
    g.h = r.y2 - r.y1;
    g.w = r.x2 - r.x1;
    g.mw = (g.w + 15) >> 4;
    g.mh = (g.h + 15) >> 4;
    g.bh = (g.h + 7) >> 3;
    g.bw = (g.w + 7) >> 3;
    const long long n = 6ll * g.mw * g.mh;
    g.nblocks = n > 0x7fffffffll ? 0x7fffffff : (int)n;
    return g;
}
// a row the launch cannot encode: more blocks than the workspace was sized for, or a size the SOF0 fields cannot hold
__device__ __forceinline__ bool crop_ok(const CropGeom& g, int max_blocks) {
    return g.h >= 1 && g.w >= 1 && g.h <= 65535 && g.w <= 65535 && g.nblocks <= max_blocks;
}

__global__ __launch_bounds__(kThreads) void jpeg_transform_kernel(const FrameRow* __restrict__ rows, int max_blocks,
                                                                  uint8_t* __restrict__ ws, size_t row_stride,
                                                                  const TransformTables tab) {
    __shared__ int tile[kThreads / 8][8][9];
    __shared__ __attribute__((aligned(16))) int16_t zz[kThreads / 8][64];
    const FrameRow r = rows[blockIdx.y];
    const CropGeom g = crop_geom(r);
    if (!crop_ok(g, max_blocks)) return;                                   // uniform over the workgroup
    if ((int)(blockIdx.x * (kThreads / 8)) >= g.nblocks) return;           // uniform too
    const int slot = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const int id = blockIdx.x * (kThreads / 8) + slot;
    const int mcu = id / 6, k = id - mcu * 6;
    const int my = mcu / g.mw, mx = mcu - my * g.mw;
    bool live = id < g.nblocks;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(r.src) + ((long long)r.y1 * r.W + r.x1) * 3;
    const long long pitch = (long long)r.W * 3;
    int d[8];
    if (k < 4) {
        const int by = 2 * my + (k >> 1), bx = 2 * mx + (k & 1);
        live = live && by < g.bh && bx < g.bw;          // a dummy block is made by the entropy kernel, not transformed
        if (live) {
            const uint8_t* line = src + (long long)min(by * 8 + lane, g.h - 1) * pitch;
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] = ycc_y(line + min(bx * 8 + c, g.w - 1) * 3) - 128;
        }
    } else if (live) {
        // the crop grows to an even height by repeating its last row, the DOWNSAMPLED plane then repeats its last row down to the
        // MCU height; columns are replicated to the MCU width before the 2x2 average
        const int ch = (g.h + 1) >> 1;
        const int cy = min(my * 8 + lane, ch - 1);
        const uint8_t* l0 = src + (long long)(2 * cy) * pitch;
        const uint8_t* l1 = src + (long long)min(2 * cy + 1, g.h - 1) * pitch;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int cx = mx * 8 + c;
            const int xa = min(2 * cx, g.w - 1) * 3, xb = min(2 * cx + 1, g.w - 1) * 3;
            const int s = k == 4 ? ycc_cb(l0 + xa) + ycc_cb(l0 + xb) + ycc_cb(l1 + xa) + ycc_cb(l1 + xb)
                                 : ycc_cr(l0 + xa) + ycc_cr(l0 + xb) + ycc_cr(l1 + xa) + ycc_cr(l1 + xb);
            d[c] = ((s + 1 + (cx & 1)) >> 2) - 128;
        }
    }
    if (live) {
        fdct8<true>(d);
#pragma unroll
        for (int c = 0; c < 8; ++c) tile[slot][lane][c] = d[c];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int c = 0; c < 8; ++c) d[c] = tile[slot][c][lane];      // column `lane`
        fdct8<false>(d);
        const int t = k < 4 ? 0 : 1;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int nat = c * 8 + lane;
            const unsigned q = tab.div[t][nat];
            const int v = d[c];
            const unsigned a = ((unsigned)(v < 0 ? -v : v) + (q >> 1)) / q;
            zz[slot][tab.zzpos[nat]] = (int16_t)(v < 0 ? -(int)a : (int)a);
        }
    }
    __syncthreads();
    if (live) {
        int4* out = reinterpret_cast<int4*>(ws + blockIdx.y * row_stride + (size_t)id * kBlockBytes);
        out[lane] = reinterpret_cast<const int4*>(zz[slot])[lane];
    }
}

// exclusive scan of one value per thread, in thread order; `total` is the sum over the workgroup
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* sh, unsigned& total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {
        const unsigned add = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const unsigned incl = sh[t];
    total = sh[kThreads - 1];
    __syncthreads();
    return incl - v;
}

// The DC value the entropy coder sees for block `id`.  A luma block outside the image is a dummy whose DC is that of the block
// before it in its MCU (jccoefct.c): Y01 takes Y00's, Y10 takes Y01's (itself maybe a dummy), Y11 takes Y10's.
__device__ __forceinline__ int coded_dc(const int16_t* __restrict__ coef, const CropGeom& g, int id) {
    const int mcu = id / 6;
    int k = id - mcu * 6;
    if (k < 4) {
        const int my = mcu / g.mw, mx = mcu - my * g.mw;
        const bool right_out = 2 * mx + 1 >= g.bw, bottom_out = 2 * my + 1 >= g.bh;
        if (bottom_out && k >= 2) k = 1;
        if (right_out && (k & 1)) k -= 1;
    }
    return coef[(size_t)(mcu * 6 + k) * 64];
}
__device__ __forceinline__ bool is_dummy(const CropGeom& g, int id) {
    const int mcu = id / 6, k = id - mcu * 6;
    if (k >= 4) return false;
    const int my = mcu / g.mw, mx = mcu - my * g.mw;
    return 2 * my + (k >> 1) >= g.bh || 2 * mx + (k & 1) >= g.bw;
}
// the DC predictor of block `id`: the previous block of the same component in scan order, dummies included
__device__ __forceinline__ int pred_dc(const int16_t* __restrict__ coef, const CropGeom& g, int id) {
    const int mcu = id / 6, k = id - mcu * 6;
    if (k >= 4) return mcu == 0 ? 0 : coef[(size_t)(id - 6) * 64];
    if (k > 0) return coded_dc(coef, g, id - 1);
    return mcu == 0 ? 0 : coded_dc(coef, g, id - 3);
}

// big-endian bit packer into 32-bit words.  The first word it flushes and its last, partial word are shared with the neighbouring
// threads' runs and go out with an atomic OR onto zeroed words; the words in between are this thread's alone.
struct BitSink {
    uint32_t* words;
    unsigned long long acc;
    int nb;
    bool first;
    __device__ __forceinline__ void begin(uint32_t* stage, unsigned bit0) {
        words = stage + (bit0 >> 5);
        acc = 0;
        nb = (int)(bit0 & 31);
        first = true;
    }
    __device__ __forceinline__ void put(unsigned code, int len) {     // len <= 26
        acc = (acc << len) | code;
        nb += len;
        if (nb >= 32) {
            const uint32_t wd = __builtin_bswap32((uint32_t)(acc >> (nb - 32)));
            if (first) atomicOr(words, wd); else *words = wd;
            first = false;
            ++words;
            nb -= 32;
        }
    }
    __device__ __forceinline__ void end() {
        if (nb > 0) atomicOr(words, __builtin_bswap32((uint32_t)(acc << (32 - nb))));
    }
};
struct BitCount {
    unsigned bits;
    __device__ __forceinline__ void put(unsigned, int len) { bits += (unsigned)len; }
};

template <class Sink>
__device__ __forceinline__ void put_value(unsigned hcode, int v, Sink& sink) {
    const int a = v < 0 ? -v : v;
    const int n = a ? 32 - __clz(a) : 0;                               // n = 0 only for a DC difference of 0
    const unsigned low = (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
    sink.put(((hcode >> 5) << n) | low, (int)(hcode & 31) + n);
}

// jchuff.c encode_one_block on coefficients in zigzag order
template <class Sink>
__device__ __forceinline__ void encode_block(const int16_t* __restrict__ blk, bool dummy, int dc, int pred, const uint32_t* dct,
                                             const uint32_t* act, Sink& sink) {
    const int diff = dc - pred;
    const int a = diff < 0 ? -diff : diff;
    put_value(dct[a ? 32 - __clz(a) : 0], diff, sink);
    if (dummy) {
        sink.put(act[0] >> 5, (int)(act[0] & 31));
        return;
    }
    int run = 0;
    const int4* q = reinterpret_cast<const int4*>(blk);
    for (int j = 0; j < 8; ++j) {
        const int4 v4 = q[j];
        const int w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (j == 0 && i == 0) continue;
            const int v = (int)(int16_t)((unsigned)w[i >> 1] >> (16 * (i & 1)));
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                sink.put(act[0xF0] >> 5, (int)(act[0xF0] & 31));
                run -= 16;
            }
            const int av = v < 0 ? -v : v;
            put_value(act[(run << 4) | (32 - __clz(av))], v, sink);
            run = 0;
        }
    }
    if (run > 0) sink.put(act[0] >> 5, (int)(act[0] & 31));
}

__global__ __launch_bounds__(kThreads) void jpeg_entropy_kernel(const FrameRow* __restrict__ rows, const int32_t* __restrict__ cap,
                                                                int max_blocks, int32_t* __restrict__ lengths,
                                                                uint8_t* __restrict__ ws, size_t row_stride, size_t stage_off,
                                                                const EntropyTables tab) {
    __shared__ unsigned sh[kThreads];
    __shared__ uint32_t dct[2][16];
    __shared__ uint32_t act[2][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const FrameRow r = rows[b];
    const CropGeom g = crop_geom(r);
    const int room = cap[b];
    if (!crop_ok(g, max_blocks) || room < kHeaderBytes + 2) {              // uniform over the workgroup
        if (t == 0) lengths[b] = -1;
        return;
    }
    for (int i = t; i < 32; i += kThreads) dct[i >> 4][i & 15] = tab.dc[i >> 4][i & 15];
    for (int i = t; i < 512; i += kThreads) act[i >> 8][i & 255] = tab.ac[i >> 8][i & 255];
    __syncthreads();

    const int16_t* coef = reinterpret_cast<const int16_t*>(ws + b * row_stride);
    uint32_t* stage = reinterpret_cast<uint32_t*>(ws + b * row_stride + stage_off);
    // thread t owns blocks [lo, hi)
    const int per = (g.nblocks + kThreads - 1) / kThreads;
    const int lo = min(t * per, g.nblocks), hi = min(lo + per, g.nblocks);

    BitCount cnt{0};
    for (int id = lo; id < hi; ++id) {
        const int c = (id % 6) >= 4;
        encode_block(coef + (size_t)id * 64, is_dummy(g, id), coded_dc(coef, g, id), pred_dc(coef, g, id), dct[c], act[c], cnt);
    }
    unsigned total_bits;
    const unsigned bit0 = block_scan(cnt.bits, sh, total_bits);
    const unsigned nbytes = (total_bits + 7) >> 3;

    // the words two runs may share: zero before anyone ORs into them
    if (hi > lo) {
        stage[bit0 >> 5] = 0;
        stage[(bit0 + cnt.bits) >> 5] = 0;
    }
    __threadfence();
    __syncthreads();
    if (hi > lo) {
        BitSink sink;
        sink.begin(stage, bit0);
        for (int id = lo; id < hi; ++id) {
            const int c = (id % 6) >= 4;
            encode_block(coef + (size_t)id * 64, is_dummy(g, id), coded_dc(coef, g, id), pred_dc(coef, g, id), dct[c], act[c], sink);
        }
        sink.end();
    }
    if (t == 0 && (total_bits & 7)) {                                      // the last byte is filled up with 1 bits
        const unsigned fill = 8 - (total_bits & 7);
        const uint32_t ones = ((1u << fill) - 1u) << (32 - (total_bits & 31) - fill);
        atomicOr(stage + (total_bits >> 5), __builtin_bswap32(ones));
    }
    __threadfence();
    __syncthreads();

    // byte stuffing: thread t owns staged bytes [s0, s1), whole words
    const unsigned nwords = (nbytes + 3) >> 2;
    const unsigned wper = (nwords + kThreads - 1) / kThreads;
    const unsigned w0 = min((unsigned)t * wper, nwords), w1 = min(w0 + wper, nwords);
    unsigned nff = 0;
    for (unsigned i = w0; i < w1; ++i) {
        const uint32_t v = __hip_atomic_load(stage + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < 4; ++k) nff += (i * 4 + k < nbytes && ((v >> (8 * k)) & 255u) == 255u) ? 1u : 0u;
    }
    unsigned total_ff;
    unsigned ff0 = block_scan(nff, sh, total_ff);
    const long long length = (long long)kHeaderBytes + nbytes + total_ff + 2;
    if (length > room) {                                                   // uniform: nothing of this row is written
        if (t == 0) lengths[b] = -1;
        return;
    }
    uint8_t* dst = reinterpret_cast<uint8_t*>(r.dst);
    for (int i = t; i < kHeaderBytes; i += kThreads) {
        uint8_t v = tab.header[i];
        if (i == 163) v = (uint8_t)(g.h >> 8);
        if (i == 164) v = (uint8_t)(g.h & 255);
        if (i == 165) v = (uint8_t)(g.w >> 8);
        if (i == 166) v = (uint8_t)(g.w & 255);
        dst[i] = v;
    }
    uint8_t* o = dst + kHeaderBytes + (size_t)w0 * 4 + ff0;
    for (unsigned i = w0; i < w1; ++i) {
        const uint32_t v = __hip_atomic_load(stage + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int k = 0; k < 4; ++k) {
            if (i * 4 + k >= nbytes) break;
            const uint8_t by = (uint8_t)(v >> (8 * k));
            *o++ = by;
            if (by == 255) *o++ = 0;
        }
    }
    if (t == 0) {
        dst[length - 2] = 0xFF;
        dst[length - 1] = 0xD9;
        lengths[b] = (int32_t)length;
    }
}

// ---- the restart form (w2l_jpeg_encode_rows_rst): the same scheme with byte-aligned intervals in the staging stream.
// Interval k holds MCUs [k * ri, (k + 1) * ri); its last block is followed by 1 bits up to the byte boundary (the last interval's
// too: that is the end of the stream), its first MCU predicts its DCs from 0.  Where the intervals end in the staged bytes goes into
// ends[]; the stuffing pass, which treats the padded bytes like any other, shifts each byte by 2 per marker in front of it and
// writes the marker FF D0+(k mod 8) behind the last byte of interval k < n_int - 1.
constexpr int kHeaderBytesRst = kHeaderBytes + 6;

struct EntropyTablesRst {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint8_t header[632];    // of a 1x1 file with Ri = 1: size and Ri are patched per row
};

__device__ __forceinline__ int restart_mcus(const CropGeom& g, int restart_rows) {
    const long long ri = (long long)restart_rows * g.mw;
    return ri > 65535 ? 65535 : (int)ri;
}

__device__ __forceinline__ int pred_dc_rst(const int16_t* __restrict__ coef, const CropGeom& g, int id, int ri) {
    const int mcu = id / 6, k = id - mcu * 6;
    const bool first = mcu % ri == 0;
    if (k >= 4) return first ? 0 : coef[(size_t)(id - 6) * 64];
    if (k > 0) return coded_dc(coef, g, id - 1);
    return first ? 0 : coded_dc(coef, g, id - 3);
}

// What a run of blocks adds to the staged stream.  cut = 0: `head` bits and no interval end.  cut = 1: `head` bits up to the run's
// first interval end, `mid` BYTES from there to its last interval end (whole intervals, each padded), `tail` bits behind it.
struct RunBits {
    unsigned cut, head, mid, tail;
};
__device__ __forceinline__ RunBits run_join(const RunBits& a, const RunBits& b) {       // a, then b: associative
    if (!b.cut) return a.cut ? RunBits{1u, a.head, a.mid, a.tail + b.head} : RunBits{0u, a.head + b.head, 0u, 0u};
    if (!a.cut) return RunBits{1u, a.head + b.head, b.mid, b.tail};
    return RunBits{1u, a.head, a.mid + ((a.tail + b.head + 7u) >> 3) + b.mid, b.tail};
}
// the bit at which the stream stands behind a prefix of runs that began at bit 0
__device__ __forceinline__ unsigned run_end_bit(const RunBits& p) { return p.cut ? 8u * (((p.head + 7u) >> 3) + p.mid) + p.tail : p.head; }

struct BitSinkAt : BitSink {        // a BitSink that knows the bit it stands at
    unsigned at;
    __device__ __forceinline__ void put(unsigned code, int len) {
        BitSink::put(code, len);
        at += (unsigned)len;
    }
};

__global__ __launch_bounds__(kThreads) void jpeg_entropy_rst_kernel(const FrameRow* __restrict__ rows, const int32_t* __restrict__ cap,
                                                                    int max_blocks, int restart_rows, int32_t* __restrict__ lengths,
                                                                    uint8_t* __restrict__ ws, size_t row_stride, size_t stage_off,
                                                                    size_t ends_off, const EntropyTablesRst tab) {
    __shared__ unsigned sh[kThreads];
    __shared__ RunBits runs[kThreads];
    __shared__ uint32_t dct[2][16];
    __shared__ uint32_t act[2][256];
    const int b = blockIdx.x, t = threadIdx.x;
    const FrameRow r = rows[b];
    const CropGeom g = crop_geom(r);
    const int room = cap[b];
    if (!crop_ok(g, max_blocks) || room < kHeaderBytesRst + 2) {           // uniform over the workgroup
        if (t == 0) lengths[b] = -1;
        return;
    }
    for (int i = t; i < 32; i += kThreads) dct[i >> 4][i & 15] = tab.dc[i >> 4][i & 15];
    for (int i = t; i < 512; i += kThreads) act[i >> 8][i & 255] = tab.ac[i >> 8][i & 255];
    __syncthreads();

    const int16_t* coef = reinterpret_cast<const int16_t*>(ws + b * row_stride);
    uint32_t* stage = reinterpret_cast<uint32_t*>(ws + b * row_stride + stage_off);
    uint32_t* ends = reinterpret_cast<uint32_t*>(ws + b * row_stride + ends_off);
    const int ri = restart_mcus(g, restart_rows), n_mcus = g.nblocks / 6;
    const int n_int = (n_mcus + ri - 1) / ri;                              // <= max_blocks / 6: ends[] holds them
    // thread t owns blocks [lo, hi)
    const int per = (g.nblocks + kThreads - 1) / kThreads;
    const int lo = min(t * per, g.nblocks), hi = min(lo + per, g.nblocks);

    RunBits mine{0u, 0u, 0u, 0u};
    for (int id = lo; id < hi; ++id) {
        const int c = (id % 6) >= 4;
        BitCount cnt{0};
        encode_block(coef + (size_t)id * 64, is_dummy(g, id), coded_dc(coef, g, id), pred_dc_rst(coef, g, id, ri), dct[c], act[c], cnt);
        const int mcu = id / 6;
        const bool last = id - mcu * 6 == 5 && ((mcu + 1) % ri == 0 || mcu + 1 == n_mcus);
        if (!mine.cut) {
            mine.head += cnt.bits;
            if (last) mine.cut = 1u;
        } else {
            mine.tail += cnt.bits;
            if (last) {
                mine.mid += (mine.tail + 7u) >> 3;
                mine.tail = 0u;
            }
        }
    }
    // a fixed-order inclusive scan of the runs
    runs[t] = mine;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {
        RunBits v = runs[t];
        if (t >= o) v = run_join(runs[t - o], v);
        __syncthreads();
        runs[t] = v;
        __syncthreads();
    }
    const unsigned bit0 = t ? run_end_bit(runs[t - 1]) : 0u, bit1 = run_end_bit(runs[t]);
    const unsigned nbytes = run_end_bit(runs[kThreads - 1]) >> 3;          // the last block ends an interval: a whole number
    __syncthreads();

    // the words two runs may share: zero before anyone ORs into them
    if (hi > lo) {
        stage[bit0 >> 5] = 0;
        stage[bit1 >> 5] = 0;
    }
    __threadfence();
    __syncthreads();
    if (hi > lo) {
        BitSinkAt sink;
        sink.begin(stage, bit0);
        sink.at = bit0;
        for (int id = lo; id < hi; ++id) {
            const int c = (id % 6) >= 4;
            encode_block(coef + (size_t)id * 64, is_dummy(g, id), coded_dc(coef, g, id), pred_dc_rst(coef, g, id, ri), dct[c], act[c], sink);
            const int mcu = id / 6;
            if (id - mcu * 6 == 5 && ((mcu + 1) % ri == 0 || mcu + 1 == n_mcus)) {
                const int fill = (int)((0u - sink.at) & 7u);               // the last byte is filled up with 1 bits
                if (fill) sink.put((1u << fill) - 1u, fill);
                ends[mcu / ri] = sink.at >> 3;
            }
        }
        sink.end();
    }
    __threadfence();
    __syncthreads();

    // byte stuffing: thread t owns staged bytes [s0, s1), whole words
    const unsigned nwords = (nbytes + 3) >> 2;
    const unsigned wper = (nwords + kThreads - 1) / kThreads;
    const unsigned w0 = min((unsigned)t * wper, nwords), w1 = min(w0 + wper, nwords);
    unsigned nff = 0;
    for (unsigned i = w0; i < w1; ++i) {
        const uint32_t v = __hip_atomic_load(stage + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < 4; ++k) nff += (i * 4 + k < nbytes && ((v >> (8 * k)) & 255u) == 255u) ? 1u : 0u;
    }
    unsigned total_ff;
    const unsigned ff0 = block_scan(nff, sh, total_ff);
    const long long length = (long long)kHeaderBytesRst + nbytes + total_ff + 2ll * (n_int - 1) + 2;
    if (length > room) {                                                   // uniform: nothing of this row is written
        if (t == 0) lengths[b] = -1;
        return;
    }
    uint8_t* dst = reinterpret_cast<uint8_t*>(r.dst);
    for (int i = t; i < kHeaderBytesRst; i += kThreads) {
        uint8_t v = tab.header[i];
        if (i == 163) v = (uint8_t)(g.h >> 8);
        if (i == 164) v = (uint8_t)(g.h & 255);
        if (i == 165) v = (uint8_t)(g.w >> 8);
        if (i == 166) v = (uint8_t)(g.w & 255);
        if (i == 613) v = (uint8_t)(ri >> 8);
        if (i == 614) v = (uint8_t)(ri & 255);
        dst[i] = v;
    }
    // markers in front of this thread's first byte: the intervals k < n_int - 1 that end at or before it
    int k0 = 0;
    for (int k1 = n_int - 1; k0 < k1;) {
        const int m = (k0 + k1) >> 1;
        if (__hip_atomic_load(ends + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= w0 * 4) k0 = m + 1; else k1 = m;
    }
    uint32_t next_end = k0 < n_int - 1 ? __hip_atomic_load(ends + k0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xffffffffu;
    uint8_t* o = dst + kHeaderBytesRst + (size_t)w0 * 4 + ff0 + 2 * (size_t)k0;
    for (unsigned i = w0; i < w1; ++i) {
        const uint32_t v = __hip_atomic_load(stage + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int k = 0; k < 4; ++k) {
            if (i * 4 + k >= nbytes) break;
            const uint8_t by = (uint8_t)(v >> (8 * k));
            *o++ = by;
            if (by == 255) *o++ = 0;
            if (i * 4 + k + 1 == next_end) {                               // never stuffed
                *o++ = 0xFF;
                *o++ = (uint8_t)(0xD0 + (k0 & 7));
                ++k0;
                next_end = k0 < n_int - 1 ? __hip_atomic_load(ends + k0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xffffffffu;
            }
        }
    }
    if (t == 0) {
        dst[length - 2] = 0xFF;
        dst[length - 1] = 0xD9;
        lengths[b] = (int32_t)length;
    }
}

}  // namespace

}  // namespace w2l

using namespace w2l;

extern "C" {

int w2l_jpeg_header(int h, int w, int quality, uint8_t* out) {
    W2L_REQUIRE(out && h >= 1 && h <= 65535 && w >= 1 && w <= 65535 && quality >= 1 && quality <= 100,
                "jpeg_header: sizes in [1, 65535] and quality in [1, 100]");
    uint8_t buf[640];
    const int n = build_header(h, w, quality, buf);
    W2L_REQUIRE(n == kHeaderBytes, "jpeg_header: internal header length %d", n);
    memcpy(out, buf, kHeaderBytes);
    return W2L_OK;
}

size_t w2l_jpeg_workspace_bytes(int B, int max_blocks) {
    if (B < 1 || B > 65535 || max_blocks < 1 || max_blocks > kMaxBlocksLimit) return 0;
    return (size_t)B * (row_coef_bytes(max_blocks) + row_stage_bytes(max_blocks));
}

int w2l_jpeg_encode_rows(void* stream, int B, const w2l_frame_row* rows, const int32_t* cap, int quality, int max_blocks,
                         int32_t* lengths, void* workspace, size_t workspace_bytes) {
    W2L_REQUIRE(rows && cap && lengths && workspace, "bad jpeg_encode_rows arguments");
    W2L_REQUIRE(B >= 1 && B <= 65535 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                "jpeg_encode_rows: 1 <= B <= 65535 and a 16-byte aligned row table");
    W2L_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode_rows: quality %d is outside [1, 100]", quality);
    W2L_REQUIRE(max_blocks >= 1 && max_blocks <= kMaxBlocksLimit, "jpeg_encode_rows: max_blocks %d is outside [1, 2^20]", max_blocks);
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && workspace_bytes >= w2l_jpeg_workspace_bytes(B, max_blocks),
                "jpeg_encode_rows: the workspace must be 16-byte aligned and hold w2l_jpeg_workspace_bytes(B, max_blocks) = %zu bytes",
                w2l_jpeg_workspace_bytes(B, max_blocks));
    TransformTables tt;
    EntropyTables et;
    memset(&et, 0, sizeof(et));
    for (int t = 0; t < 2; ++t) {
        uint8_t q[64];
        quant_table(quality, t, q);
        for (int i = 0; i < 64; ++i) tt.div[t][i] = (uint16_t)(8 * q[i]);
        huff_codes(kDcBits[t], kDcVals, et.dc[t], 16);
        huff_codes(kAcBits[t], kAcVals[t], et.ac[t], 256);
    }
    for (int i = 0; i < 64; ++i) tt.zzpos[kZigzag[i]] = (uint8_t)i;
    W2L_REQUIRE(build_header(1, 1, quality, et.header) == kHeaderBytes, "jpeg_encode_rows: internal header length");
    const size_t stage_off = row_coef_bytes(max_blocks), row_stride = stage_off + row_stage_bytes(max_blocks);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3(ceil_div(max_blocks, kThreads / 8), B), dim3(kThreads), 0, s,
                       reinterpret_cast<const FrameRow*>(rows), max_blocks, static_cast<uint8_t*>(workspace), row_stride, tt);
    W2L_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(B), dim3(kThreads), 0, s, reinterpret_cast<const FrameRow*>(rows), cap, max_blocks,
                       lengths, static_cast<uint8_t*>(workspace), row_stride, stage_off, et);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_jpeg_header_rst(int h, int w, int quality, int restart_rows, uint8_t* out) {
    W2L_REQUIRE(out && h >= 1 && h <= 65535 && w >= 1 && w <= 65535 && quality >= 1 && quality <= 100 && restart_rows >= 1,
                "jpeg_header_rst: sizes in [1, 65535], quality in [1, 100] and restart_rows >= 1");
    const long long ri = (long long)restart_rows * ((w + 15) / 16);
    uint8_t buf[640];
    const int n = build_header(h, w, quality, buf, ri > 65535 ? 65535 : (int)ri);
    W2L_REQUIRE(n == kHeaderBytesRst, "jpeg_header_rst: internal header length %d", n);
    memcpy(out, buf, kHeaderBytesRst);
    return W2L_OK;
}

size_t w2l_jpeg_capacity_rst(int h, int w, int restart_rows) {
    if (h < 1 || h > 65535 || w < 1 || w > 65535 || restart_rows < 1) return 0;
    const long long mw = (w + 15) / 16, n_mcus = mw * ((h + 15) / 16);
    const long long ri = restart_rows * mw > 65535 ? 65535 : restart_rows * mw;
    return (size_t)(kHeaderBytesRst + 2 + 2 * kBlockStreamBytes * 6 * n_mcus + 4 * ((n_mcus + ri - 1) / ri));
}

size_t w2l_jpeg_workspace_bytes_rst(int B, int max_blocks) {
    if (B < 1 || B > 65535 || max_blocks < 1 || max_blocks > kMaxBlocksLimit) return 0;
    return (size_t)B * (row_coef_bytes(max_blocks) + row_stage_bytes_rst(max_blocks) + row_ends_bytes_rst(max_blocks));
}

int w2l_jpeg_encode_rows_rst(void* stream, int B, const w2l_frame_row* rows, const int32_t* cap, int quality, int max_blocks,
                             int restart_rows, int32_t* lengths, void* workspace, size_t workspace_bytes) {
    W2L_REQUIRE(rows && cap && lengths && workspace, "bad jpeg_encode_rows_rst arguments");
    W2L_REQUIRE(B >= 1 && B <= 65535 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                "jpeg_encode_rows_rst: 1 <= B <= 65535 and a 16-byte aligned row table");
    W2L_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode_rows_rst: quality %d is outside [1, 100]", quality);
    W2L_REQUIRE(restart_rows >= 1, "jpeg_encode_rows_rst: restart_rows %d is below 1", restart_rows);
    W2L_REQUIRE(max_blocks >= 1 && max_blocks <= kMaxBlocksLimit, "jpeg_encode_rows_rst: max_blocks %d is outside [1, 2^20]", max_blocks);
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && workspace_bytes >= w2l_jpeg_workspace_bytes_rst(B, max_blocks),
                "jpeg_encode_rows_rst: the workspace must be 16-byte aligned and hold w2l_jpeg_workspace_bytes_rst(B, max_blocks) = %zu bytes",
                w2l_jpeg_workspace_bytes_rst(B, max_blocks));
    TransformTables tt;
    EntropyTablesRst et;
    memset(&et, 0, sizeof(et));
    for (int t = 0; t < 2; ++t) {
        uint8_t q[64];
        quant_table(quality, t, q);
        for (int i = 0; i < 64; ++i) tt.div[t][i] = (uint16_t)(8 * q[i]);
        huff_codes(kDcBits[t], kDcVals, et.dc[t], 16);
        huff_codes(kAcBits[t], kAcVals[t], et.ac[t], 256);
    }
    for (int i = 0; i < 64; ++i) tt.zzpos[kZigzag[i]] = (uint8_t)i;
    W2L_REQUIRE(build_header(1, 1, quality, et.header, 1) == kHeaderBytesRst, "jpeg_encode_rows_rst: internal header length");
    const size_t stage_off = row_coef_bytes(max_blocks), ends_off = stage_off + row_stage_bytes_rst(max_blocks);
    const size_t row_stride = ends_off + row_ends_bytes_rst(max_blocks);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3(ceil_div(max_blocks, kThreads / 8), B), dim3(kThreads), 0, s,
                       reinterpret_cast<const FrameRow*>(rows), max_blocks, static_cast<uint8_t*>(workspace), row_stride, tt);
    W2L_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_entropy_rst_kernel, dim3(B), dim3(kThreads), 0, s, reinterpret_cast<const FrameRow*>(rows), cap, max_blocks,
                       restart_rows, lengths, static_cast<uint8_t*>(workspace), row_stride, stage_off, ends_off, et);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"
