// Baseline JPEG decoding of face crops on the device: the read side of jpeg.hip (the reference's `cv2.imread(fname)` of every
// <id>.jpg, wav2lip_train.py:66 / color_syncnet_train.py:97).  The pixels are byte-equal to what libjpeg(-turbo) decodes with its
// defaults; the arithmetic is in jpeg_decode_core.h (shared with the host build of tools/jpeg_decode_host.cpp), the marker parser
// and the table builder in jpeg_decode_host.h.
//
// One memset and three launches per batch, whatever B is; workspace per row: int16 coefficients [max_blocks][64], then the
// sample planes (64 bytes per block):
//   memset                    the coefficients of all rows to zero (a block is mostly zeros: the entropy kernel writes the rest)
//   jpeg_entropy_decode_kernel   ONE LANE PER FILE (decoding is sequential within a file - DC prediction, variable-length codes -
//                             and parallel across files), 8 files per workgroup: jd::decode_scan reads the stream byte by byte, bounded by the row's byte
//                             count, looks codes up in the row's table set (global memory, through the cache: the lanes of a wave
//                             may use different sets) and scatters the dequantised non-zero coefficients; status[b] = 0 or the reason.
//   jpeg_idct_kernel          grid (ceil(max_blocks / 32), B), 8 lanes per 8x8 block: the column pass in registers, a transpose
//                             through LDS, the row pass, range limiting; 8 samples per lane into the row's planes.
//   jpeg_colour_kernel        grid (ceil(max pixels / 256), B), one pixel per lane: fancy upsampling of both chroma planes and
//                             the colour conversion, three bytes out (the image lies at any byte address).
// The last two skip a row whose status is not 0.
//
// The restart form (w2l_jpeg_decode_rows_rst: the frames of a Motion-JPEG video, inference.py:189-215 `cv2.VideoCapture`) replaces
// the entropy launch: a file with a restart interval is cut at its RSTn markers by the host (jd::restart_segments), every piece
// is byte-aligned and predicts its DCs from 0, so jpeg_segment_decode_kernel runs ONE LANE PER SEGMENT (jd::decode_mcus over the
// segment's MCU range; a file without restarts is one segment), status[b] becomes the minimum of the row's segments' reasons, and
// jpeg_segment_close_kernel refuses a row whose good segments do not hold all its MCUs.  Then the same two kernels.
#include "w2l_common.h"

#include "jpeg_decode_host.h"

namespace w2l {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocksLimit = 1 << 20;
// Files per workgroup of the entropy kernel.  A lane's decode is a chain of dependent loads (stream byte, table entry), so the
// kernel is bound by latency, not by lanes: a batch of 4096 files measured 50.4 ms at 64 files per wave, 43.4 at 16, 41.8 at 8,
// 41.0 at 4 and 39.1 at 1 (whole decode call, staging included): 16 and below are level within 5 ms.  8 is taken from that plateau
// for the fewest workgroups; it is not a measured optimum.
constexpr int kEntropyThreads = 8;

struct DecodeRow {          // mirrors w2l_jpeg_row, 32 bytes
    unsigned long long src, dst;
    int nbytes, H, W, table;
};
static_assert(sizeof(DecodeRow) == 32 && sizeof(w2l_jpeg_row) == 32, "w2l_jpeg_row is 32 bytes");

__host__ __device__ size_t coef_bytes(int max_blocks) { return (size_t)max_blocks * 128; }
__host__ __device__ size_t plane_bytes(int max_blocks) { return (size_t)max_blocks * 64; }

__global__ __launch_bounds__(kEntropyThreads) void jpeg_entropy_decode_kernel(const DecodeRow* __restrict__ rows, int B,
                                                                              const jd::TableSet* __restrict__ tables, int n_tables,
                                                                              int max_blocks, int32_t* __restrict__ status,
                                                                              int16_t* __restrict__ coef) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const DecodeRow r = rows[b];
    jd::Geom g;
    int st = jd::kBadRow;
    if (jd::geom_of(r.H, r.W, max_blocks, g) && r.nbytes >= 1 && r.table >= 0 && r.table < n_tables)
        st = jd::decode_scan(reinterpret_cast<const uint8_t*>(r.src), r.nbytes, g, tables[r.table], coef + (size_t)b * max_blocks * 64);
    status[b] = st;
}

// Segments per workgroup of the restart form.  A lane is the same latency-bound chain of dependent loads as above, and a launch
// has few segments for this machine (16 frames of 720p at one MCU row per interval are 720), so what counts is how many CUs they
// are spread over, not how full a wave is: 16 such frames decoded (whole jpeg.decode_frames call, host scan and staging included,
// tools/video_io_bench.py, median of 5) at 452 frames/s with 256 segments per workgroup, 489 with 64, 1233 with 16 and 1330 with
// 8; 16 frames of 480x640 at 1635, 1958, 2468 and 2840.  8 is taken from that run: the best in it, and the files-per-workgroup
// above.  A second run, of another process on another card, did not settle what lies below 8: at 480x640 it gave 2543 with 8, 2849 with 4
// and 3879 with 1, at 720p 743 (range 462 .. 923), 511 and 518 (387 .. 1285) - the 720p figures of that run scatter more than
// the choices differ.  16 files WITHOUT restarts (16 long segments) ran 1.8x faster with 1 per workgroup than with 8 in it.
// (-DW2L_JPEG_SEGS_PER_WG=n builds another; profiles/mjpeg/ holds every run.)
#ifndef W2L_JPEG_SEGS_PER_WG
#define W2L_JPEG_SEGS_PER_WG 8
#endif
constexpr int kSegmentThreads = W2L_JPEG_SEGS_PER_WG;
static_assert(sizeof(w2l_jpeg_segment) == 32, "w2l_jpeg_segment is 32 bytes");

// one lane per segment; status[] and covered[] were zeroed.  The minimum over a row's segments is the row's reason, and the MCUs of
// its good segments are added up for jpeg_segment_close_kernel.
__global__ __launch_bounds__(kSegmentThreads) void jpeg_segment_decode_kernel(const DecodeRow* __restrict__ rows, int B,
                                                                              const jd::TableSet* __restrict__ tables, int n_tables,
                                                                              int max_blocks, const w2l_jpeg_segment* __restrict__ segs,
                                                                              int n_segs, int32_t* __restrict__ status,
                                                                              int32_t* __restrict__ covered, int16_t* __restrict__ coef) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_segs) return;
    const w2l_jpeg_segment s = segs[i];
    if (s.row < 0 || s.row >= B) return;                                     // no row to blame: the rows' own sums will not add up
    const DecodeRow r = rows[s.row];
    jd::Geom g;
    int st = jd::kBadRow;
    if (jd::geom_of(r.H, r.W, max_blocks, g) && r.nbytes >= 1 && r.table >= 0 && r.table < n_tables && s.offset >= 0 && s.nbytes >= 1 &&
        s.nbytes <= r.nbytes - s.offset)
        st = jd::decode_mcus(reinterpret_cast<const uint8_t*>(r.src) + s.offset, s.nbytes, g, tables[r.table],
                             coef + (size_t)s.row * max_blocks * 64, s.first_mcu, s.n_mcus);
    if (st == 0)
        atomicAdd(covered + s.row, s.n_mcus);
    else
        atomicMin(status + s.row, st);
}

// a row is complete when its good segments hold all its MCUs
__global__ void jpeg_segment_close_kernel(const DecodeRow* __restrict__ rows, int B, int max_blocks, int32_t* __restrict__ status,
                                          const int32_t* __restrict__ covered) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || status[b] != 0) return;
    const DecodeRow r = rows[b];
    jd::Geom g;
    if (!jd::geom_of(r.H, r.W, max_blocks, g) || covered[b] != g.nblocks / 6) status[b] = jd::kBadRow;
}

__global__ __launch_bounds__(kThreads) void jpeg_idct_kernel(const DecodeRow* __restrict__ rows, int max_blocks,
                                                             const int32_t* __restrict__ status, const int16_t* __restrict__ coef,
                                                             uint8_t* __restrict__ planes) {
    __shared__ int tile[kThreads / 8][8][9];
    const int b = blockIdx.y;
    if (status[b] != 0) return;                                             // uniform over the workgroup
    const DecodeRow r = rows[b];
    jd::Geom g;
    if (!jd::geom_of(r.H, r.W, max_blocks, g)) return;                      // (a row with status 0 has a geometry)
    if ((int)(blockIdx.x * (kThreads / 8)) >= g.nblocks) return;            // uniform too
    const int slot = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const int id = blockIdx.x * (kThreads / 8) + slot;
    const bool live = id < g.nblocks;
    int d[8];
    if (live) {
        const int16_t* blk = coef + ((size_t)b * max_blocks + id) * 64;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = blk[k * 8 + lane];               // column `lane`
        jd::idct8(d, 11);
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[slot][k][lane] = d[k];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = tile[slot][lane][k];             // row `lane`
        jd::idct8(d, 18);
        int pitch;
        const long long org = jd::block_origin(g, id, pitch);
        uint8_t* out = planes + (size_t)b * plane_bytes(max_blocks) + org + (long long)lane * pitch;   // 8-byte aligned
        uint2 v;
        v.x = (unsigned)jd::range_limit(d[0]) | ((unsigned)jd::range_limit(d[1]) << 8) | ((unsigned)jd::range_limit(d[2]) << 16) |
              ((unsigned)jd::range_limit(d[3]) << 24);
        v.y = (unsigned)jd::range_limit(d[4]) | ((unsigned)jd::range_limit(d[5]) << 8) | ((unsigned)jd::range_limit(d[6]) << 16) |
              ((unsigned)jd::range_limit(d[7]) << 24);
        *reinterpret_cast<uint2*>(out) = v;
    }
}

__global__ __launch_bounds__(kThreads) void jpeg_colour_kernel(const DecodeRow* __restrict__ rows, int max_blocks,
                                                               const int32_t* __restrict__ status,
                                                               const uint8_t* __restrict__ planes) {
    const int b = blockIdx.y;
    if (status[b] != 0) return;
    const DecodeRow r = rows[b];
    jd::Geom g;
    if (!jd::geom_of(r.H, r.W, max_blocks, g)) return;
    const int px = (int)(blockIdx.x * kThreads + threadIdx.x);             // at most 2^20 / 6 MCUs of 256 pixels: fits an int
    if (px >= r.H * r.W) return;                                           // H * W <= 256 MCUs' pixels, too
    const int y = px / r.W, x = px - y * r.W;
    uint8_t bgr[3];
    jd::pixel_bgr(planes + (size_t)b * plane_bytes(max_blocks), g, y, x, bgr);
    uint8_t* out = reinterpret_cast<uint8_t*>(r.dst) + (size_t)px * 3;
    out[0] = bgr[0];
    out[1] = bgr[1];
    out[2] = bgr[2];
}

}  // namespace

}  // namespace w2l

using namespace w2l;

extern "C" {

int w2l_jpeg_parse(const uint8_t* data, size_t n, w2l_jpeg_info* info) {
    W2L_REQUIRE(data && info, "jpeg_parse: NULL argument");
    jd::ErrText err;
    const int rc = jd::parse(data, n, info, err);
    if (rc) set_error("%s", err.text);
    return rc;
}

size_t w2l_jpeg_table_bytes(void) { return sizeof(jd::TableSet); }

int w2l_jpeg_build_tables(const w2l_jpeg_info* info, void* out) {
    W2L_REQUIRE(info && out, "jpeg_build_tables: NULL argument");
    jd::ErrText err;
    jd::TableSet t;
    const int rc = jd::build_tables(info, t, err);
    if (rc) {
        set_error("%s", err.text);
        return rc;
    }
    memcpy(out, &t, sizeof(t));
    return W2L_OK;
}

size_t w2l_jpeg_decode_workspace_bytes(int B, int max_blocks) {
    if (B < 1 || B > 65535 || max_blocks < 1 || max_blocks > kMaxBlocksLimit) return 0;
    return (size_t)B * (coef_bytes(max_blocks) + plane_bytes(max_blocks));
}

int w2l_jpeg_decode_rows(void* stream, int B, const w2l_jpeg_row* rows, const void* tables, int n_tables, int max_blocks,
                         int32_t* status, void* workspace, size_t workspace_bytes) {
    W2L_REQUIRE(rows && tables && status && workspace, "bad jpeg_decode_rows arguments");
    W2L_REQUIRE(B >= 1 && B <= 65535 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                "jpeg_decode_rows: 1 <= B <= 65535 and a 16-byte aligned row table");
    W2L_REQUIRE(n_tables >= 1 && n_tables <= 65535 && (reinterpret_cast<uintptr_t>(tables) & 15) == 0,
                "jpeg_decode_rows: 1 <= n_tables <= 65535 and 16-byte aligned table sets");
    W2L_REQUIRE(max_blocks >= 1 && max_blocks <= kMaxBlocksLimit, "jpeg_decode_rows: max_blocks %d is outside [1, 2^20]", max_blocks);
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && workspace_bytes >= w2l_jpeg_decode_workspace_bytes(B, max_blocks),
                "jpeg_decode_rows: the workspace must be 16-byte aligned and hold w2l_jpeg_decode_workspace_bytes(B, max_blocks) = %zu bytes",
                w2l_jpeg_decode_workspace_bytes(B, max_blocks));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const DecodeRow* rw = reinterpret_cast<const DecodeRow*>(rows);
    int16_t* coef = static_cast<int16_t*>(workspace);
    uint8_t* planes = static_cast<uint8_t*>(workspace) + (size_t)B * coef_bytes(max_blocks);
    W2L_HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)B * coef_bytes(max_blocks), s));
    hipLaunchKernelGGL(jpeg_entropy_decode_kernel, dim3(ceil_div(B, kEntropyThreads)), dim3(kEntropyThreads), 0, s, rw, B,
                       static_cast<const jd::TableSet*>(tables), n_tables, max_blocks, status, coef);
    W2L_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(ceil_div(max_blocks, kThreads / 8), B), dim3(kThreads), 0, s, rw, max_blocks, status, coef,
                       planes);
    W2L_HIP_CHECK(hipGetLastError());
    // a file of max_blocks blocks has at most max_blocks / 6 MCUs of 256 pixels
    const long long max_px = (long long)(max_blocks / 6 + 1) * 256;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((max_px + kThreads - 1) / kThreads), B), dim3(kThreads), 0, s, rw, max_blocks,
                       status, planes);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_jpeg_parse_rst(const uint8_t* data, size_t n, w2l_jpeg_info* info, int32_t* restart_interval) {
    W2L_REQUIRE(data && info && restart_interval, "jpeg_parse_rst: NULL argument");
    jd::ErrText err;
    int ri = 0;
    const int rc = jd::parse(data, n, info, err, &ri);
    *restart_interval = ri;
    if (rc) set_error("%s", err.text);
    return rc;
}

int w2l_jpeg_restart_segments(const uint8_t* ecs, size_t ecs_bytes, int restart_interval, int n_mcus, w2l_jpeg_segment* out, int cap) {
    W2L_REQUIRE(ecs && (out || cap == 0), "jpeg_restart_segments: NULL argument");
    jd::ErrText err;
    const int rc = jd::restart_segments(ecs, ecs_bytes, restart_interval, n_mcus, out, cap, err);
    if (rc < 0) set_error("%s", err.text);
    return rc;
}

size_t w2l_jpeg_decode_workspace_bytes_rst(int B, int max_blocks) {
    if (B < 1 || B > 65535 || max_blocks < 1 || max_blocks > kMaxBlocksLimit) return 0;
    return w2l_jpeg_decode_workspace_bytes(B, max_blocks) + (((size_t)B * 4 + 15) & ~(size_t)15);    // + covered[B]
}

int w2l_jpeg_decode_rows_rst(void* stream, int B, const w2l_jpeg_row* rows, const void* tables, int n_tables, int max_blocks,
                             const w2l_jpeg_segment* segments, int n_segments, int32_t* status, void* workspace,
                             size_t workspace_bytes) {
    W2L_REQUIRE(rows && tables && segments && status && workspace, "bad jpeg_decode_rows_rst arguments");
    W2L_REQUIRE(B >= 1 && B <= 65535 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                "jpeg_decode_rows_rst: 1 <= B <= 65535 and a 16-byte aligned row table");
    W2L_REQUIRE(n_tables >= 1 && n_tables <= 65535 && (reinterpret_cast<uintptr_t>(tables) & 15) == 0,
                "jpeg_decode_rows_rst: 1 <= n_tables <= 65535 and 16-byte aligned table sets");
    W2L_REQUIRE(n_segments >= 1 && n_segments <= (1 << 24) && (reinterpret_cast<uintptr_t>(segments) & 15) == 0,
                "jpeg_decode_rows_rst: 1 <= n_segments <= 2^24 and a 16-byte aligned segment table");
    W2L_REQUIRE(max_blocks >= 1 && max_blocks <= kMaxBlocksLimit, "jpeg_decode_rows_rst: max_blocks %d is outside [1, 2^20]", max_blocks);
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && workspace_bytes >= w2l_jpeg_decode_workspace_bytes_rst(B, max_blocks),
                "jpeg_decode_rows_rst: the workspace must be 16-byte aligned and hold w2l_jpeg_decode_workspace_bytes_rst(B, max_blocks) = %zu bytes",
                w2l_jpeg_decode_workspace_bytes_rst(B, max_blocks));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const DecodeRow* rw = reinterpret_cast<const DecodeRow*>(rows);
    // workspace: coefficients, covered[B] (both zeroed by one memset), then the planes
    int16_t* coef = static_cast<int16_t*>(workspace);
    const size_t covered_bytes = ((size_t)B * 4 + 15) & ~(size_t)15;
    int32_t* covered = reinterpret_cast<int32_t*>(static_cast<uint8_t*>(workspace) + (size_t)B * coef_bytes(max_blocks));
    uint8_t* planes = reinterpret_cast<uint8_t*>(covered) + covered_bytes;
    W2L_HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)B * coef_bytes(max_blocks) + covered_bytes, s));
    W2L_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)B * 4, s));
    hipLaunchKernelGGL(jpeg_segment_decode_kernel, dim3(ceil_div(n_segments, kSegmentThreads)), dim3(kSegmentThreads), 0, s, rw, B,
                       static_cast<const jd::TableSet*>(tables), n_tables, max_blocks, segments, n_segments, status, covered, coef);
    W2L_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_segment_close_kernel, dim3(ceil_div(B, kThreads)), dim3(kThreads), 0, s, rw, B, max_blocks, status, covered);
    W2L_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(ceil_div(max_blocks, kThreads / 8), B), dim3(kThreads), 0, s, rw, max_blocks, status, coef,
                       planes);
    W2L_HIP_CHECK(hipGetLastError());
    const long long max_px = (long long)(max_blocks / 6 + 1) * 256;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((max_px + kThreads - 1) / kThreads), B), dim3(kThreads), 0, s, rw, max_blocks,
                       status, planes);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"
