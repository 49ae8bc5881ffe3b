// The two cv2.resize calls either side of the generator and the paste-back, on uint8 frames resident in HBM
// (reference inference.py:121-126 face crop -> 96x96; :270-271 generated 96x96 -> box size, pasted into the frame).
// cv::resize(INTER_LINEAR) semantics for CV_8UC3 (OpenCV 4.1.0 modules/imgproc/src/resize.cpp): copy when the sizes match,
// the 2x2 INTER_AREA fast path for an exact 2x down-scale, otherwise the 11-bit fixed-point bilinear path (horizontal pass
// in int32, vertical pass ((b0*(S0>>4))>>16 + (b1*(S1>>4))>>16 + 2)>>2).  One thread per destination pixel (3 channels);
// byte traffic only — HBM-bound, no LDS needed (each source pixel is touched by <= 4 neighbouring threads: L1/L2 hits).
#include "w2l_common.h"
#include "resize_px.h"

namespace w2l {

__global__ void crop_resize_kernel(int B, const uint8_t* __restrict__ frames, int H, int W,
                                   const int32_t* __restrict__ frame_idx, const int32_t* __restrict__ boxes, int S,
                                   uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    const int4 box = *reinterpret_cast<const int4*>(boxes + 4 * b);   // y1, y2, x1, x2
    const int fi = frame_idx ? frame_idx[b] : b;
    const uint8_t* src = frames + ((long long)fi * H + box.x) * W * 3 + (long long)box.z * 3;
    const int Hs = box.y - box.x, Ws = box.w - box.z;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < S * S; i += gridDim.x * blockDim.x) {
        const int dy = i / S, dx = i - dy * S;
        uint8_t px[3];
        resize_px(src, (long long)W * 3, Hs, Ws, dx, dy, S, S, px);
        uint8_t* o = out + ((long long)b * S * S + i) * 3;
        o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
    }
}

// whole-frame resize (inference.py:203: `cv2.resize(frame, (w // resize_factor, h // resize_factor))`)
__global__ void resize_frames_kernel(int B, const uint8_t* __restrict__ src, int Hs, int Ws, uint8_t* __restrict__ dst,
                                     int Hd, int Wd) {
    const int b = blockIdx.y;
    const uint8_t* s = src + (long long)b * Hs * Ws * 3;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hd * Wd; i += gridDim.x * blockDim.x) {
        const int dy = i / Wd, dx = i - dy * Wd;
        uint8_t px[3];
        resize_px(s, (long long)Ws * 3, Hs, Ws, dx, dy, Wd, Hd, px);
        uint8_t* o = dst + ((long long)b * Hd * Wd + i) * 3;
        o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
    }
}

// ---- row-table forms (evaluation/gen_videos_from_filelist.py:85-95, :221-227): every row names its own frame, so rows of
// clips with different frame shapes share one launch.  Same resize_px arithmetic as the kernels above: byte-equal results.
struct FrameRow {           // mirrors w2l_frame_row (include/w2l_hip.h), 48 bytes
    unsigned long long src, dst;
    int H, W, y1, y2, x1, x2;
    int pad0, pad1;
};
static_assert(sizeof(FrameRow) == 48, "w2l_frame_row is 48 bytes");

__global__ void crop_resize_rows_kernel(int B, const FrameRow* __restrict__ rows, int S, uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    const FrameRow r = rows[b];
    const uint8_t* src = reinterpret_cast<const uint8_t*>(r.src) + ((long long)r.y1 * r.W + r.x1) * 3;
    const int Hs = r.y2 - r.y1, Ws = r.x2 - r.x1;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < S * S; i += gridDim.x * blockDim.x) {
        const int dy = i / S, dx = i - dy * S;
        uint8_t px[3];
        resize_px(src, (long long)r.W * 3, Hs, Ws, dx, dy, S, S, px);
        uint8_t* o = out + ((long long)b * S * S + i) * 3;
        o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
    }
}

// ---- the paste-back, plain (the reference's) and with the feathered, mouth-region blend (opt-in; not the reference's output):
// one body per kernel, two instantiations; the plain one computes nothing of the blend.  Integers only.  Per box of h x w
// pixels, feather F (0..64) and top_q8 T (0..255):
//   t0 = (h*T) >> 8, hr = h - t0 (>= 1), Fe = min(F, (min(w, hr) - 1) / 2), D = (Fe+1)^2
//   wy(j) = 0 for j < t0, else min(Fe+1, j-t0+1, h-j);  wx(i) = min(Fe+1, i+1, w-i);  a = wx*wy
//   out_c = (a*p_c + (D-a)*o_c + D/2) / D, p = resize_px (unchanged), o = the frame's own pixel
// Rows above t0 (a == 0) are never resized: the kernels treat the box as starting at row y1 + t0, where a >= 1 everywhere.
// a == D (the box's centre; every pixel when F = 0) stores p without reading o.  In the band the quotient is
// umulhi(n, ceil(2^32 / D)): equal to n / D for every D = (Fe+1)^2 > 1 and n <= 255*D + D/2 (tests/test_blend_cases_cpu.py
// checks every such pair on the host); D == 1 has no band.
struct BlendBox {
    int t0, fe1;            // first blended row of the box; Fe + 1
    uint32_t D, magic;      // (Fe+1)^2; ceil(2^32 / D), unused for D == 1
};

__device__ __forceinline__ BlendBox blend_box(int h, int w, int feather, int top_q8) {
    BlendBox k;
    k.t0 = (int)(((long long)h * top_q8) >> 8);
    k.fe1 = min(feather, (min(w, h - k.t0) - 1) >> 1) + 1;
    k.D = (uint32_t)(k.fe1 * k.fe1);
    k.magic = 0xFFFFFFFFu / k.D + 1u;
    return k;
}

// weight of box-relative column i, row j >= t0
__device__ __forceinline__ uint32_t blend_weight(const BlendBox& k, int i, int j, int h, int w) {
    const int wy = min(k.fe1, min(j - k.t0 + 1, h - j));
    const int wx = min(k.fe1, min(i + 1, w - i));
    return (uint32_t)(wx * wy);
}

// px = the resized prediction's pixel, o = the frame's: px becomes the blend (a < D), or stays (a == D, o is not read)
__device__ __forceinline__ void blend_px(const BlendBox& k, uint32_t a, const uint8_t* o, uint8_t* px) {
    if (a == k.D) return;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        px[c] = (uint8_t)__umulhi(a * px[c] + (k.D - a) * o[c] + (k.D >> 1), k.magic);
}

template <bool kBlend>      // false: feather and top_q8 are not read
__global__ void resize_paste_kernel(int B, const uint8_t* __restrict__ pred, int S, const int32_t* __restrict__ boxes,
                                    const int32_t* __restrict__ frame_idx, uint8_t* frames, int H, int W, int feather,
                                    int top_q8) {
    const int b = blockIdx.y;
    const int4 box = *reinterpret_cast<const int4*>(boxes + 4 * b);
    const int fo = frame_idx ? frame_idx[b] : b;
    const int h = box.y - box.x, w = box.w - box.z;
    BlendBox k = {};
    if constexpr (kBlend) k = blend_box(h, w, feather, top_q8);
    const uint8_t* src = pred + (long long)b * S * S * 3;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (h - k.t0) * w; i += gridDim.x * blockDim.x) {
        const int dy = k.t0 + i / w, dx = i - (dy - k.t0) * w;
        uint8_t px[3];
        resize_px(src, (long long)S * 3, S, S, dx, dy, w, h, px);
        uint8_t* o = frames + (((long long)fo * H + box.x + dy) * W + box.z + dx) * 3;
        if constexpr (kBlend) blend_px(k, blend_weight(k, dx, dy, h, w), o, px);
        o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
    }
}

// One pass over the whole output frame: a thread owns 4 consecutive pixels (12 bytes = 3 dwords of the flattened frame).  A
// group that lies outside the box in 4-byte aligned frames moves as three dwords (skipped when the paste is in place); any
// other group goes pixel by pixel, box pixels from the resized prediction.  HBM-bound byte traffic, no LDS.  With the blend the
// box is its blended part (rows y1 + t0 .. y2); a box pixel reads o from src and writes dst in one thread, so src == dst stays
// in place.
template <bool kBlend>      // false: feather and top_q8 are not read
__global__ void compose_rows_kernel(int B, const uint8_t* __restrict__ pred, int S, const FrameRow* __restrict__ rows, int feather,
                                    int top_q8) {
    const int b = blockIdx.y;
    const FrameRow r = rows[b];
    const uint8_t* src = reinterpret_cast<const uint8_t*>(r.src);
    uint8_t* dst = reinterpret_cast<uint8_t*>(r.dst);
    const uint8_t* p = pred + (long long)b * S * S * 3;
    const int h = r.y2 - r.y1, w = r.x2 - r.x1;
    BlendBox k = {};
    if constexpr (kBlend) k = blend_box(h, w, feather, top_q8);
    const int y1 = r.y1 + k.t0;                         // first pasted frame row
    const int npx = r.H * r.W;                          // < 2^31 / 3 (checked by the caller's max_frame_pixels)
    const int ngroups = (npx + 3) >> 2;
    const bool in_place = src == dst;
    const bool dwords = (((r.src | r.dst) & 3) == 0);
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += gridDim.x * blockDim.x) {
        const int i0 = g << 2, i1 = min(i0 + 4, npx);
        const int ya = i0 / r.W, xa = i0 - ya * r.W;
        const int yb = (i1 - 1) / r.W, xb = (i1 - 1) - yb * r.W;
        // the group touches the box iff one of its frame rows does within its span of columns (frames narrower than 4 pixels,
        // where a group can span three rows or more, take the per-pixel path)
        const bool a_in = ya >= y1 && ya < r.y2 && xa < r.x2 && (ya == yb ? xb : r.W - 1) >= r.x1;
        const bool b_in = yb != ya && yb >= y1 && yb < r.y2 && xb >= r.x1;
        if (r.W >= 4 && !a_in && !b_in) {
            if (in_place) continue;
            if (dwords && i1 - i0 == 4) {
                const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + (long long)i0 * 3);
                uint32_t* d4 = reinterpret_cast<uint32_t*>(dst + (long long)i0 * 3);
                const uint32_t v0 = s4[0], v1 = s4[1], v2 = s4[2];
                d4[0] = v0; d4[1] = v1; d4[2] = v2;
                continue;
            }
        }
        for (int i = i0; i < i1; ++i) {
            const int y = i / r.W, x = i - y * r.W;
            const uint8_t* q = src + (long long)i * 3;
            uint8_t* o = dst + (long long)i * 3;
            if (y >= y1 && y < r.y2 && x >= r.x1 && x < r.x2) {
                uint8_t px[3];
                resize_px(p, (long long)S * 3, S, S, x - r.x1, y - r.y1, w, h, px);
                if constexpr (kBlend) blend_px(k, blend_weight(k, x - r.x1, y - r.y1, h, w), q, px);
                o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
            } else if (!in_place) {
                o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
            }
        }
    }
}

// ---- whole-frame row-table resize (evaluation/real_videos_inference.py:239-245 the `max_frame_res` cap at read time, :51-70
// rescale_frames by an integer factor): every row names its own source and destination frame and their sizes, so frames of any
// shapes share one launch and two rows may read one source.  Same resize_px arithmetic: byte-equal to resize_frames_kernel.
// An item is 4 neighbouring pixels of one destination line (12 bytes): the vertical tap is computed once per item, the
// horizontal taps once per pixel, and the 12 bytes leave as three dwords when their address is 4-byte aligned.  Destinations lie
// at any byte address (H*W*3 is rarely a multiple of 4, and so is W*3), so a line that starts m bytes past a dword boundary
// stores 4-m bytes, the two aligned dwords inside the item and m bytes; the ragged last item of a line goes byte by byte.
// Source reads are byte gathers (<= 4 items share a source pixel: L1/L2 hits).  HBM-bound, no LDS.
struct ResizeRow {          // mirrors w2l_resize_row (include/w2l_hip.h), 32 bytes
    unsigned long long src, dst;
    int Hs, Ws, Hd, Wd;
};
static_assert(sizeof(ResizeRow) == 32, "w2l_resize_row is 32 bytes");

__global__ __launch_bounds__(256) void resize_rows_kernel(int B, const ResizeRow* __restrict__ rows) {
    const int b = blockIdx.y;
    const ResizeRow r = rows[b];
    const uint8_t* src = reinterpret_cast<const uint8_t*>(r.src);
    uint8_t* dst = reinterpret_cast<uint8_t*>(r.dst);
    const long long sstride = (long long)r.Ws * 3, dstride = (long long)r.Wd * 3;
    const int groups = (r.Wd + 3) >> 2;
    const int nitems = r.Hd * groups;                   // <= Hd*Wd < 2^29 (checked by the caller's max_dst_pixels)
    const bool direct = resize_is_direct(r.Hs, r.Ws, r.Hd, r.Wd);
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nitems; item += gridDim.x * blockDim.x) {
        const int dy = item / groups, x0 = (item - dy * groups) << 2;
        const int np = min(4, r.Wd - x0);
        uint8_t px[4][3];
        if (direct) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < np) resize_px(src, sstride, r.Hs, r.Ws, x0 + k, dy, r.Wd, r.Hd, px[k]);
        } else {
            const AxisTap ty = axis_tap(dy, r.Hs, r.Hd, false);
            const uint8_t* r0 = src + ty.s0 * sstride;
            const uint8_t* r1 = src + ty.s1 * sstride;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < np) lerp_px(r0, r1, axis_tap(x0 + k, r.Ws, r.Wd, true), ty, px[k]);
        }
        uint8_t* o = dst + dy * dstride + (long long)x0 * 3;
        if (np < 4) {
            for (int k = 0; k < np; ++k) {
                o[3 * k] = px[k][0]; o[3 * k + 1] = px[k][1]; o[3 * k + 2] = px[k][2];
            }
            continue;
        }
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k >> 2] |= (uint32_t)px[k / 3][k % 3] << (8 * (k & 3));
        const unsigned m = (unsigned)(reinterpret_cast<uintptr_t>(o) & 3);
        if (m == 0) {
            uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
            o4[0] = w[0]; o4[1] = w[1]; o4[2] = w[2];
            continue;
        }
        // bytes [0, 4-m) | dwords at byte 4-m and 8-m of the item (both aligned) | bytes [12-m, 12)
        const unsigned head = 4 - m, sh = 8 * head;
        for (unsigned k = 0; k < head; ++k) o[k] = (uint8_t)(w[0] >> (8 * k));
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o + head);
        o4[0] = (uint32_t)((((unsigned long long)w[1] << 32) | w[0]) >> sh);
        o4[1] = (uint32_t)((((unsigned long long)w[2] << 32) | w[1]) >> sh);
        for (unsigned k = 0; k < m; ++k) o[12 - m + k] = (uint8_t)(w[2] >> (8 * (head + k)));
    }
}

}  // namespace w2l

using namespace w2l;

// the plain and the blend entry of each paste share a launcher (`name` opens the messages; blend: the <true> instantiation)
static int resize_paste_launch(const char* name, bool blend, void* stream, int B, const uint8_t* pred, int S, const int32_t* boxes,
                               const int32_t* frame_idx, uint8_t* frames, int H, int W, int max_box_pixels, int feather, int top_q8) {
    W2L_REQUIRE(pred && boxes && frames && B >= 1 && H >= 1 && W >= 1 && S >= 1 && max_box_pixels >= 1, "bad %s arguments", name);
    W2L_REQUIRE(B <= 65535 && (reinterpret_cast<uintptr_t>(boxes) & 15) == 0, "%s: B <= 65535 and 16-byte aligned boxes", name);
    W2L_REQUIRE(feather >= 0 && feather <= 64 && top_q8 >= 0 && top_q8 <= 255, "%s: feather in [0, 64], top_q8 in [0, 255]", name);
    int gx = ceil_div(max_box_pixels, 256);
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(blend ? resize_paste_kernel<true> : resize_paste_kernel<false>, dim3(gx, B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), B, pred, S, boxes, frame_idx, frames, H, W, feather, top_q8);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

static int compose_rows_launch(const char* name, bool blend, void* stream, int B, const uint8_t* pred, int S, const w2l_frame_row* rows,
                               int max_frame_pixels, int feather, int top_q8) {
    W2L_REQUIRE(pred && rows && S >= 1 && max_frame_pixels >= 1 && max_frame_pixels <= (1 << 29), "bad %s arguments", name);
    W2L_REQUIRE(B >= 1 && B <= 65535 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                "%s: 1 <= B <= 65535 and a 16-byte aligned row table", name);
    W2L_REQUIRE(feather >= 0 && feather <= 64 && top_q8 >= 0 && top_q8 <= 255, "%s: feather in [0, 64], top_q8 in [0, 255]", name);
    int gx = ceil_div(ceil_div(max_frame_pixels, 4), 256);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(blend ? compose_rows_kernel<true> : compose_rows_kernel<false>, dim3(gx, B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), B, pred, S, reinterpret_cast<const FrameRow*>(rows), feather, top_q8);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

extern "C" {

int w2l_crop_resize_u8(void* stream, int B, const uint8_t* frames, int H, int W, const int32_t* frame_idx,
                       const int32_t* boxes, int S, uint8_t* out) {
    W2L_REQUIRE(frames && boxes && out && B >= 1 && H >= 1 && W >= 1 && S >= 1, "bad crop_resize arguments");
    W2L_REQUIRE(B <= 65535 && (reinterpret_cast<uintptr_t>(boxes) & 15) == 0, "crop_resize: B <= 65535 and 16-byte aligned boxes");
    int gx = ceil_div(S * S, 256);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(crop_resize_kernel, dim3(gx, B), dim3(256), 0, static_cast<hipStream_t>(stream), B, frames, H, W,
                       frame_idx, boxes, S, out);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_resize_u8(void* stream, int B, const uint8_t* src, int Hs, int Ws, uint8_t* dst, int Hd, int Wd) {
    W2L_REQUIRE(src && dst && B >= 1 && Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1, "bad resize arguments");
    W2L_REQUIRE(B <= 65535 && (long long)Hd * Wd < (1ll << 31) && (long long)Hs * Ws < (1ll << 31), "resize: frame too large");
    int gx = ceil_div(Hd * Wd, 256);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(resize_frames_kernel, dim3(gx, B), dim3(256), 0, static_cast<hipStream_t>(stream), B, src, Hs, Ws, dst,
                       Hd, Wd);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_resize_paste_u8(void* stream, int B, const uint8_t* pred, int S, const int32_t* boxes, const int32_t* frame_idx,
                        uint8_t* frames, int H, int W, int max_box_pixels) {
    return resize_paste_launch("resize_paste", false, stream, B, pred, S, boxes, frame_idx, frames, H, W, max_box_pixels, 0, 0);
}

int w2l_resize_blend_u8(void* stream, int B, const uint8_t* pred, int S, const int32_t* boxes, const int32_t* frame_idx,
                        uint8_t* frames, int H, int W, int max_box_pixels, int feather, int top_q8) {
    return resize_paste_launch("resize_blend", true, stream, B, pred, S, boxes, frame_idx, frames, H, W, max_box_pixels, feather,
                               top_q8);
}

int w2l_crop_resize_rows_u8(void* stream, int B, const w2l_frame_row* rows, int S, uint8_t* out) {
    W2L_REQUIRE(rows && out && S >= 1, "bad crop_resize_rows arguments");
    W2L_REQUIRE(B >= 1 && B <= 65535 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                "crop_resize_rows: 1 <= B <= 65535 and a 16-byte aligned row table");
    int gx = ceil_div(S * S, 256);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(crop_resize_rows_kernel, dim3(gx, B), dim3(256), 0, static_cast<hipStream_t>(stream), B,
                       reinterpret_cast<const FrameRow*>(rows), S, out);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_compose_rows_u8(void* stream, int B, const uint8_t* pred, int S, const w2l_frame_row* rows, int max_frame_pixels) {
    return compose_rows_launch("compose_rows", false, stream, B, pred, S, rows, max_frame_pixels, 0, 0);
}

int w2l_compose_blend_rows_u8(void* stream, int B, const uint8_t* pred, int S, const w2l_frame_row* rows, int max_frame_pixels,
                              int feather, int top_q8) {
    return compose_rows_launch("compose_blend_rows", true, stream, B, pred, S, rows, max_frame_pixels, feather, top_q8);
}

int w2l_resize_rows_u8(void* stream, int B, const w2l_resize_row* rows, int max_dst_pixels) {
    W2L_REQUIRE(rows && max_dst_pixels >= 1 && max_dst_pixels <= (1 << 29), "bad resize_rows arguments");
    W2L_REQUIRE(B >= 1 && B <= 65535 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                "resize_rows: 1 <= B <= 65535 and a 16-byte aligned row table");
    int gx = ceil_div(ceil_div(max_dst_pixels, 4), 256);
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(resize_rows_kernel, dim3(gx, B), dim3(256), 0, static_cast<hipStream_t>(stream), B,
                       reinterpret_cast<const ResizeRow*>(rows));
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"
