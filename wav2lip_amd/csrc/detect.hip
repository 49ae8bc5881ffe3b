// S3FD face-detector glue kernels (reference face_detection/detection/sfd/): everything between the 3x3 convolutions, which
// are the SAME fused conv launches as the generator's (conv_igemm.hip / conv_wino.hip with bias + ReLU, no BatchNorm).
// The pack, max-pool and L2Norm ops exist for fp32 tensors and, with the suffix _bf16, for the bf16-storage path (channel strides
// in elements, multiples of 8): one templated kernel body and one set of argument checks per op.
//   w2l_s3fd_pack       detect.py:57-58 + api.py:62  uint8 BGR frames -> RGB order, minus (104,117,123), fp32 NHWC4; bf16:
//                       the same integers (exact), zeros in every other channel
//   w2l_s3fd_pack_rows  the same per frame of an address table: frames of several clips in one batch, read where they lie
//   w2l_s3fd_pack_rows_scaled[_bf16]  inference.py:202-203 (`cv2.resize(frame, (w // k, h // k))`) fused into the row-table pack:
//                       the detector reads a frame at reduced size, the reduced frame is never stored
//   w2l_maxpool2x2      net_s3fd.py:75,79,85,91,97   F.max_pool2d(h, 2, 2) (exact in bf16 too)
//   w2l_l2norm_scale    net_s3fd.py:6-19             x / (sqrt(sum_c x^2) + 1e-10) * weight[c]; bf16: fp32 arithmetic, one rounding
//   w2l_s3fd_decode     net_s3fd.py:123-126 (max-out background), detect.py:66-84 (softmax, priors, decode)
//   w2l_s3fd_nms        sfd_detector.py:39-45 gate + bbox.py:44-64 greedy NMS, bit-exact keep list
//   w2l_s3fd_first_rect sfd_detector.py:45 + api.py:61-77  first kept box above 0.5 -> int rect, one row per image
//   w2l_s3fd_first_rect_scaled  the same with the box mapped back to the full frame (x * sx, y * sy) before the clip and int()
//   w2l_s3fd_top_rects  sfd_detector.py:45 + api.py:61-77 for the first K kept boxes above 0.5 instead of d[0] alone (opt-in)
//   w2l_face_track_segments  one of those candidates per frame, followed through a clip by overlap (opt-in; not the reference's
//                       rule, which takes d[0] of every frame): rects and flags in w2l_s3fd_first_rect's format
//   w2l_face_tracks_all_segments  every face of a segment followed at once in F track slots, best pair first (opt-in; what
//                       run_pipeline.py does before calculate_scores_real_videos.py:38-40 scores every face track)
//   w2l_face_boxes_segments  inference.py:59-66, :90-104 / gen_videos_from_filelist.py:35-42, :61-77  pads, clipping, temporal
//                       smoothing and "no face" of many clips in one launch
//   w2l_face_boxes_stream  the same finish for LIVE streams, tick by tick: a box is written once the T - 1 frames after it are there
//   w2l_face_boxes_runs, w2l_face_boxes_stream_runs  the two finishes with frames without a face passed through (opt-in)
// All HBM-bound, NHWC, 16-byte vectors where the channel count allows.
#include "w2l_common.h"
#include "w2l_storage.h"
#include "resize_px.h"

namespace w2l {

// ---- the glue between the convolutions: one kernel body per op, S = StF32 / StBf16 (w2l_storage.h) the storage of its tensors.
// What the detector's two storages do NOT share is stated here, once:
template <class S>
struct GlueSt;
template <>
struct GlueSt<StF32> {
    static constexpr int kPackGridCap = 16384;
    static constexpr bool kConvbLimit = false;
    // any channel stride from 3 on; only the 16-byte store of a stride that is a multiple of 4 needs an aligned base
    static bool pack_ok(const void* y, int y_cs) { return y_cs >= 3 && ((y_cs & 3) != 0 || (reinterpret_cast<uintptr_t>(y) & 15) == 0); }
    static constexpr const char* kPackRule = "y_cs >= 3, and y 16-byte aligned where y_cs % 4 == 0";
};
template <>
struct GlueSt<StBf16> {
    static constexpr int kPackGridCap = 65536;
    // the tensors feed w2l_convb launches, which address a buffer with 32-bit byte offsets: no buffer of 2 GiB or more
    static constexpr bool kConvbLimit = true;
    static bool pack_ok(const void* y, int y_cs) { return y_cs >= 8 && (y_cs & 7) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0; }
    static constexpr const char* kPackRule = "y_cs % 8 == 0 and y 16-byte aligned";
};

// A packed pixel leaves through one of these.  fp32: one 16-byte store of (c0, c1, c2, 0) where the stride is a multiple of 4 -
// channels >= 4 stay as they are - else three scalar stores.  bf16 (y_cs % 8 == 0): every 8-channel group is written, group 0
// with the pixel (integers with |v| <= 152: exact), the rest with zeros.
__device__ __forceinline__ void s3fd_store_px(float* o, int y_cs, float c0, float c1, float c2) {
    if (y_cs >= 4 && (y_cs & 3) == 0) *reinterpret_cast<f32x4*>(o) = f32x4{c0, c1, c2, 0.f};
    else { o[0] = c0; o[1] = c1; o[2] = c2; }
}
__device__ __forceinline__ void s3fd_store_px(__bf16* o, int y_cs, float c0, float c1, float c2) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)0.f;
    for (int g = 1; g < (y_cs >> 3); ++g) *reinterpret_cast<bf16x8*>(o + g * 8) = v;
    v[0] = (__bf16)c0; v[1] = (__bf16)c1; v[2] = (__bf16)c2;
    *reinterpret_cast<bf16x8*>(o) = v;
}

// one thread per pixel, all its channel groups (the detector packs at y_cs = 4 and 8: one group)
template <class S>
__global__ void s3fd_pack_kernel(long long npix, const uint8_t* __restrict__ x, typename S::elem* __restrict__ y, int y_cs,
                                 float m0, float m1, float m2) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        float c0, c1, c2;
        s3fd_pixel(x + i * 3, m0, m1, m2, c0, c1, c2);
        s3fd_store_px(y + i * y_cs, y_cs, c0, c1, c2);
    }
}

// The row-table form: blockIdx.y is the image, its frame lies at frames[b].  A thread owns four consecutive pixels (12 bytes =
// three dwords of an aligned frame); HBM-bound byte traffic, no LDS.
template <class S>
__global__ void s3fd_pack_rows_kernel(int npix, const uint64_t* __restrict__ frames, typename S::elem* __restrict__ y, int y_cs,
                                      float m0, float m1, float m2) {
    const int b = blockIdx.y;
    const uint64_t addr = frames[b];
    const uint8_t* x = reinterpret_cast<const uint8_t*>(addr);
    const bool dwords = (addr & 3) == 0;
    typename S::elem* yb = y + (long long)b * npix * y_cs;
    const int ngroups = (npix + 3) >> 2;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += gridDim.x * blockDim.x) {
        const int i0 = g << 2, n = min(4, npix - i0);
        uint8_t px[12];
        s3fd_load_group(x + (long long)i0 * 3, dwords, n, px);
        for (int k = 0; k < n; ++k) {
            float c0, c1, c2;
            s3fd_pixel(px + 3 * k, m0, m1, m2, c0, c1, c2);
            s3fd_store_px(yb + (long long)(i0 + k) * y_cs, y_cs, c0, c1, c2);
        }
    }
}

// ---- the reduced-resolution pack (--face_det_scale k): image b of y [B,Hd,Wd,y_cs] is the pack of cv2.resize(frame b, (Wd, Hd)),
// the arithmetic of resize_px / resize_rows_kernel (resize_px.h, resize.hip) followed by s3fd_pixel, so the result is byte-equal
// to w2l_resize_rows_u8 into a scratch frame + w2l_s3fd_pack_rows on it - without the scratch frame.  An item is 4 neighbouring
// destination pixels of one line, as in resize_rows_kernel: the vertical tap once per item, the horizontal tap once per pixel;
// a pixel leaves as one 16-byte store (fp32 at 4 channels, bf16 at 8).  The two tap-free branches read contiguous bytes (12 of
// one line for the copy, 24 of each of two lines for the exact 2x average): dword loads where their address is 4-byte aligned -
// frames lie at any byte address and Ws * 3 is rarely a multiple of 4, so that is decided per line segment.  The bilinear branch
// gathers bytes (neighbouring items share source pixels: L1/L2 hits).  HBM-bound: reads <= Hs*Ws*3 bytes, writes Hd*Wd*16; no LDS.
template <int N>
__device__ __forceinline__ void load_span(const uint8_t* __restrict__ p, uint8_t out[N]) {
    static_assert(N % 4 == 0, "whole dwords");
    if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int k = 0; k < N / 4; ++k) {
            const uint32_t v = q[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) out[4 * k + e] = (uint8_t)(v >> (8 * e));
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = p[k];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void s3fd_pack_rows_scaled_kernel(int Hs, int Ws, int Hd, int Wd,
                                                                    const uint64_t* __restrict__ frames, T* __restrict__ y,
                                                                    int y_cs, float m0, float m1, float m2) {
    const int b = blockIdx.y;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(frames[b]);
    const long long sstride = (long long)Ws * 3;
    T* yb = y + (long long)b * Hd * Wd * y_cs;
    const int groups = (Wd + 3) >> 2;
    const int nitems = Hd * groups;                     // <= Hd*Wd <= 2^29 (checked by the entry point)
    const bool same = Hs == Hd && Ws == Wd, half = Hs == 2 * Hd && Ws == 2 * Wd;
    for (int item = blockIdx.x * blockDim.x + threadIdx.x; item < nitems; item += gridDim.x * blockDim.x) {
        const int dy = item / groups, x0 = (item - dy * groups) << 2;
        const int np = min(4, Wd - x0);
        uint8_t px[4][3];
        if (same && np == 4) {
            uint8_t raw[12];
            load_span<12>(src + dy * sstride + (long long)x0 * 3, raw);
#pragma unroll
            for (int k = 0; k < 12; ++k) px[k / 3][k % 3] = raw[k];
        } else if (half && np == 4) {
            const uint8_t* p0 = src + (2 * dy) * sstride + (long long)x0 * 6;
            uint8_t r0[24], r1[24];
            load_span<24>(p0, r0);
            load_span<24>(p0 + sstride, r1);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    px[k][c] = (uint8_t)(((int)r0[6 * k + c] + r0[6 * k + 3 + c] + r1[6 * k + c] + r1[6 * k + 3 + c] + 2) >> 2);
        } else if (same || half) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < np) resize_px(src, sstride, Hs, Ws, x0 + k, dy, Wd, Hd, px[k]);
        } else {
            const AxisTap ty = axis_tap(dy, Hs, Hd, false);
            const uint8_t* r0 = src + ty.s0 * sstride;
            const uint8_t* r1 = src + ty.s1 * sstride;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < np) lerp_px(r0, r1, axis_tap(x0 + k, Ws, Wd, true), ty, px[k]);
        }
        T* o = yb + ((long long)dy * Wd + x0) * y_cs;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < np) {
                float c0, c1, c2;
                s3fd_pixel(px[k], m0, m1, m2, c0, c1, c2);
                s3fd_store_px(o + (long long)k * y_cs, y_cs, c0, c1, c2);
            }
        }
    }
}

// one thread per (output pixel, 16-byte channel group); a maximum of bf16 values is exact
template <class S>
__global__ void maxpool2x2_kernel(int N, int H, int W, int CG, const typename S::elem* __restrict__ x, int x_cs,
                                  typename S::elem* __restrict__ y, int y_cs) {
    constexpr int VEC = S::VEC;
    const int Ho = H / 2, Wo = W / 2;
    const long long total = (long long)N * Ho * Wo * CG;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cg = (int)(i % CG);
        long long pix = i / CG;
        const int ox = (int)(pix % Wo);
        pix /= Wo;
        const int oy = (int)(pix % Ho);
        const int n = (int)(pix / Ho);
        const typename S::elem* p = x + (((long long)n * H + 2 * oy) * W + 2 * ox) * x_cs + cg * VEC;
        float a[VEC], b[VEC], c[VEC], d[VEC], o[VEC];
        S::ld(p, a);
        S::ld(p + x_cs, b);
        S::ld(p + (long long)W * x_cs, c);
        S::ld(p + (long long)W * x_cs + x_cs, d);
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = fmaxf(fmaxf(a[e], b[e]), fmaxf(c[e], d[e]));
        S::st(y + (((long long)n * Ho + oy) * Wo + ox) * y_cs + cg * VEC, o);
    }
}

// A lane's sum of squares grows by one vector.  The two storages add in different orders - fp32 the four products first, bf16 the
// eight one after the other - and each keeps its own: the detector's boxes do not move by a bit.
__device__ __forceinline__ float add_squares(float s, const float (&v)[4]) {
    return s + (v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
}
__device__ __forceinline__ float add_squares(float s, const float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e] * v[e];
    return s;
}

// one wave per pixel, a lane takes 16 bytes of every 64 * VEC channels: fp32 sum of squares over the channels, then
// x / norm * weight[c] in fp32 (bf16: rounded once on the store)
template <class S>
__global__ void l2norm_scale_kernel(long long rows, int C, const typename S::elem* __restrict__ x, int x_cs,
                                    const float* __restrict__ w, typename S::elem* __restrict__ y, int y_cs) {
    constexpr int VEC = S::VEC;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const typename S::elem* p = x + row * x_cs;
    float s = 0.f;
    for (int c = lane * VEC; c < C; c += 64 * VEC) {
        float v[VEC];
        S::ld(p + c, v);
        s = add_squares(s, v);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float norm = sqrtf(s) + 1e-10f;
    for (int c = lane * VEC; c < C; c += 64 * VEC) {
        float v[VEC], ww[VEC], o[VEC];
        S::ld(p + c, v);
        ldv<VEC>(w + c, ww);
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = v[e] / norm * ww[e];
        S::st(y + row * y_cs + c, o);
    }
}

// one thread per feature-map position: (x1, y1, x2, y2, score)
__global__ void s3fd_decode_kernel(int B, int FH, int FW, int stride, const float* __restrict__ cls, int cls_cs, int ncls,
                                   const float* __restrict__ reg, int reg_cs, float* __restrict__ out) {
    const long long total = (long long)B * FH * FW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        s3fd_decode_px(cls + i * cls_cs, ncls, reg + i * reg_cs, stride, (int)(i % FW), (int)((i / FW) % FH), out + i * 5);
}


// ---- greedy non-maximum suppression of one image's candidate boxes (bbox.py:44-64; sfd_detector.py:39-45 gates the
// candidates at score > 0.05 first).  One 1024-thread workgroup per image:
//   1. candidates = table rows with score > gate, as 64-bit keys (score bits << 32 | row): positive floats order like their bit
//      patterns, so a descending key order is "score descending, later row first among equal scores" - the order a reversed
//      stable ascending sort gives (the reference reverses numpy's unstable argsort: equal scores have no defined order there)
//   2. rank sort: rank[c] = #{j : key[j] > key[c]} (all pairs, n^2 / 1024 compares per thread: a few hundred candidates per
//      frame, 10^4 at worst), order[rank] = row
//   3. the reference's loop: the best remaining box is kept; every remaining box whose overlap with it is NOT <= thresh is
//      removed (a NaN overlap - empty union - removes, as `np.where(ovr <= thresh)` does).  "Remaining" is a bit per
//      candidate in LDS; one parallel pass + one barrier per KEPT box.
// The overlap is the reference's float32 expression, operation by operation, no contraction: w * h / (area_i + area_j - w * h)
// with area = (x2 - x1 + 1) * (y2 - y1 + 1), so the keep list is bit-exact.
constexpr int kNmsThreads = 1024;
constexpr int kNmsMaxCand = 1 << 18;              // remaining-bits in LDS: 32 KB; bounds the boxes that PASS THE GATE, not the table

// sort key of a score: order-preserving for every float (sign bit set -> all bits flipped, else the sign bit set), so that negative
// scores and -0.0 rank below the positive ones as bbox.py:50 `scores.argsort()[::-1]` ranks them; ties by the higher row index
__device__ __forceinline__ unsigned nms_score_key(float sc) {
    const unsigned u = __float_as_uint(sc);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float nms_area(const float* b) {
    return __fmul_rn(__fadd_rn(__fsub_rn(b[2], b[0]), 1.f), __fadd_rn(__fsub_rn(b[3], b[1]), 1.f));
}

__global__ __launch_bounds__(kNmsThreads) void s3fd_nms_kernel(int P, const float* __restrict__ table, float gate, float thresh,
                                                               unsigned long long* __restrict__ keys, int* __restrict__ order,
                                                               int* __restrict__ keep, int* __restrict__ counts) {
    __shared__ unsigned s_alive[kNmsMaxCand / 32];
    __shared__ int s_n, s_kept;
    const int b = blockIdx.x, t = threadIdx.x;
    const float* tb = table + (long long)b * P * 5;
    unsigned long long* kb = keys + (long long)b * P;
    int* ob = order + (long long)b * P;
    int* kp = keep + (long long)b * P;
    if (t == 0) { s_n = 0; s_kept = 0; }
    __syncthreads();
    for (int i = t; i < P; i += kNmsThreads) {
        const float sc = tb[i * 5 + 4];
        if (sc > gate) kb[atomicAdd(&s_n, 1)] = ((unsigned long long)nms_score_key(sc) << 32) | (unsigned)i;
    }
    __syncthreads();
    const int n = s_n;
    if (n > kNmsMaxCand) {          // more survivors of the gate than the alive bitmap holds: reported, the caller's host pass runs
        if (t == 0) counts[b] = -1;
        return;
    }
    for (int c = t; c < n; c += kNmsThreads) {
        const unsigned long long k = kb[c];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += kb[j] > k ? 1 : 0;
        ob[rank] = (int)(k & 0xffffffffu);
    }
    for (int w = t; w < (n + 31) / 32; w += kNmsThreads) s_alive[w] = 0xffffffffu;
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        if (!((s_alive[i >> 5] >> (i & 31)) & 1u)) continue;      // uniform: written before the last barrier
        const float* bi = tb + ob[i] * 5;
        const float x1 = bi[0], y1 = bi[1], x2 = bi[2], y2 = bi[3];
        const float ai = nms_area(bi);
        if (t == 0) kp[s_kept++] = ob[i];
        for (int j = i + 1 + t; j < n; j += kNmsThreads) {
            if (!((s_alive[j >> 5] >> (j & 31)) & 1u)) continue;
            const float* bj = tb + ob[j] * 5;
            const float xx1 = fmaxf(x1, bj[0]), yy1 = fmaxf(y1, bj[1]), xx2 = fminf(x2, bj[2]), yy2 = fminf(y2, bj[3]);
            const float w = fmaxf(0.f, __fadd_rn(__fsub_rn(xx2, xx1), 1.f)), h = fmaxf(0.f, __fadd_rn(__fsub_rn(yy2, yy1), 1.f));
            const float inter = __fmul_rn(w, h);
            const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ai, nms_area(bj)), inter));
            if (!(ovr <= thresh)) atomicAnd(&s_alive[j >> 5], ~(1u << (j & 31)));
        }
        __syncthreads();
    }
    if (t == 0) counts[b] = s_kept;
}

// ---- the per-frame rect of get_detections_for_batch (api.py:61-77) from the NMS output: the first kept row, in keep order, whose
// score is > thresh (sfd_detector.py:45 `x[-1] > 0.5`, then d[0]), its coordinates clipped at 0 (`np.clip(d, 0, None)`) and
// truncated as Python's int() truncates.  One wave per image scans the keep list 64 entries at a time; the lowest lane that
// decides (a passing row, or a row index outside the table) writes the image's result.  A coordinate Python's int() would
// refuse or that int32 cannot hold (NaN, inf, >= 2^31) is not converted: the image is flagged and the caller's host rule runs.
// kScaled (w2l_s3fd_first_rect_scaled, the detector ran on a reduced frame): x1, x2 are multiplied by sx and y1, y2 by sy first -
// one fp32 multiply each, never contracted - and the clip, the truncation and the flag are decided on the product.
constexpr int kRectNone = 0, kRectFound = 1, kRectHost = 2;

template <bool kScaled>
__global__ __launch_bounds__(64) void s3fd_first_rect_kernel(int P, const float* __restrict__ table, const int* __restrict__ keep,
                                                             const int* __restrict__ counts, float thresh, float sx, float sy,
                                                             int* __restrict__ rects, int* __restrict__ flags) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* tb = table + (long long)b * P * 5;
    const int* kp = keep + (long long)b * P;
    const int n = counts[b];
    int* r = rects + (long long)b * 4;
    if (n < 0 || n > P) {                               // not a final count (an unresolved overflow): the host decides
        if (lane == 0) { r[0] = r[1] = r[2] = r[3] = 0; flags[b] = kRectHost; }
        return;
    }
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        int row = -1;
        bool bad = false, pass = false;
        if (i < n) {
            row = kp[i];
            bad = row < 0 || row >= P;
            pass = !bad && tb[(long long)row * 5 + 4] > thresh;
        }
        const unsigned long long hit = __ballot(bad || pass);
        if (hit == 0ull) continue;                      // uniform: every lane sees the same ballot
        if (lane == __ffsll((long long)hit) - 1) {
            int flag = kRectFound, v[4] = {0, 0, 0, 0};
            if (bad) flag = kRectHost;
            else {
                const float* d = tb + (long long)row * 5;
                for (int k = 0; k < 4; ++k) {
                    const float c = kScaled ? __fmul_rn(d[k], (k & 1) ? sy : sx) : d[k];
                    const float x = c > 0.f ? c : 0.f;
                    if (!(c == c) || !(x < 2147483648.f)) { flag = kRectHost; break; }       // NaN, +inf, >= 2^31
                    v[k] = (int)x;                                                          // x >= 0: truncation = int()
                }
                if (flag == kRectHost) v[0] = v[1] = v[2] = v[3] = 0;
            }
            r[0] = v[0]; r[1] = v[1]; r[2] = v[2]; r[3] = v[3];
            flags[b] = flag;
        }
        return;
    }
    if (lane == 0) { r[0] = r[1] = r[2] = r[3] = 0; flags[b] = kRectNone; }
}

// ---- tracked face selection (opt-in; not the reference's rule, which is s3fd_first_rect_kernel's d[0]).
// Candidates of a frame: the first K rows of the keep list, in its order, whose score is > thresh, each converted as
// s3fd_first_rect_kernel converts its one row (one __fmul_rn by sx / sy - a multiply by 1.0f gives the same bits, so one body
// serves both - the clip at 0, the truncation).  One wave per image scans the keep list 64 entries at a time; a ballot and the
// popcount of the lanes below give a passing lane its slot, and the scan stops after the K-th passing row: rows after it are not
// looked at, so a keep entry outside the table counts only up to and including that row.  A coordinate that is NaN or above
// 32767 after the clip and the truncation (that covers +inf and >= 2^31) flags the frame: with coordinates in 0..32767 every
// product of the track below is exact in int64.  A flagged frame has no candidates, and unused slots are zeros.
constexpr int kTrackMaxCands = 16;
constexpr int kTrackMaxCoord = 32767;

__global__ __launch_bounds__(64) void s3fd_top_rects_kernel(int P, const float* __restrict__ table, const int* __restrict__ keep,
                                                            const int* __restrict__ counts, float thresh, float sx, float sy, int K,
                                                            int* __restrict__ cands, int* __restrict__ ncand, int* __restrict__ flags) {
    __shared__ int s_c[kTrackMaxCands][4];
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* tb = table + (long long)b * P * 5;
    const int* kp = keep + (long long)b * P;
    const int n = counts[b];
    int* cb = cands + (long long)b * K * 4;
    bool host = n < 0 || n > P;                         // not a final count (an unresolved overflow): the host decides
    int taken = 0;
    for (int base = 0; !host && taken < K && base < n; base += 64) {      // uniform: host and taken are the same on every lane
        const int i = base + lane;
        int row = -1;
        bool bad = false, pass = false;
        if (i < n) {
            row = kp[i];
            bad = row < 0 || row >= P;
            pass = !bad && tb[(long long)row * 5 + 4] > thresh;
        }
        const unsigned long long passing = __ballot(pass);
        const int slot = taken + __popcll(passing & ((1ull << lane) - 1ull));      // passing rows before this one
        const bool examined = i < n && slot < K;        // up to and including the K-th passing row
        bool refuse = bad && examined;
        if (pass && examined) {
            const float* d = tb + (long long)row * 5;
            for (int k = 0; k < 4; ++k) {
                const float c = __fmul_rn(d[k], (k & 1) ? sy : sx);
                const float x = c > 0.f ? c : 0.f;
                if (!(c == c) || !(x < (float)(kTrackMaxCoord + 1))) { refuse = true; break; }
                s_c[slot][k] = (int)x;                  // x >= 0: truncation = int()
            }
        }
        host = __ballot(refuse) != 0ull;
        taken = min(K, taken + __popcll(passing));
    }
    __syncthreads();
    if (lane < 4 * K) cb[lane] = (!host && (lane >> 2) < taken) ? s_c[lane >> 2][lane & 3] : 0;
    if (lane == 0) {
        ncand[b] = host ? 0 : taken;
        flags[b] = host ? kRectHost : (taken > 0 ? kRectFound : kRectNone);
    }
}

// The track over a clip (or over the frames a live stream adds in a tick): one wave per segment walks its frames in order with the
// state (ref rect, has, missed) in registers, the same on every lane.  Lane k < K holds candidate k of the frame; the next frame's
// candidates are loaded while this one decides.  All integer arithmetic: inter = max(0, min(x2) - max(x1)) * max(0, min(y2) -
// max(y1)), union = area(c) + area(ref) - inter, no + 1; a candidate continues the track when inter > 0 and inter * 256 >=
// q * union (then both rects have positive sides and union > 0), the largest IoU wins - inter_a * union_b > inter_b * union_a in
// int64 - and ties go to the lower index.  Without a track the frame's candidates seed one by `pick`, ties to the lower index.
// A frame flagged neither found nor none is written as kRectHost with zeros and leaves the state alone.
struct TrackSeg { int row0, n, slot, seen; };
static_assert(sizeof(TrackSeg) == 16 && sizeof(w2l_track_segment) == 16, "w2l_track_segment is 16 bytes");
constexpr int kTrackStateInts = 8;                      // (x1, y1, x2, y2, has, missed, 0, 0)
constexpr int kTrackBadSegment = 3;                     // status of a segment that is not followed (as kBoxStreamBadSegment)
constexpr int kTrackMaxReseed = 250;                    // missed frames tolerated at the most
constexpr int kPickScore = 0, kPickLargest = 1, kPickLeft = 2, kPickRight = 3;
typedef int i32x4 __attribute__((ext_vector_type(4)));

// the lowest lane of each group of 16 ends up with the group's minimum of (key, index): lanes 0..15 hold the candidates
__device__ __forceinline__ int track_argmin(long long key, int idx) {
    for (int o = 8; o > 0; o >>= 1) {
        const long long k2 = __shfl_xor(key, o);
        const int i2 = __shfl_xor(idx, o);
        if (k2 < key || (k2 == key && i2 < idx)) { key = k2; idx = i2; }
    }
    return __shfl(idx, 0);
}

__global__ __launch_bounds__(64) void face_track_segments_kernel(const TrackSeg* __restrict__ segs, const int* __restrict__ cands,
                                                                 const int* __restrict__ ncand, const int* __restrict__ cflags,
                                                                 int n_rows, int K, int pick, int L, int q, int* __restrict__ state,
                                                                 int n_slots, int* __restrict__ rects, int* __restrict__ flags,
                                                                 int* __restrict__ status) {
    const int lane = threadIdx.x;
    const TrackSeg s = segs[blockIdx.x];
    if (s.n < 0 || s.row0 < 0 || (long long)s.row0 + s.n > n_rows || s.slot < -1 || s.slot >= n_slots || s.seen < 0) {    // uniform
        if (lane == 0) status[blockIdx.x] = kTrackBadSegment;
        return;
    }
    if (lane == 0) status[blockIdx.x] = 0;
    int rx1 = 0, ry1 = 0, rx2 = 0, ry2 = 0, has = 0, missed = 0;
    int* slot = s.slot >= 0 ? state + (long long)s.slot * kTrackStateInts : nullptr;
    if (slot && s.seen > 0) {                           // read before anything is written: every lane takes the same words
        rx1 = slot[0]; ry1 = slot[1]; rx2 = slot[2]; ry2 = slot[3];
        has = slot[4] != 0;
        missed = min(max(slot[5], 0), kTrackMaxReseed + 1);
    }
    const bool mine = lane < K;
    auto load = [&](int i, i32x4* c, int* nc, int* cf) {
        const long long row = (long long)s.row0 + i;
        *c = mine ? *reinterpret_cast<const i32x4*>(cands + (row * K + lane) * 4) : i32x4{0, 0, 0, 0};
        *nc = ncand[row];
        *cf = cflags[row];
    };
    i32x4 c_next = {0, 0, 0, 0};
    int nc_next = 0, cf_next = kRectNone;
    if (s.n > 0) load(0, &c_next, &nc_next, &cf_next);
    for (int i = 0; i < s.n; ++i) {
        const i32x4 c = c_next;
        const int cf = cf_next;
        const int nc = cf == kRectFound ? min(max(nc_next, 0), K) : 0;
        if (i + 1 < s.n) load(i + 1, &c_next, &nc_next, &cf_next);
        const long long row = (long long)s.row0 + i;
        int out_flag = kRectNone, best = -1;
        if (cf != kRectFound && cf != kRectNone) out_flag = kRectHost;      // uniform from here on: cf, nc and the state are
        else {
            const bool valid = lane < nc;
            const long long area = (long long)(c.z - c.x) * (c.w - c.y);
            if (has) {
                const long long iw = max(0, min(c.z, rx2) - max(c.x, rx1)), ih = max(0, min(c.w, ry2) - max(c.y, ry1));
                long long inter = iw * ih;
                long long uni = area + (long long)(rx2 - rx1) * (ry2 - ry1) - inter;
                int idx = lane;
                if (!(valid && inter > 0 && inter * 256 >= (long long)q * uni)) { inter = 0; uni = 1; idx = 0x7fffffff; }
                for (int o = 8; o > 0; o >>= 1) {       // the group's best (IoU, then the lower index) on each of its lanes
                    const long long i2 = __shfl_xor(inter, o), u2 = __shfl_xor(uni, o);
                    const int x2 = __shfl_xor(idx, o);
                    const long long a = i2 * uni, bb = inter * u2;
                    if (a > bb || (a == bb && x2 < idx)) { inter = i2; uni = u2; idx = x2; }
                }
                idx = __shfl(idx, 0);
                if (idx != 0x7fffffff) best = idx;
                else if (++missed > L) has = 0;         // the track is dropped and seeded again on this same frame
            }
            if (!has && nc > 0) {
                long long key = 0;
                if (pick == kPickLargest) key = -area;
                else if (pick == kPickLeft) key = (long long)c.x + c.z;
                else if (pick == kPickRight) key = -((long long)c.x + c.z);
                best = track_argmin(valid ? key : 0x7fffffffffffffffll, valid ? lane : 0x7fffffff);
            }
            if (best >= 0) {
                rx1 = __shfl(c.x, best); ry1 = __shfl(c.y, best); rx2 = __shfl(c.z, best); ry2 = __shfl(c.w, best);
                has = 1;
                missed = 0;
                out_flag = kRectFound;
            }
        }
        if (lane == 0) {
            const bool found = out_flag == kRectFound;
            *reinterpret_cast<i32x4*>(rects + row * 4) = found ? i32x4{rx1, ry1, rx2, ry2} : i32x4{0, 0, 0, 0};
            flags[row] = out_flag;
        }
    }
    if (slot && lane < kTrackStateInts) {               // without a track the rect and the count mean nothing: zeros
        const int w[kTrackStateInts] = {has ? rx1 : 0, has ? ry1 : 0, has ? rx2 : 0, has ? ry2 : 0, has, has ? missed : 0, 0, 0};
        slot[lane] = w[lane];
    }
}

// ---- every face of a segment (opt-in `all_faces`): the same candidates, the same integer overlap and the same L,
// but F track slots at once instead of one reference rect.  One wave per segment walks the frames in order.  Lane t < F owns slot
// t - (ref rect, alive, missed) in its registers - and lane c < K holds candidate c; the next frame's candidates are loaded while
// this one decides.  Per frame the refs and the candidates go through a few hundred bytes of LDS, from which the F * K <= 256
// pairs (slot p / K, candidate p % K, pair p = lane + 64 j) take their inter and union, four per lane.  A greedy round is one
// wave argmax over the pairs still in the contest - the largest IoU by the cross-multiplied int64 comparison, ties to the lower
// key slot * 16 + candidate - and removes its slot and its candidate; the rounds end when no overlapping pair is left, after at
// most min(alive, m) of them.  The masks of slots and candidates still in the contest are the same on every lane, so every branch
// of the walk is uniform.  Then the misses, and the seeds: the i-th unclaimed candidate takes the i-th lowest free slot.
constexpr int kFacesMaxSlots = 16;
struct BoxSeg { int row0, n, H, W; };
static_assert(sizeof(BoxSeg) == 16 && sizeof(w2l_box_segment) == 16, "w2l_box_segment is 16 bytes");

__global__ __launch_bounds__(64) void face_tracks_all_segments_kernel(const BoxSeg* __restrict__ segs, const int* __restrict__ cands,
                                                                      const int* __restrict__ ncand, const int* __restrict__ cflags,
                                                                      int n_rows, int K, int F, int L, int q, int* __restrict__ rects_out,
                                                                      int* __restrict__ flags_out, int* __restrict__ status) {
    __shared__ i32x4 s_c[kTrackMaxCands];
    __shared__ i32x4 s_ref[kFacesMaxSlots];
    const int lane = threadIdx.x;
    const BoxSeg s = segs[blockIdx.x];
    int* st = status + (long long)blockIdx.x * 4;
    if (s.n < 0 || s.row0 < 0 || (long long)s.row0 + s.n > n_rows) {       // uniform
        if (lane < 4) st[lane] = lane == 0 ? kTrackBadSegment : 0;
        return;
    }
    const bool mine = lane < K, owner = lane < F;
    int ps[4], pc[4];                                       // the slot and the candidate of this lane's four pairs; -1: no pair
    for (int j = 0; j < 4; ++j) {
        const int p = lane + 64 * j;
        ps[j] = p < F * K ? p / K : -1;
        pc[j] = p < F * K ? p % K : -1;
    }
    i32x4 ref = {0, 0, 0, 0};
    int alive = 0, missed = 0, started = 0, dropped = 0, peak = 0;
    auto load = [&](int i, i32x4* c, int* nc, int* cf) {
        const long long row = (long long)s.row0 + i;
        *c = mine ? *reinterpret_cast<const i32x4*>(cands + (row * K + lane) * 4) : i32x4{0, 0, 0, 0};
        *nc = ncand[row];
        *cf = cflags[row];
    };
    i32x4 c_next = {0, 0, 0, 0};
    int nc_next = 0, cf_next = kRectNone;
    if (s.n > 0) load(0, &c_next, &nc_next, &cf_next);
    for (int i = 0; i < s.n; ++i) {
        const i32x4 c = c_next;
        const int cf = cf_next;
        const int m = cf == kRectFound ? min(max(nc_next, 0), K) : 0;
        if (i + 1 < s.n) load(i + 1, &c_next, &nc_next, &cf_next);
        const long long row = (long long)s.row0 + i;
        int out_flag = kRectNone;
        if (cf != kRectFound && cf != kRectNone) out_flag = kRectHost;      // uniform: the state is left alone
        else {
            __syncthreads();                                // the frame before has read its candidates
            if (mine) s_c[lane] = c;
            if (owner) s_ref[lane] = ref;
            unsigned av_s = (unsigned)__ballot(owner && alive);             // slots and candidates still in the contest
            unsigned av_c = (1u << m) - 1u;
            __syncthreads();
            long long inter[4], uni[4];
            for (int j = 0; j < 4; ++j) {
                inter[j] = 0;
                uni[j] = 1;
                if (ps[j] >= 0 && ((av_s >> ps[j]) & 1u) && pc[j] < m) {
                    const i32x4 a = s_c[pc[j]], r = s_ref[ps[j]];
                    const long long iw = max(0, min(a.z, r.z) - max(a.x, r.x)), ih = max(0, min(a.w, r.w) - max(a.y, r.y));
                    const long long in = iw * ih;
                    const long long un = (long long)(a.z - a.x) * (a.w - a.y) + (long long)(r.z - r.x) * (r.w - r.y) - in;
                    if (in > 0 && in * 256 >= (long long)q * un) { inter[j] = in; uni[j] = un; }
                }
            }
            while (av_s != 0u && av_c != 0u) {              // at most min(alive, m) rounds
                long long bi = 0, bu = 1;
                int bk = 0x7fffffff;
                for (int j = 0; j < 4; ++j) {               // this lane's best pair; its keys rise with j
                    if (inter[j] > 0 && ((av_s >> ps[j]) & 1u) && ((av_c >> pc[j]) & 1u) && inter[j] * bu > bi * uni[j]) {
                        bi = inter[j]; bu = uni[j]; bk = ps[j] * 16 + pc[j];
                    }
                }
                for (int o = 32; o > 0; o >>= 1) {          // the wave's best (IoU, then the lower key) on every lane
                    const long long i2 = __shfl_xor(bi, o), u2 = __shfl_xor(bu, o);
                    const int k2 = __shfl_xor(bk, o);
                    const long long a = i2 * bu, b = bi * u2;
                    if (a > b || (a == b && k2 < bk)) { bi = i2; bu = u2; bk = k2; }
                }
                if (bk == 0x7fffffff) break;                // uniform: every lane holds the same pair
                const int ms = bk >> 4, mc = bk & 15;
                av_s &= ~(1u << ms);
                av_c &= ~(1u << mc);
                if (lane == ms) { ref = s_c[mc]; missed = 0; out_flag = kRectFound; }
            }
            if (owner && alive && ((av_s >> lane) & 1u) && ++missed > L) { alive = 0; missed = 0; }      // not matched
            const unsigned free_s = ~(unsigned)__ballot(owner && alive) & ((1u << F) - 1u);    // a slot freed just now counts
            const int n_free = __popc(free_s), n_left = __popc(av_c);
            started += min(n_free, n_left);
            dropped += max(0, n_left - n_free);
            if (owner && ((free_s >> lane) & 1u)) {
                const int rank = __popc(free_s & ((1u << lane) - 1u));      // the rank-th free slot takes the rank-th unclaimed
                if (rank < n_left) {
                    unsigned left = av_c;
                    for (int k = 0; k < rank; ++k) left &= left - 1u;
                    ref = s_c[__ffs(left) - 1];
                    alive = 1;
                    missed = 0;
                    out_flag = kRectFound;
                }
            }
            peak = max(peak, __popc((unsigned)__ballot(owner && alive)));
        }
        if (owner) {
            const long long o = (long long)lane * n_rows + row;
            *reinterpret_cast<i32x4*>(rects_out + o * 4) = out_flag == kRectFound ? ref : i32x4{0, 0, 0, 0};
            flags_out[o] = out_flag;
        }
    }
    if (lane < 4) st[lane] = lane == 0 ? 0 : lane == 1 ? started : lane == 2 ? dropped : peak;
}

// ---- the per-clip finish of face_detect (inference.py:90-104; gen_videos_from_filelist.py:61-77 is the same code) for many
// clips: one wave per segment = one clip's rows [row0, row0 + n) of the rect / flag arenas w2l_s3fd_first_rect filled.
//   1. the flags: any row the device did not convert (kRectHost, or a word that is no flag at all) -> status (2, first such row):
//      the detector would have met it before face_detect looks for None; else, in the strict mode, any kRectNone -> (1, first such
//      row), the "Face not detected" ValueError; boxes of such a segment are zeros.
//   2. the padded box of a row, in the output's (y1, y2, x1, x2) order: (max(0, y1 - top), min(H, y2 + bottom), max(0, x1 - left),
//      min(W, x2 + right)) - near edges clipped at 0 and far edges at the frame ONLY, as there.
//   3. get_smoothened_boxes (inference.py:59-66), in place and in row order: row i <= n - T is the mean of the T unsmoothed rows
//      from i on (every row of its window comes after it), so those rows are independent and go lane by lane.  The rows after
//      that all take Python's `boxes[n - T:]`: rows [ws, n) with ws = n - T, or for n < T the wrapped negative start
//      max(0, 2n - T); that window holds rows already smoothed, so they run in order - one lane per coordinate (the four columns
//      never mix) over a copy of the window in LDS.  A mean is an exact integer sum, one fp64 division, truncation towards zero:
//      numpy's float64 mean assigned into an integer array.
// face_boxes_runs_wave below is the one device statement of steps 2 and 3, for clips and for live streams, strict or with the
// pass-through for frames without a face.
constexpr int kBoxMaxT = 64;

template <class Seg>      // BoxSeg or BoxStreamSeg: anything with the frame size H, W
__device__ __forceinline__ int padded_coord(const int* r, int c, const Seg& s, int top, int bottom, int left, int right) {
    long long v;
    if (c == 0) v = max(0ll, (long long)r[1] - top);
    else if (c == 1) v = min((long long)s.H, (long long)r[3] + bottom);
    else if (c == 2) v = max(0ll, (long long)r[0] - left);
    else v = min((long long)s.W, (long long)r[2] + right);
    return (int)v;
}

__device__ __forceinline__ int trunc_mean(long long sum, int len) { return (int)((double)sum / (double)len); }

// ---- the same finish for LIVE streams, one launch per tick (inference.py:59-66, :90-104): one wave per segment = the rows one
// stream added to the arenas in this tick.  get_smoothened_boxes looks FORWARD: box i <= n - T is the mean of the unsmoothed
// rows i .. i + T - 1, so it is final once row i + T - 1 is there, whatever follows; only the rows after n - T depend on the end
// (the in-place boxes[n - T:] window).  The strict stream therefore carries its last max(T, 1) RAW rects from tick to tick (a slot
// of `carry`, [kBoxMaxT][4]: its first min(n, max(T, 1)) rows are rewritten, no other word), and the rows a launch holds are
// [carry: min(seen, max(T, 1)) rows][the new rows]  = frames [seen - carried, n), n = seen + n_new.  While open it writes frames
// [max(0, seen - T + 1), max(0, n - T + 1)) by the forward rule; with `closed` every remaining frame by step 3's tail on the whole
// length n - its entry n - T, already smoothed there, is the forward mean of raw rows and is computed again.  The slot is read
// into LDS before anything is written to it.
struct BoxStreamSeg { int row0, n_new, H, W, slot, seen, closed, out0; };
static_assert(sizeof(BoxStreamSeg) == 32 && sizeof(w2l_box_stream_segment) == 32, "w2l_box_stream_segment is 32 bytes");
constexpr int kBoxStreamBadSegment = 3;

// frames [lo, hi) are what a tick writes for a segment (host and device: the same expression)
__host__ __device__ inline void box_stream_range(long long seen, long long n, int closed, int T, long long* lo, long long* hi) {
    if (T == 0) { *lo = seen; *hi = n; return; }
    *lo = seen - T + 1 > 0 ? seen - T + 1 : 0;
    *hi = closed ? n : (n - T + 1 > 0 ? n - T + 1 : 0);
}

// ---- the finish with "no face" as a state of a frame instead of the end of its clip (the opt-in pass-through).
// One rule for clips and streams:
//   hold   an undetected frame i takes the raw rect of the last detected frame p < i while i - p <= hold (it is BOXED, as a
//          detected frame is); else, and before the first detection, it is a GAP: box zeros, valid 0.
//   runs   maximal sequences of boxed frames; each is finished by steps 2 and 3 above as a clip of those frames alone.
// The strict finish is the case in which every frame is detected: one run that ends at the close, no gap, and no `valid` output.
// A wave walks its frames in chunks of 64 with three chunks of held-filled rows (x1, y1, x2, y2, boxed) in an LDS ring: the fill of a
// chunk is a max-scan for "last detected frame" continued from the chunk before; a boxed frame i whose next T - 1 frames are all
// boxed takes the forward mean of raw rows (those reach into the next chunk), any other boxed frame lies in the tail of its run,
// and the tail of a run that ends at b (frame b is a gap, or the end of a closed video) reads raw rows back to b - T (those reach
// into the chunk before; frames before the first one held count as gaps, which gives a run shorter than T its wrapped window)
// and runs in order, one lane per coordinate.  T = 0 is T = 1 here: the truncated mean of one integer.
// The pass-through stream holds the frames [seen - min(seen, 2T), seen) in its carry slot: a run may have ended up to T - 2 frames
// before the tick's first new frame and its tail then reads back to seen - 2T + 2.  The strict stream's only tail is the one at
// the close, which reads back to n - T >= seen - T: its min(seen, T) raw rects suffice, and enter the ring as boxed rows.
constexpr int kHoldMax = 250;                            // frames a rect is held for at the most
constexpr int kRunsCarryRows = 2 * kBoxMaxT;             // rows of a slot: (x1, y1, x2, y2, boxed) of the last 2 * max(T, 1) frames
constexpr int kRunsCarryInts = kRunsCarryRows * 5 + 4;   // then (frames since the last detection, capped at kHoldMax + 1; 0; 0; 0)
constexpr int kRunsRing = 3 * 64;

// One segment.  Frames [f0, n) with f0 = seen - c: the c carried rows (s_carry), then rows of the arenas (rc, fl: frame `seen` is
// their row 0).  Writes boxes and valid of the frames [lo, hi) at bx / vd (frame lo is row 0 there; vd may be NULL).  Afterwards
// the ring holds the last three chunks and *p_out the last detected frame (-1: none within reach).
template <class Seg>
__device__ __forceinline__ void face_boxes_runs_wave(const Seg& s, const int* __restrict__ rc, const int* __restrict__ fl, int seen,
                                                     long long n, bool closed, int c, int dist0, int top, int bottom, int left,
                                                     int right, int Tm, int hold, long long lo, long long hi, int* __restrict__ bx,
                                                     int* __restrict__ vd, const int (*s_carry)[5], int (*s_ring)[5],
                                                     int (*s_win)[4], long long* p_out) {
    const int lane = threadIdx.x;
    const long long f0 = (long long)seen - c;
    long long p = (c > 0 && s_carry[c - 1][4] != 0 && dist0 <= hold && seen - 1 - dist0 >= 0) ? (long long)seen - 1 - dist0 : -1;
    const int nch = (int)((n - f0 + 63) / 64);
    auto fill = [&](int k) {                             // chunk k into its third of the ring; every lane takes part in the scan
        const long long g0 = f0 + 64ll * k, i = g0 + lane;
        int v = (i >= seen && i < n && fl[i - seen] == kRectFound) ? lane : -1;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(v, o);
            if (lane >= o) v = max(v, t);
        }
        const long long pl = v >= 0 ? g0 + v : p;        // the last detected frame at or before i
        int r[5] = {0, 0, 0, 0, 0};
        if (i < seen) {
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = s_carry[i - f0][q];
            r[4] = s_carry[i - f0][4] != 0;
        } else if (i < n && pl >= 0 && i - pl <= hold) {
            const int* src = pl >= seen ? rc + (pl - seen) * 4 : &s_carry[c - 1][0];
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = src[q];
            r[4] = 1;
        }
        int* dst = s_ring[(64 * k + lane) % kRunsRing];
#pragma unroll
        for (int q = 0; q < 5; ++q) dst[q] = r[q];
        const int vl = __shfl(v, 63);
        if (vl >= 0) p = g0 + vl;
    };
    auto row = [&](long long i) -> const int* { return s_ring[(int)((i - f0) % kRunsRing)]; };
    auto boxed = [&](long long i) -> bool { return i >= f0 && i < n && row(i)[4] != 0; };
    if (nch > 0) fill(0);
    for (int k = 0; k < nch; ++k) {
        if (k + 1 < nch) fill(k + 1);
        __syncthreads();
        const long long g0 = f0 + 64ll * k;
        {                                                // gap rows, and the boxed rows with T boxed rows from them on
            const long long i = g0 + lane;
            if (i >= lo && i < hi) {
                int* o = bx + (i - lo) * 4;
                const bool me = boxed(i);
                if (vd) vd[i - lo] = me;
                bool all = me;
                for (int j = 1; j < Tm && all; ++j) all = boxed(i + j);
                if (!me) o[0] = o[1] = o[2] = o[3] = 0;
                else if (all) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        long long sum = 0;
                        for (int j = 0; j < Tm; ++j) sum += padded_coord(row(i + j), q, s, top, bottom, left, right);
                        o[q] = trunc_mean(sum, Tm);
                    }
                }
            }
        }
        // the runs that end at b in (g0, g0 + 64] and have a row to write: frame b - 1 is boxed and frame b is a gap or the end
        const long long b_mine = g0 + 1 + lane;
        unsigned long long ends = __ballot(b_mine <= n && b_mine - 1 >= lo && boxed(b_mine - 1) && (b_mine == n ? closed : !boxed(b_mine)));
        while (ends != 0ull) {                           // uniform
            const long long b = g0 + __ffsll((long long)ends);
            ends &= ends - 1;
            const unsigned long long gaps = __ballot(lane < Tm && !boxed(b - 1 - lane));
            // the run's length where it is shorter than T: Python's boxes[len - T:] then wraps to max(0, 2 * len - T)
            const int len = gaps != 0ull ? __ffsll((long long)gaps) - 1 : Tm;
            const long long seq0 = b - len;              // rows from here on run in order
            const long long ws = gaps != 0ull ? seq0 + max(0, 2 * len - Tm) : seq0;
            const int L = (int)(b - ws);                 // 1 <= L <= T <= kBoxMaxT
            __syncthreads();                             // the window of the run before this one has been read
            if (lane < L) {
#pragma unroll
                for (int q = 0; q < 4; ++q) s_win[lane][q] = padded_coord(row(ws + lane), q, s, top, bottom, left, right);
            }
            __syncthreads();
            if (lane < 4) {
                for (long long i = seq0; i < b; ++i) {
                    long long sum = 0;
                    for (int j = 0; j < L; ++j) sum += s_win[j][lane];
                    const int mean = trunc_mean(sum, L);
                    if (i >= ws) s_win[i - ws][lane] = mean;
                    if (i >= lo && i < hi) bx[(i - lo) * 4 + lane] = mean;      // the others went out, or go out, in another tick
                }
            }
        }
        __syncthreads();                                 // the next fill overwrites the chunk before this one
    }
    *p_out = p;
}

// the first row of [0, n) whose flag is neither found nor none, and the first that is none (0x7fffffff: no such row), the same on
// every lane
__device__ __forceinline__ void first_unfound_rows(const int* __restrict__ fl, int n, int* host, int* none) {
    int first_host = 0x7fffffff, first_none = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 64) {
        const int f = fl[i];
        if (f == kRectNone) first_none = min(first_none, i);
        else if (f != kRectFound) first_host = min(first_host, i);
    }
    for (int o = 32; o > 0; o >>= 1) {
        first_host = min(first_host, __shfl_xor(first_host, o));
        first_none = min(first_none, __shfl_xor(first_none, o));
    }
    *host = first_host;
    *none = first_none;
}

// kStrict: a "none" row ends the segment as a host row does (a host row wins), `valid` and `hold` are not read
template <bool kStrict>
__global__ __launch_bounds__(64) void face_boxes_runs_kernel(const BoxSeg* __restrict__ segs, const int* __restrict__ rects,
                                                             const int* __restrict__ flags, int n_rows, int top, int bottom, int left,
                                                             int right, int T, int hold, int* __restrict__ boxes,
                                                             int* __restrict__ valid, int* __restrict__ status) {
    __shared__ int s_ring[kRunsRing][5];
    __shared__ int s_win[kBoxMaxT][4];
    const int lane = threadIdx.x;
    const BoxSeg s = segs[blockIdx.x];
    int* st = status + 2 * (long long)blockIdx.x;
    if (s.n <= 0 || s.row0 < 0 || (long long)s.row0 + s.n > n_rows) {       // uniform: a segment outside the arenas is not followed
        if (lane == 0) { st[0] = s.n <= 0 ? 0 : kBoxStreamBadSegment; st[1] = 0; }
        return;
    }
    const int* fl = flags + s.row0;
    int* bx = boxes + (long long)s.row0 * 4;
    int* vd = kStrict ? nullptr : valid + s.row0;
    int host, none;
    first_unfound_rows(fl, s.n, &host, &none);
    const bool is_host = host != 0x7fffffff;
    if (is_host || (kStrict && none != 0x7fffffff)) {    // uniform: left to the host, or to the caller's "Face not detected"
        for (int i = lane; i < 4 * s.n; i += 64) bx[i] = 0;
        for (int i = lane; vd && i < s.n; i += 64) vd[i] = 0;
        if (lane == 0) { st[0] = is_host ? 2 : 1; st[1] = is_host ? host : none; }
        return;
    }
    if (lane == 0) { st[0] = 0; st[1] = 0; }
    long long p;
    face_boxes_runs_wave(s, rects + (long long)s.row0 * 4, fl, 0, s.n, true, 0, kHoldMax + 1, top, bottom, left, right, max(T, 1),
                         kStrict ? 0 : hold, 0, s.n, bx, vd, nullptr, s_ring, s_win, &p);
}

// kStrict as above; the carry slot is then [kBoxMaxT][4] raw rects of the last max(T, 1) frames, every one of them boxed
template <bool kStrict>
__global__ __launch_bounds__(64) void face_boxes_stream_runs_kernel(const BoxStreamSeg* __restrict__ segs, const int* __restrict__ rects,
                                                                    const int* __restrict__ flags, int n_rows, int* __restrict__ carry,
                                                                    int n_slots, int top, int bottom, int left, int right, int T,
                                                                    int hold, int* __restrict__ boxes, int* __restrict__ valid,
                                                                    int n_out, int* __restrict__ status) {
    constexpr int kCols = kStrict ? 4 : 5;               // words of a carried row
    __shared__ int s_carry[kStrict ? kBoxMaxT : kRunsCarryRows][5];
    __shared__ int s_ring[kRunsRing][5];
    __shared__ int s_win[kBoxMaxT][4];
    const int lane = threadIdx.x;
    const BoxStreamSeg s = segs[blockIdx.x];
    int* st = status + 2 * (long long)blockIdx.x;
    // the launcher checked the host copy of the table; a device copy that says otherwise is not followed
    const long long n = (long long)s.seen + s.n_new;
    bool bad = s.n_new < 0 || s.seen < 0 || s.slot < 0 || s.slot >= n_slots || s.row0 < 0 || (long long)s.row0 + s.n_new > n_rows ||
               n > 0x7fffffffll || s.out0 < 0;
    const int Tm = max(T, 1);
    long long lo = 0, hi = 0;
    if (!bad) {
        box_stream_range(s.seen, n, s.closed, Tm, &lo, &hi);
        bad = s.out0 + (hi - lo) > n_out;
    }
    if (bad) {                                           // uniform
        if (lane == 0) { st[0] = kBoxStreamBadSegment; st[1] = 0; }
        return;
    }
    const int* fl = flags + s.row0;
    int host, none;
    first_unfound_rows(fl, s.n_new, &host, &none);
    const bool is_host = host != 0x7fffffff;
    if (is_host || (kStrict && none != 0x7fffffff)) {    // uniform: no box written, the carry left as it was
        if (lane == 0) { st[0] = is_host ? 2 : 1; st[1] = s.seen + (is_host ? host : none); }
        return;
    }
    if (lane == 0) { st[0] = 0; st[1] = 0; }
    const int reach = kStrict ? Tm : 2 * Tm;
    const int c = min(s.seen, reach);                    // carried rows: frames [seen - c, seen)
    int* slot = carry + (long long)s.slot * (kStrict ? kBoxMaxT * 4 : kRunsCarryInts);
    for (int i = lane; i < c * kCols; i += 64) s_carry[i / kCols][i % kCols] = slot[i];
    int dist0 = kHoldMax + 1;                            // frames since the last detection: beyond any hold
    if constexpr (kStrict) {
        if (lane < c) s_carry[lane][4] = 1;
    } else if (s.seen > 0) {
        dist0 = min(max(slot[kRunsCarryRows * 5], 0), kHoldMax + 1);
    }
    __syncthreads();
    long long p;
    face_boxes_runs_wave(s, rects + (long long)s.row0 * 4, fl, s.seen, n, s.closed != 0, c, dist0, top, bottom, left, right, Tm,
                         kStrict ? 0 : hold, lo, hi, boxes + (long long)s.out0 * 4, kStrict ? nullptr : valid + s.out0, s_carry,
                         s_ring, s_win, &p);
    // the next tick's carry: the last min(n, reach) rows, which the ring still holds, and the distance from the detection
    const int keep = (int)min(n, (long long)reach);
    const long long f0 = (long long)s.seen - c;
    for (int i = lane; i < keep * kCols; i += 64) slot[i] = s_ring[(int)((n - keep + i / kCols - f0) % kRunsRing)][i % kCols];
    if (!kStrict && lane == 0) {
        const long long d = p >= s.seen ? n - 1 - p : (long long)dist0 + s.n_new;
        slot[kRunsCarryRows * 5] = (int)min(d, (long long)(kHoldMax + 1));
    }
}

// ---- the span rule for finished clips (opt-in `track_spans`): which rows of a segment a scorer may see.  Unlike the
// hold it looks FORWARD: a miss between two detections p < q with q - p <= bridge + 1 is interpolated, anything else is a gap, and a
// maximal sequence of detected and bridged rows - a span, which begins and ends on a detection - is kept iff it has min_len rows and
// a mean size (the larger of the width and height sums) of min_size.  The outputs have the format of the inputs, so
// face_boxes_runs_kernel<false> with hold 0 finishes them.
// One wave per segment walks the rows in chunks of 64.  A ballot gives the chunk's detections; a lane's last detection at or before
// its row is the highest such bit at or below the lane, else the carried one, and its next one the lowest bit at or above, else the
// first detection behind the chunk (at most bridge + 1 <= 251 rows past the chunk's last row: up to four more ballots on the flags).
// Every row goes out at once as if its span were kept; the spans that END in the chunk (its last row is here; the first detection
// behind the chunk says whether the last row's span goes on) are then decided from the carried length, detection count and sums,
// and the rows of a dropped one - in this chunk and the ones before it - are zeroed again, behind a fence: other lanes wrote them.
// Span rows are written once, in order, by lane 0.
constexpr int kSpanMaxBridge = 250, kSpanMaxSize = 32767, kSpanMaxLen = 1 << 30;
constexpr int kSpanReachChunks = 4;                      // 64 * 4 rows behind a chunk cover bridge + 1 rows behind its last row
static_assert(64 * kSpanReachChunks >= kSpanMaxBridge + 1, "the next detection is looked for this far");

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ long long floor_div(long long a, long long b) {     // b > 0
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__global__ __launch_bounds__(64) void face_spans_segments_kernel(const BoxSeg* __restrict__ segs, const int* rects, const int* flags,
                                                                 int n_rows, int bridge, int min_len, int min_size, int* rects_out,
                                                                 int* flags_out, int* spans, int* __restrict__ status) {
    const int lane = threadIdx.x;
    const BoxSeg s = segs[blockIdx.x];
    int* st = status + 2 * (long long)blockIdx.x;
    if (s.n <= 0 || s.row0 < 0 || (long long)s.row0 + s.n > n_rows) {       // uniform: a segment outside the arenas is not followed
        if (lane == 0) { st[0] = s.n <= 0 ? 0 : kBoxStreamBadSegment; st[1] = 0; }
        return;
    }
    const long long n = s.n;
    const int* fl = flags + s.row0;
    const int4* rc = reinterpret_cast<const int4*>(rects) + s.row0;
    int* fo = flags_out + s.row0;
    int4* ro = reinterpret_cast<int4*>(rects_out) + s.row0;
    int4* sp = reinterpret_cast<int4*>(spans) + s.row0;
    int host, none;
    first_unfound_rows(fl, s.n, &host, &none);
    if (host != 0x7fffffff) {                            // uniform: left to the host, the finish will report the same row
        for (long long i = lane; i < n; i += 64) { fo[i] = fl[i]; ro[i] = rc[i]; }
        if (lane == 0) { st[0] = 2; st[1] = host; }
        return;
    }
    const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
    long long p_last = -1, nxt = -1;                     // the last detection before the chunk, the first one behind it (-1: none)
    long long a = 0, L = 0, nd = 0, sw = 0, sh = 0;      // the span that is open at the chunk's start: first row, rows, detections, sums
    bool open = false;
    int kept = 0;
    for (long long g0 = 0; g0 < n; g0 += 64) {
        const long long i = g0 + lane;
        const bool det = i < n && fl[i] == kRectFound;
        const unsigned long long dm = __ballot(det);
        if (nxt < g0 + 64) {                             // uniform; a detection found earlier that still lies behind the chunk stands
            nxt = -1;
            for (int j = 1; j <= kSpanReachChunks && nxt < 0; ++j) {
                const long long r = g0 + 64ll * j + lane;
                const unsigned long long m = __ballot(r < n && fl[r] == kRectFound);
                if (m != 0ull) nxt = g0 + 64ll * j + __ffsll((long long)m) - 1;
            }
        }
        const unsigned long long lo = dm & upto, hi = dm & ~below;
        const long long p = lo != 0ull ? g0 + 63 - __clzll((long long)lo) : p_last;
        const long long q = hi != 0ull ? g0 + __ffsll((long long)hi) - 1 : nxt;
        const bool in = i < n && p >= 0 && q >= 0 && q - p <= (long long)bridge + 1;
        int4 r = make_int4(0, 0, 0, 0);
        if (det) r = rc[i];
        else if (in) {                                   // p < i < q, 2 <= q - p <= 251: the products stay below 2^39 in magnitude
            const int4 rp = rc[p], rq = rc[q];
            const long long wp = q - i, wq = i - p, d = q - p;
            r.x = (int)floor_div(rp.x * wp + rq.x * wq, d);
            r.y = (int)floor_div(rp.y * wp + rq.y * wq, d);
            r.z = (int)floor_div(rp.z * wp + rq.z * wq, d);
            r.w = (int)floor_div(rp.w * wp + rq.w * wq, d);
        }
        if (i < n) { fo[i] = in; ro[i] = r; }
        if (dm != 0ull) p_last = g0 + 63 - __clzll((long long)dm);
        unsigned long long im = __ballot(in);
        // the span of the chunk's last row goes on iff the first detection behind the chunk is within reach of the last one so far
        const bool goes_on = (im >> 63) != 0ull && nxt >= 0 && nxt - p_last <= (long long)bridge + 1;
        while (im != 0ull) {                             // uniform: the chunk's runs of rows that are in a span, in order
            const int b0 = __ffsll((long long)im) - 1;
            const unsigned long long from = ~((1ull << b0) - 1ull), gaps = ~im & from;
            const int b1 = gaps != 0ull ? __ffsll((long long)gaps) - 1 : 64;
            const unsigned long long run = from & (b1 == 64 ? ~0ull : (1ull << b1) - 1ull);
            const bool mine = ((run >> lane) & 1ull) != 0ull;
            const long long rw = wave_sum(mine ? (long long)r.z - r.x : 0ll), rh = wave_sum(mine ? (long long)r.w - r.y : 0ll);
            if (!(open && b0 == 0)) { a = g0 + b0; L = nd = sw = sh = 0; }
            L += b1 - b0;
            nd += __popcll(dm & run);
            sw += rw;
            sh += rh;
            open = b1 == 64 && goes_on;
            if (!open) {                                 // the span [a, a + L) ends here
                if (L >= min_len && max(sw, sh) >= (long long)min_size * L) {
                    if (lane == 0) sp[kept] = make_int4((int)a, (int)L, (int)nd, 0);
                    ++kept;
                } else {
                    __threadfence();                     // the rows went out from other lanes, in this chunk and before
                    for (long long j = a + lane; j < a + L; j += 64) { fo[j] = 0; ro[j] = make_int4(0, 0, 0, 0); }
                }
            }
            im &= ~run;
        }
    }
    for (long long j = kept + lane; j < n; j += 64) sp[j] = make_int4(0, 0, 0, 0);
    if (lane == 0) { st[0] = 0; st[1] = kept; }
}

// ---- key-frame detection (opt-in `det_stride`): the detector saw only the key frames 0, N, 2N, ... and n - 1 of a
// segment of n frames; this launch turns their compact rect / flag rows into the n rows every later stage reads.  Key j lies at
// pos(j) = min(j * N, n - 1) and there are m = (n - 1 + N - 1) / N + 1 of them, so a row finds its keys by one division: row i with
// j = i / N is key j when i == j * N, key m - 1 when i == n - 1, and lies between keys j and j + 1 otherwise.  A key row is copied;
// a row between two keys flagged 1 takes w2l_face_spans_segments' interpolation, any other row is flag 0 and zeros.
// Row-parallel: workgroup (x = segment, y) strides over the segment's rows, one thread per row, no thread reads what another wrote.
struct StrideSeg {
    int key_row0, row0, n, zero;
};
static_assert(sizeof(StrideSeg) == 16 && sizeof(w2l_stride_segment) == 16, "w2l_stride_segment is 16 bytes");
constexpr int kStrideMax = 32, kStrideThreads = 256, kStrideGridCap = 64;

__global__ __launch_bounds__(kStrideThreads) void face_rects_expand_segments_kernel(const StrideSeg* __restrict__ segs, int N,
                                                                                    const int* __restrict__ key_rects,
                                                                                    const int* __restrict__ key_flags, int n_key_rows,
                                                                                    int* __restrict__ rects, int* __restrict__ flags,
                                                                                    int n_rows, int* __restrict__ status) {
    const StrideSeg s = segs[blockIdx.x];
    const bool first = blockIdx.y == 0 && threadIdx.x == 0;
    if (s.n <= 0) {                                      // uniform
        if (first) status[blockIdx.x] = 0;
        return;
    }
    const long long n = s.n, m = (n - 1 + N - 1) / N + 1;
    if (s.key_row0 < 0 || s.key_row0 + m > n_key_rows || s.row0 < 0 || s.row0 + n > n_rows) {     // uniform: not followed
        if (first) status[blockIdx.x] = kBoxStreamBadSegment;
        return;
    }
    const int* kf = key_flags + s.key_row0;
    const int4* kr = reinterpret_cast<const int4*>(key_rects) + s.key_row0;
    int* fo = flags + s.row0;
    int4* ro = reinterpret_cast<int4*>(rects) + s.row0;
    for (long long i = (long long)blockIdx.y * kStrideThreads + threadIdx.x; i < n; i += (long long)gridDim.y * kStrideThreads) {
        const long long j = i / N, p = j * N;
        int4 r = make_int4(0, 0, 0, 0);
        int f = 0;
        if (i == n - 1) {
            f = kf[m - 1];
            r = kr[m - 1];
        } else if (i == p) {
            f = kf[j];
            r = kr[j];
        } else if (kf[j] == kRectFound && kf[j + 1] == kRectFound) {      // p < i < q <= n - 1, so key j + 1 <= m - 1 exists
            const long long q = min(p + N, n - 1), wp = q - i, wq = i - p, d = q - p;
            const int4 rp = kr[j], rq = kr[j + 1];      // d <= 32: the products stay below 2^37 in magnitude
            r.x = (int)floor_div(rp.x * wp + rq.x * wq, d);
            r.y = (int)floor_div(rp.y * wp + rq.y * wq, d);
            r.z = (int)floor_div(rp.z * wp + rq.z * wq, d);
            r.w = (int)floor_div(rp.w * wp + rq.w * wq, d);
            f = kRectFound;
        }
        fo[i] = f;
        ro[i] = r;
    }
    if (first) status[blockIdx.x] = 0;
}

constexpr int kPackRowsGridCap = 1024;        // workgroups per image of the row-table packs, full size and reduced

template <class S>
static bool convb_fits(long long elems) {
    return !GlueSt<S>::kConvbLimit || elems * (long long)sizeof(typename S::elem) < (1ll << 31);
}
static bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

// ---- one set of checks and one launch per glue op; the two entry points of an op forward here, S::suffix names the one called
template <class S>
static int s3fd_pack_t(hipStream_t s, long long npix, const uint8_t* bgr, typename S::elem* y, int y_cs) {
    W2L_REQUIRE(bgr && y && npix >= 1, "s3fd_pack%s: bad arguments", S::suffix);
    W2L_REQUIRE(GlueSt<S>::pack_ok(y, y_cs), "s3fd_pack%s: y_cs=%d: %s", S::suffix, y_cs, GlueSt<S>::kPackRule);
    W2L_REQUIRE(convb_fits<S>(npix * y_cs), "s3fd_pack%s: buffer larger than 2 GiB: split the batch", S::suffix);
    hipLaunchKernelGGL(s3fd_pack_kernel<S>, dim3(grid_cap(npix, 256, GlueSt<S>::kPackGridCap)), dim3(256), 0, s, npix, bgr, y, y_cs,
                       104.f, 117.f, 123.f);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

// the checks every row-table pack shares; the frame addresses live in device memory and are the caller's
static int pack_rows_check(const char* name, const char* suffix, int B, const void* frames, const void* y) {
    W2L_REQUIRE(frames && y, "%s%s: NULL argument", name, suffix);
    W2L_REQUIRE(B >= 1 && B <= 65535, "%s%s: B=%d outside 1..65535", name, suffix, B);
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 7) == 0, "%s%s: the address table must be 8-byte aligned", name, suffix);
    return W2L_OK;
}

template <class S>
static int s3fd_pack_rows_t(hipStream_t s, int B, int H, int W, const uint64_t* frames, typename S::elem* y, int y_cs) {
    if (int e = pack_rows_check("s3fd_pack_rows", S::suffix, B, frames, y)) return e;
    W2L_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= (1ll << 29), "s3fd_pack_rows%s: H, W >= 1 and H * W <= 2^29", S::suffix);
    W2L_REQUIRE(GlueSt<S>::pack_ok(y, y_cs), "s3fd_pack_rows%s: y_cs=%d: %s", S::suffix, y_cs, GlueSt<S>::kPackRule);
    W2L_REQUIRE(convb_fits<S>((long long)B * H * W * y_cs), "s3fd_pack_rows%s: buffer larger than 2 GiB: split the batch", S::suffix);
    const int npix = H * W;
    hipLaunchKernelGGL(s3fd_pack_rows_kernel<S>, dim3(grid_cap((npix + 3) / 4, 256, kPackRowsGridCap), B), dim3(256), 0, s, npix,
                       frames, y, y_cs, 104.f, 117.f, 123.f);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

template <class S>
static int s3fd_pack_rows_scaled_t(hipStream_t s, int B, int Hs, int Ws, int Hd, int Wd, const uint64_t* frames, typename S::elem* y,
                                   int y_cs) {
    constexpr const char* name = "s3fd_pack_rows_scaled";
    if (int e = pack_rows_check(name, S::suffix, B, frames, y)) return e;
    W2L_REQUIRE(Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1, "%s%s: sizes %d x %d -> %d x %d must all be at least 1", name, S::suffix, Hs,
                Ws, Hd, Wd);
    W2L_REQUIRE((long long)Hs * Ws <= (1ll << 29) && (long long)Hd * Wd <= (1ll << 29), "%s%s: Hs * Ws and Hd * Wd <= 2^29", name,
                S::suffix);
    W2L_REQUIRE(aligned16(y), "%s%s: y must be 16-byte aligned", name, S::suffix);
    W2L_REQUIRE(y_cs >= S::VEC && y_cs % S::VEC == 0, "%s%s: y_cs=%d must be a multiple of %d (16-byte pixel stores)", name, S::suffix,
                y_cs, S::VEC);
    W2L_REQUIRE(convb_fits<S>((long long)B * Hd * Wd * y_cs), "%s%s: buffer larger than 2 GiB: split the batch", name, S::suffix);
    hipLaunchKernelGGL(s3fd_pack_rows_scaled_kernel<typename S::elem>,
                       dim3(grid_cap((long long)Hd * ((Wd + 3) / 4), 256, kPackRowsGridCap), B), dim3(256), 0, s, Hs, Ws, Hd, Wd, frames,
                       y, y_cs, 104.f, 117.f, 123.f);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

template <class S>
static int maxpool2x2_t(hipStream_t s, int N, int H, int W, int C, const typename S::elem* x, int x_cs, typename S::elem* y, int y_cs) {
    constexpr int VEC = S::VEC;
    W2L_REQUIRE(x && y && N >= 1 && H >= 2 && W >= 2 && C >= VEC && C % VEC == 0, "maxpool2x2%s: bad arguments (C %% %d == 0, H, W >= 2)",
                S::suffix, VEC);
    W2L_REQUIRE(x_cs % VEC == 0 && y_cs % VEC == 0 && x_cs >= C && y_cs >= C && aligned16(x, y),
                "maxpool2x2%s: 16-byte aligned tensors with channel strides that are multiples of %d", S::suffix, VEC);
    W2L_REQUIRE(convb_fits<S>((long long)N * H * W * x_cs), "maxpool2x2%s: buffer larger than 2 GiB: split the batch", S::suffix);
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / VEC);
    hipLaunchKernelGGL(maxpool2x2_kernel<S>, dim3(grid_cap(total, 256, 65536)), dim3(256), 0, s, N, H, W, C / VEC, x, x_cs, y, y_cs);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

template <class S>
static int l2norm_scale_t(hipStream_t s, long long rows, int C, const typename S::elem* x, int x_cs, const float* weight,
                          typename S::elem* y, int y_cs) {
    constexpr int VEC = S::VEC;
    W2L_REQUIRE(x && y && weight && rows >= 1 && C >= VEC && C % VEC == 0, "l2norm_scale%s: bad arguments (C %% %d == 0)", S::suffix, VEC);
    W2L_REQUIRE(x_cs % VEC == 0 && y_cs % VEC == 0 && x_cs >= C && y_cs >= C && aligned16(x, y, weight),
                "l2norm_scale%s: 16-byte aligned tensors with channel strides that are multiples of %d", S::suffix, VEC);
    W2L_REQUIRE(convb_fits<S>(rows * x_cs) && convb_fits<S>(rows * y_cs), "l2norm_scale%s: buffer larger than 2 GiB: split the batch",
                S::suffix);
    const long long blocks = (rows + 3) / 4;
    W2L_REQUIRE(blocks < (1ll << 31), "l2norm_scale%s: too many rows", S::suffix);
    hipLaunchKernelGGL(l2norm_scale_kernel<S>, dim3((unsigned)blocks), dim3(256), 0, s, rows, C, x, x_cs, weight, y, y_cs);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // namespace w2l

using namespace w2l;

extern "C" {

static hipStream_t hs(void* stream) { return static_cast<hipStream_t>(stream); }
static __bf16* bf(void* p) { return static_cast<__bf16*>(p); }
static const __bf16* bf(const void* p) { return static_cast<const __bf16*>(p); }

int w2l_s3fd_pack(void* stream, long long npix, const uint8_t* bgr, float* y, int y_cs) {
    return s3fd_pack_t<StF32>(hs(stream), npix, bgr, y, y_cs);
}
int w2l_s3fd_pack_bf16(void* stream, long long npix, const uint8_t* bgr, void* y, int y_cs) {
    return s3fd_pack_t<StBf16>(hs(stream), npix, bgr, bf(y), y_cs);
}

int w2l_s3fd_pack_rows(void* stream, int B, int H, int W, const uint64_t* frames, float* y, int y_cs) {
    return s3fd_pack_rows_t<StF32>(hs(stream), B, H, W, frames, y, y_cs);
}
int w2l_s3fd_pack_rows_bf16(void* stream, int B, int H, int W, const uint64_t* frames, void* y, int y_cs) {
    return s3fd_pack_rows_t<StBf16>(hs(stream), B, H, W, frames, bf(y), y_cs);
}

int w2l_s3fd_pack_rows_scaled(void* stream, int B, int Hs, int Ws, int Hd, int Wd, const uint64_t* frames, float* y, int y_cs) {
    return s3fd_pack_rows_scaled_t<StF32>(hs(stream), B, Hs, Ws, Hd, Wd, frames, y, y_cs);
}
int w2l_s3fd_pack_rows_scaled_bf16(void* stream, int B, int Hs, int Ws, int Hd, int Wd, const uint64_t* frames, void* y, int y_cs) {
    return s3fd_pack_rows_scaled_t<StBf16>(hs(stream), B, Hs, Ws, Hd, Wd, frames, bf(y), y_cs);
}

int w2l_maxpool2x2(void* stream, int N, int H, int W, int C, const float* x, int x_cs, float* y, int y_cs) {
    return maxpool2x2_t<StF32>(hs(stream), N, H, W, C, x, x_cs, y, y_cs);
}
int w2l_maxpool2x2_bf16(void* stream, int N, int H, int W, int C, const void* x, int x_cs, void* y, int y_cs) {
    return maxpool2x2_t<StBf16>(hs(stream), N, H, W, C, bf(x), x_cs, bf(y), y_cs);
}

int w2l_l2norm_scale(void* stream, long long rows, int C, const float* x, int x_cs, const float* weight, float* y, int y_cs) {
    return l2norm_scale_t<StF32>(hs(stream), rows, C, x, x_cs, weight, y, y_cs);
}
int w2l_l2norm_scale_bf16(void* stream, long long rows, int C, const void* x, int x_cs, const float* weight, void* y, int y_cs) {
    return l2norm_scale_t<StBf16>(hs(stream), rows, C, bf(x), x_cs, weight, bf(y), y_cs);
}

int w2l_s3fd_decode(void* stream, int B, int FH, int FW, int stride, const float* cls, int cls_cs, int ncls, const float* reg,
                    int reg_cs, float* out) {
    W2L_REQUIRE(cls && reg && out && B >= 1 && FH >= 1 && FW >= 1 && stride >= 1, "bad s3fd_decode arguments");
    W2L_REQUIRE((ncls == 2 || ncls == 4) && cls_cs >= ncls && reg_cs >= 4, "s3fd_decode: ncls must be 2 or 4");
    const long long total = (long long)B * FH * FW;
    hipLaunchKernelGGL(s3fd_decode_kernel, dim3(grid_cap(total, 256, 16384)), dim3(256), 0, static_cast<hipStream_t>(stream), B, FH, FW,
                       stride, cls, cls_cs, ncls, reg, reg_cs, out);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_s3fd_nms(void* stream, int B, int P, const float* table, float gate, float thresh, int* keep, int* counts,
                 void* scratch, long long scratch_bytes) {
    W2L_REQUIRE(table && keep && counts && scratch && B >= 1 && P >= 1, "bad s3fd_nms arguments");
    W2L_REQUIRE((long long)B * P * 5 < (1ll << 31), "s3fd_nms: table too large");
    W2L_REQUIRE(scratch_bytes >= (long long)B * P * 12 && (reinterpret_cast<uintptr_t>(scratch) & 7) == 0,
                "s3fd_nms: scratch must hold 12 bytes per box (8-byte aligned), got %lld for %d x %d", scratch_bytes, B, P);
    unsigned long long* keys = static_cast<unsigned long long*>(scratch);
    int* order = reinterpret_cast<int*>(keys + (long long)B * P);
    hipLaunchKernelGGL(s3fd_nms_kernel, dim3(B), dim3(kNmsThreads), 0, static_cast<hipStream_t>(stream), P, table, gate, thresh,
                       keys, order, keep, counts);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_s3fd_first_rect(void* stream, int B, int P, const float* table, const int* keep, const int* counts, float thresh,
                        int* rects, int* flags) {
    W2L_REQUIRE(table && keep && counts && rects && flags && B >= 1 && P >= 1, "bad s3fd_first_rect arguments");
    W2L_REQUIRE((long long)B * P * 5 < (1ll << 31), "s3fd_first_rect: table too large");
    hipLaunchKernelGGL(s3fd_first_rect_kernel<false>, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), P, table, keep,
                       counts, thresh, 1.f, 1.f, rects, flags);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_s3fd_first_rect_scaled(void* stream, int B, int P, const float* table, const int* keep, const int* counts, float thresh,
                               float sx, float sy, int* rects, int* flags) {
    W2L_REQUIRE(table && keep && counts && rects && flags && B >= 1 && P >= 1, "bad s3fd_first_rect_scaled arguments");
    W2L_REQUIRE((long long)B * P * 5 < (1ll << 31), "s3fd_first_rect_scaled: table too large");
    W2L_REQUIRE(sx > 0.f && sy > 0.f && sx < INFINITY && sy < INFINITY,
                "s3fd_first_rect_scaled: sx=%g and sy=%g must be finite and positive", (double)sx, (double)sy);
    hipLaunchKernelGGL(s3fd_first_rect_kernel<true>, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), P, table, keep,
                       counts, thresh, sx, sy, rects, flags);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_s3fd_top_rects(void* stream, int B, int P, const float* table, const int* keep, const int* counts, float thresh, float sx,
                       float sy, int K, int32_t* cands, int32_t* ncand, int32_t* flags) {
    W2L_REQUIRE(table && keep && counts && cands && ncand && flags && B >= 1 && P >= 1, "bad s3fd_top_rects arguments");
    W2L_REQUIRE((long long)B * P * 5 < (1ll << 31), "s3fd_top_rects: table too large");
    W2L_REQUIRE(sx > 0.f && sy > 0.f && sx < INFINITY && sy < INFINITY, "s3fd_top_rects: sx=%g and sy=%g must be finite and positive",
                (double)sx, (double)sy);
    W2L_REQUIRE(K >= 1 && K <= kTrackMaxCands, "s3fd_top_rects: K=%d outside 1..%d", K, kTrackMaxCands);
    hipLaunchKernelGGL(s3fd_top_rects_kernel, dim3(B), dim3(64), 0, static_cast<hipStream_t>(stream), P, table, keep, counts, thresh,
                       sx, sy, K, cands, ncand, flags);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_face_track_segments(void* stream, int n_seg, const w2l_track_segment* segs, const int32_t* cands, const int32_t* ncand,
                            const int32_t* cflags, int n_rows, int K, int pick, int L, int q, int32_t* state, int n_slots,
                            int32_t* rects, int32_t* flags, int32_t* status) {
    W2L_REQUIRE(segs && cands && ncand && cflags && rects && flags && status, "face_track_segments: NULL argument");
    W2L_REQUIRE(n_seg >= 1 && n_rows >= 0, "face_track_segments: n_seg=%d must be at least 1 and n_rows=%d at least 0", n_seg, n_rows);
    W2L_REQUIRE(n_slots >= 0 && (state || n_slots == 0), "face_track_segments: n_slots=%d slots need a state table", n_slots);
    W2L_REQUIRE(K >= 1 && K <= kTrackMaxCands, "face_track_segments: K=%d outside 1..%d", K, kTrackMaxCands);
    W2L_REQUIRE(pick >= kPickScore && pick <= kPickRight, "face_track_segments: pick=%d outside 0..3", pick);
    W2L_REQUIRE(L >= 0 && L <= kTrackMaxReseed, "face_track_segments: L=%d outside 0..%d", L, kTrackMaxReseed);
    W2L_REQUIRE(q >= 1 && q <= 256, "face_track_segments: q=%d outside 1..256", q);
    W2L_REQUIRE(((reinterpret_cast<uintptr_t>(segs) | reinterpret_cast<uintptr_t>(cands) | reinterpret_cast<uintptr_t>(rects)) & 15) == 0,
                "face_track_segments: the segment table, cands and rects must be 16-byte aligned");
    hipLaunchKernelGGL(face_track_segments_kernel, dim3(n_seg), dim3(64), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const TrackSeg*>(segs), cands, ncand, cflags, n_rows, K, pick, L, q, state, n_slots, rects, flags,
                       status);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

// the argument checks the four box finishes share (`name` opens the messages; `pointers`: none of the entry's pointers is NULL)
static int face_boxes_check(const char* name, bool pointers, int n_seg, const void* segs, int T, int hold) {
    W2L_REQUIRE(pointers, "%s: NULL argument", name);
    W2L_REQUIRE(n_seg >= 1, "%s: n_seg=%d must be at least 1", name, n_seg);
    W2L_REQUIRE(T >= 0 && T <= kBoxMaxT, "%s: T=%d outside 0..%d", name, T, kBoxMaxT);
    W2L_REQUIRE(hold >= 0 && hold <= kHoldMax, "%s: hold=%d outside 0..%d", name, hold, kHoldMax);
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(segs) & 15) == 0, "%s: the segment table must be 16-byte aligned", name);
    return W2L_OK;
}

// the clip form of the strict finish names no arena size: its segments are followed as they stand
int w2l_face_boxes_segments(void* stream, int n_seg, const w2l_box_segment* segs, const int32_t* rects, const int32_t* flags,
                            int top, int bottom, int left, int right, int T, int32_t* boxes, int32_t* status) {
    if (int e = face_boxes_check("face_boxes_segments", segs && rects && flags && boxes && status, n_seg, segs, T, 0)) return e;
    hipLaunchKernelGGL(face_boxes_runs_kernel<true>, dim3(n_seg), dim3(64), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const BoxSeg*>(segs), rects, flags, 0x7fffffff, top, bottom, left, right, T, 0, boxes,
                       static_cast<int*>(nullptr), status);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

// the checks of a tick's segment table on its host copy, shared by the two stream finishes (`name` opens the messages)
static int box_stream_table_check(const char* name, int n_seg, const w2l_box_stream_segment* segs_host, int n_rows, int n_slots, int T,
                                  int n_out) {
    W2L_REQUIRE(n_rows >= 0 && n_slots >= 1 && n_out >= 0, "%s: n_rows=%d, n_slots=%d, n_out=%d", name, n_rows, n_slots, n_out);
    // a tick has a segment per live stream: the pairwise checks below are a few thousand comparisons, and allocate nothing
    for (int k = 0; k < n_seg; ++k) {
        const w2l_box_stream_segment& s = segs_host[k];
        W2L_REQUIRE(s.n_new >= 0 && s.seen >= 0, "%s: segment %d: n_new=%d and seen=%d must not be negative", name, k, s.n_new, s.seen);
        W2L_REQUIRE((long long)s.seen + s.n_new <= 0x7fffffffll, "%s: segment %d: more than 2^31 - 1 frames", name, k);
        W2L_REQUIRE(s.slot >= 0 && s.slot < n_slots, "%s: segment %d: slot %d outside [0, %d)", name, k, s.slot, n_slots);
        W2L_REQUIRE(s.row0 >= 0 && (long long)s.row0 + s.n_new <= n_rows, "%s: segment %d: rows [%d, %d + %d) outside the %d arena rows",
                    name, k, s.row0, s.row0, s.n_new, n_rows);
        long long lo, hi;
        box_stream_range(s.seen, (long long)s.seen + s.n_new, s.closed, T, &lo, &hi);
        W2L_REQUIRE(s.out0 >= 0 && s.out0 + (hi - lo) <= n_out, "%s: segment %d: output rows [%d, %d + %lld) outside the %d rows", name,
                    k, s.out0, s.out0, hi - lo, n_out);
        for (int j = 0; j < k; ++j) {
            const w2l_box_stream_segment& o = segs_host[j];      // checked above: its counts are in range
            W2L_REQUIRE(o.slot != s.slot, "%s: segments %d and %d name carry slot %d", name, j, k, s.slot);
            long long olo, ohi;
            box_stream_range(o.seen, (long long)o.seen + o.n_new, o.closed, T, &olo, &ohi);
            W2L_REQUIRE(hi == lo || ohi == olo || s.out0 + (hi - lo) <= o.out0 || o.out0 + (ohi - olo) <= s.out0,
                        "%s: the output rows of segments %d and %d overlap", name, j, k);
        }
    }
    return W2L_OK;
}

int w2l_face_boxes_stream(void* stream, int n_seg, const w2l_box_stream_segment* segs_host, const w2l_box_stream_segment* segs,
                          const int32_t* rects, const int32_t* flags, int n_rows, int32_t* carry, int n_slots, int top, int bottom,
                          int left, int right, int T, int32_t* boxes, int n_out, int32_t* status) {
    if (int e = face_boxes_check("face_boxes_stream", segs_host && segs && rects && flags && carry && boxes && status, n_seg, segs, T, 0))
        return e;
    if (int e = box_stream_table_check("face_boxes_stream", n_seg, segs_host, n_rows, n_slots, T, n_out)) return e;
    hipLaunchKernelGGL(face_boxes_stream_runs_kernel<true>, dim3(n_seg), dim3(64), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const BoxStreamSeg*>(segs), rects, flags, n_rows, carry, n_slots, top, bottom, left, right, T,
                       0, boxes, static_cast<int*>(nullptr), n_out, status);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_face_boxes_runs(void* stream, int n_seg, const w2l_box_segment* segs, const int32_t* rects, const int32_t* flags, int n_rows,
                        int top, int bottom, int left, int right, int T, int hold, int32_t* boxes, int32_t* valid, int32_t* status) {
    if (int e = face_boxes_check("face_boxes_runs", segs && rects && flags && boxes && valid && status, n_seg, segs, T, hold)) return e;
    W2L_REQUIRE(n_rows >= 0, "face_boxes_runs: n_seg=%d must be at least 1 and n_rows=%d at least 0", n_seg, n_rows);
    hipLaunchKernelGGL(face_boxes_runs_kernel<false>, dim3(n_seg), dim3(64), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const BoxSeg*>(segs), rects, flags, n_rows, top, bottom, left, right, T, hold, boxes, valid,
                       status);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_face_tracks_all_segments(void* stream, int n_seg, const w2l_box_segment* segs, const int32_t* cands, const int32_t* ncand,
                                 const int32_t* cflags, int n_rows, int K, int F, int L, int q, int32_t* rects_out, int32_t* flags_out,
                                 int32_t* status) {
    W2L_REQUIRE(segs && cands && ncand && cflags && rects_out && flags_out && status, "face_tracks_all_segments: NULL argument");
    W2L_REQUIRE(n_seg >= 1 && n_rows >= 0, "face_tracks_all_segments: n_seg=%d must be at least 1 and n_rows=%d at least 0", n_seg,
                n_rows);
    W2L_REQUIRE(K >= 1 && K <= kTrackMaxCands, "face_tracks_all_segments: K=%d outside 1..%d", K, kTrackMaxCands);
    W2L_REQUIRE(F >= 1 && F <= kFacesMaxSlots, "face_tracks_all_segments: F=%d outside 1..%d", F, kFacesMaxSlots);
    W2L_REQUIRE(L >= 0 && L <= kTrackMaxReseed, "face_tracks_all_segments: L=%d outside 0..%d", L, kTrackMaxReseed);
    W2L_REQUIRE(q >= 1 && q <= 256, "face_tracks_all_segments: q=%d outside 1..256", q);
    W2L_REQUIRE((long long)F * n_rows < (1ll << 29), "face_tracks_all_segments: F * n_rows = %lld rows, 2^29 or more",
                (long long)F * n_rows);
    W2L_REQUIRE(aligned16(segs, cands, rects_out),
                "face_tracks_all_segments: the segment table, cands and rects_out must be 16-byte aligned");
    hipLaunchKernelGGL(face_tracks_all_segments_kernel, dim3(n_seg), dim3(64), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const BoxSeg*>(segs), cands, ncand, cflags, n_rows, K, F, L, q, rects_out, flags_out, status);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_face_spans_segments(void* stream, int n_seg, const w2l_box_segment* segs, const int32_t* rects, const int32_t* flags, int n_rows,
                            int bridge, int min_len, int min_size, int32_t* rects_out, int32_t* flags_out, int32_t* spans,
                            int32_t* status) {
    W2L_REQUIRE(segs && rects && flags && rects_out && flags_out && spans && status, "face_spans_segments: NULL argument");
    W2L_REQUIRE(n_seg >= 1 && n_rows >= 0, "face_spans_segments: n_seg=%d must be at least 1 and n_rows=%d at least 0", n_seg, n_rows);
    W2L_REQUIRE(bridge >= 0 && bridge <= kSpanMaxBridge, "face_spans_segments: bridge=%d outside 0..%d", bridge, kSpanMaxBridge);
    W2L_REQUIRE(min_len >= 1 && min_len <= kSpanMaxLen, "face_spans_segments: min_len=%d outside 1..%d", min_len, kSpanMaxLen);
    W2L_REQUIRE(min_size >= 0 && min_size <= kSpanMaxSize, "face_spans_segments: min_size=%d outside 0..%d", min_size, kSpanMaxSize);
    W2L_REQUIRE(aligned16(segs, rects, rects_out) && aligned16(spans),
                "face_spans_segments: the segment table, rects, rects_out and spans must be 16-byte aligned");
    hipLaunchKernelGGL(face_spans_segments_kernel, dim3(n_seg), dim3(64), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const BoxSeg*>(segs), rects, flags, n_rows, bridge, min_len, min_size, rects_out, flags_out,
                       spans, status);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_face_rects_expand_segments(void* stream, int n_seg, const w2l_stride_segment* segs, int N, const int32_t* key_rects,
                                   const int32_t* key_flags, int n_key_rows, int32_t* rects, int32_t* flags, int n_rows,
                                   int32_t* status) {
    W2L_REQUIRE(segs && key_rects && key_flags && rects && flags && status, "face_rects_expand_segments: NULL argument");
    W2L_REQUIRE(n_seg >= 1 && n_key_rows >= 0 && n_rows >= 0,
                "face_rects_expand_segments: n_seg=%d must be at least 1, n_key_rows=%d and n_rows=%d at least 0", n_seg, n_key_rows,
                n_rows);
    W2L_REQUIRE(N >= 1 && N <= kStrideMax, "face_rects_expand_segments: N=%d outside 1..%d", N, kStrideMax);
    W2L_REQUIRE(aligned16(segs, key_rects, rects),
                "face_rects_expand_segments: the segment table, key_rects and rects must be 16-byte aligned");
    const int chunks = (n_rows + kStrideThreads - 1) / kStrideThreads;       // a segment has at most n_rows rows
    hipLaunchKernelGGL(face_rects_expand_segments_kernel, dim3(n_seg, std::min(std::max(chunks, 1), kStrideGridCap)),
                       dim3(kStrideThreads), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const StrideSeg*>(segs), N,
                       key_rects, key_flags, n_key_rows, rects, flags, n_rows, status);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_face_boxes_stream_runs(void* stream, int n_seg, const w2l_box_stream_segment* segs_host, const w2l_box_stream_segment* segs,
                               const int32_t* rects, const int32_t* flags, int n_rows, int32_t* carry, int n_slots, int top, int bottom,
                               int left, int right, int T, int hold, int32_t* boxes, int32_t* valid, int n_out, int32_t* status) {
    if (int e = face_boxes_check("face_boxes_stream_runs", segs_host && segs && rects && flags && carry && boxes && valid && status, n_seg,
                                 segs, T, hold))
        return e;
    if (int e = box_stream_table_check("face_boxes_stream_runs", n_seg, segs_host, n_rows, n_slots, T, n_out)) return e;
    hipLaunchKernelGGL(face_boxes_stream_runs_kernel<false>, dim3(n_seg), dim3(64), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const BoxStreamSeg*>(segs), rects, flags, n_rows, carry, n_slots, top, bottom, left, right, T,
                       hold, boxes, valid, n_out, status);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"
