// The S3FD face detector's glue on the opt-in bf16-storage path (face_detection/s3fd.py _GraphB): the ops between the backbone
// convolutions, which are w2l_convb launches (bias as the fp32 shift, ReLU), and the fused detection head.
//   w2l_s3fd_pack_bf16       detect.py:57-58 + api.py:62  uint8 BGR -> RGB minus (104,117,123), bf16 NHWC (integers: exact)
//   w2l_s3fd_pack_rows_bf16  the same per frame of an address table (frames of several clips in one batch, read in place)
//   w2l_maxpool2x2_bf16      net_s3fd.py:75,79,85,91,97   F.max_pool2d(h, 2, 2) on bf16 (max is exact)
//   w2l_l2norm_scale_bf16    net_s3fd.py:6-19             sum of squares in fp32, one rounding on the store
//   w2l_s3fd_headb_*         net_s3fd.py:99-120 (conf + loc convolutions of one level) + net_s3fd.py:123-126 + detect.py:66-84:
//                            one 3x3 contraction on v_mfma_f32_16x16x32_bf16 and the decode from the fp32 accumulators
// Layout: NHWC bf16, channel strides in elements and multiples of 8, 16-byte aligned pointers.
#include "w2l_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct w2l_s3fd_headb {
    int cin, ncls;
    __bf16* w = nullptr;    // [cin / 32][9 taps][8 columns][32 channels]: columns 0..3 conf (ncls of them), 4..7 loc
    float* b = nullptr;     // [8], same columns
};

namespace w2l {

constexpr long long kLim2G = 1ll << 31;     // the convb launches' per-buffer rule (32-bit byte offsets)

static inline int grid1db(long long work, int block, int cap = 65536) {
    long long g = (work + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

__global__ void s3fd_pack_bf16_kernel(long long npix, const uint8_t* __restrict__ x, __bf16* __restrict__ y, int y_cs) {
    const int groups = y_cs >> 3;
    const long long total = npix * groups;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long pix = i / groups;
        const int g = (int)(i - pix * groups);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)0.f;
        if (g == 0) {
            // the fp32 pack's values (w2l_s3fd_pack): integers with |v| <= 152, exact in bf16
            float c0, c1, c2;
            s3fd_pixel(x + pix * 3, 104.f, 117.f, 123.f, c0, c1, c2);
            o[0] = (__bf16)c0; o[1] = (__bf16)c1; o[2] = (__bf16)c2;
        }
        *reinterpret_cast<bf16x8*>(y + pix * y_cs + g * 8) = o;
    }
}

// The row-table form (s3fd_pack_rows_kernel of detect.hip): blockIdx.y is the image, a thread owns four consecutive pixels and
// writes every 8-channel group of each (group 0: the pixel, the rest zeros)
__global__ void s3fd_pack_rows_bf16_kernel(int npix, const uint64_t* __restrict__ frames, __bf16* __restrict__ y, int y_cs) {
    const int b = blockIdx.y;
    const uint64_t addr = frames[b];
    const uint8_t* x = reinterpret_cast<const uint8_t*>(addr);
    const bool dwords = (addr & 3) == 0;
    __bf16* yb = y + (long long)b * npix * y_cs;
    const int ngroups = (npix + 3) >> 2, groups = y_cs >> 3;
    for (int g4 = blockIdx.x * blockDim.x + threadIdx.x; g4 < ngroups; g4 += gridDim.x * blockDim.x) {
        const int i0 = g4 << 2, n = min(4, npix - i0);
        uint8_t px[12];
        s3fd_load_group(x + (long long)i0 * 3, dwords, n, px);
        for (int k = 0; k < n; ++k) {
            float c0, c1, c2;
            s3fd_pixel(px + 3 * k, 104.f, 117.f, 123.f, c0, c1, c2);
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (__bf16)0.f;
            __bf16* op = yb + (long long)(i0 + k) * y_cs;
            for (int g = 1; g < groups; ++g) *reinterpret_cast<bf16x8*>(op + g * 8) = o;
            o[0] = (__bf16)c0; o[1] = (__bf16)c1; o[2] = (__bf16)c2;
            *reinterpret_cast<bf16x8*>(op) = o;
        }
    }
}

// one thread per (output pixel, 8-channel group)
__global__ void maxpool2x2_bf16_kernel(int N, int H, int W, int C8, const __bf16* __restrict__ x, int x_cs, __bf16* __restrict__ y,
                                       int y_cs) {
    const int Ho = H / 2, Wo = W / 2;
    const long long total = (long long)N * Ho * Wo * C8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % C8);
        long long pix = i / C8;
        const int ox = (int)(pix % Wo);
        pix /= Wo;
        const int oy = (int)(pix % Ho);
        const int n = (int)(pix / Ho);
        const __bf16* p = x + (((long long)n * H + 2 * oy) * W + 2 * ox) * x_cs + c8 * 8;
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(p + x_cs);
        const bf16x8 c = *reinterpret_cast<const bf16x8*>(p + (long long)W * x_cs);
        const bf16x8 d = *reinterpret_cast<const bf16x8*>(p + (long long)W * x_cs + x_cs);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            o[e] = (__bf16)fmaxf(fmaxf((float)a[e], (float)b[e]), fmaxf((float)c[e], (float)d[e]));   // exact: a max of bf16 values
        *reinterpret_cast<bf16x8*>(y + (((long long)n * Ho + oy) * Wo + ox) * y_cs + c8 * 8) = o;
    }
}

// one wave per pixel: fp32 sum of squares over the channels, then x / norm * weight[c] in fp32, rounded once (RNE)
__global__ void l2norm_scale_bf16_kernel(long long rows, int C, const __bf16* __restrict__ x, int x_cs, const float* __restrict__ w,
                                         __bf16* __restrict__ y, int y_cs) {
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const __bf16* p = x + row * x_cs;
    float s = 0.f;
    for (int c = lane * 8; c < C; c += 512) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(p + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += (float)v[e] * (float)v[e];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float norm = sqrtf(s) + 1e-10f;
    for (int c = lane * 8; c < C; c += 512) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(p + c);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + c), w1 = *reinterpret_cast<const f32x4*>(w + c + 4);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)((float)v[e] / norm * (e < 4 ? w0[e] : w1[e - 4]));
        *reinterpret_cast<bf16x8*>(y + row * y_cs + c) = o;
    }
}

// ---- the fused detection head
// weights: one thread per packed element; columns without a filter (ncls = 2: columns 2, 3) are zero
__global__ void s3fd_headb_pack_kernel(int cin, int ncls, const float* __restrict__ conf_w, const float* __restrict__ conf_b,
                                       const float* __restrict__ loc_w, const float* __restrict__ loc_b, __bf16* __restrict__ w,
                                       float* __restrict__ b) {
    const long long total = (long long)cin * 9 * 8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i & 31);
        const int j = (int)((i >> 5) & 7);
        const long long r = i >> 8;
        const int t = (int)(r % 9);
        const int c = (int)(r / 9) * 32 + k;
        float v = 0.f;
        if (j < ncls) v = conf_w[((long long)j * cin + c) * 9 + t];          // torch OIHW [ncls][cin][3][3], tap t = ky * 3 + kx
        else if (j >= 4) v = loc_w[((long long)(j - 4) * cin + c) * 9 + t];
        w[i] = (__bf16)v;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const int j = threadIdx.x;
        b[j] = j < ncls ? (conf_b ? conf_b[j] : 0.f) : (j >= 4 ? (loc_b ? loc_b[j - 4] : 0.f) : 0.f);
    }
}

// A workgroup of four waves computes an 8 x 16 tile of output positions: per 32-channel chunk the (8+2) x (16+2) halo box is
// staged in LDS (every feature is read from HBM once plus the halo), each wave owns two rows of 16 positions = two 16x16 MFMA
// tiles (M = positions, N = 16 columns of which 8 are used, K = 32 channels of one tap), nine taps per chunk.  The fp32
// accumulators + bias go through LDS to one lane per position, which decodes them with s3fd_decode_kernel's fp32 operations
// (detect.hip) and writes the (x1, y1, x2, y2, score) row.  Logits never leave the chip.
constexpr int kHTW = 16, kHTH = 8, kHBW = kHTW + 2, kHBH = kHTH + 2, kHBox = kHBW * kHBH;

__global__ __launch_bounds__(256) void s3fd_headb_kernel(int FH, int FW, int stride, int cin, int ncls, const __bf16* __restrict__ x,
                                                         int x_cs, const __bf16* __restrict__ wp, const float* __restrict__ bias,
                                                         float* __restrict__ out) {
    __shared__ bf16x8 s_box[kHBox * 4];            // [box pixel][4 slots of 8 channels], slot = group ^ ((pixel >> 2) & 3)
    __shared__ float s_ep[4][2][16][8];            // [wave][row][position][column]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kHTW, y0 = blockIdx.y * kHTH, n = blockIdx.z;
    const __bf16* xb = x + (long long)n * FH * FW * x_cs;
    const int col = lane & 15, grp = lane >> 4;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int nchunk = cin >> 5;
    for (int q = 0; q < nchunk; ++q) {
        // B fragments of the nine taps: lane holds column `col`, channels 8 * grp .. + 7 (columns 8..15 are zero)
        bf16x8 bw[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (col < 8) bw[t] = *reinterpret_cast<const bf16x8*>(wp + ((long long)(q * 9 + t) * 8 + col) * 32 + grp * 8);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) bw[t][e] = (__bf16)0.f;
            }
        }
        __syncthreads();                           // the previous chunk's box has been read
        for (int i = tid; i < kHBox * 4; i += 256) {
            const int p = i >> 2, g = i & 3;
            const int iy = y0 - 1 + p / kHBW, ix = x0 - 1 + p % kHBW;
            bf16x8 v;
            if (iy >= 0 && iy < FH && ix >= 0 && ix < FW) v = *reinterpret_cast<const bf16x8*>(xb + ((long long)iy * FW + ix) * x_cs + q * 32 + g * 8);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (__bf16)0.f;
            }
            s_box[p * 4 + (g ^ ((p >> 2) & 3))] = v;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ky = t / 3, kx = t - 3 * (t / 3);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int p = (wave * 2 + r + ky) * kHBW + col + kx;      // A: row = position `col` of the wave's row r, K = channels
                const bf16x8 a = s_box[p * 4 + (grp ^ ((p >> 2) & 3))];
                acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bw[t], acc[r], 0, 0, 0);
            }
        }
    }
    // C/D of 16x16x32: lane holds column (lane & 15) of rows 4 * (lane >> 4) + e
    if (col < 8) {
        const float bj = bias[col];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) s_ep[wave][r][grp * 4 + e][col] = acc[r][e] + bj;
    }
    __syncthreads();
    if (lane < 32) {
        const int r = lane >> 4, pos = lane & 15;
        const int hy = y0 + wave * 2 + r, wx = x0 + pos;
        if (hy < FH && wx < FW) {
            const float* c = s_ep[wave][r][pos];
            const float* l = c + 4;
            // s3fd_decode_kernel (detect.hip), operation for operation
            float bg, fg;
            if (ncls == 4) { bg = fmaxf(fmaxf(c[0], c[1]), c[2]); fg = c[3]; }
            else { bg = c[0]; fg = c[1]; }
            const float mx = fmaxf(bg, fg);
            const float eb = expf(bg - mx), ef = expf(fg - mx);
            const float score = ef / (eb + ef);
            const float axc = (float)stride / 2.f + (float)wx * (float)stride;
            const float ayc = (float)stride / 2.f + (float)hy * (float)stride;
            const float pw = (float)(stride * 4);
            float cx = axc + l[0] * 0.1f * pw;
            float cy = ayc + l[1] * 0.1f * pw;
            const float bw_ = pw * expf(l[2] * 0.2f);
            const float bh = pw * expf(l[3] * 0.2f);
            cx -= bw_ / 2.f;
            cy -= bh / 2.f;
            float* o = out + (((long long)n * FH + hy) * FW + wx) * 5;
            o[0] = cx; o[1] = cy; o[2] = bw_ + cx; o[3] = bh + cy; o[4] = score;
        }
    }
}

static int headb_pack(w2l_s3fd_headb* h, const float* conf_w, const float* conf_b, const float* loc_w, const float* loc_b,
                      hipStream_t s) {
    const long long total = (long long)h->cin * 9 * 8;
    hipLaunchKernelGGL(s3fd_headb_pack_kernel, dim3(grid1db(total, 256, 1024)), dim3(256), 0, s, h->cin, h->ncls, conf_w, conf_b,
                       loc_w, loc_b, h->w, h->b);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // namespace w2l

using namespace w2l;

extern "C" {

int w2l_s3fd_pack_bf16(void* stream, long long npix, const uint8_t* bgr, void* y, int y_cs) {
    W2L_REQUIRE(bgr && y && npix >= 1 && y_cs >= 8 && (y_cs & 7) == 0, "bad s3fd_pack_bf16 arguments (y_cs %% 8 == 0)");
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(y) & 15) == 0, "s3fd_pack_bf16: y must be 16-byte aligned");
    W2L_REQUIRE(npix * y_cs * 2 < kLim2G, "s3fd_pack_bf16: buffer larger than 2 GiB: split the batch");
    hipLaunchKernelGGL(s3fd_pack_bf16_kernel, dim3(grid1db(npix * (y_cs / 8), 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       npix, bgr, static_cast<__bf16*>(y), y_cs);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_s3fd_pack_rows_bf16(void* stream, int B, int H, int W, const uint64_t* frames, void* y, int y_cs) {
    W2L_REQUIRE(frames && y && B >= 1 && H >= 1 && W >= 1 && y_cs >= 8 && (y_cs & 7) == 0, "bad s3fd_pack_rows_bf16 arguments (y_cs %% 8 == 0)");
    W2L_REQUIRE(B <= 65535 && (long long)H * W <= (1ll << 29), "s3fd_pack_rows_bf16: B <= 65535 and H * W <= 2^29");
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 7) == 0, "s3fd_pack_rows_bf16: the address table must be 8-byte aligned");
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(y) & 15) == 0, "s3fd_pack_rows_bf16: y must be 16-byte aligned");
    W2L_REQUIRE((long long)B * H * W * y_cs * 2 < kLim2G, "s3fd_pack_rows_bf16: buffer larger than 2 GiB: split the batch");
    const int npix = H * W;
    hipLaunchKernelGGL(s3fd_pack_rows_bf16_kernel, dim3(grid1db((npix + 3) / 4, 256, 1024), B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), npix, frames, static_cast<__bf16*>(y), y_cs);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_maxpool2x2_bf16(void* stream, int N, int H, int W, int C, const void* x, int x_cs, void* y, int y_cs) {
    W2L_REQUIRE(x && y && N >= 1 && H >= 2 && W >= 2 && C >= 8 && (C & 7) == 0, "bad maxpool2x2_bf16 arguments (C %% 8 == 0, H, W >= 2)");
    W2L_REQUIRE((x_cs & 7) == 0 && (y_cs & 7) == 0 && x_cs >= C && y_cs >= C &&
                    ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0,
                "maxpool2x2_bf16: 16-byte aligned tensors with channel strides that are multiples of 8");
    W2L_REQUIRE((long long)N * H * W * x_cs * 2 < kLim2G, "maxpool2x2_bf16: buffer larger than 2 GiB: split the batch");
    const long long total = (long long)N * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(maxpool2x2_bf16_kernel, dim3(grid1db(total, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), N, H, W,
                       C / 8, static_cast<const __bf16*>(x), x_cs, static_cast<__bf16*>(y), y_cs);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_l2norm_scale_bf16(void* stream, long long rows, int C, const void* x, int x_cs, const float* weight, void* y, int y_cs) {
    W2L_REQUIRE(x && y && weight && rows >= 1 && C >= 8 && (C & 7) == 0, "bad l2norm_scale_bf16 arguments (C %% 8 == 0)");
    W2L_REQUIRE((x_cs & 7) == 0 && (y_cs & 7) == 0 && x_cs >= C && y_cs >= C &&
                    ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(weight)) & 15) == 0,
                "l2norm_scale_bf16: 16-byte aligned tensors with channel strides that are multiples of 8");
    W2L_REQUIRE(rows * x_cs * 2 < kLim2G && rows * y_cs * 2 < kLim2G, "l2norm_scale_bf16: buffer larger than 2 GiB: split the batch");
    const long long blocks = (rows + 3) / 4;
    hipLaunchKernelGGL(l2norm_scale_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), rows, C,
                       static_cast<const __bf16*>(x), x_cs, weight, static_cast<__bf16*>(y), y_cs);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_s3fd_headb_create(int cin, int ncls, const float* conf_w, const float* conf_b, const float* loc_w, const float* loc_b,
                          void* stream, w2l_s3fd_headb_t** out) {
    W2L_REQUIRE(out && conf_w && loc_w, "NULL argument");
    W2L_REQUIRE(cin >= 32 && cin % 32 == 0, "s3fd_headb: cin=%d must be a multiple of 32", cin);
    W2L_REQUIRE(ncls == 2 || ncls == 4, "s3fd_headb: ncls must be 2 or 4");
    w2l_s3fd_headb* h = new (std::nothrow) w2l_s3fd_headb();
    if (!h) { set_error("out of host memory"); return W2L_ERR_NOMEM; }
    h->cin = cin; h->ncls = ncls;
    if (hipMalloc(&h->w, sizeof(__bf16) * (size_t)cin * 9 * 8) != hipSuccess || hipMalloc(&h->b, sizeof(float) * 8) != hipSuccess) {
        w2l_s3fd_headb_destroy(h);
        set_error("s3fd_headb: device allocation failed");
        return W2L_ERR_HIP;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = headb_pack(h, conf_w, conf_b, loc_w, loc_b, s);
    if (rc == W2L_OK && hipStreamSynchronize(s) != hipSuccess) { set_error("sync after s3fd_headb packing failed"); rc = W2L_ERR_HIP; }
    if (rc != W2L_OK) { w2l_s3fd_headb_destroy(h); return rc; }
    *out = h;
    return W2L_OK;
}

int w2l_s3fd_headb_update(w2l_s3fd_headb_t* h, const float* conf_w, const float* conf_b, const float* loc_w, const float* loc_b,
                          void* stream) {
    W2L_REQUIRE(h && conf_w && loc_w, "NULL argument");
    return headb_pack(h, conf_w, conf_b, loc_w, loc_b, static_cast<hipStream_t>(stream));
}

int w2l_s3fd_headb_destroy(w2l_s3fd_headb_t* h) {
    if (!h) return W2L_OK;
    if (h->w) (void)hipFree(h->w);
    if (h->b) (void)hipFree(h->b);
    delete h;
    return W2L_OK;
}

int w2l_s3fd_headb_decode(const w2l_s3fd_headb_t* h, void* stream, int B, int FH, int FW, int stride, const void* x, int x_cs,
                          float* table) {
    W2L_REQUIRE(h && x && table, "NULL argument");
    W2L_REQUIRE(B >= 1 && FH >= 1 && FW >= 1 && stride >= 1, "bad s3fd_headb_decode shape B=%d FH=%d FW=%d stride=%d", B, FH, FW, stride);
    W2L_REQUIRE(B <= 65535, "s3fd_headb_decode: B=%d > 65535", B);
    W2L_REQUIRE(x_cs >= h->cin && (x_cs & 7) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0,
                "s3fd_headb_decode: x must be 16-byte aligned with x_cs %% 8 == 0 and >= cin=%d, got %d", h->cin, x_cs);
    W2L_REQUIRE((long long)B * FH * FW * x_cs * 2 < kLim2G && (long long)B * FH * FW * 5 * 4 < kLim2G,
                "s3fd_headb_decode: buffer larger than 2 GiB: split the batch");
    const dim3 grid((FW + kHTW - 1) / kHTW, (FH + kHTH - 1) / kHTH, B);
    W2L_REQUIRE(grid.y <= 65535, "s3fd_headb_decode: FH=%d too large", FH);
    hipLaunchKernelGGL(s3fd_headb_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), FH, FW, stride, h->cin, h->ncls,
                       static_cast<const __bf16*>(x), x_cs, h->w, h->b, table);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"
