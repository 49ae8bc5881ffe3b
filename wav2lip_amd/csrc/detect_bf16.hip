// The S3FD face detector's fused detection head on the opt-in bf16-storage path (face_detection/s3fd.py), and nothing else: the
// glue between the backbone convolutions - pack, max pool, L2Norm - is one templated body per op for fp32 and bf16 in detect.hip.
//   w2l_s3fd_headb_*         net_s3fd.py:99-120 (conf + loc convolutions of one level) + net_s3fd.py:123-126 + detect.py:66-84:
//                            one 3x3 contraction on v_mfma_f32_16x16x32_bf16 and the decode from the fp32 accumulators
// Layout: NHWC bf16, channel strides in elements and multiples of 8, 16-byte aligned pointers.
#include "w2l_common.h"
#include "w2l_storage.h"

struct w2l_s3fd_headb {
    int cin, ncls;
    __bf16* w = nullptr;    // [cin / 32][9 taps][8 columns][32 channels]: columns 0..3 conf (ncls of them), 4..7 loc
    float* b = nullptr;     // [8], same columns
};

namespace w2l {

constexpr long long kLim2G = 1ll << 31;     // the convb launches' per-buffer rule (32-bit byte offsets)

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
// accumulators + bias go through LDS to one lane per position, which decodes them (s3fd_decode_px, w2l_common.h) and writes the
// (x1, y1, x2, y2, score) row.  Logits never leave the chip.
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
            s3fd_decode_px(c, ncls, c + 4, stride, wx, hy, out + (((long long)n * FH + hy) * FW + wx) * 5);
        }
    }
}

static int headb_pack(w2l_s3fd_headb* h, const float* conf_w, const float* conf_b, const float* loc_w, const float* loc_b,
                      hipStream_t s) {
    const long long total = (long long)h->cin * 9 * 8;
    hipLaunchKernelGGL(s3fd_headb_pack_kernel, dim3(grid_cap(total, 256, 1024)), dim3(256), 0, s, h->cin, h->ncls, conf_w, conf_b,
                       loc_w, loc_b, h->w, h->b);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // namespace w2l

using namespace w2l;

extern "C" {

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
