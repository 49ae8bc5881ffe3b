// Colour matching of generated faces to the crops they were generated from (opt-in; not the reference's output), between the
// generator and the paste: u8 [B,S,S,3] prediction and crop in HBM, the rule of include/w2l_hip.h (w2l_color_match_u8) with the
// arithmetic of color_match_core.h.  One workgroup of 256 lanes per row (27 KB at S = 96), three steps with a barrier between:
//   1. sums: the upper half of a row is its first 3*N bytes; a lane takes groups of 4 pixels (three dwords where the row is
//      4-byte aligned, bytes otherwise and for the short last group) and keeps 12 uint32 partial sums (prediction and crop, value
//      and square, per channel); a xor butterfly folds a wave, LDS the four waves.  Integer sums: the order does not matter.
//   2. lanes 0..2 compute a channel's gain; then every lane computes the transfer of ONE byte value for the three channels into
//      a 3 x 256 byte table in LDS: the 64-bit floor division runs 768 times per row, not once per byte.
//   3. every lane maps groups of 4 pixels of the whole row through the table.  A lane reads and writes the same 12 bytes, and
//      every read of step 1 lies before the barrier, so out == pred works in place.
// HBM-bound byte traffic (a row is read 1.5 times and written once); with 128 rows half the CUs idle for the few microseconds
// the launch takes, against a generator batch of milliseconds: nothing cleverer is built.
#include "w2l_common.h"
#include "color_match_core.h"

namespace w2l {

constexpr int kCmLanes = 256, kCmWaves = kCmLanes / 64;

// `npx` (1..4) consecutive pixels at `p` into px[12]; nothing outside them is read
__device__ __forceinline__ void cm_load_group(const uint8_t* p, bool dwords, int npx, uint8_t px[12]) {
    if (dwords && npx == 4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        const uint32_t v[3] = {q[0], q[1], q[2]};
#pragma unroll
        for (int k = 0; k < 12; ++k) px[k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
    } else {
        for (int k = 0; k < 3 * npx; ++k) px[k] = p[k];
    }
}

__global__ __launch_bounds__(kCmLanes) void color_match_kernel(int B, const uint8_t* pred, const uint8_t* __restrict__ ref, int S,
                                                               int mode, uint8_t* out) {
    __shared__ uint32_t part[kCmWaves][12];     // [wave][sp, so, qp, qo of channel 0 | channel 1 | channel 2]
    __shared__ uint32_t tot[3][2];              // Sp, So of a channel
    __shared__ int32_t gain[3];
    __shared__ uint8_t lut[3 * 256];
    const int b = blockIdx.x, t = threadIdx.x;
    const size_t row = (size_t)b * S * S * 3;
    const uint8_t* p = pred + row;
    const uint8_t* r = ref + row;
    uint8_t* o = out + row;
    const int N = (S >> 1) * S;                 // pixels of the upper half
    const bool p4 = (reinterpret_cast<uintptr_t>(p) & 3) == 0, r4 = (reinterpret_cast<uintptr_t>(r) & 3) == 0;

    uint32_t acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0u;
    for (int g = t; g < (N + 3) >> 2; g += kCmLanes) {
        const int npx = min(4, N - (g << 2));
        uint8_t a[12], c[12];
        cm_load_group(p + (size_t)g * 12, p4, npx, a);
        cm_load_group(r + (size_t)g * 12, r4, npx, c);
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            if (k < 3 * npx) {
                const uint32_t x = a[k], y = c[k];
                const int ch = k % 3;
                acc[4 * ch + 0] += x;
                acc[4 * ch + 1] += y;
                acc[4 * ch + 2] += x * x;
                acc[4 * ch + 3] += y * y;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k)
        for (int d = 32; d > 0; d >>= 1) acc[k] += __shfl_xor(acc[k], d);
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) part[t >> 6][k] = acc[k];
    }
    __syncthreads();
    if (t < 3) {
        uint32_t s[4];
        for (int k = 0; k < 4; ++k) {
            s[k] = 0u;
            for (int w = 0; w < kCmWaves; ++w) s[k] += part[w][4 * t + k];
        }
        gain[t] = cm::gain_q8(mode, (uint32_t)N, cm::Sums{s[0], s[1], s[2], s[3]});
        tot[t][0] = s[0];
        tot[t][1] = s[1];
    }
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        lut[ch * 256 + t] = cm::transfer(gain[ch], (uint32_t)N, tot[ch][0], tot[ch][1], (uint32_t)t);
    __syncthreads();

    const bool o4 = (reinterpret_cast<uintptr_t>(o) & 3) == 0;
    for (int g = t; g < (S * S) >> 2; g += kCmLanes) {      // S even: S*S pixels are whole groups of 4
        uint8_t a[12];
        cm_load_group(p + (size_t)g * 12, p4, 4, a);
#pragma unroll
        for (int k = 0; k < 12; ++k) a[k] = lut[(k % 3) * 256 + a[k]];
        uint8_t* q = o + (size_t)g * 12;
        if (o4) {
            uint32_t v[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k >> 2] |= (uint32_t)a[k] << (8 * (k & 3));
            uint32_t* q4 = reinterpret_cast<uint32_t*>(q);
            q4[0] = v[0]; q4[1] = v[1]; q4[2] = v[2];
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) q[k] = a[k];
        }
    }
}

}  // namespace w2l

using namespace w2l;

extern "C" {

int w2l_color_match_u8(void* stream, int B, const uint8_t* pred, const uint8_t* ref, int S, int mode, uint8_t* out) {
    W2L_REQUIRE(B >= 0, "color_match: B >= 0 (got %d)", B);
    W2L_REQUIRE(S >= 2 && S <= cm::kMaxS && (S & 1) == 0, "color_match: S even and in [2, %d] (got %d)", cm::kMaxS, S);
    W2L_REQUIRE(mode == cm::kModeMean || mode == cm::kModeFull, "color_match: mode 1 (mean) or 2 (full) (got %d)", mode);
    if (B == 0) return W2L_OK;
    W2L_REQUIRE(pred && ref && out, "color_match: NULL pointer");
    hipLaunchKernelGGL(color_match_kernel, dim3(B), dim3(kCmLanes), 0, static_cast<hipStream_t>(stream), B, pred, ref, S, mode, out);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"
