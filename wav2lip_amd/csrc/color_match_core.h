// Colour matching of a generated face to the crop it was generated from, the arithmetic: the gain from the four sums of a
// channel and the per-pixel transfer, with no HIP type in them, so that the same text is the device code of
// csrc/color_match.hip and the plain host C++ of tools/color_match_host.cpp (which runs it under the host sanitizers).
// Integer work only: the bytes are a function of the input bytes (the rule: include/w2l_hip.h, w2l_color_match_u8).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define W2L_CM_FN __host__ __device__ __forceinline__
#else
#define W2L_CM_FN inline
#endif

namespace w2l {
namespace cm {

enum { kModeMean = 1, kModeFull = 2 };
constexpr int kMaxS = 256;          // N = S/2 * S <= 2^15: sums of squares stay below 2^32, N*Q below 2^47
constexpr int32_t kGainOne = 256, kGainMin = 128, kGainMax = 512;   // Q8, [0.5, 2]

// the sums of one channel over the N pixels of the upper half: prediction and reference, values and squares
struct Sums {
    uint32_t sp, so, qp, qo;
};

// floor(sqrt(q)) held to [kGainMin, kGainMax]: the ends by comparison, between them a bisection on r*r <= q (r <= 512: 32-bit)
W2L_CM_FN int32_t clamped_isqrt(uint64_t q) {
    if (q >= (uint64_t)kGainMax * kGainMax) return kGainMax;
    if (q < (uint64_t)kGainMin * kGainMin) return kGainMin;
    const uint32_t v = (uint32_t)q;
    uint32_t lo = kGainMin, hi = kGainMax;      // lo*lo <= v < hi*hi
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (mid * mid <= v) lo = mid; else hi = mid;
    }
    return (int32_t)lo;
}

// the Q8 ratio of the standard deviations, reference over prediction; 256 in mean mode and for a flat prediction
W2L_CM_FN int32_t gain_q8(int mode, uint32_t N, const Sums& s) {
    if (mode != kModeFull) return kGainOne;
    const uint64_t vp = (uint64_t)N * s.qp - (uint64_t)s.sp * s.sp;     // N*Q >= S^2 (Cauchy-Schwarz): no wrap
    const uint64_t vo = (uint64_t)N * s.qo - (uint64_t)s.so * s.so;     // < 2^46, so vo << 16 fits
    if (vp == 0) return kGainOne;
    return clamped_isqrt((vo << 16) / vp);
}

// out = clamp(floor((g*(N*x - Sp) + 256*So + 128*N) / (256*N)), 0, 255); the numerator is signed, the division a floor
W2L_CM_FN uint8_t transfer(int32_t g, uint32_t N, uint32_t Sp, uint32_t So, uint32_t x) {
    const int64_t num = (int64_t)g * ((int64_t)N * x - (int64_t)Sp) + 256 * (int64_t)So + 128 * (int64_t)N;
    const int64_t den = 256 * (int64_t)N;
    int64_t q = num / den;
    if (num % den < 0) --q;
    return (uint8_t)(q < 0 ? 0 : q > 255 ? 255 : q);
}

}  // namespace cm
}  // namespace w2l
