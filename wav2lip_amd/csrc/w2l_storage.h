// Storage traits of the HBM-bound kernels that exist for fp32 and for bf16 tensors (train_rows.hip, detect.hip): the element type
// and how a thread moves 16 bytes of it - 4 fp32 or 8 bf16 channels - to and from fp32 registers.  The storage type is a template
// argument of those kernels, never a run-time switch.
#pragma once
#include <hip/hip_runtime.h>

namespace w2l {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// VEC consecutive fp32 values (per-channel vectors, fp32 rows) -> registers
template <int VEC>
__device__ __forceinline__ void ldv(const float* p, float* v) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = a[e];
    }
}

struct StF32 {
    typedef float elem;
    static constexpr int kVecLog2 = 2, VEC = 1 << kVecLog2;
    static constexpr const char* suffix = "";
    static __device__ __forceinline__ void ld(const float* p, float* v) { ldv<4>(p, v); }
    static __device__ __forceinline__ void st(float* p, const float* v) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};
struct StBf16 {
    typedef __bf16 elem;
    static constexpr int kVecLog2 = 3, VEC = 1 << kVecLog2;
    static constexpr const char* suffix = "_bf16";
    static __device__ __forceinline__ void ld(const __bf16* p, float* v) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)b[e];
    }
    static __device__ __forceinline__ void st(__bf16* p, const float* v) {   // the one rounding of a stored element (RNE)
        bf16x8 b;
#pragma unroll
        for (int e = 0; e < 8; ++e) b[e] = (__bf16)v[e];
        *reinterpret_cast<bf16x8*>(p) = b;
    }
};

}  // namespace w2l
