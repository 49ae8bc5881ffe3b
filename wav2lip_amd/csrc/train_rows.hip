// HBM-bound row kernels of the training path, ONE implementation for both storage types: BatchNorm in batch-statistics mode
// (forward + backward), activation backward, channel sums (bias gradients) and row adds.
//
// Replaces, on the reference's training loops (wav2lip_train.py:201-262, color_syncnet_train.py:140-190,
// hq_wav2lip_train.py:204-310), the torch autograd nodes of nn.BatchNorm2d in train mode (models/conv.py:10,40),
// ReLU / LeakyReLU / Sigmoid (models/conv.py:12,27,43; models/wav2lip.py:85,152) and the residual add (models/conv.py:17-18).
//
// Tensors are NHWC "[rows][cs]" views (rows = N*H*W pixels, C channels, cs channel stride in elements) of fp32 or bf16 elements;
// the storage type is a template argument (StF32 / StBf16, w2l_storage.h), never a run-time switch.  Every thread moves 16 bytes per row
// and tensor - 4 fp32 or 8 bf16 channels - so a bf16 pass costs half the bytes of its fp32 twin.  Statistics, per-channel vectors
// and every intermediate are fp32 / fp64 in both: column reductions accumulate in fp64 per thread, combine per workgroup through
// LDS and finish in a second kernel in a fixed order (deterministic, no atomics); one rounding to bf16 per stored element.
#include <math.h>
#include <mutex>
#include <vector>

#include "w2l_common.h"
#include "w2l_storage.h"

namespace w2l {

// ---------------------------------------------------------------- what the training reductions add to a storage trait (w2l_storage.h)
template <class S>
struct TrainSt;
template <>
struct TrainSt<StF32> {
    static constexpr bool kMaskFromZ = false;   // no fp32 caller omits y: the recomputed ReLU mask is compiled out
    // column reduction: one row per iteration and one LDS round that carries both sums side by side.  The bf16 shape below has
    // not been measured for fp32 (it costs 9 more VGPRs in the BatchNorm-backward reduction), so fp32 keeps the shape it had
    static constexpr int kRowsInFlight = 1, kLdsRounds = 1;
};
template <>
struct TrainSt<StBf16> {
    static constexpr bool kMaskFromZ = true;    // BatchNorm backward may recompute the ReLU mask as z*scale + shift > 0 (y == NULL)
    // column reduction: two rows per iteration, all their loads issued before the first is consumed (with one load in flight per
    // thread it ran at 1.5 - 2.5 TB/s: latency, not bandwidth); the two sums go through LDS one after the other (18 KB, not 32)
    static constexpr int kRowsInFlight = 2, kLdsRounds = 2;
};

// Branch-free forms for the row loops: `act` is wave-uniform, and a switch per ELEMENT compiles to a scalar branch per element
// (62 branches in the BatchNorm-backward apply kernel, 165 in its reduction: these bandwidth kernels ran at 2-3 TB/s).
// Gradient: slope `neg` on the non-positive side (1 = none, 0 = ReLU, 0.01 = LeakyReLU), y(1-y) bit-selected for the sigmoid.
// The forward is act_leaky (w2l_common.h): a select on v < 0, equal to the switch forms on every input including NaN and +-inf.
struct ActK {
    float neg;
    unsigned sigmask;     // all ones for the sigmoid, else 0
};
__device__ __forceinline__ ActK act_consts(int act) {
    ActK k;
    k.neg = act == W2L_ACT_RELU ? 0.f : (act == W2L_ACT_LEAKY ? 0.01f : 1.f);
    k.sigmask = act == W2L_ACT_SIGMOID ? 0xffffffffu : 0u;
    return k;
}
__device__ __forceinline__ float act_grad_k(const ActK k, float y) {
    const float gr = y > 0.f ? 1.f : k.neg;
    const float gs = y * (1.f - y);
    return __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, gs) & k.sigmask) | (__builtin_bit_cast(unsigned, gr) & ~k.sigmask));
}
// forward on NE values: one wave-uniform branch per row (the sigmoid needs expf), none per element
template <int NE>
__device__ __forceinline__ void act_fwd_n(const ActK k, float* v) {
    if (k.sigmask) {
#pragma unroll
        for (int e = 0; e < NE; ++e) v[e] = 1.0f / (1.0f + expf(-v[e]));
    } else {
#pragma unroll
        for (int e = 0; e < NE; ++e) v[e] = act_leaky(v[e], k.neg);
    }
}

// ---------------------------------------------------------------- column reductions
enum ColMode { kColStats = 0, kColBnBwd = 1, kColSum = 2 };

template <class S>
struct ColArgs {
    const typename S::elem* a;    // stats: z;  bn_bwd: dy;  sum: the tensor
    const typename S::elem* y;    // bn_bwd: block output (activation mask)
    const typename S::elem* z;    // bn_bwd: pre-BN conv output
    const float* mean;  // bn_bwd, padded to C
    const float* rstd;
    const float* scale; // bn_bwd with y == NULL (no residual, ReLU): the mask is recomputed as z*scale + shift > 0
    const float* shift;
    double* partial;    // [nblocks][2][C]
    long long rows;
    int C, a_cs, y_cs, z_cs, act;
    int rows_per_block;
};

// thread -> (VEC-channel group cg = t % CG, row lane t / CG); needs C % VEC == 0 and C <= 1024
template <class S, int MODE>
__global__ __launch_bounds__(256) void col_reduce_kernel(const ColArgs<S> a) {
    constexpr int VEC = S::VEC;
    constexpr int ROUNDS = TrainSt<S>::kLdsRounds;
    // one round: both sums side by side (fp32: 256 x 8 doubles = 16 KB); two rounds: one sum at a time + 1 pad column, the
    // combine walks rows CG apart (bf16: 256 x 9 doubles = 18 KB)
    __shared__ double red[256][ROUNDS == 1 ? 2 * VEC : VEC + 1];
    const int CG = a.C >> S::kVecLog2;
    const int RPP = 256 / CG;
    const int t = threadIdx.x;
    const int cg = t % CG;
    const int rl = t / CG;
    double s0[VEC], s1[VEC];                 // sum; sum of squares / of products
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s0[e] = 0; s1[e] = 0; }
    if (rl < RPP) {
        const long long r0 = (long long)blockIdx.x * a.rows_per_block;
        const long long r1 = r0 + a.rows_per_block < a.rows ? r0 + a.rows_per_block : a.rows;
        float mu[VEC], rs[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) { mu[e] = 0.f; rs[e] = 0.f; }
        float sc[VEC], sh[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) { sc[e] = 0.f; sh[e] = 0.f; }
        const bool no_y = TrainSt<S>::kMaskFromZ && (MODE == kColBnBwd) && a.y == nullptr;
        const ActK ak = act_consts(a.act);
        if (MODE == kColBnBwd) { ldv<VEC>(a.mean + cg * VEC, mu); ldv<VEC>(a.rstd + cg * VEC, rs); }
        if (no_y) { ldv<VEC>(a.scale + cg * VEC, sc); ldv<VEC>(a.shift + cg * VEC, sh); }
        auto accum = [&](const float* v, const float* yv, const float* zv) {
            if (MODE == kColStats) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) { s0[e] += (double)v[e]; s1[e] += (double)v[e] * (double)v[e]; }
            } else if (MODE == kColSum) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) s0[e] += (double)v[e];
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float yy = no_y ? zv[e] * sc[e] + sh[e] : yv[e];      // the forward's own expression (affine_act)
                    const float g = v[e] * act_grad_k(ak, yy);
                    const float zh = (zv[e] - mu[e]) * rs[e];
                    s0[e] += (double)g;
                    s1[e] += (double)g * (double)zh;
                }
            }
        };
        // rows r0 + rl, + RPP, + 2 RPP, ... in this order whether one or two are loaded per iteration
        long long r = r0 + rl;
        if (TrainSt<S>::kRowsInFlight == 2) {
            for (; r + RPP < r1; r += 2 * RPP) {
                float va[VEC], vb[VEC], ya[VEC], yb[VEC], za[VEC], zb[VEC];
                S::ld(a.a + r * a.a_cs + cg * VEC, va);
                S::ld(a.a + (r + RPP) * a.a_cs + cg * VEC, vb);
                if (MODE == kColBnBwd) {
                    if (!no_y) {
                        S::ld(a.y + r * a.y_cs + cg * VEC, ya);
                        S::ld(a.y + (r + RPP) * a.y_cs + cg * VEC, yb);
                    }
                    S::ld(a.z + r * a.z_cs + cg * VEC, za);
                    S::ld(a.z + (r + RPP) * a.z_cs + cg * VEC, zb);
                }
                accum(va, ya, za);
                accum(vb, yb, zb);
            }
        }
        for (; r < r1; r += RPP) {
            float v[VEC], yv[VEC], zv[VEC];
            S::ld(a.a + r * a.a_cs + cg * VEC, v);
            if (MODE == kColBnBwd) {
                if (!no_y) S::ld(a.y + r * a.y_cs + cg * VEC, yv);
                S::ld(a.z + r * a.z_cs + cg * VEC, zv);
            }
            accum(v, yv, zv);
        }
    }
    // in-workgroup combine through LDS, row lanes j = 0 .. RPP-1 in order
    if (ROUNDS == 1) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) { red[t][e] = s0[e]; red[t][VEC + e] = s1[e]; }
        __syncthreads();
        if (t < CG) {
            double o[2 * VEC];
#pragma unroll
            for (int e = 0; e < 2 * VEC; ++e) o[e] = 0;
            for (int j = 0; j < RPP; ++j)
#pragma unroll
                for (int e = 0; e < 2 * VEC; ++e) o[e] += red[t + j * CG][e];
            double* dst = a.partial + (long long)blockIdx.x * 2 * a.C;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { dst[t * VEC + e] = o[e]; dst[a.C + t * VEC + e] = o[VEC + e]; }
        }
    } else {   // the sum, then the sum of squares / products
        double o0[VEC], o1[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) red[t][e] = s0[e];
        __syncthreads();
        if (t < CG) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) o0[e] = 0;
            for (int j = 0; j < RPP; ++j)
#pragma unroll
                for (int e = 0; e < VEC; ++e) o0[e] += red[t + j * CG][e];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < VEC; ++e) red[t][e] = s1[e];
        __syncthreads();
        if (t < CG) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) o1[e] = 0;
            for (int j = 0; j < RPP; ++j)
#pragma unroll
                for (int e = 0; e < VEC; ++e) o1[e] += red[t + j * CG][e];
            double* dst = a.partial + (long long)blockIdx.x * 2 * a.C;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { dst[t * VEC + e] = o0[e]; dst[a.C + t * VEC + e] = o1[e]; }
        }
    }
}

struct ColFinalArgs {
    const double* partial;
    int nblocks, C, Cvalid;   // C: padded channels of the partials; Cvalid: channels that exist (outputs beyond are skipped)
    long long rows;
    // stats
    const float* gamma;
    const float* beta;
    float eps, momentum;
    float* mean;
    float* rstd;
    float* scale;       // gamma*rstd
    float* shift;       // beta - mean*gamma*rstd
    float* running_mean;
    float* running_var;
    // bn_bwd / sum
    float* out0;        // sum of g (d beta) / column sum
    float* out1;        // sum of g*zhat (d gamma)
};

// 64 channels per workgroup; the partial blocks are split 4 ways across the waves and summed with 4 independent loads in
// flight per thread (a serial walk over ~1000 partials costs >100 us of pure latency), then combined through LDS in a
// fixed order
template <int MODE>
__global__ __launch_bounds__(256) void col_final_kernel(const ColFinalArgs a) {
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    double s0 = 0, s1 = 0;
    if (c < a.C) {
        const long long st = 2ll * a.C;
        const double* p = a.partial + c;
        double t0[4] = {0, 0, 0, 0}, t1[4] = {0, 0, 0, 0};
        int b = part;
        for (; b + 12 < a.nblocks; b += 16) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                t0[u] += p[(long long)(b + 4 * u) * st];
                if (MODE != kColSum) t1[u] += p[(long long)(b + 4 * u) * st + a.C];
            }
        }
        for (; b < a.nblocks; b += 4) {
            t0[0] += p[(long long)b * st];
            if (MODE != kColSum) t1[0] += p[(long long)b * st + a.C];
        }
        s0 = (t0[0] + t0[1]) + (t0[2] + t0[3]);
        s1 = (t1[0] + t1[1]) + (t1[2] + t1[3]);
    }
    red[0][part][cl] = s0;
    red[1][part][cl] = s1;
    __syncthreads();
    if (part != 0 || c >= a.C) return;
    s0 = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
    s1 = (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]);
    const bool live = c < a.Cvalid;
    if (MODE == kColStats) {
        const double m = s0 / (double)a.rows;
        double var = s1 / (double)a.rows - m * m;
        if (var < 0) var = 0;
        const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
        const float mf = (float)m;
        // the per-channel vectors are padded to C (multiple of the vector width) so that the elementwise kernels can load them as
        // vectors: pad channels get the identity of a zero tensor (mean 0, scale 0, shift 0)
        a.mean[c] = live ? mf : 0.f;
        a.rstd[c] = live ? rstd : 0.f;
        const float sc = live ? (a.gamma ? a.gamma[c] : 1.f) * rstd : 0.f;
        a.scale[c] = sc;
        a.shift[c] = live ? (a.beta ? a.beta[c] : 0.f) - mf * sc : 0.f;
        if (live && a.running_mean) a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mf;
        if (live && a.running_var) {
            const double unb = a.rows > 1 ? var * (double)a.rows / (double)(a.rows - 1) : var;
            a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * (float)unb;
        }
    } else {
        if (a.out0) a.out0[c] = live ? (float)s0 : 0.f;
        if (a.out1) a.out1[c] = live ? (float)s1 : 0.f;
    }
}

// fp64 scratch for the reduction partials, one fixed 16 MiB buffer PER STREAM (covers 512 workgroups x 1024 channels x 2
// sums and the 1024 L1 partials): stream-ordered reuse, no sharing between streams.  Every user - the reductions here in either
// storage type, the conv-epilogue partials below, w2l_l1_mean (train.hip) - enqueues the kernel that fills the partials and the
// kernel that consumes them back to back on that stream, so one buffer serves them all.
struct PartialWs {
    hipStream_t stream;
    double* ptr;
};
static std::mutex g_partial_mutex;
static std::vector<PartialWs> g_partial_table;
constexpr size_t kPartialBytes = (size_t)16 << 20;
double* partial_ws(hipStream_t stream, size_t bytes) {
    if (bytes > kPartialBytes) { set_error("reduction scratch request of %zu bytes exceeds the fixed buffer", bytes); return nullptr; }
    std::lock_guard<std::mutex> lock(g_partial_mutex);
    for (const PartialWs& w : g_partial_table)
        if (w.stream == stream) return w.ptr;
    double* p = nullptr;
    if (hipMalloc(&p, kPartialBytes) != hipSuccess) { set_error("hipMalloc(reduction scratch) failed"); return nullptr; }
    g_partial_table.push_back(PartialWs{stream, p});
    return p;
}

// `what` names the entry point (the storage suffix is added here), `tensor` the argument (" dy", or "")
template <class S>
static int row_check(long long rows, int C, const void* p, int cs, const char* what, const char* tensor) {
    constexpr int VEC = S::VEC;
    W2L_REQUIRE(rows >= 1 && C >= VEC && (C & (VEC - 1)) == 0 && C <= 1024, "%s%s%s: C=%d must be a multiple of %d in [%d, 1024]", what,
                S::suffix, tensor, C, VEC, VEC);
    W2L_REQUIRE(p && cs >= C && (cs & (VEC - 1)) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0,
                "%s%s%s: tensor must be 16-byte aligned with a channel stride that is a multiple of %d (cs=%d)", what, S::suffix, tensor,
                VEC, cs);
    return W2L_OK;
}

template <int MODE>
static int col_final_launch(ColFinalArgs f, hipStream_t s) {
    hipLaunchKernelGGL(col_final_kernel<MODE>, dim3(ceil_div(f.C, 64)), dim3(256), 0, s, f);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

template <class S, int MODE>
static int col_reduce_launch(ColArgs<S> a, ColFinalArgs f, hipStream_t s) {
    const int CG = a.C >> S::kVecLog2;
    const int RPP = 256 / CG;
    // at most 512 workgroups: the finalize pass walks every partial with C / 64 workgroups, so 1 024 partials cost it more than
    // the reduction gains from them (cfg4 26.3 -> 26.1 ms at 512, 26.6 at 256; session r03ze)
    long long per = (a.rows + 511) / 512;
    const long long min_rows = (long long)RPP * (64 / S::VEC);   // at least 64 elements per thread
    if (per < min_rows) per = min_rows;
    a.rows_per_block = (int)per;
    const int nblocks = (int)((a.rows + per - 1) / per);
    a.partial = partial_ws(s, (size_t)nblocks * 2 * a.C * sizeof(double));
    if (!a.partial) return W2L_ERR_NOMEM;
    hipLaunchKernelGGL((col_reduce_kernel<S, MODE>), dim3(nblocks), dim3(256), 0, s, a);
    W2L_HIP_CHECK(hipGetLastError());
    f.partial = a.partial;
    f.nblocks = nblocks;
    f.C = a.C;
    f.rows = a.rows;
    return col_final_launch<MODE>(f, s);
}

// ---- BatchNorm statistics from the conv epilogue's per-wave column partials (conv_bf16.hip): fp32 [npart][2][cout_p] ->
// fp64 [R][2][C] by R <= 256 workgroups (64 channels x 4 row lanes, four loads in flight per thread, fixed order), then the
// same finalize as the stand-alone reduction
__global__ __launch_bounds__(256) void stats_partial_reduce_kernel(const float* __restrict__ part, int npart, int cout_p, int C,
                                                                   int rows_per_block, double* __restrict__ out) {
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cl;
    const int r0 = blockIdx.x * rows_per_block, r1 = min(npart, r0 + rows_per_block);
    double s0 = 0, s1 = 0;
    if (c < C) {
        const long long st = 2ll * cout_p;
        const float* p = part + c;
        double t0[4] = {0, 0, 0, 0}, t1[4] = {0, 0, 0, 0};
        int r = r0 + q;
        for (; r + 12 < r1; r += 16) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                t0[u] += (double)p[(long long)(r + 4 * u) * st];
                t1[u] += (double)p[(long long)(r + 4 * u) * st + cout_p];
            }
        }
        for (; r < r1; r += 4) {
            t0[0] += (double)p[(long long)r * st];
            t1[0] += (double)p[(long long)r * st + cout_p];
        }
        s0 = (t0[0] + t0[1]) + (t0[2] + t0[3]);
        s1 = (t1[0] + t1[1]) + (t1[2] + t1[3]);
    }
    red[0][q][cl] = s0;
    red[1][q][cl] = s1;
    __syncthreads();
    if (q == 0 && c < C) {
        double* dst = out + (long long)blockIdx.x * 2 * C;
        dst[c] = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
        dst[C + c] = (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]);
    }
}

// both levels: `f` carries C, Cvalid, rows and the outputs of the finalize
template <int MODE>
static int from_partials(hipStream_t s, const float* part, int npart, int cout_p, ColFinalArgs f) {
    int R = ceil_div(npart, 64);
    if (R > 256) R = 256;
    if (R < 1) R = 1;
    const int rpb = ceil_div(npart, R);
    R = ceil_div(npart, rpb);
    double* out = partial_ws(s, (size_t)R * 2 * f.C * sizeof(double));
    if (!out) return W2L_ERR_NOMEM;
    hipLaunchKernelGGL(stats_partial_reduce_kernel, dim3(R, ceil_div(f.C, 64)), dim3(256), 0, s, part, npart, cout_p, f.C, rpb, out);
    W2L_HIP_CHECK(hipGetLastError());
    f.partial = out;
    f.nblocks = R;
    return col_final_launch<MODE>(f, s);
}

int bn_stats_from_partials(hipStream_t s, const float* part, int npart, int cout_p, long long rows, int C, int Cvalid,
                           const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                           float* mean, float* rstd, float* scale, float* shift) {
    ColFinalArgs f = {};
    f.C = C; f.Cvalid = Cvalid; f.rows = rows;
    f.gamma = gamma; f.beta = beta; f.eps = eps; f.momentum = momentum;
    f.mean = mean; f.rstd = rstd; f.scale = scale; f.shift = shift;
    f.running_mean = running_mean; f.running_var = running_var;
    return from_partials<kColStats>(s, part, npart, cout_p, f);
}

// the two BatchNorm-backward column sums from a data-gradient conv's epilogue partials (w2l_convb_forward_bnbwd): the same two
// levels, finished as the stand-alone reduction finishes them (out0 = sum g -> dbeta, out1 = sum g * zhat -> dgamma)
int bn_bwd_sums_from_partials(hipStream_t s, const float* part, int npart, int cout_p, int C, int Cvalid, float* dgamma, float* dbeta) {
    ColFinalArgs f = {};
    f.C = C; f.Cvalid = Cvalid; f.rows = 1;
    f.out0 = dbeta; f.out1 = dgamma;
    return from_partials<kColBnBwd>(s, part, npart, cout_p, f);
}

// ---------------------------------------------------------------- elementwise over [rows][C]
template <class S>
struct EwArgs {
    const typename S::elem* a;     // affine: z;            bn_bwd_apply: dy;      act_bwd: dy
    const typename S::elem* b;     // affine: res or NULL;  bn_bwd_apply: y;       act_bwd: y
    const typename S::elem* c;     //                       bn_bwd_apply: z
    typename S::elem* out;         // affine: y;            bn_bwd_apply: dz;      act_bwd: dz
    typename S::elem* out2;        //                       in-place g (= masked dy) or NULL
    const float* v0;     // per-channel, padded to C: affine scale;   bwd: scale_eff;   act_bwd: scale or NULL
    const float* v1;     //                           affine shift;   bwd: mean
    const float* v2;     //                                           bwd: rstd
    const float* v3;     //                                           bwd: sum_g
    const float* v4;     //                                           bwd: sum_gz
    const float* v5;     // bn_bwd without y: the forward shift (beta - mean * gamma * rstd); the mask is z*v0 + v5 > 0
    long long rows;
    int C, a_cs, b_cs, c_cs, out_cs, out2_cs, act;
    float inv_rows;
};

enum EwMode { kEwAffine = 0, kEwBnBwd = 1, kEwActBwd = 2, kEwAdd = 3 };

// thread -> (VEC-channel group t % CG, row lane t / CG): the per-channel vectors are loaded once per thread
template <class S, int MODE>
__global__ __launch_bounds__(256) void ew_kernel(const EwArgs<S> a) {
    constexpr int VEC = S::VEC;
    const int CG = a.C >> S::kVecLog2;
    const int RPP = 256 / CG;
    const int c = (threadIdx.x % CG) * VEC;
    const int rl = threadIdx.x / CG;
    if (rl >= RPP) return;
    float v0[VEC], v1[VEC], v2[VEC], v3[VEC], v4[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { v0[e] = 1.f; v1[e] = 0.f; v2[e] = 0.f; v3[e] = 0.f; v4[e] = 0.f; }
    if (a.v0) ldv<VEC>(a.v0 + c, v0);
    if (a.v1) ldv<VEC>(a.v1 + c, v1);
    if (a.v2) ldv<VEC>(a.v2 + c, v2);
    if (a.v3) ldv<VEC>(a.v3 + c, v3);
    if (a.v4) ldv<VEC>(a.v4 + c, v4);
    float v5[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) v5[e] = 0.f;
    if (TrainSt<S>::kMaskFromZ && MODE == kEwBnBwd && a.v5) ldv<VEC>(a.v5 + c, v5);
    const ActK ak = act_consts(a.act);
    for (long long r = (long long)blockIdx.x * RPP + rl; r < a.rows; r += (long long)gridDim.x * RPP) {
        float av[VEC], o[VEC];
        S::ld(a.a + r * a.a_cs + c, av);
        if (MODE == kEwAffine) {          // v0 scale, v1 shift
            float rv[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) rv[e] = 0.f;
            if (a.b) S::ld(a.b + r * a.b_cs + c, rv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = av[e] * v0[e] + v1[e] + rv[e];
            act_fwd_n<VEC>(ak, o);
        } else if (MODE == kEwBnBwd) {   // v0 gamma*rstd, v1 mean, v2 rstd, v3 sum g, v4 sum g*zhat
            float yv[VEC], zv[VEC], g[VEC];
            S::ld(a.c + r * a.c_cs + c, zv);
            if (!TrainSt<S>::kMaskFromZ || a.b) S::ld(a.b + r * a.b_cs + c, yv);
            else {
#pragma unroll
                for (int e = 0; e < VEC; ++e) yv[e] = zv[e] * v0[e] + v5[e];
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                g[e] = av[e] * act_grad_k(ak, yv[e]);
                const float zh = (zv[e] - v1[e]) * v2[e];
                o[e] = v0[e] * (g[e] - v3[e] * a.inv_rows - zh * (v4[e] * a.inv_rows));
            }
            if (a.out2) S::st(a.out2 + r * a.out2_cs + c, g);
        } else if (MODE == kEwActBwd) {  // v0 scale (or ones)
            float yv[VEC], g[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) yv[e] = 1.f;
            if (a.b) S::ld(a.b + r * a.b_cs + c, yv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                g[e] = av[e] * act_grad_k(ak, yv[e]);
                o[e] = g[e] * v0[e];
            }
            if (a.out2) S::st(a.out2 + r * a.out2_cs + c, g);
        } else {
            float bv[VEC];
            S::ld(a.b + r * a.b_cs + c, bv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = av[e] + bv[e];
        }
        S::st(a.out + r * a.out_cs + c, o);
    }
}

template <class S, int MODE>
static int ew_launch(const EwArgs<S>& a, hipStream_t s) {
    const int RPP = 256 / (a.C >> S::kVecLog2);
    hipLaunchKernelGGL((ew_kernel<S, MODE>), dim3(grid_cap(a.rows, RPP * 4, 16384)), dim3(256), 0, s, a);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

// ---------------------------------------------------------------- the row operations, one host function per pair of entry points
template <class S>
static int bn_train_stats(hipStream_t s, long long rows, int C, int Cvalid, const typename S::elem* z, int z_cs, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                          float* rstd, float* scale, float* shift) {
    if (row_check<S>(rows, C, z, z_cs, "bn_train_stats", "") != W2L_OK) return W2L_ERR_ARG;
    W2L_REQUIRE(mean && rstd && scale && shift, "bn_train_stats%s: NULL output", S::suffix);
    W2L_REQUIRE(Cvalid >= 1 && Cvalid <= C, "bn_train_stats%s: Cvalid=%d outside [1, C=%d]", S::suffix, Cvalid, C);
    ColArgs<S> a = {};
    a.a = z; a.a_cs = z_cs; a.rows = rows; a.C = C;
    ColFinalArgs f = {};
    f.Cvalid = Cvalid; f.gamma = gamma; f.beta = beta; f.eps = eps; f.momentum = momentum;
    f.mean = mean; f.rstd = rstd; f.scale = scale; f.shift = shift;
    f.running_mean = running_mean; f.running_var = running_var;
    return col_reduce_launch<S, kColStats>(a, f, s);
}

template <class S>
static int affine_act(hipStream_t s, long long rows, int C, const typename S::elem* z, int z_cs, const float* scale, const float* shift,
                      const typename S::elem* res, int res_cs, int act, typename S::elem* y, int y_cs) {
    if (row_check<S>(rows, C, z, z_cs, "affine_act", " z") != W2L_OK || row_check<S>(rows, C, y, y_cs, "affine_act", " y") != W2L_OK)
        return W2L_ERR_ARG;
    W2L_REQUIRE(scale && shift, "affine_act%s: NULL scale/shift", S::suffix);
    W2L_REQUIRE(res == nullptr || row_check<S>(rows, C, res, res_cs, "affine_act", " res") == W2L_OK, "affine_act%s: bad residual", S::suffix);
    EwArgs<S> a = {};
    a.a = z; a.a_cs = z_cs; a.b = res; a.b_cs = res_cs; a.out = y; a.out_cs = y_cs;
    a.v0 = scale; a.v1 = shift; a.rows = rows; a.C = C; a.act = act;
    return ew_launch<S, kEwAffine>(a, s);
}

// the elementwise half of the BatchNorm backward, given the two column sums (arguments checked by the callers)
template <class S>
static int bn_bwd_apply(hipStream_t s, long long rows, int C, const typename S::elem* dy, int dy_cs, const typename S::elem* y, int y_cs,
                        const typename S::elem* z, int z_cs, int act, const float* mean, const float* rstd, const float* scale,
                        const float* shift, const float* dgamma, const float* dbeta, typename S::elem* dz, int dz_cs,
                        typename S::elem* g_out, int g_cs) {
    EwArgs<S> e = {};
    e.a = dy; e.a_cs = dy_cs; e.b = y; e.b_cs = y_cs; e.c = z; e.c_cs = z_cs; e.out = dz; e.out_cs = dz_cs;
    e.out2 = g_out; e.out2_cs = g_cs;
    e.v0 = scale; e.v1 = mean; e.v2 = rstd; e.v3 = dbeta; e.v4 = dgamma; e.v5 = shift;
    e.rows = rows; e.C = C; e.act = act; e.inv_rows = (float)(1.0 / (double)rows);
    return ew_launch<S, kEwBnBwd>(e, s);
}

template <class S>
static int bn_train_bwd(hipStream_t s, long long rows, int C, int Cvalid, const typename S::elem* dy, int dy_cs, const typename S::elem* y,
                        int y_cs, const typename S::elem* z, int z_cs, int act, const float* mean, const float* rstd, const float* scale,
                        const float* shift, float* dgamma, float* dbeta, typename S::elem* dz, int dz_cs, typename S::elem* g_out,
                        int g_cs) {
    if (row_check<S>(rows, C, dy, dy_cs, "bn_train_bwd", " dy") != W2L_OK ||
        (y != nullptr && row_check<S>(rows, C, y, y_cs, "bn_train_bwd", " y") != W2L_OK) ||
        row_check<S>(rows, C, z, z_cs, "bn_train_bwd", " z") != W2L_OK || row_check<S>(rows, C, dz, dz_cs, "bn_train_bwd", " dz") != W2L_OK)
        return W2L_ERR_ARG;
    W2L_REQUIRE(mean && rstd && scale && dgamma && dbeta, "bn_train_bwd%s: NULL argument", S::suffix);
    W2L_REQUIRE(Cvalid >= 1 && Cvalid <= C, "bn_train_bwd%s: Cvalid=%d outside [1, C=%d]", S::suffix, Cvalid, C);
    W2L_REQUIRE(y != nullptr || (TrainSt<S>::kMaskFromZ && shift != nullptr && act == W2L_ACT_RELU && g_out == nullptr),
                "bn_train_bwd%s: y may be omitted only in bf16 storage, for a ReLU block without residual, with the forward shift given",
                S::suffix);
    W2L_REQUIRE(g_out == nullptr || row_check<S>(rows, C, g_out, g_cs, "bn_train_bwd", " g") == W2L_OK, "bn_train_bwd%s: bad g_out", S::suffix);
    ColArgs<S> a = {};
    a.a = dy; a.a_cs = dy_cs; a.y = y; a.y_cs = y_cs; a.z = z; a.z_cs = z_cs; a.mean = mean; a.rstd = rstd;
    a.scale = scale; a.shift = shift; a.rows = rows; a.C = C; a.act = act;
    ColFinalArgs f = {};
    f.Cvalid = Cvalid; f.out0 = dbeta; f.out1 = dgamma;
    const int rc = col_reduce_launch<S, kColBnBwd>(a, f, s);
    if (rc != W2L_OK) return rc;
    return bn_bwd_apply<S>(s, rows, C, dy, dy_cs, y, y_cs, z, z_cs, act, mean, rstd, scale, shift, dgamma, dbeta, dz, dz_cs, g_out, g_cs);
}

template <class S>
static int act_bwd(hipStream_t s, long long rows, int C, const typename S::elem* dy, int dy_cs, const typename S::elem* y, int y_cs,
                   int act, const float* scale, typename S::elem* dz, int dz_cs, typename S::elem* g_out, int g_cs) {
    if (row_check<S>(rows, C, dy, dy_cs, "act_bwd", " dy") != W2L_OK || row_check<S>(rows, C, dz, dz_cs, "act_bwd", " dz") != W2L_OK)
        return W2L_ERR_ARG;
    W2L_REQUIRE(act == W2L_ACT_NONE || row_check<S>(rows, C, y, y_cs, "act_bwd", " y") == W2L_OK, "act_bwd%s: bad y", S::suffix);
    W2L_REQUIRE(g_out == nullptr || row_check<S>(rows, C, g_out, g_cs, "act_bwd", " g") == W2L_OK, "act_bwd%s: bad g_out", S::suffix);
    EwArgs<S> e = {};
    e.a = dy; e.a_cs = dy_cs; e.b = act == W2L_ACT_NONE ? nullptr : y; e.b_cs = y_cs; e.out = dz; e.out_cs = dz_cs;
    e.out2 = g_out; e.out2_cs = g_cs; e.v0 = scale; e.rows = rows; e.C = C; e.act = act;
    return ew_launch<S, kEwActBwd>(e, s);
}

template <class S>
static int add_rows(hipStream_t s, long long rows, int C, const typename S::elem* a, int a_cs, const typename S::elem* b, int b_cs,
                    typename S::elem* out, int out_cs) {
    if (row_check<S>(rows, C, a, a_cs, "add_rows", " a") != W2L_OK || row_check<S>(rows, C, b, b_cs, "add_rows", " b") != W2L_OK ||
        row_check<S>(rows, C, out, out_cs, "add_rows", " out") != W2L_OK)
        return W2L_ERR_ARG;
    EwArgs<S> e = {};
    e.a = a; e.a_cs = a_cs; e.b = b; e.b_cs = b_cs; e.out = out; e.out_cs = out_cs; e.rows = rows; e.C = C;
    return ew_launch<S, kEwAdd>(e, s);
}

template <class S>
static int col_sum(hipStream_t s, long long rows, int C, const typename S::elem* x, int x_cs, float* out) {
    if (row_check<S>(rows, C, x, x_cs, "col_sum", "") != W2L_OK) return W2L_ERR_ARG;
    W2L_REQUIRE(out, "col_sum%s: NULL output", S::suffix);
    ColArgs<S> a = {};
    a.a = x; a.a_cs = x_cs; a.rows = rows; a.C = C;
    ColFinalArgs f = {};
    f.Cvalid = C; f.out0 = out;
    return col_reduce_launch<S, kColSum>(a, f, s);
}

static inline const __bf16* as_bf16(const void* p) { return static_cast<const __bf16*>(p); }
static inline __bf16* as_bf16(void* p) { return static_cast<__bf16*>(p); }

}  // namespace w2l

using namespace w2l;

extern "C" {

int w2l_bn_train_stats(void* stream, long long rows, int C, const float* z, int z_cs, const float* gamma,
                       const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                       float* mean, float* rstd, float* scale, float* shift) {
    return bn_train_stats<StF32>(static_cast<hipStream_t>(stream), rows, C, C, z, z_cs, gamma, beta, eps, momentum, running_mean,
                                 running_var, mean, rstd, scale, shift);
}
int w2l_bn_train_stats_bf16(void* stream, long long rows, int C, int Cvalid, const void* z, int z_cs, const float* gamma,
                            const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                            float* rstd, float* scale, float* shift) {
    return bn_train_stats<StBf16>(static_cast<hipStream_t>(stream), rows, C, Cvalid, as_bf16(z), z_cs, gamma, beta, eps, momentum,
                                  running_mean, running_var, mean, rstd, scale, shift);
}

int w2l_affine_act(void* stream, long long rows, int C, const float* z, int z_cs, const float* scale,
                   const float* shift, const float* res, int res_cs, int act, float* y, int y_cs) {
    return affine_act<StF32>(static_cast<hipStream_t>(stream), rows, C, z, z_cs, scale, shift, res, res_cs, act, y, y_cs);
}
int w2l_affine_act_bf16(void* stream, long long rows, int C, const void* z, int z_cs, const float* scale, const float* shift,
                        const void* res, int res_cs, int act, void* y, int y_cs) {
    return affine_act<StBf16>(static_cast<hipStream_t>(stream), rows, C, as_bf16(z), z_cs, scale, shift, as_bf16(res), res_cs, act, as_bf16(y), y_cs);
}

int w2l_bn_train_bwd(void* stream, long long rows, int C, const float* dy, int dy_cs, const float* y, int y_cs,
                     const float* z, int z_cs, int act, const float* mean, const float* rstd, const float* scale,
                     float* dgamma, float* dbeta, float* dz, int dz_cs, float* g_out, int g_cs) {
    return bn_train_bwd<StF32>(static_cast<hipStream_t>(stream), rows, C, C, dy, dy_cs, y, y_cs, z, z_cs, act, mean, rstd, scale, nullptr,
                               dgamma, dbeta, dz, dz_cs, g_out, g_cs);
}
int w2l_bn_train_bwd_bf16(void* stream, long long rows, int C, int Cvalid, const void* dy, int dy_cs, const void* y, int y_cs,
                          const void* z, int z_cs, int act, const float* mean, const float* rstd, const float* scale,
                          const float* shift, float* dgamma, float* dbeta, void* dz, int dz_cs, void* g_out, int g_cs) {
    return bn_train_bwd<StBf16>(static_cast<hipStream_t>(stream), rows, C, Cvalid, as_bf16(dy), dy_cs, as_bf16(y), y_cs, as_bf16(z), z_cs, act, mean, rstd,
                                scale, shift, dgamma, dbeta, as_bf16(dz), dz_cs, as_bf16(g_out), g_cs);
}

// bf16 only: the elementwise half alone, for blocks whose column sums came out of a data-gradient conv's epilogue
int w2l_bn_train_bwd_apply_bf16(void* stream, long long rows, int C, const void* dy, int dy_cs, const void* y, int y_cs,
                                const void* z, int z_cs, int act, const float* mean, const float* rstd, const float* scale,
                                const float* shift, const float* dgamma, const float* dbeta, void* dz, int dz_cs, void* g_out,
                                int g_cs) {
    const char* what = "bn_train_bwd_apply";
    if (row_check<StBf16>(rows, C, dy, dy_cs, what, " dy") != W2L_OK ||
        (y != nullptr && row_check<StBf16>(rows, C, y, y_cs, what, " y") != W2L_OK) ||
        row_check<StBf16>(rows, C, z, z_cs, what, " z") != W2L_OK || row_check<StBf16>(rows, C, dz, dz_cs, what, " dz") != W2L_OK)
        return W2L_ERR_ARG;
    W2L_REQUIRE(mean && rstd && scale && dgamma && dbeta, "bn_train_bwd_apply_bf16: bad argument");
    W2L_REQUIRE(y != nullptr || act == W2L_ACT_NONE || (shift != nullptr && act == W2L_ACT_RELU && g_out == nullptr),
                "bn_train_bwd_apply_bf16: y may be omitted only for a ReLU block without residual, with the forward shift given, or "
                "with act = none when dy already is the masked gradient");
    W2L_REQUIRE(g_out == nullptr || row_check<StBf16>(rows, C, g_out, g_cs, what, " g") == W2L_OK, "bn_train_bwd_apply_bf16: bad g_out");
    return bn_bwd_apply<StBf16>(static_cast<hipStream_t>(stream), rows, C, as_bf16(dy), dy_cs, as_bf16(y), y_cs, as_bf16(z), z_cs, act, mean, rstd, scale,
                                shift, dgamma, dbeta, as_bf16(dz), dz_cs, as_bf16(g_out), g_cs);
}

int w2l_act_bwd(void* stream, long long rows, int C, const float* dy, int dy_cs, const float* y, int y_cs, int act,
                const float* scale, float* dz, int dz_cs, float* g_out, int g_cs) {
    return act_bwd<StF32>(static_cast<hipStream_t>(stream), rows, C, dy, dy_cs, y, y_cs, act, scale, dz, dz_cs, g_out, g_cs);
}
int w2l_act_bwd_bf16(void* stream, long long rows, int C, const void* dy, int dy_cs, const void* y, int y_cs, int act,
                     const float* scale, void* dz, int dz_cs, void* g_out, int g_cs) {
    return act_bwd<StBf16>(static_cast<hipStream_t>(stream), rows, C, as_bf16(dy), dy_cs, as_bf16(y), y_cs, act, scale, as_bf16(dz), dz_cs, as_bf16(g_out), g_cs);
}

int w2l_add_rows(void* stream, long long rows, int C, const float* a, int a_cs, const float* b, int b_cs, float* out,
                 int out_cs) {
    return add_rows<StF32>(static_cast<hipStream_t>(stream), rows, C, a, a_cs, b, b_cs, out, out_cs);
}
int w2l_add_rows_bf16(void* stream, long long rows, int C, const void* a, int a_cs, const void* b, int b_cs, void* out, int out_cs) {
    return add_rows<StBf16>(static_cast<hipStream_t>(stream), rows, C, as_bf16(a), a_cs, as_bf16(b), b_cs, as_bf16(out), out_cs);
}

int w2l_col_sum(void* stream, long long rows, int C, const float* x, int x_cs, float* out) {
    return col_sum<StF32>(static_cast<hipStream_t>(stream), rows, C, x, x_cs, out);
}
int w2l_col_sum_bf16(void* stream, long long rows, int C, const void* x, int x_cs, float* out) {
    return col_sum<StBf16>(static_cast<hipStream_t>(stream), rows, C, as_bf16(x), x_cs, out);
}

}  // extern "C"
