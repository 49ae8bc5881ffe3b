// Training-side kernels of libw2l_hip.so beside the row kernels (train_rows.hip): loss forward/backward pairs, a fused
// multi-tensor Adam and the LSE-style sync scoring.
//
// Replaces, on the reference's training loops (wav2lip_train.py:201-262, color_syncnet_train.py:140-190,
// hq_wav2lip_train.py:204-310), the torch autograd nodes of: nn.L1Loss (wav2lip_train.py:191),
// cosine_similarity + BCELoss (wav2lip_train.py:179-184), F.normalize (models/syncnet.py:62-63),
// F.binary_cross_entropy (models/wav2lip.py:171) and optim.Adam (wav2lip_train.py:359).
#include <math.h>
#include <new>
#include <vector>

#include "w2l_common.h"

namespace w2l {

// ---------------------------------------------------------------- losses
// stage 1 of a deterministic mean: per-workgroup fp64 partial of sum |a-b|
__global__ __launch_bounds__(256) void l1_partial_kernel(long long n, const float* __restrict__ a,
                                                         const float* __restrict__ b, double* __restrict__ partial) {
    __shared__ double red[4];
    double s = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        s += (double)fabsf(a[i] - b[i]);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// one wave: lane l sums partials l, l + 64, ... (four in flight), then a fixed-order xor fold - deterministic, and 3 us instead of the
// 57 us one thread needed to walk ~2 000 partials (it sits on the critical path between the generator's forward and backward)
__global__ void mean_final_kernel(int nblocks, const double* __restrict__ partial, double inv_n, float* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    const int l = threadIdx.x;
    double t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    int i = l;
    for (; i + 192 < nblocks; i += 256) {
        t0 += partial[i];
        t1 += partial[i + 64];
        t2 += partial[i + 128];
        t3 += partial[i + 192];
    }
    for (; i < nblocks; i += 64) t0 += partial[i];
    double s = (t0 + t1) + (t2 + t3);
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (l == 0) out[0] = (float)(s * inv_n);
}
// d/da mean|a-b| = sign(a-b)/n, scaled by the upstream gradient gout[0] (device scalar)
__global__ void l1_bwd_kernel(long long n, const float* __restrict__ a, const float* __restrict__ b,
                              const float* __restrict__ gout, float inv_n, float* __restrict__ da) {
    const float gsc = (gout ? gout[0] : 1.f) * inv_n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float d = a[i] - b[i];
        da[i] = d > 0.f ? gsc : (d < 0.f ? -gsc : 0.f);
    }
}

// one wave per row: gradient of mean BCE(cos(a,v), y) w.r.t. a and v
__global__ void cosine_bce_bwd_kernel(int N, int C, const float* __restrict__ a, const float* __restrict__ v,
                                      const float* __restrict__ y, const float* __restrict__ gout,
                                      float* __restrict__ da, float* __restrict__ dv) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* pa = a + (long long)row * C;
    const float* pv = v + (long long)row * C;
    float dot = 0.f, na = 0.f, nv = 0.f;
    for (int c = lane; c < C; c += 64) {
        dot += pa[c] * pv[c];
        na += pa[c] * pa[c];
        nv += pv[c] * pv[c];
    }
    for (int o = 32; o > 0; o >>= 1) {
        dot += __shfl_xor(dot, o);
        na += __shfl_xor(na, o);
        nv += __shfl_xor(nv, o);
    }
    const float prod = na * nv;
    const bool clamped = prod < 1e-16f;
    const float den = sqrtf(fmaxf(prod, 1e-16f));
    const float cs = dot / den;
    // BCE backward (ATen): (p - y) / max((1 - p) * p, 1e-12) * grad / N
    const float dcos = (gout ? gout[0] : 1.f) / (float)N * (cs - y[row]) / fmaxf((1.f - cs) * cs, 1e-12f);
    // cos = dot / sqrt(na*nv):  d/da = v/den - dot * nv * a / den^3   (the second term vanishes under the eps clamp)
    const float k1 = dcos / den;
    const float ka = clamped ? 0.f : dcos * dot * nv / (den * den * den);
    const float kv = clamped ? 0.f : dcos * dot * na / (den * den * den);
    for (int c = lane; c < C; c += 64) {
        da[(long long)row * C + c] = k1 * pv[c] - ka * pa[c];
        dv[(long long)row * C + c] = k1 * pa[c] - kv * pv[c];
    }
}

// y = x / max(|x|, 1e-12):  dx = (dy - y * <y, dy>) / max(|x|, 1e-12)
__global__ void l2norm_bwd_kernel(int N, int C, const float* __restrict__ x, int x_cs, const float* __restrict__ dy,
                                  float* __restrict__ dx, int dx_cs) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* px = x + (long long)row * x_cs;
    const float* pd = dy + (long long)row * C;
    float ss = 0.f, xd = 0.f;
    for (int c = lane; c < C; c += 64) {
        ss += px[c] * px[c];
        xd += px[c] * pd[c];
    }
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_xor(ss, o);
        xd += __shfl_xor(xd, o);
    }
    const float nrm = sqrtf(ss);
    const float d = fmaxf(nrm, 1e-12f);
    const float k = nrm > 1e-12f ? xd / (d * d * d) : 0.f;   // under the clamp the norm is a constant
    for (int c = lane; c < C; c += 64) dx[(long long)row * dx_cs + c] = pd[c] / d - px[c] * k;
}

__global__ void bce_bwd_kernel(int N, const float* __restrict__ p, const float* __restrict__ y,
                               const float* __restrict__ gout, float* __restrict__ dp) {
    const float gsc = (gout ? gout[0] : 1.f) / (float)N;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
        dp[i] = gsc * (p[i] - y[i]) / fmaxf((1.f - p[i]) * p[i], 1e-12f);
}

// ---------------------------------------------------------------- fused multi-tensor Adam
struct AdamChunk {
    int tensor;
    int start;   // element offset of the chunk inside the tensor (chunks are kAdamChunk elements)
};
constexpr int kAdamChunk = 16384;

__global__ __launch_bounds__(256) void adam_kernel(const w2l_adam_tensor* __restrict__ tensors,
                                                   const AdamChunk* __restrict__ chunks, float lr, float beta1,
                                                   float beta2, float eps, float weight_decay, float bc1, float bc2_sqrt) {
    const AdamChunk ch = chunks[blockIdx.x];
    const w2l_adam_tensor tt = tensors[ch.tensor];
    const long long end = (long long)ch.start + kAdamChunk < tt.n ? (long long)ch.start + kAdamChunk : tt.n;
    const float step_size = lr / bc1;
    for (long long i = ch.start + threadIdx.x; i < end; i += blockDim.x) {
        float g = tt.grad[i];
        const float p = tt.param[i];
        if (weight_decay != 0.f) g += weight_decay * p;
        // torch.optim.Adam (single-tensor form): exp_avg.lerp_(grad, 1-beta1); exp_avg_sq = beta2*v + (1-beta2) g^2;
        // denom = sqrt(v)/sqrt(bias_correction2) + eps; p -= (lr/bias_correction1) * m / denom
        const float m = tt.exp_avg[i] + (g - tt.exp_avg[i]) * (1.f - beta1);
        const float v = beta2 * tt.exp_avg_sq[i] + (1.f - beta2) * g * g;
        tt.exp_avg[i] = m;
        tt.exp_avg_sq[i] = v;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        tt.param[i] = p - step_size * (m / denom);
    }
}

}  // namespace w2l

using namespace w2l;

struct w2l_adam {
    int ntensors = 0;
    int nchunks = 0;
    w2l_adam_tensor* tensors_dev = nullptr;
    AdamChunk* chunks_dev = nullptr;
};

extern "C" {

int w2l_l1_mean(void* stream, long long n, const float* a, const float* b, float* loss_out) {
    W2L_REQUIRE(a && b && loss_out && n >= 1, "bad l1_mean arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nb = grid_cap(n, 256 * 16, 1024);
    double* partial = partial_ws(s, (size_t)nb * sizeof(double));
    if (!partial) return W2L_ERR_NOMEM;
    hipLaunchKernelGGL(l1_partial_kernel, dim3(nb), dim3(256), 0, s, n, a, b, partial);
    W2L_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(64), 0, s, nb, partial, 1.0 / (double)n, loss_out);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_l1_bwd(void* stream, long long n, const float* a, const float* b, const float* gout, float* da) {
    W2L_REQUIRE(a && b && da && n >= 1, "bad l1_bwd arguments");
    hipLaunchKernelGGL(l1_bwd_kernel, dim3(grid_cap(n, 256, 16384)), dim3(256), 0, static_cast<hipStream_t>(stream), n, a,
                       b, gout, (float)(1.0 / (double)n), da);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_cosine_bce_bwd(void* stream, int N, int C, const float* a, const float* v, const float* y, const float* gout,
                       float* da, float* dv) {
    W2L_REQUIRE(a && v && y && da && dv && N >= 1 && C >= 1, "bad cosine_bce_bwd arguments");
    hipLaunchKernelGGL(cosine_bce_bwd_kernel, dim3(ceil_div(N, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), N, C, a,
                       v, y, gout, da, dv);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_l2norm_bwd(void* stream, int N, int C, const float* x, int x_cs, const float* dy, float* dx, int dx_cs) {
    W2L_REQUIRE(x && dy && dx && N >= 1 && C >= 1 && x_cs >= C && dx_cs >= C, "bad l2norm_bwd arguments");
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(ceil_div(N, 4)), dim3(256), 0, static_cast<hipStream_t>(stream), N, C, x,
                       x_cs, dy, dx, dx_cs);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_bce_bwd(void* stream, int N, const float* p, const float* y, const float* gout, float* dp) {
    W2L_REQUIRE(p && y && dp && N >= 1, "bad bce_bwd arguments");
    hipLaunchKernelGGL(bce_bwd_kernel, dim3(grid_cap(N, 256, 1024)), dim3(256), 0, static_cast<hipStream_t>(stream), N, p, y,
                       gout, dp);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_adam_create(int ntensors, const long long* sizes_host, w2l_adam_t** out) {
    W2L_REQUIRE(ntensors >= 1 && sizes_host && out, "bad adam_create arguments");
    w2l_adam* h = new (std::nothrow) w2l_adam();
    if (!h) { set_error("out of host memory"); return W2L_ERR_NOMEM; }
    std::vector<AdamChunk> chunks;
    for (int i = 0; i < ntensors; ++i) {
        if (sizes_host[i] < 0 || sizes_host[i] >= (1ll << 31)) { delete h; set_error("adam: tensor %d has %lld elements", i, sizes_host[i]); return W2L_ERR_ARG; }
        for (long long s = 0; s < sizes_host[i]; s += kAdamChunk) chunks.push_back(AdamChunk{i, (int)s});
    }
    h->ntensors = ntensors;
    h->nchunks = (int)chunks.size();
    if (hipMalloc(&h->tensors_dev, sizeof(w2l_adam_tensor) * ntensors) != hipSuccess ||
        hipMalloc(&h->chunks_dev, sizeof(AdamChunk) * (chunks.empty() ? 1 : chunks.size())) != hipSuccess) {
        set_error("hipMalloc(adam tables) failed");
        w2l_adam_destroy(h);
        return W2L_ERR_NOMEM;
    }
    if (!chunks.empty() &&
        hipMemcpy(h->chunks_dev, chunks.data(), sizeof(AdamChunk) * chunks.size(), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("upload of the adam chunk table failed");
        w2l_adam_destroy(h);
        return W2L_ERR_HIP;
    }
    *out = h;
    return W2L_OK;
}

int w2l_adam_destroy(w2l_adam_t* h) {
    if (!h) return W2L_OK;
    if (h->tensors_dev) (void)hipFree(h->tensors_dev);
    if (h->chunks_dev) (void)hipFree(h->chunks_dev);
    delete h;
    return W2L_OK;
}

int w2l_adam_step(w2l_adam_t* h, void* stream, const w2l_adam_tensor* tensors_host, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step) {
    W2L_REQUIRE(h && tensors_host && step >= 1, "bad adam_step arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    W2L_HIP_CHECK(hipMemcpyAsync(h->tensors_dev, tensors_host, sizeof(w2l_adam_tensor) * h->ntensors, hipMemcpyHostToDevice, s));
    if (h->nchunks == 0) return W2L_OK;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adam_kernel, dim3(h->nchunks), dim3(256), 0, s, h->tensors_dev, h->chunks_dev, lr, beta1, beta2, eps,
                       weight_decay, (float)bc1, (float)sqrt(bc2));
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- LSE-style sync scoring (evaluation/scores_LSE)
namespace w2l {
// calc_pdist of evaluation/scores_LSE/SyncNetInstance_calc_scores.py:19-31: f2 is zero-padded by `vshift` rows on both
// sides; out[i][j] = || f1[i] - f2p[i+j] + 1e-6 ||_2 (F.pairwise_distance adds its eps to the difference), j < 2*vshift+1.
// One wave per (i, j).
__global__ void shifted_pdist_kernel(int T, int C, int vshift, const float* __restrict__ f1, const float* __restrict__ f2,
                                     float* __restrict__ out) {
    const int win = 2 * vshift + 1;
    const int item = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (item >= T * win) return;
    const int i = item / win, j = item - i * win;
    const int r = i + j - vshift;                 // row of the unpadded f2
    const bool inside = r >= 0 && r < T;
    const float d = shifted_pdist_wave(f1 + (long long)i * C, f2 + (long long)(inside ? r : 0) * C, inside, C, lane);
    if (lane == 0) out[item] = d;
}
}  // namespace w2l

extern "C" int w2l_shifted_pdist(void* stream, int T, int C, int vshift, const float* f1, const float* f2, float* out) {
    W2L_REQUIRE(f1 && f2 && out && T >= 1 && C >= 1 && vshift >= 0, "bad shifted_pdist arguments");
    const int items = T * (2 * vshift + 1);
    hipLaunchKernelGGL(w2l::shifted_pdist_kernel, dim3(w2l::ceil_div(items, 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       T, C, vshift, f1, f2, out);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}
