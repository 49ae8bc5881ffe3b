// Filelist scoring (evaluation/scores_LSE/calculate_scores_LRS.py:28-50 over SyncNetInstance_calc_scores.py:19-31,105-137) with
// the windows of many clips in shared SyncNet batches: the kernel that builds a batch's two network inputs from a row table (fp32,
// or bf16 for the bf16-storage plan), the kernel that normalises that plan's two bf16 outputs into the fp32 embedding arenas, and
// the kernel that turns the embeddings of a group of clips into one score row per clip.
#include <math.h>

#include "w2l_common.h"

namespace w2l {

struct SyncRow {                 // w2l_sync_row
    unsigned long long frames;   // u8 [5][S][S][3]
    unsigned long long mel;      // fp32 [80][T]
    int T, start;
    int pad[2];
};
static_assert(sizeof(SyncRow) == 32, "w2l_sync_row is 32 bytes");

struct Segment {                 // w2l_lse_segment
    int row0, n;
};
static_assert(sizeof(Segment) == 8, "w2l_lse_segment is 8 bytes");

constexpr int kSyncT = 5;        // frames per window (hparams.syncnet_T)
constexpr int kSyncMels = 80;
constexpr int kSyncCols = 16;    // mel columns per window (syncnet_mel_step_size)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Row b of both SyncNet inputs.  A face item is 4 neighbouring pixels of one output line: per frame t the 12 bytes are three
// dwords of the frame line when the address allows it (bytes otherwise, and at a ragged line end), each byte is read once, and
// the item writes its pixels' channels 0 .. face_cs-1 whole.  A mel item is one (mel row, column).  T = float, or __bf16 for the
// bf16-storage plan: the fp32 value rounded once (RNE), 8 channels (16 bytes) per store
template <typename T>
__global__ __launch_bounds__(256) void sync_window_rows_kernel(const SyncRow* __restrict__ rows, int S, T* __restrict__ face_in,
                                                               int face_cs, T* __restrict__ mel_in, int mel_cs) {
    const int b = blockIdx.y;
    const SyncRow r = rows[b];
    const int Ho = S >> 1, groups = (S + 3) >> 2;
    const int nface = Ho * groups;
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item < nface) {
        const int y = item / groups, x0 = (item - y * groups) * 4;
        const int np = S - x0 < 4 ? S - x0 : 4;
        const uint8_t* frames = reinterpret_cast<const uint8_t*>(r.frames);
        float v[4][3 * kSyncT + 1];
#pragma unroll
        for (int t = 0; t < kSyncT; ++t) {
            const uint8_t* p = frames + (((size_t)t * S + (Ho + y)) * S + x0) * 3;
            uint32_t w[3] = {0u, 0u, 0u};
            if (np == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
                w[0] = q[0];
                w[1] = q[1];
                w[2] = q[2];
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k)
                    if (k < np * 3) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
            }
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k / 3][3 * t + k % 3] = (float)((w[k >> 2] >> (8 * (k & 3))) & 255u) / 255.f;
        }
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            if (px >= np) break;
            v[px][3 * kSyncT] = 0.f;
            T* op = face_in + (((size_t)b * Ho + y) * S + x0 + px) * face_cs;
            if constexpr (sizeof(T) == 2) {
                bf16x8* o = reinterpret_cast<bf16x8*>(op);
                bf16x8 zero;
#pragma unroll
                for (int c = 0; c < 8; ++c) zero[c] = (__bf16)0.f;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    bf16x8 h;
#pragma unroll
                    for (int c = 0; c < 8; ++c) h[c] = (__bf16)v[px][8 * q + c];
                    o[q] = h;
                }
                for (int q = 2; q < (face_cs >> 3); ++q) o[q] = zero;
            } else {
                const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
                float4* o = reinterpret_cast<float4*>(op);
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = make_float4(v[px][4 * q], v[px][4 * q + 1], v[px][4 * q + 2], v[px][4 * q + 3]);
                for (int q = 4; q < (face_cs >> 2); ++q) o[q] = zero;
            }
        }
        return;
    }
    const int m = item - nface;
    if (m >= kSyncMels * kSyncCols) return;
    const int s = r.start + (m & (kSyncCols - 1));
    const float* mel = reinterpret_cast<const float*>(r.mel);
    const float val = (s >= 0 && s < r.T) ? mel[(long long)(m >> 4) * r.T + s] : 0.f;
    T* op = mel_in + ((size_t)b * kSyncMels * kSyncCols + m) * mel_cs;
    if constexpr (sizeof(T) == 2) {
        bf16x8* o = reinterpret_cast<bf16x8*>(op);
        bf16x8 h;
#pragma unroll
        for (int c = 0; c < 8; ++c) h[c] = (__bf16)0.f;
        for (int q = 1; q < (mel_cs >> 3); ++q) o[q] = h;
        h[0] = (__bf16)val;
        o[0] = h;
    } else {
        float4* o = reinterpret_cast<float4*>(op);
        o[0] = make_float4(val, 0.f, 0.f, 0.f);
        for (int q = 1; q < (mel_cs >> 2); ++q) o[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// The tail of the bf16-storage SyncNet plan: F.normalize(p=2, dim=1) of both encoders' outputs in one launch.  blockIdx.y picks the
// encoder, one wave per row; a lane reads 8 channels (16 bytes) at a time, the sum of squares is fp32 (a bf16 square is exact in
// fp32), and y = x / max(sqrt(sum), 1e-12) goes out as two float4 per 8 channels.  Channels C .. cs-1 are never read.
__global__ __launch_bounds__(256) void sync_embeddings_bf16_kernel(int B, int C, const __bf16* __restrict__ audio_x, int audio_cs,
                                                                   const __bf16* __restrict__ face_x, int face_cs,
                                                                   float* __restrict__ audio_out, float* __restrict__ face_out) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    const bool face = blockIdx.y != 0;
    const __bf16* p = face ? face_x + (size_t)row * face_cs : audio_x + (size_t)row * audio_cs;
    float* y = (face ? face_out : audio_out) + (size_t)row * C;
    float s = 0.f;
    for (int c = lane * 8; c < C; c += 512) {
        const bf16x8 h = *reinterpret_cast<const bf16x8*>(p + c);
#pragma unroll
        for (int k = 0; k < 8; ++k) s += (float)h[k] * (float)h[k];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float d = fmaxf(sqrtf(s), 1e-12f);
    for (int c = lane * 8; c < C; c += 512) {
        const bf16x8 h = *reinterpret_cast<const bf16x8*>(p + c);
        float4* o = reinterpret_cast<float4*>(y + c);
        o[0] = make_float4((float)h[0] / d, (float)h[1] / d, (float)h[2] / d, (float)h[3] / d);
        o[1] = make_float4((float)h[4] / d, (float)h[5] / d, (float)h[6] / d, (float)h[7] / d);
    }
}

// order of the selection below: NaN before every number (torch.min returns the first NaN, and conf = median - NaN is NaN as
// torch.median's), then by value, equal values by index
__device__ __forceinline__ bool score_before(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a < b || (a == b && ia < ib);
}

constexpr int kScoreWaves = 16;

// One workgroup per segment (clip).  Rows i0 .. i0+15 of the distance table are computed side by side, one wave per row, into LDS;
// thread j then adds them to column j's fp64 sum in row order, so the order of every sum is fixed.  mdist[j] = sum / n rounded to
// fp32 once.  Then every thread j < win ranks its value among the win values: rank 0 is the minimum at its lowest index, rank
// (win-1)/2 the lower median.
__global__ __launch_bounds__(1024) void lse_score_segments_kernel(const Segment* __restrict__ segs, int C, int vshift,
                                                                  const float* __restrict__ f1, const float* __restrict__ f2,
                                                                  float* __restrict__ mdist, float* __restrict__ scores) {
    __shared__ float d[kScoreWaves][256];
    __shared__ float m[256];
    __shared__ float s_min;
    const int win = 2 * vshift + 1;
    const Segment sg = segs[blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float* md = mdist + (long long)blockIdx.x * win;
    float* sc = scores + (long long)blockIdx.x * 4;
    if (sg.n < 1) {                                    // an empty segment owns no row: nothing is read
        if (tid < win) md[tid] = NAN;
        if (tid < 4) sc[tid] = tid == 3 ? 0.f : NAN;
        return;
    }
    const float* a0 = f1 + (long long)sg.row0 * C;
    const float* b0 = f2 + (long long)sg.row0 * C;
    double acc = 0.0;
    for (int i0 = 0; i0 < sg.n; i0 += kScoreWaves) {
        const int i = i0 + wave;
        if (i < sg.n) {
            for (int j = 0; j < win; ++j) {
                const int r = i + j - vshift;          // row of the segment's own unpadded f2
                const bool inside = r >= 0 && r < sg.n;
                const float v = shifted_pdist_wave(a0 + (long long)i * C, b0 + (long long)(inside ? r : 0) * C, inside, C, lane);
                if (lane == 0) d[wave][j] = v;
            }
        }
        __syncthreads();
        if (tid < win) {
            const int cnt = sg.n - i0 < kScoreWaves ? sg.n - i0 : kScoreWaves;
            for (int w = 0; w < cnt; ++w) acc += (double)d[w][tid];
        }
        __syncthreads();
    }
    float mine = 0.f;
    if (tid < win) {
        mine = (float)(acc / (double)sg.n);
        m[tid] = mine;
        md[tid] = mine;
    }
    __syncthreads();
    int rank = -1;
    if (tid < win) {
        rank = 0;
        for (int k = 0; k < win; ++k) rank += score_before(m[k], k, mine, tid) ? 1 : 0;
        if (rank == 0) {
            s_min = mine;
            sc[0] = mine;
            sc[2] = (float)(vshift - tid);
            sc[3] = (float)sg.n;
        }
    }
    __syncthreads();
    if (rank == (win - 1) / 2) sc[1] = mine - s_min;
}

}  // namespace w2l

using namespace w2l;

template <typename T>
static int sync_window_rows_t(void* stream, int B, const w2l_sync_row* rows, int S, T* face_in, int face_cs, T* mel_in, int mel_cs,
                              const char* name) {
    constexpr int VEC = 16 / (int)sizeof(T);      // channels of one 16-byte store
    W2L_REQUIRE(rows && face_in && mel_in && S >= 2 && S <= 4096, "bad %s arguments", name);
    W2L_REQUIRE(B >= 1 && B <= 65535 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                "%s: 1 <= B <= 65535 and a 16-byte aligned row table", name);
    W2L_REQUIRE(face_cs >= 16 && face_cs % VEC == 0 && mel_cs >= VEC && mel_cs % VEC == 0,
                "%s: face_cs=%d (>= 16) and mel_cs=%d (>= %d) must be multiples of %d", name, face_cs, mel_cs, VEC, VEC);
    W2L_REQUIRE(((reinterpret_cast<uintptr_t>(face_in) | reinterpret_cast<uintptr_t>(mel_in)) & 15) == 0, "%s: 16-byte aligned outputs",
                name);
    const int items = (S / 2) * ((S + 3) / 4) + kSyncMels * kSyncCols;
    hipLaunchKernelGGL(sync_window_rows_kernel<T>, dim3(ceil_div(items, 256), B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const SyncRow*>(rows), S, face_in, face_cs, mel_in, mel_cs);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

extern "C" {

int w2l_sync_window_rows(void* stream, int B, const w2l_sync_row* rows, int S, float* face_in, int face_cs, float* mel_in, int mel_cs) {
    return sync_window_rows_t<float>(stream, B, rows, S, face_in, face_cs, mel_in, mel_cs, "sync_window_rows");
}

int w2l_sync_window_rows_bf16(void* stream, int B, const w2l_sync_row* rows, int S, void* face_in, int face_cs, void* mel_in,
                              int mel_cs) {
    return sync_window_rows_t<__bf16>(stream, B, rows, S, static_cast<__bf16*>(face_in), face_cs, static_cast<__bf16*>(mel_in), mel_cs,
                                      "sync_window_rows_bf16");
}

int w2l_sync_embeddings_bf16(void* stream, int B, int C, const void* audio_x, int audio_cs, const void* face_x, int face_cs,
                             float* audio_out, float* face_out) {
    W2L_REQUIRE(audio_x && face_x && audio_out && face_out && B >= 1 && C >= 8, "bad sync_embeddings_bf16 arguments");
    W2L_REQUIRE(C % 8 == 0 && audio_cs >= C && face_cs >= C && audio_cs % 8 == 0 && face_cs % 8 == 0,
                "sync_embeddings_bf16: C=%d and the strides %d, %d (>= C) must be multiples of 8", C, audio_cs, face_cs);
    W2L_REQUIRE(((reinterpret_cast<uintptr_t>(audio_x) | reinterpret_cast<uintptr_t>(face_x) | reinterpret_cast<uintptr_t>(audio_out) |
                  reinterpret_cast<uintptr_t>(face_out)) & 15) == 0,
                "sync_embeddings_bf16: 16-byte aligned inputs and outputs");
    hipLaunchKernelGGL(sync_embeddings_bf16_kernel, dim3(ceil_div(B, 4), 2), dim3(256), 0, static_cast<hipStream_t>(stream), B, C,
                       static_cast<const __bf16*>(audio_x), audio_cs, static_cast<const __bf16*>(face_x), face_cs, audio_out,
                       face_out);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_lse_score_segments(void* stream, int n_seg, const w2l_lse_segment* segs, int C, int vshift, const float* face_emb,
                           const float* audio_emb, float* mdist, float* scores) {
    W2L_REQUIRE(segs && face_emb && audio_emb && mdist && scores, "bad lse_score_segments arguments");
    W2L_REQUIRE(n_seg >= 1 && C >= 1 && vshift >= 0 && vshift <= 127,
                "lse_score_segments: n=%d >= 1, C=%d >= 1 and 0 <= vshift=%d <= 127", n_seg, C, vshift);
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(segs) & 7) == 0, "lse_score_segments: 8-byte aligned segment table");
    hipLaunchKernelGGL(lse_score_segments_kernel, dim3(n_seg), dim3(64 * kScoreWaves), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const Segment*>(segs), C, vshift, face_emb, audio_emb, mdist, scores);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"
