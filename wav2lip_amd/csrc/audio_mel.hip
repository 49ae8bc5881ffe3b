// audio.melspectrogram on gfx950: one workgroup per STFT frame, everything fused:
//   pre-emphasis (f64) -> reflect pad -> periodic-Hann window (f64) -> 800-point real DFT (f64, direct, twiddle
//   table in LDS) -> cast to complex64 -> |.| (f32) -> 80-bin Slaney mel (f32) -> 20*log10(max(1e-5,.)) - 20
//   -> clip(8*((S+100)/100) - 4, -4, 4).
// Follows audio.py:45-51 (melspectrogram), :20-23 (preemphasis = scipy lfilter([1,-k],[1])), :57-61 (_stft =
// librosa.stft(n_fft=800, hop=200, win=800): center=True, reflect pad, f64 FFT stored as complex64), :92-105,
// :110-116 of the reference with hparams.py:32-69.  The numerics mirror oracle/audio_ref.py step by step.
// HBM-bound in principle (200 new samples in, 80 floats out per frame); at clip lengths the launch is latency-bound.
#include <math.h>

#include <new>
#include <vector>

#include "w2l_common.h"

namespace w2l {

constexpr int kNfft = 800;
constexpr int kHop = 200;
constexpr int kBins = kNfft / 2 + 1;  // 401
constexpr int kMels = 80;
constexpr double kPreemph = 0.97;

struct MelKArgs {
    const float* wav;
    long long nsamples;
    const float* basis;    // [80][401]
    const double* window;  // [800]
    const double2* twiddle;  // [800] (cos, sin)(2*pi*j/800)
    float* mel;            // [80][T]
    int T;
};

// One spectrogram column, shared by the whole-waveform kernel and the many-stream kernel: `src(j)` is sample j of the signal
// (j already reflected into it) as a double; everything from the pre-emphasis on is this one body, so the two kernels agree bit
// for bit.  out[m * out_stride] receives mel bin m of column t.
template <typename Src>
__device__ __forceinline__ double preemph_sample(const Src& src, long long j) {
    // scipy lfilter (direct form II transposed), b = [1, -k]: y[n] = x[n] + (-k * x[n-1]), products and sums
    // rounded separately in f64 (no fused multiply-add)
    const double x0 = src(j);
    if (j == 0) return x0;
    return __dadd_rn(x0, __dmul_rn(-kPreemph, src(j - 1)));
}

template <typename Src>
__device__ __forceinline__ void mel_column(const Src& src, long long t, long long nsamples, const float* __restrict__ basis,
                                           const double* __restrict__ window, const double2* __restrict__ twiddle,
                                           float* __restrict__ out, long long out_stride) {
    __shared__ double s_frame[kNfft];
    __shared__ double2 s_tw[kNfft];
    __shared__ float s_mag[kBins + 3];
    const int tid = threadIdx.x;
    const long long pad = kNfft / 2;

    for (int n = tid; n < kNfft; n += 256) {
        long long j = t * kHop + n - pad;
        if (j < 0) j = -j;                                   // np.pad(mode='reflect'): no edge repeat
        if (nsamples >= 0 && j >= nsamples) j = 2 * (nsamples - 1) - j;   // nsamples < 0: the end is not known yet (open stream)
        s_frame[n] = __dmul_rn(window[n], preemph_sample(src, j));
        s_tw[n] = twiddle[n];
    }
    __syncthreads();

    for (int k = tid; k < kBins; k += 256) {
        double re = 0.0, im = 0.0;
        int idx = 0;  // (k*n) mod 800
        for (int n = 0; n < kNfft; ++n) {
            const double2 w = s_tw[idx];
            const double v = s_frame[n];
            re = fma(v, w.x, re);
            im = fma(-v, w.y, im);
            idx += k;
            if (idx >= kNfft) idx -= kNfft;
        }
        // complex64 storage, then np.abs in f32
        s_mag[k] = hypotf((float)re, (float)im);
    }
    __syncthreads();

    if (tid < kMels) {
        const float* b = basis + tid * kBins;
        float acc = 0.f;
        for (int k = 0; k < kBins; ++k) acc = fmaf(b[k], s_mag[k], acc);
        // _amp_to_db: min_level = exp(-100/20*ln 10) = 1e-5 ; 20*log10(max(min_level, x)) ; then - ref_level_db (20)
        const float min_level = 1e-5f;
        float S = 20.0f * log10f(fmaxf(min_level, acc)) - 20.0f;
        // _normalize, symmetric + clipping: clip(2*4*((S+100)/100) - 4, -4, 4)
        float v = 8.0f * ((S + 100.0f) / 100.0f) - 4.0f;
        v = fminf(fmaxf(v, -4.0f), 4.0f);
        out[(long long)tid * out_stride] = v;
    }
}

struct WavSrc {
    const float* wav;
    __device__ __forceinline__ double operator()(long long j) const { return (double)wav[j]; }
};

__global__ __launch_bounds__(256) void mel_frame_kernel(const MelKArgs a) {
    const int t = blockIdx.x;
    mel_column(WavSrc{a.wav}, (long long)t, a.nsamples, a.basis, a.window, a.twiddle, a.mel + t, (long long)a.T);
}

// The newly final columns of MANY streams in one launch (w2l_mel_stream / w2l_mel_col, include/w2l_hip.h): one workgroup per
// (stream, column) entry.  A stream holds only the samples [first, first + held) of its signal; the host checks that they cover
// what the listed columns read, and the kernel clamps every index into the held range, so that a wrong table gives wrong
// numbers and not a fault.  Entries that name no stream, hold no samples or fall outside the window write nothing.
struct MelStream {
    unsigned long long samples;
    long long first, total;
    unsigned long long window;
    int held, cap;
    long long col0;
};
struct MelCol {
    int stream, rsv;
    long long col;
};
static_assert(sizeof(MelStream) == 48 && sizeof(MelCol) == 16, "w2l_mel_stream is 48 bytes, w2l_mel_col 16");

struct StreamSrc {
    const float* samples;
    long long first;
    int held;
    __device__ __forceinline__ double operator()(long long j) const {
        long long i = j - first;
        i = i < 0 ? 0 : (i >= held ? held - 1 : i);
        return (double)samples[i];
    }
};

struct MelStreamKArgs {
    const MelStream* streams;
    int nstreams;
    const MelCol* cols;
    const float* basis;
    const double* window;
    const double2* twiddle;
};

__global__ __launch_bounds__(256) void mel_stream_cols_kernel(const MelStreamKArgs a) {
    const MelCol c = a.cols[blockIdx.x];
    if (c.stream < 0 || c.stream >= a.nstreams) return;      // uniform over the workgroup: no barrier is skipped by a part of it
    const MelStream s = a.streams[c.stream];
    const long long rel = c.col - s.col0;
    if (s.held < 1 || !s.samples || !s.window || c.col < 0 || rel < 0 || rel >= s.cap) return;
    mel_column(StreamSrc{reinterpret_cast<const float*>(s.samples), s.first, s.held}, c.col, s.total, a.basis, a.window,
               a.twiddle, reinterpret_cast<float*>(s.window) + rel, (long long)s.cap);
}

// T = float, or __bf16 (the bf16-storage inference path: each value rounded once, RNE)
template <typename T>
__global__ void mel_gather_kernel(const float* __restrict__ mel, int T_, const int* __restrict__ starts, int B,
                                  T* __restrict__ out, int out_cs, int c_zero_to) {
    const long long total = (long long)B * kMels * 16;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 15);
        const int m = (int)((i >> 4) % kMels);
        const int b = (int)(i / (16 * kMels));
        const int s = starts[b] + j;
        T* o = out + i * out_cs;
        o[0] = (T)((s >= 0 && s < T_) ? mel[(long long)m * T_ + s] : 0.f);
        for (int c = 1; c < c_zero_to; ++c) o[c] = (T)0.f;
    }
}

// mel_gather_kernel with one spectrogram per row (w2l_mel_row: rows of different clips share a batch)
struct MelRow {
    unsigned long long mel;
    int T, start;
};
static_assert(sizeof(MelRow) == 16, "w2l_mel_row is 16 bytes");

template <typename T>
__global__ void mel_gather_rows_kernel(const MelRow* __restrict__ rows, int B, T* __restrict__ out, int out_cs, int c_zero_to) {
    const long long total = (long long)B * kMels * 16;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 15);
        const int m = (int)((i >> 4) % kMels);
        const int b = (int)(i / (16 * kMels));
        const MelRow r = rows[b];
        const float* mel = reinterpret_cast<const float*>(r.mel);
        const int s = r.start + j;
        T* o = out + i * out_cs;
        o[0] = (T)((s >= 0 && s < r.T) ? mel[(long long)m * r.T + s] : 0.f);
        for (int c = 1; c < c_zero_to; ++c) o[c] = (T)0.f;
    }
}

}  // namespace w2l

using namespace w2l;

struct w2l_mel {
    float* basis = nullptr;
    double* window = nullptr;
    double2* twiddle = nullptr;
};

// ---------------------------------------------------------------- sample-rate conversion (audio.py:9-10 -> librosa.load)
// resampy's band-limited sinc interpolation (resample_f): one thread per output sample walks the left wing (x[n], x[n-1], ...)
// and then the right wing (x[n+1], ...) of the Kaiser-windowed sinc, in that order, rounding the float32 accumulator after
// every term exactly as the reference's numba loop does (y is float32, the weights float64).  __dmul_rn / __dadd_rn keep the
// compiler from contracting the products into FMAs (numpy rounds the product, then the sum).
struct ResampleKArgs {
    const float* x;
    const double* tr;     // time register of every output sample (host: repeated float64 addition)
    const double* win;    // half window [nwin] (already scaled by the ratio when downsampling)
    const double* delta;  // its first differences, last entry 0
    float* y;
    int n_in, n_out, nwin, num_table, index_step;
    double scale;
};

__global__ void resample_sinc_kernel(const ResampleKArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_out) return;
    const double time_register = a.tr[t];
    const int n = (int)time_register;
    float acc = 0.f;
    double frac = __dmul_rn(a.scale, time_register - (double)n);
    double index_frac = __dmul_rn(frac, (double)a.num_table);
    int offset = (int)index_frac;
    double eta = index_frac - (double)offset;
    const int i_max = min(n + 1, (a.nwin - offset) / a.index_step);
    for (int i = 0; i < i_max; ++i) {
        const int idx = offset + i * a.index_step;
        const double w = __dadd_rn(a.win[idx], __dmul_rn(eta, a.delta[idx]));
        acc = (float)__dadd_rn((double)acc, __dmul_rn(w, (double)a.x[n - i]));
    }
    frac = a.scale - frac;
    index_frac = __dmul_rn(frac, (double)a.num_table);
    offset = (int)index_frac;
    eta = index_frac - (double)offset;
    const int k_max = min(a.n_in - n - 1, (a.nwin - offset) / a.index_step);
    for (int k = 0; k < k_max; ++k) {
        const int idx = offset + k * a.index_step;
        const double w = __dadd_rn(a.win[idx], __dmul_rn(eta, a.delta[idx]));
        acc = (float)__dadd_rn((double)acc, __dmul_rn(w, (double)a.x[n + k + 1]));
    }
    a.y[t] = acc;
}

// The same interpolation, incrementally and for MANY streams of any source rates in one launch (w2l_resample_stream_entry /
// w2l_resample_block, include/w2l_hip.h; wav2lip_amd/streaming.py): one workgroup per block entry, one thread per output sample.
// A stream holds only the source samples [src_first, src_first + src_held) of its signal.  An output is FINAL - equal to the same
// output of the whole signal - once its right wing is no longer cut by the end of the data; the host lists final outputs only
// and checks that the held samples cover what they read.  The kernel does not clamp a read: an output whose wings leave the held
// range, an entry that names no stream and an output outside the destination are skipped, so that a wrong table writes nothing.
// The time register of a block's first output comes from the host (repeated float64 addition); thread j adds the increment j
// more times with __dadd_rn: the additions of the reference loop, in its order.
struct ResampleStream {
    unsigned long long src;
    long long src_first, src_total, n_res;
    unsigned long long dst;
    long long dst_first;
    unsigned long long win, delta, carry;
    long long carry_first;
    double scale, inc;
    int src_held, dst_cap, index_step, nwin, carry_held, rsv[3];
};
struct ResampleBlock {
    int stream, count;
    long long t0;
    double tr0;
    int copy, rsv;
};
static_assert(sizeof(ResampleStream) == 128 && sizeof(ResampleBlock) == 32, "w2l_resample_stream_entry is 128 bytes, w2l_resample_block 32");
constexpr int kResampleBlock = 128;

struct ResampleStreamKArgs {
    const ResampleStream* streams;
    int nstreams;
    const ResampleBlock* blocks;
    int num_table;
};

__global__ __launch_bounds__(kResampleBlock) void resample_stream_kernel(const ResampleStreamKArgs a) {
    const ResampleBlock b = a.blocks[blockIdx.x];
    const int j = threadIdx.x;
    if (b.stream < 0 || b.stream >= a.nstreams || j >= b.count || b.count > kResampleBlock || b.t0 < 0) return;
    const ResampleStream s = a.streams[b.stream];
    const long long t = b.t0 + j;
    const long long rel = t - s.dst_first;
    if (!s.dst || rel < 0 || rel >= s.dst_cap) return;
    float* y = reinterpret_cast<float*>(s.dst) + rel;
    if (b.copy) {                                  // the tail of the stream's previous buffer, carried into the fresh one
        const long long c = t - s.carry_first;
        if (s.carry && c >= 0 && c < s.carry_held) *y = reinterpret_cast<const float*>(s.carry)[c];
        return;
    }
    if (s.n_res >= 0 && t >= s.n_res) {            // librosa's fix_length: the padded zero behind resampy's last output
        *y = 0.f;
        return;
    }
    if (!s.src || !s.win || !s.delta || s.index_step < 1 || s.src_held < 1) return;
    double time_register = b.tr0;
    for (int i = 0; i < j; ++i) time_register = __dadd_rn(time_register, s.inc);
    const long long n = (long long)time_register;
    const double* win = reinterpret_cast<const double*>(s.win);
    const double* delta = reinterpret_cast<const double*>(s.delta);
    double frac = __dmul_rn(s.scale, time_register - (double)n);
    double index_frac = __dmul_rn(frac, (double)a.num_table);
    int offset = (int)index_frac;
    double eta = index_frac - (double)offset;
    const long long i_max = min(n + 1, (long long)((s.nwin - offset) / s.index_step));
    frac = s.scale - frac;
    const double index_frac_r = __dmul_rn(frac, (double)a.num_table);
    const int offset_r = (int)index_frac_r;
    long long k_max = (s.nwin - offset_r) / s.index_step;
    if (s.src_total >= 0) k_max = min(s.src_total - n - 1, k_max);
    // what the two wings read: x[n - i_max + 1 .. n] and x[n + 1 .. n + k_max], all of it inside the held samples or nothing
    const long long lo = n - (i_max > 0 ? i_max - 1 : 0), hi = n + (k_max > 0 ? k_max : 0);
    if (n < 0 || offset < 0 || offset_r < 0 || lo < s.src_first || hi >= s.src_first + s.src_held) return;
    const float* x = reinterpret_cast<const float*>(s.src) + (n - s.src_first);
    float acc = 0.f;
    for (long long i = 0; i < i_max; ++i) {
        const int idx = offset + (int)i * s.index_step;
        const double w = __dadd_rn(win[idx], __dmul_rn(eta, delta[idx]));
        acc = (float)__dadd_rn((double)acc, __dmul_rn(w, (double)x[-i]));
    }
    eta = index_frac_r - (double)offset_r;
    for (long long k = 0; k < k_max; ++k) {
        const int idx = offset_r + (int)k * s.index_step;
        const double w = __dadd_rn(win[idx], __dmul_rn(eta, delta[idx]));
        acc = (float)__dadd_rn((double)acc, __dmul_rn(w, (double)x[k + 1]));
    }
    *y = acc;
}

extern "C" {

int w2l_mel_num_frames(long long nsamples) { return (int)(1 + nsamples / kHop); }

int w2l_mel_create(const float* mel_basis_host, const double* window_host, w2l_mel_t** out) {
    W2L_REQUIRE(mel_basis_host && window_host && out, "NULL argument");
    w2l_mel* m = new (std::nothrow) w2l_mel();
    if (!m) { set_error("out of host memory"); return W2L_ERR_NOMEM; }
    std::vector<double2> tw(kNfft);
    for (int j = 0; j < kNfft; ++j) {
        const double ang = 2.0 * M_PI * (double)j / (double)kNfft;
        tw[j].x = cos(ang);
        tw[j].y = sin(ang);
    }
    int rc = W2L_OK;
    if (hipMalloc(&m->basis, sizeof(float) * kMels * kBins) != hipSuccess ||
        hipMalloc(&m->window, sizeof(double) * kNfft) != hipSuccess ||
        hipMalloc(&m->twiddle, sizeof(double2) * kNfft) != hipSuccess) {
        set_error("hipMalloc failed in w2l_mel_create");
        rc = W2L_ERR_NOMEM;
    } else if (hipMemcpy(m->basis, mel_basis_host, sizeof(float) * kMels * kBins, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(m->window, window_host, sizeof(double) * kNfft, hipMemcpyHostToDevice) != hipSuccess ||
               hipMemcpy(m->twiddle, tw.data(), sizeof(double2) * kNfft, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("hipMemcpy failed in w2l_mel_create");
        rc = W2L_ERR_HIP;
    }
    if (rc != W2L_OK) { w2l_mel_destroy(m); return rc; }
    *out = m;
    return W2L_OK;
}

int w2l_mel_destroy(w2l_mel_t* m) {
    if (!m) return W2L_OK;
    if (m->basis) (void)hipFree(m->basis);
    if (m->window) (void)hipFree(m->window);
    if (m->twiddle) (void)hipFree(m->twiddle);
    delete m;
    return W2L_OK;
}

int w2l_melspectrogram(const w2l_mel_t* m, void* stream, const float* wav, long long nsamples, float* mel) {
    W2L_REQUIRE(m && wav && mel, "NULL argument");
    W2L_REQUIRE(nsamples > kNfft / 2, "need more than %d samples for reflect padding (got %lld)", kNfft / 2, nsamples);
    MelKArgs a;
    a.wav = wav; a.nsamples = nsamples; a.basis = m->basis; a.window = m->window; a.twiddle = m->twiddle;
    a.mel = mel; a.T = w2l_mel_num_frames(nsamples);
    hipLaunchKernelGGL(mel_frame_kernel, dim3(a.T), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_mel_stream_cols(const w2l_mel_t* m, void* stream, const w2l_mel_stream* streams, int nstreams, const w2l_mel_col* cols,
                        int ncols) {
    W2L_REQUIRE(m && streams && cols, "NULL argument");
    W2L_REQUIRE(nstreams >= 1 && nstreams <= 65535 && ncols >= 1 && ncols <= (1 << 20),
                "mel_stream_cols: 1 <= nstreams <= 65535 and 1 <= ncols <= 1048576 (got %d, %d)", nstreams, ncols);
    W2L_REQUIRE(((reinterpret_cast<uintptr_t>(streams) | reinterpret_cast<uintptr_t>(cols)) & 15) == 0,
                "mel_stream_cols: 16-byte aligned stream and column tables");
    MelStreamKArgs a;
    a.streams = reinterpret_cast<const MelStream*>(streams); a.nstreams = nstreams;
    a.cols = reinterpret_cast<const MelCol*>(cols);
    a.basis = m->basis; a.window = m->window; a.twiddle = m->twiddle;
    hipLaunchKernelGGL(mel_stream_cols_kernel, dim3((unsigned)ncols), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"

namespace w2l {
template <typename T_>
static int mel_gather_t(void* stream, const float* mel, int T, const int32_t* starts, int B, T_* out, int out_cs, int c_zero_to) {
    W2L_REQUIRE(mel && starts && out && T >= 16 && B >= 1, "bad mel_gather arguments");
    if (c_zero_to < 1) c_zero_to = 1;
    W2L_REQUIRE(out_cs >= c_zero_to, "mel_gather: out_cs=%d < c_zero_to=%d", out_cs, c_zero_to);
    const long long total = (long long)B * kMels * 16;
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(mel_gather_kernel<T_>, dim3((unsigned)g), dim3(256), 0, static_cast<hipStream_t>(stream), mel, T,
                       starts, B, out, out_cs, c_zero_to);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}
template <typename T_>
static int mel_gather_rows_t(void* stream, const w2l_mel_row* rows, int B, T_* out, int out_cs, int c_zero_to) {
    W2L_REQUIRE(rows && out, "bad mel_gather_rows arguments");
    W2L_REQUIRE(B >= 1 && B <= 65535 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0,
                "mel_gather_rows: 1 <= B <= 65535 and a 16-byte aligned row table");
    if (c_zero_to < 1) c_zero_to = 1;
    W2L_REQUIRE(out_cs >= c_zero_to, "mel_gather_rows: out_cs=%d < c_zero_to=%d", out_cs, c_zero_to);
    const long long total = (long long)B * kMels * 16;
    long long g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(mel_gather_rows_kernel<T_>, dim3((unsigned)g), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const MelRow*>(rows), B, out, out_cs, c_zero_to);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}
}  // namespace w2l

extern "C" {

int w2l_mel_gather_rows(void* stream, const w2l_mel_row* rows, int B, float* out, int out_cs, int c_zero_to) {
    return mel_gather_rows_t<float>(stream, rows, B, out, out_cs, c_zero_to);
}

int w2l_mel_gather_rows_bf16(void* stream, const w2l_mel_row* rows, int B, void* out, int out_cs, int c_zero_to) {
    return mel_gather_rows_t<__bf16>(stream, rows, B, static_cast<__bf16*>(out), out_cs, c_zero_to);
}

int w2l_mel_gather(void* stream, const float* mel, int T, const int32_t* starts, int B, float* out, int out_cs,
                   int c_zero_to) {
    return mel_gather_t<float>(stream, mel, T, starts, B, out, out_cs, c_zero_to);
}

int w2l_mel_gather_bf16(void* stream, const float* mel, int T, const int32_t* starts, int B, void* out, int out_cs,
                        int c_zero_to) {
    return mel_gather_t<__bf16>(stream, mel, T, starts, B, static_cast<__bf16*>(out), out_cs, c_zero_to);
}

int w2l_resample_sinc(void* stream, const float* x, int n_in, const double* tr, int n_out, double sample_ratio,
                      const double* win, const double* delta, int nwin, int num_table, float* y) {
    W2L_REQUIRE(x && tr && win && delta && y, "NULL argument");
    W2L_REQUIRE(n_in >= 1 && n_out >= 1 && nwin >= 2 && num_table >= 1 && sample_ratio > 0.0, "bad resample arguments");
    ResampleKArgs a;
    a.x = x; a.tr = tr; a.win = win; a.delta = delta; a.y = y;
    a.n_in = n_in; a.n_out = n_out; a.nwin = nwin; a.num_table = num_table;
    a.scale = sample_ratio < 1.0 ? sample_ratio : 1.0;
    a.index_step = (int)(a.scale * num_table);
    W2L_REQUIRE(a.index_step >= 1, "sample ratio %g too small for a table of %d samples per zero crossing", sample_ratio, num_table);
    hipLaunchKernelGGL(resample_sinc_kernel, dim3((unsigned)((n_out + 127) / 128)), dim3(128), 0, static_cast<hipStream_t>(stream), a);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_resample_stream(void* stream, const w2l_resample_stream_entry* streams_host, const w2l_resample_stream_entry* streams,
                        int nstreams, const w2l_resample_block* blocks, int nblocks, int num_table) {
    W2L_REQUIRE(streams_host && streams && blocks, "resample_stream: NULL argument");
    W2L_REQUIRE(nstreams >= 1 && nstreams <= 65535 && nblocks >= 1 && nblocks <= (1 << 20) && num_table >= 1,
                "resample_stream: 1 <= nstreams <= 65535, 1 <= nblocks <= 1048576 and num_table >= 1 (got %d, %d, %d)", nstreams,
                nblocks, num_table);
    W2L_REQUIRE(((reinterpret_cast<uintptr_t>(streams_host) | reinterpret_cast<uintptr_t>(streams) |
                  reinterpret_cast<uintptr_t>(blocks)) & 15) == 0,
                "resample_stream: 16-byte aligned stream and block tables");
    for (int k = 0; k < nstreams; ++k) {
        const w2l_resample_stream_entry& s = streams_host[k];
        W2L_REQUIRE(s.src && s.dst16 && s.win && s.delta, "resample_stream: stream %d has a NULL pointer", k);
        W2L_REQUIRE(s.index_step >= 1, "resample_stream: stream %d: index_step %d; the sample ratio is too small for the table", k,
                    s.index_step);
        W2L_REQUIRE(s.src_held >= 1 && s.dst_cap >= 1 && s.nwin >= 2 && s.src_first >= 0 && s.dst_first >= 0 && s.carry_held >= 0 &&
                        (s.carry_held == 0 || s.carry) && s.scale > 0.0 && s.scale <= 1.0 && s.inc > 0.0,
                    "resample_stream: stream %d: counts out of range", k);
    }
    ResampleStreamKArgs a;
    a.streams = reinterpret_cast<const ResampleStream*>(streams); a.nstreams = nstreams;
    a.blocks = reinterpret_cast<const ResampleBlock*>(blocks); a.num_table = num_table;
    hipLaunchKernelGGL(resample_stream_kernel, dim3((unsigned)nblocks), dim3(kResampleBlock), 0, static_cast<hipStream_t>(stream), a);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"
