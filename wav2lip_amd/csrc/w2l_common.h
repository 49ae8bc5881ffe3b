// Internal helpers shared by the HIP translation units of libw2l_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>

#include "../../include/w2l_hip.h"

namespace w2l {

void set_error(const char* fmt, ...);
// executed-FLOP counter (api.hip): families 0 = fp32 conv (forward / data gradient), 1 = fp32 weight gradient (direct GEMM),
// 2 = fp32 Winograd weight gradient, 3 = bf16c conv, 4 = bf16c weight gradient, 5 = bf16-storage conv, 6 = bf16-storage weight
// gradient, 7 = non-matrix-core reduction kernels (tiny heads)
bool flops_counting();
void flops_add(long long flops, int family);

#define W2L_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            w2l::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
                           __FILE__, __LINE__);                                          \
            return W2L_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

#define W2L_REQUIRE(cond, ...)                \
    do {                                      \
        if (!(cond)) {                        \
            w2l::set_error(__VA_ARGS__);      \
            return W2L_ERR_ARG;               \
        }                                     \
    } while (0)

// The ReLU / LeakyReLU / identity family as ONE expression of the negative-side slope (0, 0.01, 1): a select, not
// fma(neg, min(v, 0), max(v, 0)) - that form turned ReLU(-inf) into 0 * -inf = NaN and a NaN input into 0 (min / max drop the
// NaN), which hides a diverged training step.  Here NaN propagates (v < 0 is false: v itself), ReLU(-inf) = 0 (the one product
// that is not a number is 0 * -inf) and LeakyReLU(-inf) = -inf, as torch.  Used by every training-path kernel, split or not.
__device__ __forceinline__ float act_leaky(float v, float neg) {
    const float nv = neg * v;
    return v < 0.f ? (nv == nv ? nv : 0.f) : v;
}

// One entry of calc_pdist (evaluation/scores_LSE/SyncNetInstance_calc_scores.py:19-31), computed by one wave: || a - b + 1e-6 ||_2
// over C channels, `inside` false standing for a zero-padding row of b (b is then not read).  Lane l sums channels l, l + 64, ...,
// a xor butterfly folds the 64 partials, every lane returns the root.  shifted_pdist_kernel (train.hip) and
// lse_score_segments_kernel (sync_score.hip) both call it, so that their distances agree bit for bit.
__device__ __forceinline__ float shifted_pdist_wave(const float* __restrict__ a, const float* __restrict__ b, bool inside, int C,
                                                    int lane) {
    float s = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = a[c] - (inside ? b[c] : 0.f) + 1e-6f;
        s += d * d;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return sqrtf(s);
}

// The S3FD detector's input pixel: one BGR byte triple -> RGB order (api.py:62 `images[..., ::-1]`) minus the per-channel mean in
// float64, cast to float32 (detect.py:57-63).  Every pack kernel calls it - s3fd_pack_kernel, s3fd_pack_rows_kernel and
// s3fd_pack_rows_scaled_kernel (detect.hip), each for fp32 and bf16 storage - so that all forms agree byte for byte.
__device__ __forceinline__ void s3fd_pixel(const uint8_t* bgr, float m0, float m1, float m2, float& c0, float& c1, float& c2) {
    c0 = (float)((double)bgr[2] - (double)m0);
    c1 = (float)((double)bgr[1] - (double)m1);
    c2 = (float)((double)bgr[0] - (double)m2);
}

// `npx` (1..4) consecutive pixels of a u8 [.,3] frame at `p` into px[12]: three dword loads when the frame is 4-byte aligned (a
// group of four pixels is 12 bytes, so every full group of an aligned frame is aligned too), bytes otherwise and for the frame's
// last, shorter group.  Nothing outside the npx pixels is read.
__device__ __forceinline__ void s3fd_load_group(const uint8_t* __restrict__ p, bool dwords, int npx, uint8_t px[12]) {
    if (dwords && npx == 4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        const uint32_t v[3] = {q[0], q[1], q[2]};
#pragma unroll
        for (int k = 0; k < 12; ++k) px[k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
    } else {
        for (int k = 0; k < 3 * npx; ++k) px[k] = p[k];
    }
}

// One position (wx, hy) of an S3FD level of the given stride, from its class logits c[ncls] and box regression l[4] to the row
// (x1, y1, x2, y2, score) at o: max-out background label (net_s3fd.py:123-126), F.softmax over the two classes, the prior and the
// decode with variances (0.1, 0.2) (detect.py:66-84, bbox.py:91-108).  s3fd_decode_kernel (detect.hip) reads the logits from HBM,
// the fused bf16 head (s3fd_headb_kernel, detect_bf16.hip) from its fp32 accumulators in LDS.
__device__ __forceinline__ void s3fd_decode_px(const float* c, int ncls, const float* l, int stride, int wx, int hy, float* o) {
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
    const float bw = pw * expf(l[2] * 0.2f);
    const float bh = pw * expf(l[3] * 0.2f);
    cx -= bw / 2.f;
    cy -= bh / 2.f;
    o[0] = cx; o[1] = cy; o[2] = bw + cx; o[3] = bh + cy; o[4] = score;
}

// Workgroup ids are dealt round-robin to the 8 XCDs (id % 8), each with its own L2.  This maps the hardware id to a
// logical id such that every XCD walks one CONTIGUOUS range of logical ids: neighbouring tiles (which share input halos
// and A/B operand tiles) then meet in the same L2 instead of being fetched from HBM once per XCD.
#ifndef W2L_NO_XCD_REMAP
__host__ __device__ __forceinline__ unsigned xcd_remap(unsigned id, unsigned n) {
    constexpr unsigned kXcd = 8;
    const unsigned xcd = id % kXcd, local = id / kXcd;
    const unsigned base = n / kXcd, rem = n % kXcd;
    return xcd * base + (xcd < rem ? xcd : rem) + local;
}
#else
__host__ __device__ __forceinline__ unsigned xcd_remap(unsigned id, unsigned) { return id; }
#endif

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }
// workgroups for `work` items at `block` per workgroup, between 1 and `cap` (grid-stride kernels)
static inline int grid_cap(long long work, int block, int cap) {
    long long g = (work + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// ---- train_rows.hip, used by other translation units
// the stream's fp64 reduction scratch (one fixed buffer per stream; NULL + error when `bytes` exceeds it): the caller enqueues the
// kernel that fills it and the kernel that consumes it back to back on that stream
double* partial_ws(hipStream_t stream, size_t bytes);
// BatchNorm statistics / the two BatchNorm-backward column sums from a conv epilogue's fp32 per-wave partials [npart][2][cout_p]
int bn_stats_from_partials(hipStream_t s, const float* part, int npart, int cout_p, long long rows, int C, int Cvalid,
                           const float* gamma, const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                           float* mean, float* rstd, float* scale, float* shift);
int bn_bwd_sums_from_partials(hipStream_t s, const float* part, int npart, int cout_p, int C, int Cvalid, float* dgamma, float* dbeta);

// HBM bytes a launch fetches under the two tile orders of a (phase-major) grid whose 8 XCDs each walk a contiguous range of tiles,
// x = input bytes, w = weight bytes, tn = cout-tiles, passes = phases: cout-tiles FASTEST - every XCD holds 1/8 of the M-tiles and
// streams all of the weights; cout-tile SLOWEST - an XCD's range is tn / 8 of the M-tiles of the one or two cout-tiles it touches.
// The model ranks every launch of the batch-128 plan as FETCH_SIZE measures them (profiles/r05/l_*).
static inline long long fetch_cout_fastest(long long x, long long w, int tn, int passes) { return passes * x + 8 * w; }
static inline long long fetch_cout_slowest(long long x, long long w, int tn, int passes) {
    const int touched = tn >= 8 ? tn : 8 + (8 % tn ? tn - 1 : 0);   // (XCD, cout-tile) pairs
    return passes * x * (tn < 8 ? tn : 8) + w * touched / tn;
}

// ---- conv implicit-GEMM kernel arguments ---------------------------------------------------
constexpr int kMaxPhases = 9;   // convT k3 s1 p0 on 1x1 -> 3x3 has 9 single-tap phases
constexpr int kMaxTaps = 49;    // 7x7 stems
constexpr int kBK = 32;         // K-step of the implicit GEMM (floats)

struct ConvPhase {
    int ntaps;      // taps contributing to this output phase
    int kp;         // padded K length of this phase's weight slab = round_up(ntaps*cin_p, kBK)
    int po_y, po_x; // output position offset of the phase
    int tap_off;    // first entry of this phase in the tap table
    int pad_;
    long long w_off;  // float offset of this phase's slab [cout_p][kp] in the packed weights
};

struct ConvKArgs {
    const float* x;
    float* y;
    const float* res;
    const float* w;
    const __bf16* wsplit;   // the packed weights as three bf16 planes per phase (split-operand kernel), else unused
    const float* scale;
    const float* shift;
    const int* taps;  // packed (dy & 0xffff) | (dx << 16), relative input offsets per tap
    int N, H, W, cin_p, x_cs;
    int Ho, Wo, cout, cout_p, y_cs, res_cs;
    int Hq, Wq;       // q-grid: one implicit-GEMM row per (n, qy, qx)
    int sy, sx;       // input pixel = q*s + d(tap)
    int omy, omx;     // output pixel = q*om + po(phase)
    int act;
    int ncols;        // valid GEMM columns: cout, or pair*cout for an x-paired variant
    int pair;         // 1, or 2: GEMM column j is channel j % cout of output pixel ox + j / cout (x-paired small-cout conv)
    // fused 1x1 head (models/wav2lip.py:84-85): out[o] = head_act( sum_c head_w[o][c] * act(...)[c] + head_b[o] ), o < head_c;
    // when head_w != NULL the kernel writes head_c channels per pixel to y instead of cout
    const float* head_w;
    const float* head_b;
    int head_c, head_act;
    int vec_epilogue;  // 1: float4 epilogue (cout, strides and pointers 16-byte friendly)
    int M;            // N*Hq*Wq
    int tiles_m, tiles_n;
    int ksplit;           // gridDim.z: K-steps are cut into ksplit ranges of steps_per_split
    int steps_per_split;
    float* ws;            // split-K partial sums [ksplit][N*Ho*Wo][cout_p] (ksplit > 1)
    int order, order_r;   // workgroup -> (phase, tile_m, tile_n) order, see igemm_block_coords
    ConvPhase ph[kMaxPhases];
};

// Which (phase, M-tile, cout-tile) a workgroup of the implicit-GEMM grid (x = tiles, y = phases; z = K-splits, untouched) computes.
// Workgroups are handed to the 8 XCDs round-robin in dispatch order and every XCD has its own 4 MB L2, so WHAT runs side by side and
// back to back on one XCD decides how often an operand is fetched from HBM (measured per launch with FETCH_SIZE, profiles/r05/l_*):
//   kOrderPhaseMajor:   the plain grid order - all tiles of phase 0, then all of phase 1, ...; inside a phase every XCD walks a
//                       contiguous range of M-tiles, cout-tiles fastest.  A stride-2 transposed layer makes four passes over
//                       its input this way (512 -> 128 at 24x24, 128 frames: 151 MB of input, 763 MB fetched).
//   kOrderCoutSlowest:  phase-major too, but inside a phase the cout-tile is the SLOWEST index: an XCD's range covers one or two
//                       cout-tiles and streams its share of the M-tiles past their weights - for layers whose weights outweigh
//                       their input (512 -> 512 at 3x3: every XCD fetched all of the weights, 126 MB; now 1/8 of them each, 30 MB).
//   kOrderPhaseBlocked: groups of order_r M-tiles; an XCD runs phase 0 of a group (all cout-tiles), then phase 1 of the SAME group,
//                       ...: the group's input rows are still in L2 for phases 1-3 (438 MB fetched, same duration).  Needs several
//                       groups per XCD: phases differ in length (1 / 2 / 2 / 4 taps), and an XCD that holds one group's light phases
//                       while its neighbour holds the heavy ones finishes early (1024 -> 384 at 6x6: +19 %).
// What did NOT work, measured (profiles/r05/l_*): the phases of one M-tile SIDE BY SIDE on an XCD - phase fastest, or groups shorter
// than a round of 32 workgroups - fetches less but runs 30-40 % longer on every transposed layer: workgroups of different phases
// differ 1 : 2 : 2 : 4 in length, and the chip runs best when the workgroups in flight are alike.
enum { kOrderPhaseMajor = 0, kOrderCoutSlowest = 1, kOrderPhaseBlocked = 2 };
__host__ __device__ __forceinline__ void igemm_block_decode(int order, int order_r, int tiles_m, int tiles_n, unsigned bx, unsigned by,
                                                            unsigned nx, unsigned ny, int& phase, int& tile_m, int& tile_n) {
    const unsigned tm = (unsigned)tiles_m, tn = (unsigned)tiles_n;
    if (order != kOrderPhaseBlocked) {
        const unsigned b = xcd_remap(bx, nx);
        phase = (int)by;
        if (order == kOrderCoutSlowest) { tile_m = (int)(b % tm); tile_n = (int)(b / tm); }
        else { tile_n = (int)(b % tn); tile_m = (int)(b / tn); }
        return;
    }
    const unsigned j = xcd_remap(by * nx + bx, nx * ny);
    const unsigned R = (unsigned)order_r, G = R * tn * ny;
    const unsigned g = j / G, r = j - g * G;
    const unsigned left = tm - g * R, Re = left < R ? left : R;
    phase = (int)(r / (Re * tn));
    const unsigned rr = r % (Re * tn);
    tile_n = (int)(rr % tn);
    tile_m = (int)(g * R + rr / tn);
}
__device__ __forceinline__ void igemm_block_coords(const ConvKArgs& a, int& phase, int& tile_m, int& tile_n) {
    igemm_block_decode(a.order, a.order_r, a.tiles_m, a.tiles_n, blockIdx.x, blockIdx.y, gridDim.x, gridDim.y, phase, tile_m, tile_n);
}

// ---- Winograd F(2x2,3x3) kernel arguments (conv_wino.hip) -----------------------------------
struct WinoKArgs {
    const float* x;
    float* y;
    const float* res;
    const float* u;      // transformed weights in MFMA B-fragment order (wino_pack)
    const float* scale;
    const float* shift;
    int N, H, W, cin, x_cs;   // output is N x H x W too (3x3, stride 1, pad 1)
    int cout, y_cs, res_cs;
    int TH, TW, M;       // 2x2 output tiles per image and in total (filled by wino_launch)
    int nks;             // cin / 8
    int tiles_n, tiles_m;
    int act;
    int m_fastest;       // conv_wino.hip only: work items run M-tile fastest (weight-heavy layers), else cout-tile fastest
};

constexpr int kNumWinoCfgs = 2;    // configurations of conv_wino.hip (kWino); configuration ids: kIdList in conv_igemm.hip
int wino_init_attrs();
bool wino_cfg_ok(int cfg, int cin, int cout);
long long wino_u_floats(int cin, int cout);
int wino_pack(const float* w, float* u, int cin, int cout, int transposed, hipStream_t stream);
int wino_launch(int cfg, WinoKArgs a, hipStream_t stream, long long* flops_out);
// second-generation kernel (conv_wino2.hip)
constexpr int kNumWino2Cfgs = 2;   // its configurations (kW2Cfgs)
bool wino2_ok(int cfg, int cin, int cout, int head_c);
int wino2_init_attrs();
int wino2_launch(int cfg, const WinoKArgs& a, const float* head_w, const float* head_b, int head_c, int head_act,
                 hipStream_t stream, long long* flops_out);

// quarter-split shape of the second-generation kernel (32 tiles x 32 couts, two workgroups per CU; conv_wino2.hip): the
// configuration id after conv_wino4's; same transformed weights as the other F(2x2) kernels
bool wino2q_ok(int cin, int cout, int head_c);
int wino2q_init_attrs();
int wino2q_launch(const WinoKArgs& a, const float* head_w, const float* head_b, int head_c, int head_act, hipStream_t stream,
                  long long* flops_out);

// F(4x4,3x3) Winograd kernel (conv_wino4.hip): the configuration id after conv_tp2's; its own 36-position weight transform
bool wino4_ok(int cin, int cout);
long long wino4_u_floats(int cin, int cout);
int wino4_pack(const float* w, float* u, int cin, int cout, int transposed, hipStream_t stream);
int wino4_init_attrs();
int wino4_launch(const WinoKArgs& a, const float* u4, hipStream_t stream, long long* flops_out);

// split-operand F(2x2,3x3) Winograd kernel (conv_wino2s.hip): fp32 result from the bf16 matrix cores; its own pre-split
// 16-position weight transform, split from the F(2x2) fp32 weights on first use
bool wino2s_ok(int cin, int cout);
long long wino2s_u_elems(int cin, int cout);
int wino2s_pack(const float* wino_u32, __bf16* u, int cin, int cout, hipStream_t stream);   // from wino_pack's fp32 U
int wino2s_launch(const WinoKArgs& a, const __bf16* u, hipStream_t stream, long long* flops_out);
void wino2s_plane_geom(int bh, int bw, int ni, int* pitch, int* istride);
// the (bh, bw, ni) block each grouped family's launcher picks for a shape (host code; w2l_conv_block_plan)
void wino2_block_plan(int cfg, int N, int H, int W, int out[3]);   // cfg kNumWino2Cfgs: the quarter-split shape
void wino2s_block_plan(int N, int H, int W, int out[3]);
void tp2_block_plan(int N, int H, int W, int out[3]);
void tp2s_block_plan(int N, int H, int W, int out[3]);
void k3s_block_plan(int N, int H, int W, int out[3]);

// fused-phase stride-2 transposed 3x3 convolution (conv_tp2.hip): the configuration id after the Winograd families
bool tp2_ok(const w2l_conv_geom& g);
long long tp2_u_floats(int cin, int cout);
int tp2_pack(const float* w, float* u, int cin, int cout, hipStream_t stream);
int tp2_init_attrs();
// direct 3x3 stride-1 convolution with split operands for 32-cout layers, optional fused 1x1 head (conv_k3s.hip)
bool k3s_ok(const w2l_conv_geom& g);
long long k3s_u_elems(int cin);
int k3s_pack(const float* w, __bf16* u, int cin, hipStream_t stream);
int k3s_init_attrs();
int k3s_launch(const float* x, int x_cs, float* y, int y_cs, const float* res, int res_cs, const __bf16* u, const float* scale,
               const float* shift, const float* head_w, const float* head_b, int head_c, int head_act, int N, int H, int W, int cin,
               int act, hipStream_t stream, long long* flops_out);
// its bf16-storage form with the head always fused (w2l_convb_attach_head): one plane, uint8 frames (+ optional fp32) out
long long k3sb_u_elems(int cin);
int k3sb_pack(const float* w, __bf16* u, int cin, hipStream_t stream);
int k3sb_init_attrs();
int k3sb_launch(const __bf16* x, int x_cs, uint8_t* frames, float* y, int y_cs, const __bf16* u, const float* scale, const float* shift,
                const float* head_w, const float* head_b, int head_c, int head_act, int N, int H, int W, int cin, int act,
                hipStream_t stream, long long* flops_out);
// the generator's 7x7 first layer with split operands (conv_stem7s.hip): region staged and split once, contraction out of LDS
bool stem7s_ok(const w2l_conv_geom& g);
long long stem7s_u_elems();
int stem7s_pack(const float* w, __bf16* u, int cin, hipStream_t stream);
int stem7s_init_attrs();
int stem7s_launch(const float* x, int x_cs, float* y, int y_cs, const __bf16* u, const float* scale, const float* shift, int N, int H,
                  int W, int act, hipStream_t stream, long long* flops_out);
// the same layer shape with split operands on the bf16 matrix cores (conv_tp2s.hip): pre-split weights built from tp2_pack's output
bool tp2s_ok(const w2l_conv_geom& g);
long long tp2s_u_elems(int cin, int cout);
int tp2s_pack(const float* tp2_u32, __bf16* u, int cin, int cout, hipStream_t stream);
int tp2s_init_attrs();
int tp2s_launch(const float* x, int x_cs, float* y, int y_cs, const __bf16* u, const float* scale, const float* shift, int N, int H,
                int W, int cin, int cout, int act, int ksplit, float* ws, int* ksplit_out, hipStream_t stream, long long* flops_out);
int tp2_launch(const float* x, int x_cs, float* y, int y_cs, const float* u, const float* scale, const float* shift, int N, int H,
               int W, int cin, int cout, int act, hipStream_t stream, long long* flops_out);

// bf16-storage conv launches (conv_bf16.hip, conv_box_bf16.hip): what the epilogue does beside storing the output
struct BEpilogue {
    enum Kind {
        STATS,   // BatchNorm statistics of the output (w2l_convb_forward_bn); no operands
        BNBWD,   // the output is the dy of a BatchNorm block: that block's backward sums (w2l_convb_forward_bnbwd)
        MASK     // the output is the dy of an activation block without BatchNorm: dy * act'(y) is stored (w2l_convb_forward_actbwd)
    };
    Kind kind = STATS;
    const void* z = nullptr;    // BNBWD: the block's pre-BatchNorm output
    const void* y = nullptr;    // the block's output; BNBWD of a ReLU block without residual: NULL, mask from z * scale + shift
    int z_cs = 0, y_cs = 0;
    float neg = 1.f;            // act'(.) on the non-positive side: 0 ReLU, 0.01 LeakyReLU, 1 none
    const float* mean = nullptr;
    const float* rstd = nullptr;
    const float* scale = nullptr;
    const float* shift = nullptr;
    int store_g = 0;            // BNBWD of a ReLU block: store the masked gradient (W2L_BNBWD_STORE_MASKED); MASK: column sums wanted
};
// ... and what the launch did about it: part != NULL: per-wave column partials [npart][2][cout_p] in the stream's scratch (else the
// caller runs the stand-alone reduction); masked: a MASK launch stored the masked gradient
struct BEpilogueOut {
    float* part = nullptr;
    int npart = 0;
    bool masked = false;
};

}  // namespace w2l
