// Scene-cut detection (opt-in `scene_cuts`; not the reference's behaviour): where the shots of a clip are, from the
// pixels that already lie in HBM for the detector.  The rule is in include/w2l_hip.h; two launches:
//   w2l_frame_hist_rows  the SIGNATURE of each frame of an address table: 3 channels x 32 bins of `byte >> 3`, uint32 counts.
//                        Reads every byte of every frame once - the hot kernel, bound by HBM and by LDS atomics.
//   w2l_scene_cuts       D(i) = sum |sig_i - sig_{i-1}| and the cut flags per segment of w2l_face_boxes_segments' table.
//
// The signature kernel.  A frame is head | units | tail: `head` = the 0..15 bytes up to the first 16-byte aligned address, units of
// 48 bytes (three 16-byte loads, 16 pixels), `tail` = the < 48 bytes left.  A unit starts a multiple of 3 bytes after the first
// unit, so byte j of EVERY unit has the same channel, (head + j) % 3: a lane counts into the "local" channel j % 3 with every
// index known at compile time, and the rotation by head % 3 happens once per workgroup, when the counters leave.  Head and tail
// are counted byte by byte by the frame's first workgroup, into the same local channels.  No byte outside the frame is loaded.
//
// Counters: LDS, private to a wave and, inside the wave, to lane % 16 - 4 waves x 16 copies x 96 words = 24 KB per workgroup, at
// word [wave][slot = channel * 32 + bin][copy], so the 16 copies of a slot lie in 16 different banks.  On top of that a lane
// aggregates equal neighbours: the 16 bytes of a channel in its unit are walked in order and a run of equal bins leaves as ONE
// ds_add of the run length.  A flat frame (letterbox bars, black frames), the worst case for a histogram - all 64 lanes on one
// counter, 16 times per channel and unit - becomes one add per lane, channel and unit, on 16 addresses in 16 banks with 4 lanes
// each; random bytes do 16 adds per channel and unit spread over 512 words.  A workgroup then sums its 64 copies of each slot
// and adds the 96 sums to the frame's zeroed `sig` row with integer atomics (the entry zeroes the rows on the stream first):
// integer sums, so the words do not depend on the launch geometry or on the order the workgroups arrive in.
#include "w2l_common.h"

namespace w2l {

constexpr int kSigWords = 96, kSigBins = 32;
constexpr int kHistLanes = 256, kHistWaves = kHistLanes / 64, kHistCopies = 16;
constexpr int kHistUnit = 48;                  // bytes of a unit: 16 pixels, three 16-byte loads
constexpr int kHistUnitsPerLane = 4;           // units a lane takes when the grid is not capped
constexpr int kHistMaxGroups = 64;             // workgroups a frame is split over at the most
constexpr int kCutBadSegment = 3;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the 16 bytes of local channel C in the 12 dwords of a unit, in order, runs of equal bins leaving as one add each
template <int C>
__device__ __forceinline__ void hist_channel(const uint32_t (&w)[12], uint32_t* __restrict__ mine) {
    uint32_t* h = mine + C * kSigBins * kHistCopies;
    int cur = (int)((w[C >> 2] >> (8 * (C & 3) + 3)) & 31u), run = 1;
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        const int j = C + 3 * k;
        const int b = (int)((w[j >> 2] >> (8 * (j & 3) + 3)) & 31u);
        if (b != cur) {
            atomicAdd(h + cur * kHistCopies, (uint32_t)run);
            cur = b;
            run = 0;
        }
        ++run;
    }
    atomicAdd(h + cur * kHistCopies, (uint32_t)run);
}

// grid.x = B * groups: workgroup g of frame b takes the units g * 256 + t, stepping groups * 256
__global__ __launch_bounds__(kHistLanes) void frame_hist_rows_kernel(int nbytes, int groups, const uint64_t* __restrict__ frames,
                                                                     uint32_t* __restrict__ sig) {
    __shared__ uint32_t cnt[kHistWaves * kSigWords * kHistCopies];
    const int t = threadIdx.x;
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
    for (int i = t; i < kHistWaves * kSigWords * kHistCopies; i += kHistLanes) cnt[i] = 0;
    __syncthreads();
    const uint64_t addr = frames[b];
    const uint8_t* x = reinterpret_cast<const uint8_t*>(addr);
    const int head = min((int)((16 - (addr & 15)) & 15), nbytes);
    const int nunits = (nbytes - head) / kHistUnit;
    const int tail0 = head + nunits * kHistUnit;         // first byte of the tail; nbytes - tail0 < 48
    uint32_t* mine = cnt + (t >> 6) * (kSigWords * kHistCopies) + (t & (kHistCopies - 1));
    for (int u = g * kHistLanes + t; u < nunits; u += groups * kHistLanes) {
        const u32x4* p = reinterpret_cast<const u32x4*>(x + head + (size_t)u * kHistUnit);      // 16-byte aligned by `head`
        const u32x4 v0 = p[0], v1 = p[1], v2 = p[2];
        const uint32_t w[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
        hist_channel<0>(w, mine);
        hist_channel<1>(w, mine);
        hist_channel<2>(w, mine);
    }
    if (g == 0) {                                        // head and tail, byte by byte: local channel = (offset - head) mod 3
        int off = -1;
        if (t < head) off = t;
        else if (t >= 64 && t - 64 < nbytes - tail0) off = tail0 + (t - 64);
        if (off >= 0) {
            const int lc = (off - head + 18) % 3;        // head <= 15: the sum is never negative
            atomicAdd(mine + (lc * kSigBins + (x[off] >> 3)) * kHistCopies, 1u);
        }
    }
    __syncthreads();
    if (t < kSigWords) {
        uint32_t s = 0;
        for (int w = 0; w < kHistWaves; ++w) {
            const uint32_t* c = cnt + (w * kSigWords + t) * kHistCopies;
#pragma unroll
            for (int k = 0; k < kHistCopies; ++k) s += c[k];
        }
        const int lc = t >> 5, ch = (lc + head) % 3;     // byte j of a unit is byte head + j (mod 3) of the frame
        if (s) atomicAdd(sig + (size_t)b * kSigWords + ch * kSigBins + (t & 31), s);
    }
}

struct CutSeg { int row0, n, H, W; };
static_assert(sizeof(CutSeg) == sizeof(w2l_box_segment), "the cut kernel reads w2l_box_segment rows");

// one wave per segment, 64 rows at a time: a lane reads its own row and the row before it
__global__ __launch_bounds__(64) void scene_cuts_kernel(const CutSeg* __restrict__ segs, const uint32_t* __restrict__ sig, int n_rows,
                                                        int q, int* __restrict__ cuts, int* __restrict__ dist, int* __restrict__ status) {
    const int lane = threadIdx.x;
    const CutSeg s = segs[blockIdx.x];
    if (s.n <= 0) {
        if (lane == 0) status[blockIdx.x] = 0;
        return;
    }
    const long long hw = (long long)s.H * s.W;
    if (s.row0 < 0 || (long long)s.row0 + s.n > n_rows || s.H < 1 || s.W < 1 || 6 * hw >= (1ll << 31)) {        // uniform
        if (lane == 0) status[blockIdx.x] = kCutBadSegment;
        return;
    }
    if (lane == 0) status[blockIdx.x] = 0;
    const long long bound = (long long)q * 6 * hw;
    for (int i = lane; i < s.n; i += 64) {
        const long long row = (long long)s.row0 + i;
        long long d = 0;
        if (i > 0) {
            const uint32_t* a = sig + row * kSigWords;
            const uint32_t* p = a - kSigWords;
            for (int k = 0; k < kSigWords; ++k) {
                const long long x = (long long)a[k] - (long long)p[k];
                d += x < 0 ? -x : x;
            }
        }
        cuts[row] = (i > 0 && d * 256 > bound) ? 1 : 0;
        if (dist) dist[row] = (int)min(d, (long long)INT32_MAX);     // D <= 6 H W < 2^31 for signatures of H x W frames
    }
}

}  // namespace w2l

using namespace w2l;

extern "C" {

int w2l_frame_hist_rows(void* stream, int B, int H, int W, const uint64_t* frames, uint32_t* sig) {
    W2L_REQUIRE(frames && sig, "frame_hist_rows: NULL argument");
    W2L_REQUIRE(B >= 1, "frame_hist_rows: B=%d must be at least 1", B);
    W2L_REQUIRE(H >= 1 && W >= 1 && 6ll * H * W < (1ll << 31), "frame_hist_rows: H, W >= 1 and 6 * H * W < 2^31 (got %d x %d)", H, W);
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(frames) & 7) == 0 && (reinterpret_cast<uintptr_t>(sig) & 3) == 0,
                "frame_hist_rows: the address table must be 8-byte aligned and sig 4-byte aligned");
    const int nbytes = H * W * 3;
    const int groups = grid_cap(nbytes / kHistUnit, kHistLanes * kHistUnitsPerLane, kHistMaxGroups);
    W2L_REQUIRE((long long)B * groups < (1ll << 31), "frame_hist_rows: B=%d frames of %d workgroups exceed the grid", B, groups);
    hipStream_t s = static_cast<hipStream_t>(stream);
    W2L_HIP_CHECK(hipMemsetAsync(sig, 0, (size_t)B * kSigWords * sizeof(uint32_t), s));
    hipLaunchKernelGGL(frame_hist_rows_kernel, dim3((unsigned)(B * groups)), dim3(kHistLanes), 0, s, nbytes, groups, frames, sig);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

int w2l_scene_cuts(void* stream, int n_seg, const w2l_box_segment* segs, const uint32_t* sig, int n_rows, int q, int32_t* cuts,
                   int32_t* dist, int32_t* status) {
    W2L_REQUIRE(segs && sig && cuts && status, "scene_cuts: NULL argument");
    W2L_REQUIRE(n_seg >= 1 && n_rows >= 0, "scene_cuts: n_seg=%d must be at least 1 and n_rows=%d at least 0", n_seg, n_rows);
    W2L_REQUIRE(q >= 1 && q <= 255, "scene_cuts: q=%d outside 1..255", q);
    W2L_REQUIRE((reinterpret_cast<uintptr_t>(segs) & 15) == 0, "scene_cuts: the segment table must be 16-byte aligned");
    hipLaunchKernelGGL(scene_cuts_kernel, dim3(n_seg), dim3(64), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const CutSeg*>(segs), sig, n_rows, q, cuts, dist, status);
    W2L_HIP_CHECK(hipGetLastError());
    return W2L_OK;
}

}  // extern "C"
