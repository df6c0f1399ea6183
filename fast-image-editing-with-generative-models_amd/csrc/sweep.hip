// The selector of a strength sweep: which of k finished variants is returned, decided and copied on the device (include/fie.h:
// fie_sweep_select_u8; fie_amd/sweep.py: select_numpy restates the rule).
//   sums[i] = the variant's ssim_sum (field 1 of its fie_metrics_pairs_u8 row) or, with bg, its bg_ssim_sum (field 3); ok[i] = sums[i] >= floor
//   nobody passes   the largest non-NaN sum, ties to the larger index; k - 1 when every sum is a NaN
//   rule 0          the smallest passing index: variants come strongest first, so the most editing the preservation budget allows
//   rule 1          the largest clip[i][1] among the passing, ties to the larger index; a NaN never wins; all NaN: the largest passing index
// One launch.  The k image pointers travel by value in the kernel arguments -- no pointer table in memory, no stacking copy in front.  Thread 0
// of EVERY block reads the at most 16 rows and evaluates the rule for its block (float64 / float32 compares, nothing else: every block arrives at
// the same index), then the block copies its share of the winner; block 0 also stores the index, the head and the tail.  No atomics, no block
// waits for another.
// The copy.  The output is a head of 0 .. 15 bytes up to the next 16-byte boundary of its ADDRESS, a body of aligned 16-byte stores and a tail.
// A source that is congruent to the output mod 16 is read by aligned 16-byte loads; any other source (the per-image buffers of the
// full-resolution back end are separate allocations and a view may start at any byte) through the aligned dwords that cover each four bytes
// (image_ops.h: load4), by bytes at the operand's two ends.  No access is misaligned, none leaves [src, src + bytes) or [out, out + bytes).
// Grid: 16 bytes a lane, four loads in flight a thread, at most 2048 blocks of 256 grid-striding over the body.
#include "image_ops.h"

namespace {

using fie_img::load4;

constexpr int kSweepMax = 16;
constexpr int kSweepUnroll = 4;

struct SweepImages {
    const uint8_t* p[kSweepMax];       // entries past k are NULL
};

// The rule, by one thread of the block: loops bounded by k, one row read per variant.  The other waves of the block wait at the barrier instead of
// each spending the same few hundred instructions in front of its first load.
__device__ __forceinline__ int sweep_winner(const int64_t* __restrict__ rows, const float* __restrict__ clip, int k, int rule, double floor, int bg) {
    const double* sums = reinterpret_cast<const double*>(rows) + (bg ? 3 : 1);
    int first = -1, last = -1;
    for (int i = 0; i < k; ++i)
        if (sums[4 * i] >= floor) {
            if (first < 0) first = i;
            last = i;
        }
    if (first < 0) {
        int best = -1;
        double bv = 0.0;
        for (int i = 0; i < k; ++i) {
            const double v = sums[4 * i];
            if (v == v && (best < 0 || v >= bv)) { best = i; bv = v; }
        }
        return best >= 0 ? best : k - 1;
    }
    if (rule == 0) return first;
    int best = -1;
    float bv = 0.f;
    for (int i = first; i <= last; ++i) {
        if (!(sums[4 * i] >= floor)) continue;
        const float v = clip[2 * i + 1];
        if (v == v && (best < 0 || v >= bv)) { best = i; bv = v; }
    }
    return best >= 0 ? best : last;
}

__global__ __launch_bounds__(256) void sweep_select_kernel(SweepImages imgs, int k, int64_t bytes, const int64_t* __restrict__ rows,
                                                           const float* __restrict__ clip, int rule, double floor, int bg,
                                                           uint8_t* __restrict__ out, int32_t* __restrict__ out_idx) {
    __shared__ int win;
    if (threadIdx.x == 0) win = sweep_winner(rows, clip, k, rule, floor, bg);
    __syncthreads();
    const int w = win;
    const uint8_t* src = imgs.p[0];
#pragma unroll
    for (int i = 1; i < kSweepMax; ++i) src = i == w ? imgs.p[i] : src;       // selects over the arguments: a run-time index would send them through memory
    const int64_t h = (int64_t)((0 - (uintptr_t)out) & 15);
    const int64_t head = h < bytes ? h : bytes;
    const int64_t n16 = (bytes - head) >> 4;
    const int64_t tail0 = head + (n16 << 4);
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) *out_idx = w;
        if ((int64_t)threadIdx.x < head) out[threadIdx.x] = src[threadIdx.x];
        if (tail0 + (int64_t)threadIdx.x < bytes) out[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];      // fewer than 16 bytes
    }
    const uint8_t* s0 = src + head;
    uint4* d0 = reinterpret_cast<uint4*>(out + head);
    const int64_t stride = (int64_t)gridDim.x * 256;
    const bool congruent = (((uintptr_t)s0) & 15) == 0;
    const uint8_t* send = src + bytes;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += kSweepUnroll * stride) {
        uint4 v[kSweepUnroll];
#pragma unroll
        for (int u = 0; u < kSweepUnroll; ++u) {
            const int64_t j = i + u * stride;
            if (j < n16) {
                const uint8_t* a = s0 + (j << 4);
                if (congruent)
                    v[u] = *reinterpret_cast<const uint4*>(a);
                else
                    v[u] = make_uint4(load4(a, src, send), load4(a + 4, src, send), load4(a + 8, src, send), load4(a + 12, src, send));
            }
        }
#pragma unroll
        for (int u = 0; u < kSweepUnroll; ++u) {
            const int64_t j = i + u * stride;
            if (j < n16) d0[j] = v[u];
        }
    }
}

}  // namespace

extern "C" {

int fie_sweep_select_u8(fie_ctx* ctx, const void* const* imgs, int k, int64_t bytes, const int64_t* rows, const float* clip_or_null, int rule,
                        double floor, int bg, void* out_img, int32_t* out_idx) {
    FIE_REQUIRE(ctx && imgs && rows && out_img && out_idx, "fie_sweep_select_u8: bad argument: NULL ctx, imgs, rows, out_img or out_idx");
    FIE_REQUIRE(k >= 1 && k <= kSweepMax, "fie_sweep_select_u8: bad argument: k = %d outside 1 .. %d", k, kSweepMax);
    FIE_REQUIRE(bytes >= 1 && bytes <= ((int64_t)1 << 31), "fie_sweep_select_u8: bad argument: bytes = %lld outside 1 .. 2^31", (long long)bytes);
    FIE_REQUIRE(rule == 0 || (rule == 1 && clip_or_null), "fie_sweep_select_u8: bad argument: rule = %d (0 strongest, 1 clip score, which needs the CLIP rows)",
                rule);
    FIE_REQUIRE(bg == 0 || bg == 1, "fie_sweep_select_u8: bad argument: bg = %d (0 or 1)", bg);
    FIE_REQUIRE(((uintptr_t)rows & 7) == 0 && ((uintptr_t)clip_or_null & 3) == 0 && ((uintptr_t)out_idx & 3) == 0,
                "fie_sweep_select_u8: bad argument: rows 8-byte, clip and out_idx 4-byte aligned");
    SweepImages si = {};
    uint8_t* out = static_cast<uint8_t*>(out_img);
    for (int i = 0; i < k; ++i) {
        const uint8_t* p = static_cast<const uint8_t*>(imgs[i]);
        FIE_REQUIRE(p, "fie_sweep_select_u8: bad argument: imgs[%d] is NULL", i);
        FIE_REQUIRE(p + bytes <= out || out + bytes <= p, "fie_sweep_select_u8: bad argument: the output overlaps imgs[%d]", i);
        si.p[i] = p;
    }
    const int64_t items = (bytes >> 4) + 1;
    const unsigned grid = fie_img::grid_1d((items + kSweepUnroll - 1) / kSweepUnroll, fie_img::kPointwiseBlocks);
    FIE_DESC(ctx, "sweep_select k=%d bytes=%lld rule=%d bg=%d", k, (long long)bytes, rule, bg);
    fie_launch(ctx, sweep_select_kernel, dim3(grid), dim3(256), 0, si, k, bytes, rows, clip_or_null, rule, floor, bg, out, out_idx);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
