// Prompt emphasis: the V rows of the text's cross-attention K | V scaled by a weight per text row (include/fie.h: fie_kv_emphasis).
//   X [rows, ld] f16 or f32, w f32 [rows], vflags u8 [ncols / 8]: X[r, 8 g .. 8 g + 8) *= w[r] where vflags[g] != 0, for every row r with w[r] != 1.
// One fp32 multiply per element and, for f16, the one rounding of the conversion back (nearest even; beyond 65504 an infinity).  A row of weight 1 --
// all but the 1-10 marked rows of a prompt -- is neither read nor written: its blocks leave behind one scalar load.  A thread owns whole 8-column
// groups (one 16-byte access for f16, two for f32), so no element has two writers; unflagged groups (K) and the padding beyond ncols are never touched.
// The weights are read from device memory at run time: a hipGraph replay scales by the weights of the job it replays.  No atomics, no workspace.
#include "fie_internal.h"

namespace {

constexpr int kEmphGroups = 4;             // 8-column groups per thread: 256 threads cover 8192 columns of one row

template <typename T>
__global__ __launch_bounds__(256) void kv_emphasis_kernel(T* __restrict__ X, int64_t ld, int groups, const float* __restrict__ w,
                                                          const uint8_t* __restrict__ vflags) {
    const float wr = w[blockIdx.x];
    if (wr == 1.0f) return;                // block-uniform: the row stays as the GEMM wrote it
    T* row = X + (int64_t)blockIdx.x * ld;
    const int g0 = (int)blockIdx.y * (256 * kEmphGroups) + (int)threadIdx.x;
#pragma unroll
    for (int j = 0; j < kEmphGroups; ++j) {
        const int g = g0 + j * 256;        // consecutive lanes, consecutive 16 / 32 bytes
        if (g < groups && vflags[g]) {
            float x[8];
            fie_load8(row + (int64_t)g * 8, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] *= wr;
            fie_store8(row + (int64_t)g * 8, x);
        }
    }
}

}  // namespace

extern "C" {

int fie_kv_emphasis(fie_ctx* ctx, void* X, int64_t ld, int64_t rows, int64_t ncols, const float* w, const uint8_t* vflags, int f32) {
    FIE_REQUIRE(ctx && X && w && vflags, "fie_kv_emphasis: NULL argument");
    FIE_REQUIRE(rows >= 1 && rows < ((int64_t)1 << 31), "fie_kv_emphasis: rows %lld outside 1 .. 2^31 - 1", (long long)rows);
    FIE_REQUIRE(ncols >= 8 && ncols % 8 == 0 && ncols <= ((int64_t)1 << 24), "fie_kv_emphasis: ncols %lld: a multiple of 8 in 8 .. 2^24 (c %% 8 == 0)",
                (long long)ncols);
    FIE_REQUIRE(ld >= ncols && ld % 8 == 0, "fie_kv_emphasis: ld %lld: a multiple of 8, at least ncols = %lld", (long long)ld, (long long)ncols);
    FIE_REQUIRE((uintptr_t)X % 16 == 0 && (uintptr_t)w % 4 == 0, "fie_kv_emphasis: X must be 16-byte aligned, w 4-byte aligned");
    FIE_REQUIRE(f32 == 0 || f32 == 1, "fie_kv_emphasis: f32 = %d: 0 (f16) or 1", f32);
    const int groups = (int)(ncols / 8);
    const dim3 grid((unsigned)rows, (unsigned)((groups + 256 * kEmphGroups - 1) / (256 * kEmphGroups)));
    FIE_DESC(ctx, "kv_emphasis %lldx%lld ld=%lld %s", (long long)rows, (long long)ncols, (long long)ld, f32 ? "f32" : "f16");
    if (f32)
        fie_launch(ctx, kv_emphasis_kernel<float>, grid, dim3(256), 0, (float*)X, ld, groups, w, vflags);
    else
        fie_launch(ctx, kv_emphasis_kernel<half_t>, grid, dim3(256), 0, (half_t*)X, ld, groups, w, vflags);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
