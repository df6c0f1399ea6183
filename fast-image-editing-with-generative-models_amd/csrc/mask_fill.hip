// Masked-content modes of a mask-restricted edit (include/fie.h: fie_mask_fill_rgb_u8).  The latent modes are
// fie_latent_prep_src_content's (csrc/lcm.hip).
//   fill          the hole m = (L >= 128) of a u8 RGB image replaced by a smooth continuation of its surroundings: a push-pull pyramid in
//                 integer arithmetic.  Push: per level the sums S[c] of the known pixels' values and their count w, over 2x2 children, sizes
//                 ceil-halved down to 1x1.  Pull, from the top: a cell with w > 0 resolves to its mean in 1/256 units, one without takes the
//                 9-3-3-1 bilinear tap of the resolved level above (32768 at the top: nothing known at all).  Known pixels keep their bytes.
//   edge clear    the ControlNet's edge map set to 0 inside the hole (the last pass of the same op, or that pass alone with out == NULL).
// Levels are ordered by kernel boundaries (and, inside the one-block kernel that owns every level of <= 1024 cells, by __syncthreads):
// no block waits for another, nothing synchronises with the host, every launch goes through fie_launch.
#include "image_ops.h"

namespace {

constexpr int kFillTopCells = 1024;    // a level of at most this many cells, and every level above it, belongs to the one-block kernel
constexpr int kFillMaxLevels = 32;     // ceil-halving an int side reaches 1 in at most 31 steps
constexpr int64_t kFillMaxPixels = (int64_t)1 << 24;   // 2^24 x 255 < 2^32: the level sums stay in 32 bits

// The pyramid above level 0 (level 0 is the image itself and is never stored): level k is a [h[k]][w[k]] array of uint4 {S_r, S_g, S_b, w},
// overwritten in place by {C_r, C_g, C_b, w} when it is resolved; the levels lie back to back, level 1 first.
struct FillPlan {
    int K = 0;                          // levels above level 0 (0 for a 1x1 image)
    int kt = 0;                         // first level (>= 1) of at most kFillTopCells cells
    int h[kFillMaxLevels + 1], w[kFillMaxLevels + 1];
    int64_t off[kFillMaxLevels + 2];    // off[k]: first cell of level k; off[K + 1]: cells in all
};

FillPlan fill_plan(int H, int W) {
    FillPlan p;
    p.h[0] = H; p.w[0] = W;
    p.off[0] = p.off[1] = 0;
    while (p.h[p.K] > 1 || p.w[p.K] > 1) {
        const int k = ++p.K;
        p.h[k] = (p.h[k - 1] + 1) >> 1;
        p.w[k] = (p.w[k - 1] + 1) >> 1;
        p.off[k + 1] = p.off[k] + (int64_t)p.h[k] * p.w[k];
        if (!p.kt && (int64_t)p.h[k] * p.w[k] <= kFillTopCells) p.kt = k;
    }
    return p;
}

__device__ __forceinline__ void fill_acc(uint4& s, const uint4 v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }

// sums of the children (2Y + dy, 2X + dx) that lie inside the [Hc][Wc] level below
__device__ __forceinline__ uint4 fill_push_cell(const uint4* __restrict__ child, int Hc, int Wc, int Y, int X) {
    uint4 s = make_uint4(0, 0, 0, 0);
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int y = 2 * Y + dy, x = 2 * X + dx;
            if (y < Hc && x < Wc) fill_acc(s, child[(int64_t)y * Wc + x]);
        }
    return s;
}

// the value, in 1/256 units, that the resolved level above gives cell (y, x): 9-3-3-1 over the parent and its neighbours on the cell's side, clamped
__device__ __forceinline__ void fill_pull(const uint4* __restrict__ parent, int Hp, int Wp, int y, int x, uint32_t (&c)[3]) {
    if (!parent) {                      // above the 1x1 top: no pixel of the image is known
        c[0] = c[1] = c[2] = 32768u;
        return;
    }
    const int Y = y >> 1, X = x >> 1;
    const int Y2 = min(max(Y + ((y & 1) ? 1 : -1), 0), Hp - 1), X2 = min(max(X + ((x & 1) ? 1 : -1), 0), Wp - 1);
    const uint4 a = parent[(int64_t)Y * Wp + X], b = parent[(int64_t)Y * Wp + X2], d = parent[(int64_t)Y2 * Wp + X], e = parent[(int64_t)Y2 * Wp + X2];
    c[0] = (9u * a.x + 3u * b.x + 3u * d.x + e.x + 8u) >> 4;
    c[1] = (9u * a.y + 3u * b.y + 3u * d.y + e.y + 8u) >> 4;
    c[2] = (9u * a.z + 3u * b.z + 3u * d.z + e.z + 8u) >> 4;
}

__device__ __forceinline__ void fill_resolve_cell(uint4* __restrict__ lvl, int Wk, int y, int x, const uint4* __restrict__ parent, int Hp, int Wp) {
    const int64_t i = (int64_t)y * Wk + x;
    const uint4 v = lvl[i];
    uint32_t c[3];
    if (v.w) {
        const uint64_t w = v.w, half = v.w >> 1;
        c[0] = (uint32_t)((256ull * v.x + half) / w);
        c[1] = (uint32_t)((256ull * v.y + half) / w);
        c[2] = (uint32_t)((256ull * v.z + half) / w);
    } else {
        fill_pull(parent, Hp, Wp, y, x, c);
    }
    lvl[i] = make_uint4(c[0], c[1], c[2], v.w);
}

// level 1 straight from the image: level 0 is S = known ? src : 0, w = known
__global__ __launch_bounds__(256) void fill_push0_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask, int H, int W,
                                                         uint4* __restrict__ lvl1, int H1, int W1) {
    const int64_t n = (int64_t)H1 * W1;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int Y = (int)(i / W1), X = (int)(i - (int64_t)Y * W1);
        uint4 s = make_uint4(0, 0, 0, 0);
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int y = 2 * Y + dy, x = 2 * X + dx;
                if (y >= H || x >= W) continue;
                const int64_t p = (int64_t)y * W + x;
                if (mask[p] >= 128) continue;
                fill_acc(s, make_uint4(src[p * 3], src[p * 3 + 1], src[p * 3 + 2], 1));
            }
        lvl1[i] = s;
    }
}

__global__ __launch_bounds__(256) void fill_push_kernel(const uint4* __restrict__ child, int Hc, int Wc, uint4* __restrict__ parent, int Hp, int Wp) {
    const int64_t n = (int64_t)Hp * Wp;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int Y = (int)(i / Wp), X = (int)(i - (int64_t)Y * Wp);
        parent[i] = fill_push_cell(child, Hc, Wc, Y, X);
    }
}

// ONE block: `lvl` is a pushed level of at most kFillTopCells cells with every higher level behind it.  Finishes the push up to 1x1, then
// resolves from the top back down to `lvl`.  Each pass reads only what an earlier pass, a __syncthreads() away, has written.
__global__ __launch_bounds__(256) void fill_top_kernel(uint4* __restrict__ lvl, int H, int W) {
    // level j above `lvl` (j = 0: `lvl` itself): its sides and first cell, re-derived from H, W on every use -- uniform integer work, no table
    auto level = [&](int j, int& h, int& w) {
        uint4* at = lvl;
        h = H; w = W;
        for (; j > 0; --j) {
            at += h * w;
            h = (h + 1) >> 1;
            w = (w + 1) >> 1;
        }
        return at;
    };
    int top = 0;
    for (int h = H, w = W; h > 1 || w > 1; h = (h + 1) >> 1, w = (w + 1) >> 1) ++top;
    for (int k = 1; k <= top; ++k) {
        int hc, wc, hp, wp;
        const uint4* child = level(k - 1, hc, wc);
        uint4* parent = level(k, hp, wp);
        for (int i = threadIdx.x; i < hp * wp; i += blockDim.x) parent[i] = fill_push_cell(child, hc, wc, i / wp, i % wp);
        __syncthreads();
    }
    for (int k = top; k >= 0; --k) {
        int hk, wk, hp = 0, wp = 0;
        uint4* cur = level(k, hk, wk);
        const uint4* parent = k == top ? nullptr : level(k + 1, hp, wp);
        for (int i = threadIdx.x; i < hk * wk; i += blockDim.x) fill_resolve_cell(cur, wk, i / wk, i % wk, parent, hp, wp);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void fill_resolve_kernel(uint4* __restrict__ lvl, int Hk, int Wk, const uint4* __restrict__ parent, int Hp, int Wp) {
    const int64_t n = (int64_t)Hk * Wk;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / Wk), x = (int)(i - (int64_t)y * Wk);
        fill_resolve_cell(lvl, Wk, y, x, parent, Hp, Wp);
    }
}

// level 0: the filled image (out != NULL; parent: the resolved level 1, NULL for a 1x1 image) and the cleared edge map (ctl_out != NULL)
__global__ __launch_bounds__(256) void fill_final_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask, int H, int W,
                                                         const uint4* __restrict__ parent, int H1, int W1, uint8_t* __restrict__ out,
                                                         const uint8_t* __restrict__ ctl_in, uint8_t* __restrict__ ctl_out) {
    const int64_t n = (int64_t)H * W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool hole = mask[i] >= 128;
        if (out) {
            uint8_t r = src[i * 3], g = src[i * 3 + 1], b = src[i * 3 + 2];
            if (hole) {
                const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
                uint32_t c[3];
                fill_pull(parent, H1, W1, y, x, c);
                r = (uint8_t)((c[0] + 128u) >> 8);
                g = (uint8_t)((c[1] + 128u) >> 8);
                b = (uint8_t)((c[2] + 128u) >> 8);
            }
            out[i * 3] = r; out[i * 3 + 1] = g; out[i * 3 + 2] = b;
        }
        if (ctl_out) {
            ctl_out[i * 3] = hole ? (uint8_t)0 : ctl_in[i * 3];
            ctl_out[i * 3 + 1] = hole ? (uint8_t)0 : ctl_in[i * 3 + 1];
            ctl_out[i * 3 + 2] = hole ? (uint8_t)0 : ctl_in[i * 3 + 2];
        }
    }
}

using fie_img::grid_1d;
using fie_img::kPointwiseBlocks;

}  // namespace

extern "C" {

int64_t fie_mask_fill_workspace_bytes(int H, int W) {
    if (H < 1 || W < 1 || (int64_t)H * W > kFillMaxPixels) return -1;
    const FillPlan p = fill_plan(H, W);
    return (p.off[p.K + 1] > 0 ? p.off[p.K + 1] : 1) * (int64_t)sizeof(uint4);
}

int fie_mask_fill_rgb_u8(fie_ctx* ctx, const uint8_t* src, const uint8_t* mask_l, int H, int W, void* workspace, uint8_t* out,
                         const uint8_t* ctl_in, uint8_t* ctl_out) {
    FIE_REQUIRE(ctx && mask_l, "fie_mask_fill_rgb_u8: NULL argument");
    FIE_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= kFillMaxPixels, "fie_mask_fill_rgb_u8: %d x %d outside 1 .. 2^24 pixels", H, W);
    FIE_REQUIRE(out || ctl_out, "fie_mask_fill_rgb_u8: neither an image nor an edge map to write");
    FIE_REQUIRE(!out || (src && workspace), "fie_mask_fill_rgb_u8: the fill needs src and the workspace");
    FIE_REQUIRE(!out || (uintptr_t)workspace % 16 == 0, "fie_mask_fill_rgb_u8: the workspace must be 16-byte aligned");
    FIE_REQUIRE(!ctl_out == !ctl_in, "fie_mask_fill_rgb_u8: ctl_in and ctl_out come as a pair");
    const FillPlan p = fill_plan(H, W);
    uint4* ws = (uint4*)workspace;
    if (out && p.K > 0) {
        fie_launch(ctx, fill_push0_kernel, dim3(grid_1d((int64_t)p.h[1] * p.w[1], kPointwiseBlocks)), dim3(256), 0, src, mask_l, H, W, ws + p.off[1], p.h[1], p.w[1]);
        FIE_LAUNCH_CHECK();
        for (int k = 2; k <= p.kt; ++k) {
            fie_launch(ctx, fill_push_kernel, dim3(grid_1d((int64_t)p.h[k] * p.w[k], kPointwiseBlocks)), dim3(256), 0, (const uint4*)(ws + p.off[k - 1]), p.h[k - 1],
                       p.w[k - 1], ws + p.off[k], p.h[k], p.w[k]);
            FIE_LAUNCH_CHECK();
        }
        fie_launch(ctx, fill_top_kernel, dim3(1), dim3(256), 0, ws + p.off[p.kt], p.h[p.kt], p.w[p.kt]);
        FIE_LAUNCH_CHECK();
        for (int k = p.kt - 1; k >= 1; --k) {
            fie_launch(ctx, fill_resolve_kernel, dim3(grid_1d((int64_t)p.h[k] * p.w[k], kPointwiseBlocks)), dim3(256), 0, ws + p.off[k], p.h[k], p.w[k],
                       (const uint4*)(ws + p.off[k + 1]), p.h[k + 1], p.w[k + 1]);
            FIE_LAUNCH_CHECK();
        }
    }
    fie_launch(ctx, fill_final_kernel, dim3(grid_1d((int64_t)H * W, kPointwiseBlocks)), dim3(256), 0, src, mask_l, H, W,
               (const uint4*)(out && p.K > 0 ? ws + p.off[1] : nullptr), p.K > 0 ? p.h[1] : 0, p.K > 0 ? p.w[1] : 0, out, ctl_in, ctl_out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
