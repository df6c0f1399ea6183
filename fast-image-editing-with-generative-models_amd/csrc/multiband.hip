// One-sided multi-band paste-back of a masked edit (include/fie.h: fie_multiband_blend_rgb_u8).
//   A the decoded u8 image, S the resized source, m = (mask_l >= 128), L levels.  Gaussian pyramids of D = 16 (A - S) and G = 256 m (5x5 binomial,
//   sides ceil-halved, one rounding per level); per level the one-sided weight W = max(0, 2 G - 256); from the top down
//   C_k = ((W_k (D_k - expand(D_k+1)) + 128) >> 8) + expand(C_k+1), C_L = (W_L D_L + 128) >> 8; B = clamp(S + ((C_0 + 8) >> 4)).
//   Outside the mask and at the seam every W is 0; well inside B is A; the low-frequency difference fades out over 2^L pixels towards the seam.
// Launches: 2 L (8 at L = 4).  One reduce kernel per level k = 0 .. L-1 (three difference channels and the mask in one pass), one collapse
// kernel per level k = L-1 .. 0; the top one forms C_L from level L while it stages it, the last one runs over the image, clamps, composites
// (alpha != NULL) and stores the bytes.  Level 0 is recomputed from the images and never stored.  Levels are ordered by kernel boundaries only:
// no block waits for another, no atomics, nothing synchronises with the host, every launch goes through fie_launch.
// The arithmetic is image_ops.h's; this file is built without floating-point contraction, so that the composite is blend_u8's expression as
// written (three f32 roundings, then rintf) and a host restatement in f32 agrees with it to the bit.
#include "image_ops.h"

namespace {

using namespace fie_img;

constexpr int kBandT = 16;                      // a block's tile: kBandT x kBandT cells of the level it writes, one per thread
constexpr int kBandF = 2 * kBandT + 3;          // reduce: the footprint of a tile in the level below, per axis
constexpr int kBandP = kBandT / 2 + 2;          // collapse: the tile's parents plus one clamped neighbour on each side, per axis
constexpr int64_t kBandMaxPixels = (int64_t)1 << 24;

// levels 1 .. L above the image: sides and first cell (levels lie back to back, level 1 first).  The workspace holds the C levels as int4
// in front (16-byte cells from a 16-byte-aligned base), then the {D, G} levels as short4.
struct BandPlan {
    int h[kBandMaxLevels + 1], w[kBandMaxLevels + 1];
    int64_t off[kBandMaxLevels + 2];            // off[k]: first cell of level k >= 1; off[L + 1]: cells in all
};

BandPlan band_plan(int H, int W, int levels) {
    BandPlan p;
    p.h[0] = H; p.w[0] = W;
    p.off[0] = p.off[1] = 0;
    for (int k = 1; k <= levels; ++k) {
        p.h[k] = (p.h[k - 1] + 1) >> 1;
        p.w[k] = (p.w[k - 1] + 1) >> 1;
        p.off[k + 1] = p.off[k] + (int64_t)p.h[k] * p.w[k];
    }
    return p;
}

bool band_supported(int H, int W, int levels) {
    return H >= 1 && W >= 1 && (int64_t)H * W <= kBandMaxPixels && levels >= 1 && levels <= kBandMaxLevels;
}

unsigned band_tiles(int h, int w) { return (unsigned)(((h + kBandT - 1) / kBandT) * (int64_t)((w + kBandT - 1) / kBandT)); }

__device__ __forceinline__ int4 band_load(const short4* __restrict__ lvl, int64_t i) {
    const short4 v = lvl[i];
    return make_int4(v.x, v.y, v.z, v.w);
}

// the tile of this block in a [h][w] level: first row and column
__device__ __forceinline__ void band_tile_origin(int w, int& y0, int& x0) {
    const int tiles_x = (w + kBandT - 1) / kBandT;
    const int ty = (int)(blockIdx.x / tiles_x);
    y0 = ty * kBandT;
    x0 = (int)(blockIdx.x - (unsigned)ty * tiles_x) * kBandT;
}

// parent = reduce(child).  kImage: the child is level 0, formed from the images; else the stored level `child`.  A block stages the
// (2T+3)^2 footprint of its T x T outputs once (indices clamped to the child), runs the horizontal pass over every staged row, then the vertical.
template <bool kImage>
__global__ __launch_bounds__(256) void band_reduce_kernel(const uint8_t* __restrict__ edit, const uint8_t* __restrict__ source,
                                                          const uint8_t* __restrict__ mask, const short4* __restrict__ child, int h, int w,
                                                          short4* __restrict__ parent, int hp, int wp) {
    __shared__ int4 foot[kBandF * kBandF];
    __shared__ int4 hrow[kBandF * kBandT];
    const int tid = threadIdx.x;
    int Y0, X0;
    band_tile_origin(wp, Y0, X0);
    for (int i = tid; i < kBandF * kBandF; i += 256) {
        const int r = i / kBandF, c = i - r * kBandF;
        const int gy = min(max(2 * Y0 - 2 + r, 0), h - 1), gx = min(max(2 * X0 - 2 + c, 0), w - 1);
        const int64_t p = (int64_t)gy * w + gx;
        foot[i] = kImage ? band_level0(edit + p * 3, source + p * 3, mask[p]) : band_load(child, p);
    }
    __syncthreads();
    for (int i = tid; i < kBandF * kBandT; i += 256) {
        const int r = i / kBandT, c = i - r * kBandT;
        hrow[i] = band_reduce5(foot + r * kBandF + 2 * c, 1);
    }
    __syncthreads();
    const int ly = tid / kBandT, lx = tid - ly * kBandT;
    const int Y = Y0 + ly, X = X0 + lx;
    if (Y >= hp || X >= wp) return;
    const int4 s = band_reduce5(hrow + 2 * ly * kBandT + lx, kBandT);
    parent[(int64_t)Y * wp + X] = make_short4((short)band_reduce_round(s.x), (short)band_reduce_round(s.y), (short)band_reduce_round(s.z),
                                              (short)band_reduce_round(s.w));
}

// C_k of one level from {D, G}_k, {D, G}_k+1 and C_k+1 (c_up; NULL at the top: C_k+1 = C_L is formed from level L as it is staged).
// kImage: level k is the image -- {D, G}_0 from edit / source / mask, the result clamped, composited with alpha (unless NULL) and stored as bytes;
// else {D, G}_k is `lvl` and C_k goes to c_out.  h, w: level k; hp, wp: level k + 1.
template <bool kImage>
__global__ __launch_bounds__(256) void band_collapse_kernel(const uint8_t* __restrict__ edit, const uint8_t* __restrict__ source,
                                                            const uint8_t* __restrict__ mask, const float* __restrict__ alpha,
                                                            const short4* __restrict__ lvl, int h, int w, const short4* __restrict__ up,
                                                            const int4* __restrict__ c_up, int hp, int wp, int4* __restrict__ c_out,
                                                            uint8_t* __restrict__ out) {
    __shared__ int4 pd[kBandP * kBandP];        // D_k+1 around the tile's parents
    __shared__ int4 pc[kBandP * kBandP];        // C_k+1
    const int tid = threadIdx.x;
    int y0, x0;
    band_tile_origin(w, y0, x0);
    for (int i = tid; i < kBandP * kBandP; i += 256) {
        const int r = i / kBandP, c = i - r * kBandP;
        const int gy = min(max(y0 / 2 - 1 + r, 0), hp - 1), gx = min(max(x0 / 2 - 1 + c, 0), wp - 1);
        const int64_t q = (int64_t)gy * wp + gx;
        const int4 d = band_load(up, q);
        pd[i] = d;
        if (c_up) {
            pc[i] = c_up[q];
        } else {
            const int wt = band_weight(d.w);
            pc[i] = make_int4(band_mix(wt, d.x), band_mix(wt, d.y), band_mix(wt, d.z), 0);
        }
    }
    __syncthreads();
    const int ly = tid / kBandT, lx = tid - ly * kBandT;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= h || x >= w) return;
    const int64_t p = (int64_t)y * w + x;
    int wy[3], wx[3], ed[3], ec[3];
    band_expand_weights(y, wy);
    band_expand_weights(x, wx);
    const int centre = ((ly >> 1) + 1) * kBandP + (lx >> 1) + 1;
    band_expand3(pd + centre, kBandP, wy, wx, ed);
    band_expand3(pc + centre, kBandP, wy, wx, ec);
    const int4 d = kImage ? band_level0(edit + p * 3, source + p * 3, mask[p]) : band_load(lvl, p);
    const int wt = band_weight(d.w);
    const int c0 = band_mix(wt, d.x - ed[0]) + ec[0], c1 = band_mix(wt, d.y - ed[1]) + ec[1], c2 = band_mix(wt, d.z - ed[2]) + ec[2];
    if (kImage) {
        const float* m = alpha ? alpha + p : nullptr;
        const uint8_t r = band_out(source[p * 3], c0, m), g = band_out(source[p * 3 + 1], c1, m), b = band_out(source[p * 3 + 2], c2, m);
        out[p * 3] = r; out[p * 3 + 1] = g; out[p * 3 + 2] = b;
    } else {
        c_out[p] = make_int4(c0, c1, c2, 0);
    }
}

}  // namespace

extern "C" {

int64_t fie_multiband_workspace_bytes(int H, int W, int levels) {
    if (!band_supported(H, W, levels)) return -1;
    const BandPlan p = band_plan(H, W, levels);
    return p.off[levels + 1] * (int64_t)(sizeof(int4) + sizeof(short4));
}

int fie_multiband_blend_rgb_u8(fie_ctx* ctx, const uint8_t* edit, const uint8_t* source, const uint8_t* mask_l, const float* alpha, int H, int W,
                               int levels, void* workspace, uint8_t* out) {
    FIE_REQUIRE(ctx && edit && source && mask_l && workspace && out, "fie_multiband_blend_rgb_u8: NULL argument");
    FIE_REQUIRE(levels >= 1 && levels <= kBandMaxLevels, "fie_multiband_blend_rgb_u8: levels %d outside 1 .. %d", levels, kBandMaxLevels);
    FIE_REQUIRE(band_supported(H, W, levels), "fie_multiband_blend_rgb_u8: %d x %d outside 1 .. 2^24 pixels", H, W);
    FIE_REQUIRE((uintptr_t)workspace % 16 == 0, "fie_multiband_blend_rgb_u8: the workspace must be 16-byte aligned");
    FIE_REQUIRE(!alpha || (uintptr_t)alpha % 4 == 0, "fie_multiband_blend_rgb_u8: alpha must be 4-byte aligned");
    const BandPlan p = band_plan(H, W, levels);
    int4* cws = (int4*)workspace;
    short4* dws = (short4*)(cws + p.off[levels + 1]);
    const int L = levels;
    FIE_DESC(ctx, "multiband_blend %dx%d L=%d", H, W, L);
    fie_launch(ctx, band_reduce_kernel<true>, dim3(band_tiles(p.h[1], p.w[1])), dim3(256), 0, edit, source, mask_l, (const short4*)nullptr, H, W,
               dws + p.off[1], p.h[1], p.w[1]);
    FIE_LAUNCH_CHECK();
    for (int k = 1; k < L; ++k) {
        fie_launch(ctx, band_reduce_kernel<false>, dim3(band_tiles(p.h[k + 1], p.w[k + 1])), dim3(256), 0, (const uint8_t*)nullptr,
                   (const uint8_t*)nullptr, (const uint8_t*)nullptr, (const short4*)(dws + p.off[k]), p.h[k], p.w[k], dws + p.off[k + 1], p.h[k + 1],
                   p.w[k + 1]);
        FIE_LAUNCH_CHECK();
    }
    for (int k = L - 1; k >= 1; --k) {
        fie_launch(ctx, band_collapse_kernel<false>, dim3(band_tiles(p.h[k], p.w[k])), dim3(256), 0, (const uint8_t*)nullptr, (const uint8_t*)nullptr,
                   (const uint8_t*)nullptr, (const float*)nullptr, (const short4*)(dws + p.off[k]), p.h[k], p.w[k], (const short4*)(dws + p.off[k + 1]),
                   (const int4*)(k + 1 == L ? nullptr : cws + p.off[k + 1]), p.h[k + 1], p.w[k + 1], cws + p.off[k], (uint8_t*)nullptr);
        FIE_LAUNCH_CHECK();
    }
    fie_launch(ctx, band_collapse_kernel<true>, dim3(band_tiles(H, W)), dim3(256), 0, edit, source, mask_l, alpha, (const short4*)nullptr, H, W,
               (const short4*)(dws + p.off[1]), (const int4*)(L == 1 ? nullptr : cws + p.off[1]), p.h[1], p.w[1], (int4*)nullptr, out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
