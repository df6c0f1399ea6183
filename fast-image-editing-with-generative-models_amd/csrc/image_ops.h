// The arithmetic the image-side kernels share, stated once (resize, mask, mask_fill, multiband, fullres, outpaint, tile_blend, metrics, clip_score, dino, lpips, pointwise .hip).
// Kernels that must agree bit for bit -- the fused full-resolution paste with the resize + mask_prep + composite sequence, the two patchify
// kernels with each other's K order -- agree because they call the same function here, not because one restates the other.
#pragma once
#include "fie_internal.h"

namespace fie_img {

// ---------------------------------------------------------------------------------------------------------------- launch sizing
// Blocks of 256 threads for a grid-stride loop over `items`: at most `cap`, at least 1
constexpr int kPointwiseBlocks = 2048;      // the pointwise / mask / fill kernels
constexpr int kPatchBlocks = 4096;          // the CLIP / DINO preprocessing kernels
inline unsigned grid_1d(int64_t items, int64_t cap) {
    const int64_t g = (items + 255) / 256;
    return (unsigned)(g > cap ? cap : (g < 1 ? 1 : g));
}

// The sum of a wave's 64 lanes in lane 0, by a fixed shuffle tree (float, double, uint32_t): lanes first, the caller adds waves in wave order
template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- Pillow's 8-bit resample
// src/libImaging/Resample.c: 22-bit fixed-point coefficients; one output pixel of a pass starts from one half, adds its taps, is shifted
// back and clipped to u8.  The start, the tap and the clip are shared; the loop over the taps stays in each kernel with that kernel's own
// index expression, because the compiler's unrolling (and with it the register count: 11 -> 22 in resize_v_kernel<3>) follows its shape.
constexpr int kResampleBits = 32 - 8 - 2;
constexpr int kResampleHalf = 1 << (kResampleBits - 1);

template <int C>
__device__ __forceinline__ void resample_tap(int (&s)[C], const uint8_t* px, int w) {
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] += px[c] * w;
}

__device__ __forceinline__ uint8_t resample_clip8(int v) {
    v >>= kResampleBits;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---------------------------------------------------------------------------------------------------------------- the feather
// Separable Gaussian over the binarised mask (L >= 128), clamp-to-edge, for a TW x TH tile of output pixels at (x0, y0) and 256 threads:
// stage -> barrier -> hpass -> barrier -> vsum per pixel.  Both passes add their taps k = 0 .. 2R in f32, as a host restatement does.

// bin [TH + 2R][TW + 2R]: the tile's binary mask with its clamped R-halo.  Returns this thread's OR of the bits it staged.  Pitch is the
// caller's own type (int for a dense mask, int64_t for a pitched one), so that each caller's address arithmetic compiles as it did.
template <int TW, int TH, typename Pitch>
__device__ __forceinline__ int feather_stage(uint8_t* __restrict__ bin, const uint8_t* __restrict__ mask, Pitch pitch, int H, int W, int x0, int y0, int R, int tid) {
    const int BW = TW + 2 * R, BH = TH + 2 * R;
    int any = 0;
    for (int i = tid; i < BW * BH; i += 256) {
        const int r = i / BW, c = i - r * BW;
        const int gy = min(max(y0 - R + r, 0), H - 1), gx = min(max(x0 - R + c, 0), W - 1);
        const uint8_t b = mask[(int64_t)gy * pitch + gx] >= 128 ? 1 : 0;
        bin[i] = b;
        any |= b;
    }
    return any;
}

// hrow [TH + 2R][TW]: the horizontal pass over every staged row
template <int TW, int TH>
__device__ __forceinline__ void feather_hpass(float* __restrict__ hrow, const uint8_t* __restrict__ bin, const float* __restrict__ taps, int R, int tid) {
    const int BW = TW + 2 * R, BH = TH + 2 * R;
    for (int i = tid; i < BH * TW; i += 256) {
        const int r = i / TW, c = i - r * TW;
        const uint8_t* row = bin + r * BW + c;
        float s = 0.f;
        for (int k = 0; k <= 2 * R; ++k) s += taps[k] * (float)row[k];
        hrow[i] = s;
    }
}

// the feathered mask of tile pixel (tx, ty): the vertical pass over hrow
template <int TW>
__device__ __forceinline__ float feather_vsum(const float* __restrict__ hrow, const float* __restrict__ taps, int R, int tx, int ty) {
    float s = 0.f;
    for (int k = 0; k <= 2 * R; ++k) s += taps[k] * hrow[(ty + k) * TW + tx];
    return s;
}

// ---------------------------------------------------------------------------------------------------------------- byte rows at any address
// Rows of u8 pixels start wherever the rows before them end (outpaint, tile_blend .hip): a row is stored as a head of 0 .. 3 bytes up to the next
// dword boundary of its ADDRESS, a body of whole aligned dwords and a tail of 0 .. 3 bytes, and read through aligned dwords likewise.

// where a row of `len` bytes at address `row` splits: `head` bytes in front of the first aligned dword, `body` whole dwords behind them
__device__ __forceinline__ void row_split(const uint8_t* row, int64_t len, int& head, int64_t& body) {
    const int64_t h = (int64_t)((0 - (uintptr_t)row) & 3);
    head = (int)(h < len ? h : len);
    body = (len - head) >> 2;
}

// the four bytes at `a` (any alignment) of an operand that spans [lo, hi), as one little-endian dword: from the aligned dwords that cover them
// when those lie inside the operand, else by bytes
__device__ __forceinline__ uint32_t load4(const uint8_t* a, const uint8_t* lo, const uint8_t* hi) {
    const unsigned sh = (unsigned)((uintptr_t)a & 3);
    const uint8_t* al = a - sh;
    if (sh == 0) return *reinterpret_cast<const uint32_t*>(a);
    if (al >= lo && al + 8 <= hi) {
        const uint32_t* d = reinterpret_cast<const uint32_t*>(al);
        return __builtin_amdgcn_alignbyte(d[1], d[0], sh);
    }
    return (uint32_t)a[0] | (uint32_t)a[1] << 8 | (uint32_t)a[2] << 16 | (uint32_t)a[3] << 24;
}

// ---------------------------------------------------------------------------------------------------------------- the u8 blend
// The paste-back of one byte: the source where m <= 0, the result d (in [0, 255]) where m >= 1, rint(m d + (1 - m) s) between
__device__ __forceinline__ uint8_t blend_u8(float m, float d, uint8_t s) {
    const float sf = (float)s;
    return m <= 0.f ? s : (uint8_t)rintf(m >= 1.f ? d : m * d + (1.f - m) * sf);
}

// ---------------------------------------------------------------------------------------------------------------- the multi-band blend
// One-sided Laplacian-pyramid paste-back (tests/multiband_oracle.py restates it).  Signed 32-bit integers throughout:
// a cell is an int4 {D_r, D_g, D_b, G} (difference edit - source in 1/16 levels, mask in 1/256) or {C_r, C_g, C_b, -} (the collapsed bands).
// |D| <= 4080 and 0 <= G <= 256, so a level is stored as short4; |Lap| <= 8160, every product and sum stays under 2^23.  >> floors.
constexpr int kBandMaxLevels = 6;

// level 0, never stored: D_0 = 16 (A - S), G_0 = 256 m
__device__ __forceinline__ int4 band_level0(const uint8_t* a, const uint8_t* s, uint8_t mask_l) {
    return make_int4(16 * ((int)a[0] - (int)s[0]), 16 * ((int)a[1] - (int)s[1]), 16 * ((int)a[2] - (int)s[2]), mask_l >= 128 ? 256 : 0);
}

// reduce: one axis of the 1-4-6-4-1 binomial over p[0], p[stride], .. p[4 stride]; the 2-D sum (two such passes) is rounded once
__device__ __forceinline__ int4 band_reduce5(const int4* p, int stride) {
    const int4 a = p[0], b = p[stride], c = p[2 * stride], d = p[3 * stride], e = p[4 * stride];
    return make_int4(a.x + 4 * b.x + 6 * c.x + 4 * d.x + e.x, a.y + 4 * b.y + 6 * c.y + 4 * d.y + e.y, a.z + 4 * b.z + 6 * c.z + 4 * d.z + e.z,
                     a.w + 4 * b.w + 6 * c.w + 4 * d.w + e.w);
}
__device__ __forceinline__ int band_reduce_round(int sum) { return (sum + 128) >> 8; }

// expand: the weights of one axis for output index i over the parents (i >> 1) - 1, i >> 1, (i >> 1) + 1 -- 1 6 1 at even i, 4 4 at odd
__device__ __forceinline__ void band_expand_weights(int i, int (&wt)[3]) {
    wt[0] = (i & 1) ? 0 : 1;
    wt[1] = (i & 1) ? 4 : 6;
    wt[2] = (i & 1) ? 4 : 1;
}
// the expanded value's three channels; `centre`: the parent cell (y >> 1, x >> 1) in a staged tile of `pitch` cells a row whose halo
// holds the clamped neighbours
__device__ __forceinline__ void band_expand3(const int4* centre, int pitch, const int (&wy)[3], const int (&wx)[3], int (&e)[3]) {
    int s[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int4 v = centre[(a - 1) * pitch + (b - 1)];
            const int wt = wy[a] * wx[b];
            s[0] += wt * v.x; s[1] += wt * v.y; s[2] += wt * v.z;
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) e[c] = (s[c] + 32) >> 6;
}

// the one-sided ramp W = max(0, 2 G - 256) and a band weighted by it
__device__ __forceinline__ int band_weight(int g) { return max(0, 2 * g - 256); }
__device__ __forceinline__ int band_mix(int wt, int v) { return (wt * v + 128) >> 8; }

// one byte of the result: B = clamp(S + ((C_0 + 8) >> 4), 0, 255), or with the feathered mask m the paste-back of B
__device__ __forceinline__ uint8_t band_out(uint8_t s, int c0, const float* m) {
    const int b = min(max((int)s + ((c0 + 8) >> 4), 0), 255);
    return m ? blend_u8(*m, (float)b, s) : (uint8_t)b;
}

// ---------------------------------------------------------------------------------------------------------------- patchify
// Row r = (image, patch) of a patchified image is the patch in the K order of the patch-embedding weight [C, 3, ps, ps] viewed as
// [C, 3 ps ps]: k = (c ps + py) ps + px.  One work item = 16 contiguous output bytes = E consecutive px of one patch row and channel.
struct ChannelNorm { float mean[3], std[3]; };

// fills `nm` from the caller's mean / std; `entry` names the C entry in the error text
inline int channel_norm(const char* entry, const float* mean, const float* std, ChannelNorm* nm) {
    for (int c = 0; c < 3; ++c) {
        FIE_REQUIRE(std[c] != 0.f, "%s: image_std[%d] is 0", entry, c);
        nm->mean[c] = mean[c]; nm->std[c] = std[c];
    }
    return FIE_OK;
}

// v[c] as selects over three values (indexing a kernel argument by a run-time c would send it through memory)
__device__ __forceinline__ float channel_pick(float v0, float v1, float v2, int c) { return c == 0 ? v0 : (c == 1 ? v1 : v2); }

struct PatchItem {
    int64_t row;          // image * P + patch
    int k0;               // first of the item's E columns of the row
    int b, gy, gx;        // image, patch position in the grid
    int c, py, px;        // channel, pixel position in the patch
};

// work item i of n * P * nch, nch = 3 ps ps / E items per row
template <int E>
__device__ __forceinline__ PatchItem patch_item(int64_t i, int nch, int P, int grid_w, int ps) {
    const int64_t row = i / nch;
    const int k0 = (int)(i - row * nch) * E;
    const int b = (int)(row / P), p = (int)(row % P);
    const int gy = p / grid_w, gx = p - gy * grid_w;
    const int c = k0 / (ps * ps), rem = k0 - c * ps * ps;
    const int py = rem / ps, px = rem - py * ps;
    return {row, k0, b, gy, gx, c, py, px};
}

}  // namespace fie_img
