// Full-resolution back end of an edit (include/fie.h: fie_fullres_paste_rgb_u8): the edit-size u8 result goes to the
// source's resolution (Pillow's 8-bit LANCZOS, as csrc/resize.hip) and is composited there against the source's own bytes through the
// binarised, optionally feathered source-size mask (as mask_prep_kernel and pixels_out_composite_kernel, csrc/mask.hip).  The resample, the
// feather and the blend are the functions of csrc/image_ops.h that those kernels call too.
//   launch 1   the horizontal resample of the result into tmp [h, W, 3] (fie_resize_rgb_u8 on one axis), when the width changes;
//   launch 2   one kernel over 64 x 16 output tiles: binary mask + clamped R-halo in LDS, the two feather passes, the vertical resample of
//              the tile's columns from tmp, the blend, the store.
// Neither the f32 mask nor the up-sampled image exists in memory at the output's resolution: per output pixel the kernel reads 1 mask byte,
// 3 source bytes and the taps' rows of tmp, and writes 3 bytes.  A tile whose staged mask (halo included) is all zero copies the source.
#include "image_ops.h"

namespace {

using namespace fie_img;

constexpr int kTW = 64, kTH = 16;               // output pixels per workgroup: one wave per tile row, four rows per wave
constexpr int kMaxRadius = 64;                  // LDS at R = 64: 144 x 192 mask bytes + 144 x 64 floats = 63 KB
constexpr int kRowBytes = kTW * 3;
constexpr int kSlots = kRowBytes / 4 + 2;       // 4-byte words a tile row can touch in memory, whatever its alignment

struct FullresArgs {
    const uint8_t* vin;        // [h, W, 3]: the result after the horizontal pass
    int h;
    const int* ky; const int* by; int ksy;      // NULL / 0: h == H
    const uint8_t* source; int64_t source_pitch;
    const uint8_t* mask; int64_t mask_pitch;    // NULL: a pure resize
    const float* taps; int R;
    uint8_t* dst; int64_t dst_pitch;
    int H, W;
};

// rows x nb bytes between a pitched image and the LDS tile [kTH][kRowBytes].  Memory is accessed in aligned 4-byte words where all four
// bytes belong to the tile's row and byte by byte at its two ends: right for any pitch and any byte offset, and no byte outside
// the row is read or written.
template <bool kStore>
__device__ __forceinline__ void tile_io(uint8_t* lds, uint8_t* base, int64_t pitch, int rows, int nb, int tid) {
    for (int i = tid; i < kTH * kSlots; i += 256) {
        const int r = i / kSlots, j = i - r * kSlots;
        if (r >= rows) break;
        uint8_t* g = base + (int64_t)r * pitch;
        const int lo = 4 * j - (int)(reinterpret_cast<uintptr_t>(g) & 3);
        if (lo >= nb) continue;
        uint8_t* l = lds + r * kRowBytes;
        if (lo >= 0 && lo + 4 <= nb) {
            uint32_t* gw = reinterpret_cast<uint32_t*>(g + lo);
            if (kStore) {
                *gw = (uint32_t)l[lo] | ((uint32_t)l[lo + 1] << 8) | ((uint32_t)l[lo + 2] << 16) | ((uint32_t)l[lo + 3] << 24);
            } else {
                const uint32_t v = *gw;
                l[lo] = (uint8_t)v; l[lo + 1] = (uint8_t)(v >> 8); l[lo + 2] = (uint8_t)(v >> 16); l[lo + 3] = (uint8_t)(v >> 24);
            }
        } else {
            for (int k = lo < 0 ? -lo : 0; k < 4 && lo + k < nb; ++k) {
                if (kStore) g[lo + k] = l[lo + k];
                else l[lo + k] = g[lo + k];
            }
        }
    }
}

__global__ __launch_bounds__(256) void fullres_paste_kernel(FullresArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fr_smem[];
    const int R = p.R, BW = kTW + 2 * R, BH = kTH + 2 * R;
    const int bin_bytes = max(BW * BH, kTH * kRowBytes);
    uint8_t* bin = fr_smem;                                                      // [BH][BW]; dead after the horizontal pass, then:
    uint8_t* io = fr_smem;                                                       // [kTH][kRowBytes] source bytes in, output bytes out
    float* hrow = reinterpret_cast<float*>(fr_smem + ((bin_bytes + 15) & ~15));  // [BH][kTW]
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH, tid = threadIdx.x;
    const int cols = min(kTW, p.W - x0), rows = min(kTH, p.H - y0), nb = cols * 3;
    uint8_t* src_tile = const_cast<uint8_t*>(p.source) + (int64_t)y0 * p.source_pitch + (int64_t)x0 * 3;
    uint8_t* dst_tile = p.dst + (int64_t)y0 * p.dst_pitch + (int64_t)x0 * 3;

    if (p.mask) {
        // block-uniform: no bit staged (halo included) means the feather is 0 on the whole tile, the output is the source
        if (!__syncthreads_or(feather_stage<kTW, kTH>(bin, p.mask, p.mask_pitch, p.H, p.W, x0, y0, R, tid))) {
            tile_io<false>(io, src_tile, p.source_pitch, rows, nb, tid);
            __syncthreads();
            tile_io<true>(io, dst_tile, p.dst_pitch, rows, nb, tid);
            return;
        }
        feather_hpass<kTW, kTH>(hrow, bin, p.taps, R, tid);
        __syncthreads();
        tile_io<false>(io, src_tile, p.source_pitch, rows, nb, tid);
        __syncthreads();
    }

    const int tx = tid & (kTW - 1);
    for (int ty = tid / kTW; ty < kTH; ty += 256 / kTW) {
        const int y = y0 + ty, x = x0 + tx;
        if (y >= p.H || x >= p.W) continue;
        float m = 1.f;
        if (p.mask) {
            m = feather_vsum<kTW>(hrow, p.taps, R, tx, ty);
            if (m <= 0.f) continue;               // io already holds the source bytes
        }
        int up[3];
        if (p.ky) {                               // the vertical pass of this pixel's column, as resize_v_kernel runs it
            const int ymin = p.by[2 * y], n = p.by[2 * y + 1];
            const int* k = p.ky + (int64_t)y * p.ksy;
            const uint8_t* col = p.vin + ((int64_t)ymin * p.W + x) * 3;
            int s[3] = {kResampleHalf, kResampleHalf, kResampleHalf};
            for (int t = 0; t < n; ++t) resample_tap<3>(s, col + (int64_t)t * p.W * 3, k[t]);
#pragma unroll
            for (int c = 0; c < 3; ++c) up[c] = resample_clip8(s[c]);
        } else {
            const uint8_t* px = p.vin + ((int64_t)y * p.W + x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) up[c] = px[c];
        }
        uint8_t* o = io + ty * kRowBytes + tx * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = blend_u8(m, (float)up[c], o[c]);
    }
    __syncthreads();
    tile_io<true>(io, dst_tile, p.dst_pitch, rows, nb, tid);
}

}  // namespace

extern "C" int fie_fullres_paste_rgb_u8(fie_ctx* ctx, const uint8_t* res, int h, int w, const uint8_t* source, int64_t source_pitch,
                                        const uint8_t* mask_l, int64_t mask_pitch, int H, int W, const int* kx, const int* bx, int ksx,
                                        const int* ky, const int* by, int ksy, const float* taps, int radius, uint8_t* dst,
                                        int64_t dst_pitch, uint8_t* tmp) {
    const char* name = "fie_fullres_paste_rgb_u8";
    FIE_REQUIRE(ctx && res && dst && h > 0 && w > 0 && H > 0 && W > 0, "%s: bad argument", name);
    FIE_REQUIRE((w == W || (kx && bx && ksx > 0)) && (h == H || (ky && by && ksy > 0)), "%s: missing coefficient table", name);
    FIE_REQUIRE(w == W || tmp, "%s: a change of width needs the [h, W, 3] scratch image", name);
    FIE_REQUIRE(dst_pitch >= (int64_t)W * 3, "%s: dst pitch %lld below the row's %lld bytes", name, (long long)dst_pitch, (long long)W * 3);
    if (mask_l) {
        FIE_REQUIRE(source && taps, "%s: a mask needs the source image and the feather's taps", name);
        FIE_REQUIRE(source_pitch >= (int64_t)W * 3 && mask_pitch >= W, "%s: source / mask pitch below the row's bytes", name);
        FIE_REQUIRE(radius >= 0 && radius <= kMaxRadius, "%s: radius %d outside [0, %d]", name, radius, kMaxRadius);
    }
    const uint8_t* vin = res;
    if (w != W) {                          // horizontal pass first, as Pillow does: the existing kernel, one axis
        const int rc = fie_resize_rgb_u8(ctx, res, h, w, tmp, h, W, kx, bx, ksx, nullptr, nullptr, 0, nullptr);
        if (rc != FIE_OK) return rc;
        vin = tmp;
    }
    const int R = mask_l ? radius : 0;
    FullresArgs p = {vin, h, h == H ? nullptr : ky, h == H ? nullptr : by, h == H ? 0 : ksy, source, source_pitch, mask_l, mask_pitch,
                     taps, R, dst, dst_pitch, H, W};
    const int64_t BW = kTW + 2 * R, BH = kTH + 2 * R;
    const int64_t bin_bytes = BW * BH > (int64_t)kTH * kRowBytes ? BW * BH : (int64_t)kTH * kRowBytes;
    const unsigned lds = (unsigned)(fie_roundup(bin_bytes, 16) + (mask_l ? BH * kTW * (int64_t)sizeof(float) : 0));
    FIE_DESC(ctx, "fullres_paste %dx%d -> %dx%d R=%d%s", h, w, H, W, R, mask_l ? "" : " (no mask)");
    fie_launch(ctx, fullres_paste_kernel, dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH), dim3(256), lds, p);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}
