// Mask-restricted edits (include/fie.h: fie_mask_prep, fie_mask_levels_u8, fie_mask_support_u8, fie_pixels_out_composite_*).
// The semantics are those of the diffusers inpaint pipelines for a 4-channel UNet layered on the img2img edit:
//   mask prep   binarise the edit-size u8 mask (L >= 128), nearest latent downsample m_lat[y][x] = m_px[8y][8x], optional separable
//               Gaussian feather of m_px (sigma r, radius R = ceil(3r), clamp-to-edge) for the paste-back;
//   latent prep, LCM step   the Z0 and BLEND instantiations of the kernels every edit runs (csrc/lcm.hip): the clean source latent z0 is kept,
//               and per latent pixel lat = inside ? lat : (sab_prev z0 + s1mab_prev n_init), or z0 on the last step;
//   composite   pixels_out, then the source u8 where m == 0, the decoded byte where m == 1, rint(m d + (1-m) src) between.
// Soft masks: the latent mask holds levels v in 0 .. 255, which fie_mask_levels_u8 reads off the level map; the step
// that compares them is csrc/lcm.hip's too.  pixels_out_kernel (pointwise.hip) is untouched: an unmasked edit decodes exactly as it did.
#include "image_ops.h"

namespace {

using namespace fie_img;

constexpr int kMaskTile = 16;          // 16 x 16 output pixels per workgroup
constexpr int kMaskMaxRadius = 64;     // LDS: (16 + 2R)^2 bytes of binary mask + (16 + 2R) x 16 floats of the horizontal pass

// One launch: binarise, latent downsample and the feather (R = 0: taps = {1}, m_px is the binary mask).  The binary mask of the tile
// and its clamped R-halo is staged in LDS; the horizontal pass runs over every staged row, the vertical pass over its result: the
// separable filter in the order a host restatement computes it (taps summed k = 0 .. 2R in f32): csrc/image_ops.h's feather, which the
// fused paste of csrc/fullres.hip runs on its own tiles.
__global__ __launch_bounds__(256) void mask_prep_kernel(const uint8_t* __restrict__ L, int H, int W, const float* __restrict__ taps, int R,
                                                        float* __restrict__ m_px, uint8_t* __restrict__ m_lat) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mp_smem[];
    const int T = kMaskTile + 2 * R;
    uint8_t* bin = mp_smem;                                              // [T][T]
    float* hrow = reinterpret_cast<float*>(mp_smem + ((T * T + 15) & ~15));   // [T][16]
    const int x0 = blockIdx.x * kMaskTile, y0 = blockIdx.y * kMaskTile, tid = threadIdx.x;
    feather_stage<kMaskTile, kMaskTile>(bin, L, W, H, W, x0, y0, R, tid);
    __syncthreads();
    feather_hpass<kMaskTile, kMaskTile>(hrow, bin, taps, R, tid);
    __syncthreads();
    const int ty = tid / kMaskTile, tx = tid - ty * kMaskTile;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
    m_px[(int64_t)y * W + x] = feather_vsum<kMaskTile>(hrow, taps, R, tx, ty);
    if ((y & 7) == 0 && (x & 7) == 0) m_lat[(int64_t)(y >> 3) * (W >> 3) + (x >> 3)] = bin[(ty + R) * T + tx + R];
}

// Four pixels per thread: the mask as one float4, source and output as three 4-byte words (npix % 4 == 0: H, W are multiples of 8)
template <typename T>
__global__ void pixels_out_composite_kernel(const T* src, int64_t ld, int64_t nquad, const uint8_t* source, const float* mask, uint8_t* dst) {
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 m4 = *reinterpret_cast<const float4*>(mask + q * 4);
        const uint32_t* sw = reinterpret_cast<const uint32_t*>(source + q * 12);
        uint32_t in[3] = {sw[0], sw[1], sw[2]}, out[3] = {0, 0, 0};
        const uint8_t* sb = reinterpret_cast<const uint8_t*>(in);
        uint8_t* ob = reinterpret_cast<uint8_t*>(out);
        const float* mp = &m4.x;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int64_t i = q * 4 + p;
            const float m = mp[p];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float x = (float)src[i * ld + c] * 0.5f + 0.5f;
                x = fminf(fmaxf(x, 0.f), 1.f);
                const float d = x * 255.0f;
                ob[p * 3 + c] = blend_u8(m, d, sb[p * 3 + c]);
            }
        }
        uint32_t* dw = reinterpret_cast<uint32_t*>(dst + q * 12);
        dw[0] = out[0]; dw[1] = out[1]; dw[2] = out[2];
    }
}

// The latent levels of a soft mask: lvl_lat = mask_lat ? max(levels[8y][8x], 1) : 0 -- the support stays fie_mask_prep's mask_lat bit for bit
__global__ void mask_levels_kernel(const uint8_t* __restrict__ levels, const uint8_t* __restrict__ m_lat, int lh, int lw, int W,
                                   uint8_t* __restrict__ lvl_lat) {
    const int n = lh * lw;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int y = i / lw, x = i - y * lw;
        const uint8_t v = levels[(int64_t)(8 * y) * W + 8 * x];
        lvl_lat[i] = m_lat[i] ? (v ? v : (uint8_t)1) : (uint8_t)0;
    }
}

// The support of a level map: 255 where the level is > 0
__global__ void mask_support_kernel(const uint8_t* __restrict__ levels, int64_t n, uint8_t* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = levels[i] ? 255 : 0;
}

template <typename T>
int pixels_out_composite_t(fie_ctx* ctx, const void* src, int64_t ld_in, int H, int W, const uint8_t* source, const float* mask, uint8_t* dst) {
    FIE_REQUIRE(ctx && src && source && mask && dst && H > 0 && W > 0 && ld_in >= 3, "fie_pixels_out_composite: bad argument");
    const int64_t n = (int64_t)H * W;
    FIE_REQUIRE(n % 4 == 0, "fie_pixels_out_composite: H*W must be a multiple of 4");
    FIE_REQUIRE(((uintptr_t)source | (uintptr_t)dst) % 4 == 0 && (uintptr_t)mask % 16 == 0, "fie_pixels_out_composite: misaligned buffer");
    fie_launch(ctx, pixels_out_composite_kernel<T>, dim3(grid_1d(n / 4, kPointwiseBlocks)), dim3(256), 0, (const T*)src, ld_in, n / 4, source, mask, dst);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // namespace

extern "C" {

int fie_mask_prep(fie_ctx* ctx, const uint8_t* mask_l, int H, int W, const float* taps, int radius, float* mask_px, uint8_t* mask_lat) {
    FIE_REQUIRE(ctx && mask_l && taps && mask_px && mask_lat, "fie_mask_prep: NULL argument");
    FIE_REQUIRE(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0, "fie_mask_prep: H, W must be positive multiples of 8 (got %d x %d)", H, W);
    FIE_REQUIRE(radius >= 0 && radius <= kMaskMaxRadius, "fie_mask_prep: radius %d outside [0, %d]", radius, kMaskMaxRadius);
    const int T = kMaskTile + 2 * radius;
    const unsigned lds = (unsigned)(fie_roundup((int64_t)T * T, 16) + (int64_t)T * kMaskTile * sizeof(float));
    fie_launch(ctx, mask_prep_kernel, dim3((W + kMaskTile - 1) / kMaskTile, (H + kMaskTile - 1) / kMaskTile), dim3(256), lds,
               mask_l, H, W, taps, radius, mask_px, mask_lat);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}
int fie_mask_levels_u8(fie_ctx* ctx, const uint8_t* levels_e, const uint8_t* mask_lat, int H, int W, uint8_t* lvl_lat) {
    FIE_REQUIRE(ctx && levels_e && mask_lat && lvl_lat, "fie_mask_levels_u8: NULL argument");
    FIE_REQUIRE(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && (int64_t)H * W < ((int64_t)1 << 31),
                "fie_mask_levels_u8: H, W must be positive multiples of 8 with H * W < 2^31 (got %d x %d)", H, W);
    const int lh = H / 8, lw = W / 8;
    fie_launch(ctx, mask_levels_kernel, dim3(grid_1d((int64_t)lh * lw, kPointwiseBlocks)), dim3(256), 0, levels_e, mask_lat, lh, lw, W, lvl_lat);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}
int fie_mask_support_u8(fie_ctx* ctx, const uint8_t* levels, int64_t n, uint8_t* out) {
    FIE_REQUIRE(ctx && levels && out && n > 0, "fie_mask_support_u8: bad argument");
    fie_launch(ctx, mask_support_kernel, dim3(grid_1d(n, kPointwiseBlocks)), dim3(256), 0, levels, n, out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}
int fie_pixels_out_composite_f16_u8(fie_ctx* ctx, const void* src, int64_t ld_in, int H, int W, const uint8_t* source, const float* mask,
                                    uint8_t* dst) {
    return pixels_out_composite_t<half_t>(ctx, src, ld_in, H, W, source, mask, dst);
}
int fie_pixels_out_composite_f32_u8(fie_ctx* ctx, const void* src, int64_t ld_in, int H, int W, const uint8_t* source, const float* mask,
                                    uint8_t* dst) {
    return pixels_out_composite_t<float>(ctx, src, ld_in, H, W, source, mask, dst);
}

}  // extern "C"
