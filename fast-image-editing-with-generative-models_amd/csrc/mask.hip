// Mask-restricted edits (include/fie.h: fie_mask_prep, fie_latent_prep_src, fie_lcm_step_masked, fie_lcm_step_levels, fie_mask_levels_u8,
// fie_mask_support_u8, fie_pixels_out_composite_*).
// The semantics are those of the diffusers inpaint pipelines for a 4-channel UNet layered on the img2img edit:
//   mask prep   binarise the edit-size u8 mask (L >= 128), nearest latent downsample m_lat[y][x] = m_px[8y][8x], optional separable
//               Gaussian feather of m_px (sigma r, radius R = ceil(3r), clamp-to-edge) for the paste-back;
//   latent prep today's K9 plus the clean source latent z0 it used to discard;
//   LCM step    today's K8 plus, per latent pixel, lat = m_lat ? lat : (sab_prev z0 + s1mab_prev n_init), or z0 on the last step;
//   composite   today's pixels_out, then the source u8 where m == 0, the decoded byte where m == 1, rint(m d + (1-m) src) between.
// Soft masks: the latent mask holds levels v in 0 .. 255 and the step its place j among the K steps of the edit; a pixel
// is inside after step j iff v K > 255 (K - 1 - j), i.e. it is edited for the last (v K + 254) / 255 steps.  The binary step is the case of
// levels 0 / 1 with K = 1, j = 0 (v > 0): one kernel, one more integer multiply and compare per latent pixel.
// lcm_step_kernel, latent_prep_kernel and pixels_out_kernel (pointwise.hip) are untouched: an unmasked edit launches exactly what it did.
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

template <typename T>
__global__ void latent_prep_src_kernel(const T* moments, const float* eps_post, const float* noise, int64_t HW, float sf,
                                       float sqrt_ab, float sqrt_1mab, float* lat, T* model_in, int copies, float* z0_out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
        float m[8], o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        fie_load8(moments + i * 8, m);
        float4 l, z;
        float* lp = &l.x;
        float* zp = &z.x;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float logvar = fminf(fmaxf(m[4 + c], -30.f), 20.f);
            const float z0 = (m[c] + fie_expf(0.5f * logvar) * eps_post[c * HW + i]) * sf;
            const float x = sqrt_ab * z0 + sqrt_1mab * noise[c * HW + i];
            lp[c] = x;
            zp[c] = z0;
            o[c] = x;
        }
        *reinterpret_cast<float4*>(lat + i * 4) = l;
        *reinterpret_cast<float4*>(z0_out + i * 4) = z;
        for (int k = 0; k < copies; ++k) fie_store8(model_in + ((int64_t)k * HW + i) * 8, o);
    }
}

template <typename T>
struct LcmMaskedArgs {
    const T* eps; int64_t ld_eps; int nb; float guidance;
    float* lat; const float* noise; int64_t HW;
    float sab_t, s1mab_t, c_skip, c_out, sab_p, s1mab_p;
    T* model_in; int copies; float inv_sf; T* decode_in;
    const uint8_t* m_lat; const float* z0; const float* n_init;
    int steps, thresh;                     // inside iff m_lat * steps > thresh; thresh = 255 (steps - 1 - step), 0 for a binary mask (steps = 1)
};

// Keeps a rounded product out of the backend's multiply-add fusion (-ffp-contract=fast fuses across statements): emits nothing.
__device__ __forceinline__ float fie_rounded(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// lcm_step_kernel's arithmetic, then the blend (a select: an inside pixel keeps the bits the unmasked step writes).  The step is spelled
// out operation by operation as the compiler emits lcm_step_kernel (gfx950 ISA: the guidance, the x0 numerator and c_skip x + c_out x0
// are fused multiply-adds; the noise injection sab_p den + s1mab_p z is two rounded products -- one packed multiply -- and an add).  Left to
// the compiler, the extra work here changes which products it fuses and an all-ones mask would move the last bit of the latents
// (tests/test_masked_edit_gpu.py pins the equality).
template <typename T>
__global__ void lcm_step_masked_kernel(LcmMaskedArgs<T> p) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < p.HW; i += (int64_t)gridDim.x * blockDim.x) {
        float e0[4], e1[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            e0[c] = (float)p.eps[i * p.ld_eps + c];
            e1[c] = p.nb == 2 ? (float)p.eps[(p.HW + i) * p.ld_eps + c] : e0[c];
        }
        float4 l = *reinterpret_cast<const float4*>(p.lat + i * 4);
        const float4 z = *reinterpret_cast<const float4*>(p.z0 + i * 4);
        const bool inside = (int)p.m_lat[i] * p.steps > p.thresh;
        float* lp = &l.x;
        const float* zp = &z.x;
        float o[8] = {0, 0, 0, 0, 0, 0, 0, 0}, od[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float e = e0[c];
            if (p.nb == 2) e = __builtin_fmaf(p.guidance, e1[c] - e, e);  // eps_u + g (eps_c - eps_u)
            const float x = lp[c];
            const float x0 = __builtin_fmaf(-p.s1mab_t, e, x) / p.sab_t;
            float den = __builtin_fmaf(p.c_skip, x, p.c_out * x0);
            float proper = zp[c];                                          // last step: the clean source latent
            if (p.noise) {
                den = fie_rounded(p.sab_p * den) + fie_rounded(p.s1mab_p * p.noise[c * p.HW + i]);
                proper = p.sab_p * zp[c] + p.s1mab_p * p.n_init[c * p.HW + i];
            }
            den = inside ? den : proper;
            lp[c] = den;
            o[c] = den;
            od[c] = den * p.inv_sf;
        }
        *reinterpret_cast<float4*>(p.lat + i * 4) = l;
        if (p.model_in)
            for (int k = 0; k < p.copies; ++k) fie_store8(p.model_in + ((int64_t)k * p.HW + i) * 8, o);
        if (p.decode_in) fie_store8(p.decode_in + i * 8, od);
    }
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
int latent_prep_src_t(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW, float sf, float sqrt_ab,
                      float sqrt_1mab, float* latents_out, void* model_in, int copies, float* z0_out) {
    FIE_REQUIRE(ctx && moments && eps_post && noise && latents_out && model_in && z0_out && HW > 0 && copies > 0,
                "fie_latent_prep_src: bad argument");
    fie_launch(ctx, latent_prep_src_kernel<T>, dim3(grid_1d(HW, kPointwiseBlocks)), dim3(256), 0, (const T*)moments, eps_post, noise, HW, sf, sqrt_ab, sqrt_1mab,
               latents_out, (T*)model_in, copies, z0_out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

template <typename T>
int lcm_step_masked_t(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise, int64_t HW,
                      float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev, void* model_in,
                      int copies, float inv_scaling, void* decode_in, const uint8_t* mask_lat, const float* z0, const float* noise_init,
                      int steps = 1, int step = 0, const char* who = "fie_lcm_step_masked") {
    FIE_REQUIRE(ctx && eps && latents && HW > 0, "%s: bad argument", who);
    FIE_REQUIRE(mask_lat && z0 && (noise_init || !noise), "%s: mask_lat, z0 and (before the last step) noise_init are required", who);
    FIE_REQUIRE(nb == 1 || nb == 2, "%s: nb=%d (1 or 2)", who, nb);
    FIE_REQUIRE(ld_eps % 4 == 0 && ld_eps >= 4, "%s: ld_eps must be a multiple of 4", who);
    FIE_REQUIRE(sqrt_ab_t > 0.f, "%s: sqrt(alpha_bar_t) must be positive", who);
    FIE_REQUIRE(steps >= 1 && steps <= 255 && step >= 0 && step < steps, "%s: step %d of %d steps (1 .. 255 steps, step in 0 .. steps - 1)", who, step, steps);
    LcmMaskedArgs<T> p = {(const T*)eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out,
                          sqrt_ab_prev, sqrt_1mab_prev, (T*)model_in, copies, inv_scaling, (T*)decode_in, mask_lat, z0, noise_init,
                          steps, 255 * (steps - 1 - step)};
    fie_launch(ctx, lcm_step_masked_kernel<T>, dim3(grid_1d(HW, kPointwiseBlocks)), dim3(256), 0, p);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
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
int fie_latent_prep_src(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW, float scaling_factor,
                        float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in, int copies, float* z0_out) {
    return latent_prep_src_t<half_t>(ctx, moments, eps_post, noise, HW, scaling_factor, sqrt_ab, sqrt_1mab, latents_out, model_in, copies, z0_out);
}
int fie_latent_prep_src_f32(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW, float scaling_factor,
                            float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in, int copies, float* z0_out) {
    return latent_prep_src_t<float>(ctx, moments, eps_post, noise, HW, scaling_factor, sqrt_ab, sqrt_1mab, latents_out, model_in, copies, z0_out);
}
int fie_lcm_step_masked(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise, int64_t HW,
                        float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev,
                        void* model_in, int copies, float inv_scaling, void* decode_in, const uint8_t* mask_lat, const float* z0,
                        const float* noise_init) {
    return lcm_step_masked_t<half_t>(ctx, eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                     sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in, mask_lat, z0, noise_init);
}
int fie_lcm_step_masked_f32(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise,
                            int64_t HW, float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev,
                            float sqrt_1mab_prev, void* model_in, int copies, float inv_scaling, void* decode_in, const uint8_t* mask_lat,
                            const float* z0, const float* noise_init) {
    return lcm_step_masked_t<float>(ctx, eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                    sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in, mask_lat, z0, noise_init);
}
int fie_lcm_step_levels(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise, int64_t HW,
                        float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev,
                        void* model_in, int copies, float inv_scaling, void* decode_in, const uint8_t* lvl_lat, const float* z0,
                        const float* noise_init, int steps, int step) {
    return lcm_step_masked_t<half_t>(ctx, eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                     sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in, lvl_lat, z0, noise_init, steps, step,
                                     "fie_lcm_step_levels");
}
int fie_lcm_step_levels_f32(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise,
                            int64_t HW, float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev,
                            float sqrt_1mab_prev, void* model_in, int copies, float inv_scaling, void* decode_in, const uint8_t* lvl_lat,
                            const float* z0, const float* noise_init, int steps, int step) {
    return lcm_step_masked_t<float>(ctx, eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                    sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in, lvl_lat, z0, noise_init, steps, step,
                                    "fie_lcm_step_levels_f32");
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
