// K8, K9: the two per-latent-pixel ops of the denoising loop, every flavour of each from ONE kernel body (include/fie.h: fie_latent_prep,
// fie_latent_prep_src, fie_latent_prep_src_content, fie_lcm_step, fie_lcm_step_masked, fie_lcm_step_levels; each also _f32).  Both are
// latency/HBM-bound; scheduler scalars are computed on the host in fp32/fp64 and passed by value (c_skip ~ 1e-8 underflows in
// fp16, so the LCM update is done in fp32 on an fp32 master copy of the latents).
//   latent prep   VAE posterior sample, scale, add_noise; Z0 also stores the clean source latent z0 a masked edit blends towards.  The
//                 latent content modes are a second launch: a select over the latent pixels inside the mask.
//   LCM step      guidance, x0 prediction, boundary condition, re-noise; BLEND adds, per latent pixel, lat = inside ? lat :
//                 (sab_prev z0 + s1mab_prev n_init), or z0 on the last step.  Soft masks (section 21): the latent mask
//                 holds levels v in 0 .. 255 and the step its place j among the K steps of the edit; a pixel is inside after step j iff
//                 v K > 255 (K - 1 - j).  The binary mask is the case of levels 0 / 1 with K = 1, j = 0 (v > 0).
#include "image_ops.h"

namespace {

using fie_img::grid_1d;
using fie_img::kPointwiseBlocks;

template <typename T, bool Z0>
__global__ void latent_prep_kernel(const T* moments, const float* eps_post, const float* noise, int64_t HW, float sf, float sqrt_ab,
                                   float sqrt_1mab, float* lat, T* model_in, int copies, float* z0_out) {
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
        if constexpr (Z0) *reinterpret_cast<float4*>(z0_out + i * 4) = z;
        for (int k = 0; k < copies; ++k) fie_store8(model_in + ((int64_t)k * HW + i) * 8, o);
    }
}

// the select of the latent content modes, over what latent_prep_kernel has just written: only latent pixels inside the mask are touched
template <typename T>
__global__ __launch_bounds__(256) void latent_content_kernel(const uint8_t* __restrict__ m_lat, const float* __restrict__ noise, int64_t HW,
                                                             float sqrt_1mab, int nothing, float* __restrict__ lat, T* __restrict__ model_in, int copies) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
        if (!m_lat[i]) continue;
        float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float z = noise[c * HW + i];
            o[c] = nothing ? sqrt_1mab * z : z;          // add_noise of the zero latent: one product, nothing to fuse it with
        }
        *reinterpret_cast<float4*>(lat + i * 4) = make_float4(o[0], o[1], o[2], o[3]);
        for (int k = 0; k < copies; ++k) fie_store8(model_in + ((int64_t)k * HW + i) * 8, o);
    }
}

template <typename T>
struct LcmArgs {
    const T* eps; int64_t ld_eps; int nb; float guidance;
    float* lat; const float* noise; int64_t HW;
    float sab_t, s1mab_t, c_skip, c_out, sab_p, s1mab_p;
    T* model_in; int copies; float inv_sf; T* decode_in;
    const uint8_t* m_lat; const float* z0; const float* n_init;       // BLEND only
    int steps, thresh;                     // inside iff m_lat * steps > thresh; thresh = 255 (steps - 1 - step), 0 for a binary mask (steps = 1)
};

// Keeps a rounded product out of the backend's multiply-add fusion (-ffp-contract=fast fuses across statements): emits nothing.
__device__ __forceinline__ float fie_rounded(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// One channel of one latent pixel: x, the eps rows e (and e1 with guidance) and the noise p.noise[zi] -> the next latent; BLEND then selects
// between it and the source's own z0 at that noise level (an inside pixel keeps the bits the unmasked step writes).  Every multiply-add of the
// step is written as the operation it is -- the guidance, the x0 numerator and c_skip x + c_out x0 are fused, the noise injection is two
// rounded products and an add -- so that no instantiation's bits depend on the contraction pass: with the fusion left to the compiler
// (-ffp-contract=fast) the select changed which products it fused, and an all-ones mask moved the last bit of the latents.
template <typename T, bool BLEND>
__device__ __forceinline__ float lcm_update(const LcmArgs<T>& p, float e, float e1, float x, int64_t zi, float z0, bool inside) {
    if (p.nb == 2) e = __builtin_fmaf(p.guidance, e1 - e, e);            // eps_u + g (eps_c - eps_u)
    const float x0 = __builtin_fmaf(-p.s1mab_t, e, x) / p.sab_t;
    float den = __builtin_fmaf(p.c_skip, x, p.c_out * x0);
    float proper = z0;                                                   // last step: the clean source latent
    if (p.noise) {
        den = fie_rounded(p.sab_p * den) + fie_rounded(p.s1mab_p * p.noise[zi]);
        if constexpr (BLEND) proper = p.sab_p * z0 + p.s1mab_p * p.n_init[zi];
    }
    return inside ? den : proper;
}

template <typename T, bool BLEND>
__global__ void lcm_step_kernel(LcmArgs<T> p) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < p.HW; i += (int64_t)gridDim.x * blockDim.x) {
        float e0[4], e1[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            e0[c] = (float)p.eps[i * p.ld_eps + c];
            e1[c] = p.nb == 2 ? (float)p.eps[(p.HW + i) * p.ld_eps + c] : e0[c];
        }
        float4 l = *reinterpret_cast<const float4*>(p.lat + i * 4);
        float4 z = {};
        bool inside = true;
        if constexpr (BLEND) {
            z = *reinterpret_cast<const float4*>(p.z0 + i * 4);
            inside = (int)p.m_lat[i] * p.steps > p.thresh;
        }
        float* lp = &l.x;
        const float* zp = &z.x;
        float o[8] = {0, 0, 0, 0, 0, 0, 0, 0}, od[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float den = lcm_update<T, BLEND>(p, e0[c], e1[c], lp[c], c * p.HW + i, zp[c], inside);
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

template <typename T, bool Z0>
int latent_prep_t(fie_ctx* ctx, const char* who, const void* moments, const float* eps_post, const float* noise, int64_t HW, float sf,
                  float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in, int copies, float* z0_out = nullptr) {
    FIE_REQUIRE(ctx && moments && eps_post && noise && latents_out && model_in && (z0_out || !Z0) && HW > 0 && copies > 0, "%s: bad argument", who);
    fie_launch(ctx, latent_prep_kernel<T, Z0>, dim3(grid_1d(HW, kPointwiseBlocks)), dim3(256), 0, (const T*)moments, eps_post, noise, HW, sf,
               sqrt_ab, sqrt_1mab, latents_out, (T*)model_in, copies, z0_out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

template <typename T>
int latent_prep_src_content_t(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW, float sf, float sqrt_ab,
                              float sqrt_1mab, float* latents_out, void* model_in, int copies, float* z0_out, const uint8_t* mask_lat, int mode) {
    FIE_REQUIRE(mode >= FIE_CONTENT_ORIGINAL && mode <= FIE_CONTENT_LATENT_NOTHING, "fie_latent_prep_src_content: mode %d outside [0, 3]", mode);
    FIE_REQUIRE(mask_lat, "fie_latent_prep_src_content: mask_lat is required");
    const int rc = latent_prep_t<T, true>(ctx, "fie_latent_prep_src", moments, eps_post, noise, HW, sf, sqrt_ab, sqrt_1mab, latents_out, model_in,
                                          copies, z0_out);
    if (rc != FIE_OK || mode < FIE_CONTENT_LATENT_NOISE) return rc;
    fie_launch(ctx, latent_content_kernel<T>, dim3(grid_1d(HW, kPointwiseBlocks)), dim3(256), 0, mask_lat, noise, HW, sqrt_1mab,
               mode == FIE_CONTENT_LATENT_NOTHING ? 1 : 0, latents_out, (T*)model_in, copies);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

template <typename T, bool BLEND>
int lcm_step_t(fie_ctx* ctx, const char* who, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise,
               int64_t HW, float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev, void* model_in,
               int copies, float inv_scaling, void* decode_in, const uint8_t* mask_lat = nullptr, const float* z0 = nullptr,
               const float* noise_init = nullptr, int steps = 1, int step = 0) {
    FIE_REQUIRE(ctx && eps && latents && HW > 0, "%s: bad argument", who);
    if (BLEND) FIE_REQUIRE(mask_lat && z0 && (noise_init || !noise), "%s: mask_lat, z0 and (before the last step) noise_init are required", who);
    FIE_REQUIRE(nb == 1 || nb == 2, "%s: nb=%d (1 or 2)", who, nb);
    FIE_REQUIRE(ld_eps % 4 == 0 && ld_eps >= 4, "%s: ld_eps must be a multiple of 4", who);
    FIE_REQUIRE(sqrt_ab_t > 0.f, "%s: sqrt(alpha_bar_t) must be positive", who);
    FIE_REQUIRE(steps >= 1 && steps <= 255 && step >= 0 && step < steps, "%s: step %d of %d steps (1 .. 255 steps, step in 0 .. steps - 1)", who, step, steps);
    LcmArgs<T> p = {(const T*)eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out,
                    sqrt_ab_prev, sqrt_1mab_prev, (T*)model_in, copies, inv_scaling, (T*)decode_in, mask_lat, z0, noise_init,
                    steps, 255 * (steps - 1 - step)};
    fie_launch(ctx, lcm_step_kernel<T, BLEND>, dim3(grid_1d(HW, kPointwiseBlocks)), dim3(256), 0, p);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // namespace

extern "C" {

int fie_latent_prep(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW,
                    float scaling_factor, float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in, int copies) {
    return latent_prep_t<half_t, false>(ctx, "fie_latent_prep", moments, eps_post, noise, HW, scaling_factor, sqrt_ab, sqrt_1mab, latents_out, model_in, copies);
}
int fie_latent_prep_f32(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW,
                        float scaling_factor, float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in, int copies) {
    return latent_prep_t<float, false>(ctx, "fie_latent_prep", moments, eps_post, noise, HW, scaling_factor, sqrt_ab, sqrt_1mab, latents_out, model_in, copies);
}
int fie_latent_prep_src(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW, float scaling_factor,
                        float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in, int copies, float* z0_out) {
    return latent_prep_t<half_t, true>(ctx, "fie_latent_prep_src", moments, eps_post, noise, HW, scaling_factor, sqrt_ab, sqrt_1mab, latents_out, model_in, copies, z0_out);
}
int fie_latent_prep_src_f32(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW, float scaling_factor,
                            float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in, int copies, float* z0_out) {
    return latent_prep_t<float, true>(ctx, "fie_latent_prep_src", moments, eps_post, noise, HW, scaling_factor, sqrt_ab, sqrt_1mab, latents_out, model_in, copies, z0_out);
}
int fie_latent_prep_src_content(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW, float scaling_factor,
                                float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in, int copies, float* z0_out,
                                const uint8_t* mask_lat, int mode) {
    return latent_prep_src_content_t<half_t>(ctx, moments, eps_post, noise, HW, scaling_factor, sqrt_ab, sqrt_1mab, latents_out, model_in, copies,
                                             z0_out, mask_lat, mode);
}
int fie_latent_prep_src_content_f32(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW, float scaling_factor,
                                    float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in, int copies, float* z0_out,
                                    const uint8_t* mask_lat, int mode) {
    return latent_prep_src_content_t<float>(ctx, moments, eps_post, noise, HW, scaling_factor, sqrt_ab, sqrt_1mab, latents_out, model_in, copies,
                                            z0_out, mask_lat, mode);
}

int fie_lcm_step(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise, int64_t HW,
                 float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev,
                 void* model_in, int copies, float inv_scaling, void* decode_in) {
    return lcm_step_t<half_t, false>(ctx, "fie_lcm_step", eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                     sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in);
}
int fie_lcm_step_f32(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise, int64_t HW,
                     float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev,
                     void* model_in, int copies, float inv_scaling, void* decode_in) {
    return lcm_step_t<float, false>(ctx, "fie_lcm_step", eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                    sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in);
}
int fie_lcm_step_masked(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise, int64_t HW,
                        float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev,
                        void* model_in, int copies, float inv_scaling, void* decode_in, const uint8_t* mask_lat, const float* z0, const float* noise_init) {
    return lcm_step_t<half_t, true>(ctx, "fie_lcm_step_masked", eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                    sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in, mask_lat, z0, noise_init);
}
int fie_lcm_step_masked_f32(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise, int64_t HW,
                            float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev,
                            void* model_in, int copies, float inv_scaling, void* decode_in, const uint8_t* mask_lat, const float* z0, const float* noise_init) {
    return lcm_step_t<float, true>(ctx, "fie_lcm_step_masked", eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                   sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in, mask_lat, z0, noise_init);
}
int fie_lcm_step_levels(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise, int64_t HW,
                        float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev,
                        void* model_in, int copies, float inv_scaling, void* decode_in, const uint8_t* lvl_lat, const float* z0, const float* noise_init,
                        int steps, int step) {
    return lcm_step_t<half_t, true>(ctx, "fie_lcm_step_levels", eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                    sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in, lvl_lat, z0, noise_init, steps, step);
}
int fie_lcm_step_levels_f32(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents, const float* noise, int64_t HW,
                            float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out, float sqrt_ab_prev, float sqrt_1mab_prev,
                            void* model_in, int copies, float inv_scaling, void* decode_in, const uint8_t* lvl_lat, const float* z0, const float* noise_init,
                            int steps, int step) {
    return lcm_step_t<float, true>(ctx, "fie_lcm_step_levels_f32", eps, ld_eps, nb, guidance, latents, noise, HW, sqrt_ab_t, sqrt_1mab_t, c_skip, c_out, sqrt_ab_prev,
                                   sqrt_1mab_prev, model_in, copies, inv_scaling, decode_in, lvl_lat, z0, noise_init, steps, step);
}

}  // extern "C"
