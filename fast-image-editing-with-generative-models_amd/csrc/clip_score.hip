// CLIP score on the device (include/fie.h: fie_clip_*): what stands between the u8 image and the ViT image tower, and
// between the two embeddings and the number.
//   mask      fie_clip_mask_rgb_u8: the "edited" variant -- every pixel outside the edited region set to 0, on the image at its OWN size, ahead of
//             the resize (PIE-Bench's order).  The mask may have another size: it is sampled through Pillow's NEAREST index tables
//             (fie_amd/resize.py: nearest_indices), L >= 128 = edited.
//   patches   fie_clip_patches_u8_*: centre crop, /255, (x - mean) / std, patchify and cast in one pass over the resized u8 image.  Row r = (image,
//             patch) of the output is the patch in the K order of the patch-embedding weight [C, 3, ps, ps] viewed as [C, 3 ps ps]: k = (c ps + py) ps
//             + px, so the patch convolution is a plain GEMM.  One work item = 16 contiguous output bytes (8 f16 / 4 f32: consecutive px of one
//             patch row and channel); the decode and the normalisation constants are csrc/image_ops.h's, shared with csrc/dino.hip.
//   embed     fie_vit_embed_*: x[b, 0] = cls + pos[0], x[b, 1 + i] = patch_gemm[b, i] + pos[1 + i].  (The GEMM epilogue's residual operand cannot
//             do it: output rows of an image are 1 + P apart, its input rows P.)
//   score     fie_clip_score_*: one wave per (image, text) pair; lane l adds elements l, l + 64, ... of the three fp32 sums in that order, the
//             wave adds the lanes by a fixed shuffle tree.  No atomics and no dependence on n or the pair's position; a zero norm gives 0.
#include "gemm_common.h"
#include "image_ops.h"

namespace {

using fie_gemm::static_for;
using namespace fie_img;

__global__ __launch_bounds__(256) void clip_mask_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask, int H, int W, int MH, int MW,
                                                        const int* __restrict__ ytab, const int* __restrict__ xtab, uint8_t* __restrict__ dst, int64_t total) {
    const int64_t npix = (int64_t)H * W;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / npix, p = i - b * npix;
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        const int my = ytab ? ytab[y] : y, mx = xtab ? xtab[x] : x;
        const bool keep = mask[(b * MH + my) * MW + mx] >= 128;
        dst[i * 3 + 0] = keep ? src[i * 3 + 0] : 0;
        dst[i * 3 + 1] = keep ? src[i * 3 + 1] : 0;
        dst[i * 3 + 2] = keep ? src[i * 3 + 2] : 0;
    }
}

// items: (row = image * P + patch, 16-byte chunk of the row)
template <typename T>
__global__ __launch_bounds__(256) void clip_patches_kernel(const uint8_t* __restrict__ src, int H, int W, int top, int left, int grid_w, int P, int ps,
                                                           ChannelNorm nm, T* __restrict__ out, int64_t total) {
    constexpr int E = 16 / (int)sizeof(T);
    const int K = 3 * ps * ps, nch = K / E;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const PatchItem t = patch_item<E>(i, nch, P, grid_w, ps);
        const uint8_t* s = src + (((int64_t)t.b * H + top + t.gy * ps + t.py) * W + left + t.gx * ps + t.px) * 3 + t.c;
        const float mean = channel_pick(nm.mean[0], nm.mean[1], nm.mean[2], t.c), std = channel_pick(nm.std[0], nm.std[1], nm.std[2], t.c);
        alignas(16) T v[E];
        static_for([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            v[j] = (T)(((float)s[j * 3] / 255.0f - mean) / std);
        }, std::make_integer_sequence<int, E>{});
        *reinterpret_cast<uint4*>(out + t.row * K + t.k0) = *reinterpret_cast<const uint4*>(v);
    }
}

// items: (row = image * (P + 1) + token, 8-element chunk)
template <typename T>
__global__ __launch_bounds__(256) void vit_embed_kernel(const T* __restrict__ patches, const T* __restrict__ cls, const T* __restrict__ pos, int P, int C,
                                                        T* __restrict__ out, int64_t total) {
    const int nch = C >> 3, Tn = P + 1;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / nch;
        const int ch = (int)(i - row * nch) * 8;
        const int64_t b = row / Tn;
        const int t = (int)(row - b * Tn);
        float a[8], q[8], o[8];
        fie_load8(t == 0 ? cls + ch : patches + (b * P + t - 1) * C + ch, a);
        fie_load8(pos + (int64_t)t * C + ch, q);
        static_for([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            o[j] = a[j] + q[j];
        }, std::make_integer_sequence<int, 8>{});
        fie_store8(out + row * C + ch, o);
    }
}

// one block of one wave per pair; result row = (100 cos, max(100 cos, 0))
template <typename T>
__global__ __launch_bounds__(64) void clip_score_kernel(const T* __restrict__ img, int64_t ld_img, const T* __restrict__ txt, int64_t ld_txt, int P,
                                                        float* __restrict__ out) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const T* a = img + pair * ld_img;
    const T* b = txt + pair * ld_txt;
    float dot = 0.f, na = 0.f, nb = 0.f;
    for (int j = lane; j < P; j += 64) {
        const float x = (float)a[j], y = (float)b[j];
        dot += x * y; na += x * x; nb += y * y;
    }
    dot = wave_sum(dot); na = wave_sum(na); nb = wave_sum(nb);
    if (lane == 0) {
        const float den = sqrtf(na) * sqrtf(nb);
        const float s = den > 0.f ? 100.0f * (dot / den) : 0.f;
        out[pair * 2 + 0] = s;
        out[pair * 2 + 1] = fmaxf(s, 0.f);
    }
}

template <typename T>
int clip_patches_t(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int top, int left, int size, int patch, const float* mean, const float* std,
                   void* out) {
    FIE_REQUIRE(ctx && src && mean && std && out, "fie_clip_patches_u8: NULL argument");
    FIE_REQUIRE(n > 0 && H > 0 && W > 0 && size > 0 && patch > 0, "fie_clip_patches_u8: bad shape");
    FIE_REQUIRE(patch % 8 == 0 && size % patch == 0, "fie_clip_patches_u8: image size %d / patch size %d: the patch size must divide the image size and be a multiple of 8",
                size, patch);
    FIE_REQUIRE(top >= 0 && left >= 0 && top + size <= H && left + size <= W, "fie_clip_patches_u8: crop %d x %d at (%d, %d) leaves the %d x %d image", size, size,
                top, left, H, W);
    FIE_REQUIRE((uintptr_t)out % 16 == 0, "fie_clip_patches_u8: the output must be 16-byte aligned");
    ChannelNorm nm;
    if (const int rc = channel_norm("fie_clip_patches_u8", mean, std, &nm)) return rc;
    const int g = size / patch, P = g * g;
    const int64_t total = (int64_t)n * P * (3 * patch * patch / (16 / (int)sizeof(T)));
    FIE_DESC(ctx, "clip_patches n=%d %dx%d crop=%d@(%d,%d) patch=%d", n, H, W, size, top, left, patch);
    fie_launch(ctx, clip_patches_kernel<T>, dim3(grid_1d(total, kPatchBlocks)), dim3(256), 0, src, H, W, top, left, g, P, patch, nm, (T*)out, total);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

template <typename T>
int vit_embed_t(fie_ctx* ctx, const void* patches, const void* cls, const void* pos, int n, int P, int C, void* out) {
    FIE_REQUIRE(ctx && patches && cls && pos && out, "fie_vit_embed: NULL argument");
    FIE_REQUIRE(n > 0 && P > 0 && C > 0 && C % 8 == 0, "fie_vit_embed: bad shape (n=%d, patches=%d, C=%d; C must be a multiple of 8)", n, P, C);
    FIE_REQUIRE(((uintptr_t)patches | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)out) % 16 == 0, "fie_vit_embed: operands must be 16-byte aligned");
    const int64_t total = (int64_t)n * (P + 1) * (C / 8);
    FIE_DESC(ctx, "vit_embed n=%d tokens=%d C=%d", n, P + 1, C);
    fie_launch(ctx, vit_embed_kernel<T>, dim3(grid_1d(total, kPatchBlocks)), dim3(256), 0, (const T*)patches, (const T*)cls, (const T*)pos, P, C, (T*)out, total);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

template <typename T>
int clip_score_t(fie_ctx* ctx, const void* img, int64_t ld_img, const void* txt, int64_t ld_txt, int n, int P, float* out) {
    FIE_REQUIRE(ctx && img && txt && out, "fie_clip_score: NULL argument");
    FIE_REQUIRE(n > 0 && P > 0 && ld_img >= P && ld_txt >= P, "fie_clip_score: bad shape (n=%d, P=%d, row strides %lld / %lld)", n, P, (long long)ld_img,
                (long long)ld_txt);
    FIE_DESC(ctx, "clip_score n=%d P=%d", n, P);
    fie_launch(ctx, clip_score_kernel<T>, dim3(n), dim3(64), 0, (const T*)img, ld_img, (const T*)txt, ld_txt, P, out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // namespace

extern "C" {

int fie_clip_mask_rgb_u8(fie_ctx* ctx, const uint8_t* src, const uint8_t* mask, int n, int H, int W, int MH, int MW, const int* ytab, const int* xtab,
                         uint8_t* dst) {
    FIE_REQUIRE(ctx && src && mask && dst, "fie_clip_mask_rgb_u8: NULL argument");
    FIE_REQUIRE(n > 0 && H > 0 && W > 0 && MH > 0 && MW > 0, "fie_clip_mask_rgb_u8: bad shape");
    FIE_REQUIRE((MH == H || ytab) && (MW == W || xtab), "fie_clip_mask_rgb_u8: a %d x %d mask for a %d x %d image needs the NEAREST index tables", MH, MW, H, W);
    const int64_t total = (int64_t)n * H * W;
    FIE_DESC(ctx, "clip_mask n=%d %dx%d mask %dx%d", n, H, W, MH, MW);
    fie_launch(ctx, clip_mask_kernel, dim3(grid_1d(total, kPatchBlocks)), dim3(256), 0, src, mask, H, W, MH, MW, ytab, xtab, dst, total);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

int fie_clip_patches_u8_f16(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int top, int left, int size, int patch, const float* mean,
                            const float* std, void* out) {
    return clip_patches_t<half_t>(ctx, src, n, H, W, top, left, size, patch, mean, std, out);
}
int fie_clip_patches_u8_f32(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int top, int left, int size, int patch, const float* mean,
                            const float* std, void* out) {
    return clip_patches_t<float>(ctx, src, n, H, W, top, left, size, patch, mean, std, out);
}
int fie_vit_embed_f16(fie_ctx* ctx, const void* patches, const void* cls, const void* pos, int n, int P, int C, void* out) {
    return vit_embed_t<half_t>(ctx, patches, cls, pos, n, P, C, out);
}
int fie_vit_embed_f32(fie_ctx* ctx, const void* patches, const void* cls, const void* pos, int n, int P, int C, void* out) {
    return vit_embed_t<float>(ctx, patches, cls, pos, n, P, C, out);
}
int fie_clip_score_f16(fie_ctx* ctx, const void* img, int64_t ld_img, const void* txt, int64_t ld_txt, int n, int P, float* out) {
    return clip_score_t<half_t>(ctx, img, ld_img, txt, ld_txt, n, P, out);
}
int fie_clip_score_f32(fie_ctx* ctx, const void* img, int64_t ld_img, const void* txt, int64_t ld_txt, int n, int P, float* out) {
    return clip_score_t<float>(ctx, img, ld_img, txt, ld_txt, n, P, out);
}

}  // extern "C"
