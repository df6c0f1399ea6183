// LPIPS (SqueezeNet 1.1) on the device (include/fie.h: fie_lpips_stem_u8_f32, fie_maxpool3s2_nhwc_f32, fie_lpips_layer_f32):
// what no existing op can do.  The Fire modules themselves run on csrc/f32.hip (fie_gemm_f32 / fie_conv3x3_nhwc_f32 with FIE_ACT_RELU).  All fp32.
//   stem      fie_lpips_stem_u8_f32: u8 image -> relu(conv 3 -> 64, k3, stride 2, no padding) of the scaled image.  The byte -> scaled value step
//             (x / 255, * 2 - 1, (y - shift) / scale) is a 3 x 256 table the host built with the definition's own fp32 operations; a masked
//             pixel reads entry 0.  Direct convolution: table and weights [27][64] (k = (ky * 3 + kx) * 3 + ci) are staged in LDS once per block,
//             a work item is (pixel, 4 output channels): 27 table reads, 27 x 4 FMAs on top of the bias, one 16-byte store.
//   maxpool   fie_maxpool3s2_nhwc_f32: MaxPool2d(3, 2, ceil_mode=True) on NHWC: windows clipped at the far edge, start -inf, the first of
//             equal values kept and a NaN taken, as ATen's loop does.  A work item is (output pixel, 4 channels).
//   layer     fie_lpips_layer_f32: one tap of the distance.  16 lanes own one pixel: each reads its share of the a-row and of the b-row once as
//             float4 and keeps it in registers for the two sums of squares (fp32, the 16 lanes by a fixed xor tree), the division by sqrt(1e-8 +
//             sum) and the weighted squared difference (fp32 per lane, the same tree).  A block covers kLayerPixels pixels of ONE pair: each
//             16-lane group adds its pixels in order in fp64, thread 0 adds the 16 groups in group order -> one partial per block, an ordinary
//             store.  Launch 2: one block per pair adds the partials in a fixed order in fp64 and divides by HW.  No atomics: a pair's bits depend
//             neither on P nor on its position; both sides run the same instruction sequence, so an identical pair gives exactly 0; an all-zero
//             pixel is 0 / sqrt(1e-8) = 0.
#include "image_ops.h"

namespace {

using namespace fie_img;

constexpr int kStemK = 27, kStemC = 64;

// items: (pixel of [n, OH, OW], quad of the 64 output channels)
__global__ __launch_bounds__(256) void lpips_stem_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask, int H, int W, int OH, int OW,
                                                         const float* __restrict__ lut, const float* __restrict__ w, const float* __restrict__ bias,
                                                         float* __restrict__ out, int64_t total) {
    __shared__ float s_lut[3 * 256];
    __shared__ __attribute__((aligned(16))) float s_w[kStemK * kStemC];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) s_lut[i] = lut[i];
    for (int i = threadIdx.x; i < kStemK * kStemC; i += 256) s_w[i] = w[i];
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(i & 15);
        const int64_t p = i >> 4;
        const int ox = (int)(p % OW);
        const int64_t r = p / OW;
        const int oy = (int)(r % OH);
        const int64_t b = r / OH;
        const float4 bv = *reinterpret_cast<const float4*>(bias + 4 * q);
        float acc[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int64_t row = (b * H + (2 * oy + ky)) * W + 2 * ox;        // 2 oy + 2 <= H - 1 and 2 ox + 2 <= W - 1 by the definition of OH, OW
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const bool hole = mask != nullptr && mask[row + kx] != 0;
                const uint8_t* px = src + (row + kx) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float x = s_lut[c * 256 + (hole ? 0 : px[c])];
                    const float4 wv = *reinterpret_cast<const float4*>(s_w + ((ky * 3 + kx) * 3 + c) * kStemC + 4 * q);
                    acc[0] = fmaf(x, wv.x, acc[0]);
                    acc[1] = fmaf(x, wv.y, acc[1]);
                    acc[2] = fmaf(x, wv.z, acc[2]);
                    acc[3] = fmaf(x, wv.w, acc[3]);
                }
            }
        }
        *reinterpret_cast<float4*>(out + p * kStemC + 4 * q) =
            make_float4(fmaxf(acc[0], 0.f), fmaxf(acc[1], 0.f), fmaxf(acc[2], 0.f), fmaxf(acc[3], 0.f));
    }
}

__device__ __forceinline__ float pool_take(float m, float v) { return (v > m || v != v) ? v : m; }

// items: (pixel of [n, OH, OW], quad of the C channels)
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ x, int H, int W, int C4, int OH, int OW, float* __restrict__ y, int64_t total) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % C4);
        const int64_t p = i / C4;
        const int ox = (int)(p % OW);
        const int64_t r = p / OW;
        const int oy = (int)(r % OH);
        const int64_t b = r / OH;
        const int y1 = min(2 * oy + 3, H), x1 = min(2 * ox + 3, W);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int iy = 2 * oy; iy < y1; ++iy)
            for (int ix = 2 * ox; ix < x1; ++ix) {
                const float4 v = *reinterpret_cast<const float4*>(x + (((b * H + iy) * W + ix) * C4 + q) * 4);
                m.x = pool_take(m.x, v.x); m.y = pool_take(m.y, v.y); m.z = pool_take(m.z, v.z); m.w = pool_take(m.w, v.w);
            }
        *reinterpret_cast<float4*>(y + i * 4) = m;
    }
}

// ---------------------------------------------------------------------------------------------------------------- one tap of the distance
constexpr int kLayerPixels = 64;           // pixels of one pair per block: 16 groups of 16 lanes, 4 pixels each
constexpr int kLayerMaxC = 512;
constexpr int kLayerRegs = kLayerMaxC / 64; // float4 per lane and side

// the sum over the 16 lanes of a group, in every lane, by a fixed xor tree
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Built with -ffp-contract=off (csrc/Makefile): the FMAs below are the only ones, so the a side and the b side of a pixel round alike
__device__ __forceinline__ float sq4(float4 v) { return fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, v.x * v.x))); }

// grid (blocks per pair, P)
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float* __restrict__ fa, const float* __restrict__ fb, int HW, int C, const float* __restrict__ w,
                                                          double* __restrict__ partial) {
    __shared__ double red[16];
    const int tid = threadIdx.x, sub = tid & 15, grp = tid >> 4;
    const int pair = blockIdx.y, nt = C >> 6;
    float4 wv[kLayerRegs];
#pragma unroll
    for (int t = 0; t < kLayerRegs; ++t)
        wv[t] = t < nt ? *reinterpret_cast<const float4*>(w + (sub + 16 * t) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    double sum = 0.0;
    for (int j = 0; j < kLayerPixels / 16; ++j) {
        const int px = blockIdx.x * kLayerPixels + grp * (kLayerPixels / 16) + j;        // uniform over the 16 lanes of a group
        if (px >= HW) break;
        const int64_t row = ((int64_t)pair * HW + px) * C;
        float4 a[kLayerRegs], b[kLayerRegs];
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int t = 0; t < kLayerRegs; ++t)
            if (t < nt) {
                a[t] = *reinterpret_cast<const float4*>(fa + row + (sub + 16 * t) * 4);
                b[t] = *reinterpret_cast<const float4*>(fb + row + (sub + 16 * t) * 4);
                sa += sq4(a[t]);
                sb += sq4(b[t]);
            }
        const float ra = sqrtf(1e-8f + group_sum(sa)), rb = sqrtf(1e-8f + group_sum(sb));
        float d = 0.f;
#pragma unroll
        for (int t = 0; t < kLayerRegs; ++t)
            if (t < nt) {
                const float dx = a[t].x / ra - b[t].x / rb, dy = a[t].y / ra - b[t].y / rb, dz = a[t].z / ra - b[t].z / rb, dw = a[t].w / ra - b[t].w / rb;
                d = fmaf(wv[t].x, dx * dx, d);
                d = fmaf(wv[t].y, dy * dy, d);
                d = fmaf(wv[t].z, dz * dz, d);
                d = fmaf(wv[t].w, dw * dw, d);
            }
        sum += (double)group_sum(d);
    }
    if (sub == 0) red[grp] = sum;
    __syncthreads();
    if (tid == 0) {
        double s = red[0];
#pragma unroll
        for (int g = 1; g < 16; ++g) s += red[g];
        partial[(int64_t)pair * gridDim.x + blockIdx.x] = s;
    }
}

// one block per pair: thread t adds partials t, t + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(256) void lpips_layer_final_kernel(const double* __restrict__ partial, int blocks, int HW, double* __restrict__ out, int64_t ld_out) {
    __shared__ double rs[256];
    const int tid = threadIdx.x;
    const double* p = partial + (int64_t)blockIdx.x * blocks;
    double s = 0.0;
    for (int i = tid; i < blocks; i += 256) s += p[i];
    rs[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) rs[tid] += rs[tid + o];
        __syncthreads();
    }
    if (tid == 0) out[(int64_t)blockIdx.x * ld_out] = rs[0] / (double)HW;
}

inline int layer_blocks(int HW) { return (HW + kLayerPixels - 1) / kLayerPixels; }

}  // namespace

extern "C" {

int fie_lpips_stem_u8_f32(fie_ctx* ctx, const uint8_t* src, const uint8_t* mask, int n, int H, int W, const float* lut, const float* w, const float* bias,
                          float* out) {
    FIE_REQUIRE(ctx && src && lut && w && bias && out, "fie_lpips_stem_u8_f32: NULL argument");
    FIE_REQUIRE(n > 0 && H >= 3 && W >= 3, "fie_lpips_stem_u8_f32: bad shape (n=%d, %d x %d: at least 3 x 3)", n, H, W);
    FIE_REQUIRE(((uintptr_t)out | (uintptr_t)w | (uintptr_t)bias) % 16 == 0 && (uintptr_t)lut % 4 == 0, "fie_lpips_stem_u8_f32: out, w and bias must be 16-byte aligned");
    const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
    const int64_t total = (int64_t)n * OH * OW * (kStemC / 4);
    FIE_DESC(ctx, "lpips_stem n=%d %dx%d -> %dx%dx64 mask=%d", n, H, W, OH, OW, mask ? 1 : 0);
    fie_launch(ctx, lpips_stem_kernel, dim3(grid_1d(total, kPatchBlocks)), dim3(256), 0, src, mask, H, W, OH, OW, lut, w, bias, out, total);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

int fie_maxpool3s2_nhwc_f32(fie_ctx* ctx, const float* x, int n, int H, int W, int C, float* y) {
    FIE_REQUIRE(ctx && x && y, "fie_maxpool3s2_nhwc_f32: NULL argument");
    FIE_REQUIRE(n > 0 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0, "fie_maxpool3s2_nhwc_f32: bad shape (n=%d, %d x %d x %d: at least 2 x 2, C %% 4 == 0)", n, H, W, C);
    FIE_REQUIRE(((uintptr_t)x | (uintptr_t)y) % 16 == 0, "fie_maxpool3s2_nhwc_f32: x and y must be 16-byte aligned");
    const int OH = (H - 2) / 2 + 1, OW = (W - 2) / 2 + 1;              // ceil((H - 3) / 2) + 1 (1 for H = 2); the last window starts at 2 (OH - 1) <= H - 2
    const int64_t total = (int64_t)n * OH * OW * (C / 4);
    FIE_DESC(ctx, "maxpool3s2 n=%d %dx%dx%d -> %dx%d", n, H, W, C, OH, OW);
    fie_launch(ctx, maxpool3s2_kernel, dim3(grid_1d(total, kPatchBlocks)), dim3(256), 0, x, H, W, C / 4, OH, OW, y, total);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

int64_t fie_lpips_layer_workspace_bytes(int P, int HW) {
    if (P <= 0 || HW <= 0) return -1;
    return (int64_t)P * layer_blocks(HW) * (int64_t)sizeof(double);
}

int fie_lpips_layer_f32(fie_ctx* ctx, const float* fa, const float* fb, int P, int HW, int C, const float* w, void* workspace, double* out, int64_t ld_out) {
    FIE_REQUIRE(ctx && fa && fb && w && workspace && out, "fie_lpips_layer_f32: NULL argument");
    FIE_REQUIRE(P > 0 && P <= 65535 && HW > 0 && ld_out >= 1, "fie_lpips_layer_f32: bad shape (P=%d, HW=%d, ld_out=%lld)", P, HW, (long long)ld_out);
    FIE_REQUIRE(C > 0 && C % 64 == 0 && C <= kLayerMaxC, "fie_lpips_layer_f32: C=%d must be a multiple of 64, at most %d", C, kLayerMaxC);
    FIE_REQUIRE(((uintptr_t)fa | (uintptr_t)fb | (uintptr_t)w) % 16 == 0, "fie_lpips_layer_f32: fa, fb and w must be 16-byte aligned");
    FIE_REQUIRE(((uintptr_t)workspace | (uintptr_t)out) % 8 == 0, "fie_lpips_layer_f32: workspace and out must be 8-byte aligned");
    const int blocks = layer_blocks(HW);
    double* partial = (double*)workspace;
    FIE_DESC(ctx, "lpips_layer P=%d HW=%d C=%d blocks=%d", P, HW, C, blocks);
    fie_launch(ctx, lpips_layer_kernel, dim3((unsigned)blocks, (unsigned)P), dim3(256), 0, fa, fb, HW, C, w, partial);
    FIE_LAUNCH_CHECK();
    FIE_DESC(ctx, "lpips_layer_final P=%d blocks=%d", P, blocks);
    fie_launch(ctx, lpips_layer_final_kernel, dim3((unsigned)P), dim3(256), 0, (const double*)partial, blocks, HW, out, ld_out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
