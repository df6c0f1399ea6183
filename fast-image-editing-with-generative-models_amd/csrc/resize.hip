// K13: LANCZOS resize of a u8 RGB image (or a one-band mode-L mask) on the device, bit-exact with Pillow's ImagingResample (8 bits per channel).
// Replaces `image.resize((1024, 1024), Image.LANCZOS)` at src/pipeline.py:251 of the reference (a Pillow call; the algorithm
// restated here is Pillow's src/libImaging/Resample.c: separable, horizontal pass first, 22-bit fixed-point coefficients,
// each pass rounded and clipped to u8).  The coefficient / bounds tables are Pillow's precompute_coeffs +
// normalize_coeffs_8bpc restated on the host (fie_amd/resize.py) and uploaded once per (in, out) size pair.
// The fixed-point arithmetic of one output pixel is csrc/image_ops.h's (shared with the fused paste of csrc/fullres.hip).
#include "image_ops.h"

namespace {

using namespace fie_img;

// out[y][ox][c] = clip8(half + sum_x in[y][xmin + x][c] * k[ox][x]); C = 3 (RGB) or 1 (a mode-L mask: Pillow runs the same 8-bit
// passes on one band)
template <int C>
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* in, int H, int W, int OW, const int* kk, const int* bounds, int ksize,
                                                       uint8_t* out) {
    const int ox = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (ox >= OW) return;
    const int xmin = bounds[2 * ox], n = bounds[2 * ox + 1];
    const int* k = kk + (size_t)ox * ksize;
    const uint8_t* row = in + ((size_t)y * W + xmin) * C;
    int s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = kResampleHalf;
    for (int x = 0; x < n; ++x) resample_tap<C>(s, row + C * x, k[x]);
    uint8_t* o = out + ((size_t)y * OW + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = resample_clip8(s[c]);
}

// out[oy][x][c] = clip8(half + sum_y in[ymin + y][x][c] * k[oy][y])
template <int C>
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t* in, int W, int OH, const int* kk, const int* bounds, int ksize,
                                                       uint8_t* out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
    if (x >= W) return;
    const int ymin = bounds[2 * oy], n = bounds[2 * oy + 1];
    const int* k = kk + (size_t)oy * ksize;
    const uint8_t* col = in + ((size_t)ymin * W + x) * C;
    int s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = kResampleHalf;
    for (int y = 0; y < n; ++y) resample_tap<C>(s, col + (size_t)y * W * C, k[y]);
    uint8_t* o = out + ((size_t)oy * W + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = resample_clip8(s[c]);
}

template <int C>
int resize_t(fie_ctx* ctx, const char* name, const uint8_t* src, int H, int W, uint8_t* dst, int OH, int OW, const int* kx, const int* bx,
             int ksx, const int* ky, const int* by, int ksy, uint8_t* tmp) {
    FIE_REQUIRE(ctx && src && dst && H > 0 && W > 0 && OH > 0 && OW > 0, "%s: bad argument", name);
    FIE_REQUIRE((W == OW || (kx && bx && ksx > 0)) && (H == OH || (ky && by && ksy > 0)), "%s: missing coefficient table", name);
    FIE_REQUIRE((W == OW || H == OH) || tmp, "%s: two passes need the [H, OW, C] scratch image", name);
    const uint8_t* vin = src;
    if (W != OW) {                         // horizontal pass first, as Pillow does
        uint8_t* hout = H == OH ? dst : tmp;
        fie_launch(ctx, resize_h_kernel<C>, dim3((OW + 255) / 256, H), dim3(256), 0, src, H, W, OW, kx, bx, ksx, hout);
        FIE_LAUNCH_CHECK();
        vin = hout;
    }
    if (H != OH) {
        fie_launch(ctx, resize_v_kernel<C>, dim3((OW + 255) / 256, OH), dim3(256), 0, vin, OW, OH, ky, by, ksy, dst);
        FIE_LAUNCH_CHECK();
    }
    if (W == OW && H == OH) FIE_REQUIRE(hipMemcpyAsync(dst, src, (size_t)H * W * C, hipMemcpyDeviceToDevice, ctx->stream) == hipSuccess,
                                        "%s: copy failed", name);
    return FIE_OK;
}

}  // namespace

extern "C" int fie_resize_rgb_u8(fie_ctx* ctx, const uint8_t* src, int H, int W, uint8_t* dst, int OH, int OW, const int* kx,
                                 const int* bx, int ksx, const int* ky, const int* by, int ksy, uint8_t* tmp) {
    return resize_t<3>(ctx, "fie_resize_rgb_u8", src, H, W, dst, OH, OW, kx, bx, ksx, ky, by, ksy, tmp);
}

extern "C" int fie_resize_l_u8(fie_ctx* ctx, const uint8_t* src, int H, int W, uint8_t* dst, int OH, int OW, const int* kx,
                               const int* bx, int ksx, const int* ky, const int* by, int ksy, uint8_t* tmp) {
    return resize_t<1>(ctx, "fie_resize_l_u8", src, H, W, dst, OH, OW, kx, bx, ksx, ky, by, ksy, tmp);
}
