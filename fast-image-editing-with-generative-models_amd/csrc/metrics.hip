// Edit metrics on the device (include/fie.h: fie_metrics_pairs_u8): the exact sum of squared differences and the sum of the
// SSIM map of n pairs of u8 HWC images, optionally also of their BACKGROUND pair (both images with every pixel of the edited region set to 0).
//   SSIM       oracle/metrics.py::ssim restated: pixels / 255 in fp32, normalised 11-tap Gaussian of sigma 1.5 applied separably (rows, then
//              columns), the five windowed moments x, y, xx, yy, xy, c1 = 1e-4, c2 = 9e-4.  The oracle pads by 5 with torch's `reflect` and
//              then crops those 5 pixels from the map again (torchmetrics' order), so the sum runs over the (H - 10) x (W - 10) positions whose
//              window lies inside the image; the halo is staged reflected all the same, and no reflected value reaches the sum;
//   one block  a 32 x 32 tile of one (pair, variant): the u8 tile of both images with its reflected 5-pixel halo is staged in LDS once (the
//              background variant zeroes masked pixels while staging); the SSE comes from those bytes as integers, then per channel the tile
//              is converted, the row pass writes the five moments of 42 x 32 positions to LDS and the column pass forms the SSIM map;
//   reductions per-thread sums (u32 / fp64) -> wave shuffle -> the block's four wave sums added in wave order -> ONE partial per block, an ordinary
//              store.  A second launch of one block per (pair, variant) adds the partials in tile order.  No atomics, so neither block order
//              nor the batch a pair travels in can move a bit.
// LDS: 2 x 5 292 B of bytes + 2 x 7 056 B of floats + 26 880 B of row moments = 51.6 KB, three blocks per CU.
#include "image_ops.h"

namespace {

constexpr int kT = 32;                  // tile edge (output pixels)
constexpr int kR = 5;                   // window radius
constexpr int kE = kT + 2 * kR;         // staged tile edge: 42
constexpr int kRowB = kE * 3;           // bytes per staged row: 126

struct MetricTaps { float g[2 * kR + 1]; };
struct MetricPartial { uint64_t sse; double ssim; };

// torch's `reflect` (no edge repeat).  A partial tile's halo can reach past the reflection's range; those positions only feed outputs that are
// never summed, so they are clamped to stay in bounds.
__device__ __forceinline__ int reflect_clamp(int i, int n) {
    i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return min(max(i, 0), n - 1);
}

using fie_img::wave_sum;

// grid (tiles_x, tiles_y, n * nvar); variant 1 = the background pair
__global__ __launch_bounds__(256) void metrics_tile_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, const uint8_t* __restrict__ M,
                                                           int H, int W, int nvar, MetricTaps taps, MetricPartial* __restrict__ partial) {
    __shared__ uint8_t ta[kE * kRowB], tb[kE * kRowB];
    __shared__ float fx[kE * kE], fy[kE * kE];
    __shared__ float hm[5][kE * kT];
    __shared__ double red_s[4];
    __shared__ uint32_t red_e[4];
    const int tid = threadIdx.x;
    const int pair = blockIdx.z / nvar, var = blockIdx.z - pair * nvar;
    const int x0 = blockIdx.x * kT, y0 = blockIdx.y * kT;
    const int64_t npix = (int64_t)H * W;
    const uint8_t* a = A + pair * npix * 3;
    const uint8_t* b = B + pair * npix * 3;
    const uint8_t* m = var ? M + pair * npix : nullptr;

    for (int i = tid; i < kE * kRowB; i += 256) {
        const int r = i / kRowB, cb = i - r * kRowB, px = cb / 3, ch = cb - px * 3;
        const int64_t p = (int64_t)reflect_clamp(y0 - kR + r, H) * W + reflect_clamp(x0 - kR + px, W);
        const bool keep = !m || m[p] == 0;
        ta[i] = keep ? a[p * 3 + ch] : 0;
        tb[i] = keep ? b[p * 3 + ch] : 0;
    }
    __syncthreads();

    uint32_t sse = 0;
    for (int i = tid; i < kT * kT * 3; i += 256) {
        const int r = i / (kT * 3), cb = i - r * (kT * 3);
        if (y0 + r < H && x0 + cb / 3 < W) {
            const int o = (r + kR) * kRowB + kR * 3 + cb;
            const int d = (int)ta[o] - (int)tb[o];
            sse += (uint32_t)(d * d);
        }
    }

    double ssim = 0.0;
    const float c1 = 1e-4f, c2 = 9e-4f;
    for (int ch = 0; ch < 3; ++ch) {
        for (int i = tid; i < kE * kE; i += 256) {
            const int r = i / kE, c = i - r * kE;
            fx[i] = (float)ta[r * kRowB + c * 3 + ch] / 255.0f;
            fy[i] = (float)tb[r * kRowB + c * 3 + ch] / 255.0f;
        }
        __syncthreads();
        for (int i = tid; i < kE * kT; i += 256) {
            const int r = i / kT, c = i - r * kT;
            const float* xr = fx + r * kE + c;
            const float* yr = fy + r * kE + c;
            float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
            for (int k = 0; k <= 2 * kR; ++k) {
                const float g = taps.g[k], x = xr[k], y = yr[k];
                sx += g * x; sy += g * y; sxx += g * (x * x); syy += g * (y * y); sxy += g * (x * y);
            }
            hm[0][i] = sx; hm[1][i] = sy; hm[2][i] = sxx; hm[3][i] = syy; hm[4][i] = sxy;
        }
        __syncthreads();
        const int c = tid & (kT - 1);
        for (int r = tid / kT; r < kT; r += 256 / kT) {
            float mo[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k <= 2 * kR; ++k) s += taps.g[k] * hm[q][(r + k) * kT + c];
                mo[q] = s;
            }
            const int y = y0 + r, x = x0 + c;
            if (y >= kR && y < H - kR && x >= kR && x < W - kR) {          // the oracle's crop: windows that lie inside the image
                const float mx = mo[0], my = mo[1];
                const float vxx = mo[2] - mx * mx, vyy = mo[3] - my * my, vxy = mo[4] - mx * my;
                const float v = ((2.f * mx * my + c1) * (2.f * vxy + c2)) / ((mx * mx + my * my + c1) * (vxx + vyy + c2));
                ssim += (double)v;
            }
        }
        __syncthreads();              // fx / fy / hm are rewritten by the next channel
    }

    ssim = wave_sum(ssim);
    sse = wave_sum(sse);
    if ((tid & 63) == 0) { red_s[tid >> 6] = ssim; red_e[tid >> 6] = sse; }
    __syncthreads();
    if (tid == 0) {
        MetricPartial out;
        out.sse = (uint64_t)red_e[0] + red_e[1] + red_e[2] + red_e[3];
        out.ssim = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        partial[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = out;
    }
}

// one block per (pair, variant): thread t adds partials t, t + 256, ... in that order, then a fixed tree.  result row: {sse, ssim_sum, bg_sse, bg_ssim_sum}.
__global__ __launch_bounds__(256) void metrics_final_kernel(const MetricPartial* __restrict__ partial, int tiles, int nvar, uint64_t* __restrict__ result) {
    __shared__ double rs[256];
    __shared__ uint64_t re[256];
    const int tid = threadIdx.x;
    const MetricPartial* p = partial + (int64_t)blockIdx.x * tiles;
    double s = 0.0;
    uint64_t e = 0;
    for (int i = tid; i < tiles; i += 256) { s += p[i].ssim; e += p[i].sse; }
    rs[tid] = s; re[tid] = e;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { rs[tid] += rs[tid + o]; re[tid] += re[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        const int pair = blockIdx.x / nvar, var = blockIdx.x - pair * nvar;
        uint64_t* row = result + (int64_t)pair * 4 + var * 2;
        row[0] = re[0];
        row[1] = (uint64_t)__double_as_longlong(rs[0]);
        if (nvar == 1) { row[2] = 0; row[3] = 0; }          // no mask: the background fields read 0
    }
}

inline int tiles_of(int n) { return (n + kT - 1) / kT; }

}  // namespace

extern "C" {

int64_t fie_metrics_workspace_bytes(int n, int H, int W) {
    if (n <= 0 || H < 2 * kR + 1 || W < 2 * kR + 1) return -1;
    return (int64_t)n * 2 * tiles_of(H) * tiles_of(W) * (int64_t)sizeof(MetricPartial);
}

int fie_metrics_pairs_u8(fie_ctx* ctx, const uint8_t* a, const uint8_t* b, const uint8_t* mask, int n, int H, int W, void* result, void* workspace,
                         int64_t workspace_bytes) {
    FIE_REQUIRE(ctx && a && b && result && workspace, "fie_metrics_pairs_u8: NULL argument");
    FIE_REQUIRE(H >= 2 * kR + 1 && W >= 2 * kR + 1, "fie_metrics_pairs_u8: H, W must be at least 11 (got %d x %d): the window's reflection needs them", H, W);
    const int nvar = mask ? 2 : 1;
    const int tx = tiles_of(W), ty = tiles_of(H);
    FIE_REQUIRE(n > 0 && (int64_t)n * nvar <= 65535 && ty <= 65535, "fie_metrics_pairs_u8: n=%d pairs of %d x %d exceed the launch grid", n, H, W);
    FIE_REQUIRE(workspace_bytes >= fie_metrics_workspace_bytes(n, H, W), "fie_metrics_pairs_u8: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)fie_metrics_workspace_bytes(n, H, W));
    FIE_REQUIRE(((uintptr_t)result | (uintptr_t)workspace) % 8 == 0, "fie_metrics_pairs_u8: result and workspace must be 8-byte aligned");
    MetricTaps taps;
    double g[2 * kR + 1], sum = 0.0;
    for (int k = 0; k <= 2 * kR; ++k) sum += g[k] = exp(-(double)(k - kR) * (k - kR) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k <= 2 * kR; ++k) taps.g[k] = (float)(g[k] / sum);
    FIE_DESC(ctx, "metrics n=%d %dx%d variants=%d", n, H, W, nvar);
    fie_launch(ctx, metrics_tile_kernel, dim3(tx, ty, n * nvar), dim3(256), 0, a, b, mask, H, W, nvar, taps, (MetricPartial*)workspace);
    FIE_LAUNCH_CHECK();
    fie_launch(ctx, metrics_final_kernel, dim3(n * nvar), dim3(256), 0, (const MetricPartial*)workspace, tx * ty, nvar, (uint64_t*)result);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
