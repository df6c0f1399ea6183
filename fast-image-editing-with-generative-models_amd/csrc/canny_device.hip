// K11 on the device: RGB -> gray -> Canny(low, high, aperture 3, L1 gradient), integer exact, same results as the host entry
// fie_canny_rgb_u8 (canny.cpp) and the numpy oracle.  (include/fie.h: fie_canny_rgb_device_u8)
//
//   canny_nms_kernel    one 32x8 output tile per block; the 36x12 gray halo (replicated image border) and the 34x10 Sobel /
//                       L1-magnitude halo (zero outside the image) live in LDS; writes map = 0 (none) / 1 (weak) / 2 (strong)
//   canny_hyst_kernel   hysteresis as a fixed point: a 32x32 tile + 1-pixel halo in LDS is relaxed until nothing changes
//                       (weak next to strong -> strong), written back, and a device flag records whether any tile changed;
//                       the host re-launches until the flag stays clear (8-connected closure is order independent, so the
//                       result equals the serial flood fill)
//   canny_out_kernel    map == 2 -> 255 on three channels
//   canny_ridge_kernel, canny_select_kernel, canny_classify_kernel
//                       the edge-budget form (fie_canny_rgb_device_begin_auto_u8): the thresholds are picked on the device from the histogram
//                       of the ridge magnitudes, and the three kernels stand where canny_nms_kernel stood
// The hysteresis loop reads the flag back, so this entry SYNCHRONISES the stream; it belongs to the host-side preparation
// of an edit (`FastEditor.preprocess_image`), not to the captured denoising graph.
#include "fie_internal.h"

namespace {

constexpr int kShift = 15;
constexpr int kTg22 = (int)(0.4142135623730950488016887242097 * (1 << kShift) + 0.5);
constexpr int TX = 32, TY = 8;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The LDS of one 32x8 tile: the 36x12 gray halo, the 34x10 Sobel halo and its L1 magnitudes.
struct CannyTile {
    uint8_t gray[TY + 4][TX + 4];
    short sdx[TY + 2][TX + 2], sdy[TY + 2][TX + 2];
    int smag[TY + 2][TX + 2];
};

// Gray, Sobel and the non-maximum-suppression direction test of the tile at (x0, y0), stated once for canny_nms_kernel and canny_ridge_kernel.
// Every lane of the 32x8 block calls it (it holds two barriers).  Returns this lane's RIDGE magnitude: the L1 magnitude m of its pixel when
// m > gate and the pixel passes the direction test, else 0 (also outside the image).  A kept pixel is strictly greater than a neighbour whose
// magnitude is >= 0, so a kept m is > 0 and 0 can stand for "not kept".
__device__ __forceinline__ int canny_ridge(CannyTile& t, const uint8_t* rgb, int H, int W, int x0, int y0, int gate) {
    const int tid = threadIdx.y * TX + threadIdx.x;
    for (int i = tid; i < (TY + 4) * (TX + 4); i += TX * TY) {
        const int ly = i / (TX + 4), lx = i - ly * (TX + 4);
        const int gx = clampi(x0 + lx - 2, 0, W - 1), gy = clampi(y0 + ly - 2, 0, H - 1);       // BORDER_REPLICATE
        const uint8_t* p = rgb + ((size_t)gy * W + gx) * 3;
        t.gray[ly][lx] = (uint8_t)((p[0] * 9798 + p[1] * 19235 + p[2] * 3735 + (1 << 14)) >> 15);
    }
    __syncthreads();
    for (int i = tid; i < (TY + 2) * (TX + 2); i += TX * TY) {
        const int ly = i / (TX + 2), lx = i - ly * (TX + 2);
        const int gx = x0 + lx - 1, gy = y0 + ly - 1;
        int dx = 0, dy = 0, mag = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            // gray[ly + 1][lx + 1] is this pixel; its replicated neighbours are in the halo -- except that replication is
            // relative to the IMAGE border, which the clamped halo load already encodes
            const int a = t.gray[ly][lx], b = t.gray[ly][lx + 1], c = t.gray[ly][lx + 2];
            const int d = t.gray[ly + 1][lx], f = t.gray[ly + 1][lx + 2];
            const int g = t.gray[ly + 2][lx], h = t.gray[ly + 2][lx + 1], k = t.gray[ly + 2][lx + 2];
            dx = (c + 2 * f + k) - (a + 2 * d + g);
            dy = (g + 2 * h + k) - (a + 2 * b + c);
            mag = abs(dx) + abs(dy);
        }
        t.sdx[ly][lx] = (short)dx;
        t.sdy[ly][lx] = (short)dy;
        t.smag[ly][lx] = mag;                                // 0 outside the image
    }
    __syncthreads();
    if (x0 + (int)threadIdx.x >= W || y0 + (int)threadIdx.y >= H) return 0;
    const int lx = threadIdx.x + 1, ly = threadIdx.y + 1;
    const int m = t.smag[ly][lx];
    if (m <= gate) return 0;
    const int xs = t.sdx[ly][lx], ys = t.sdy[ly][lx];
    const long long ax = abs(xs), ay = (long long)abs(ys) << kShift;
    const long long tg22x = ax * kTg22;
    bool keep;
    if (ay < tg22x) {
        keep = m > t.smag[ly][lx - 1] && m >= t.smag[ly][lx + 1];
    } else {
        const long long tg67x = tg22x + (ax << (kShift + 1));
        if (ay > tg67x) {
            keep = m > t.smag[ly - 1][lx] && m >= t.smag[ly + 1][lx];
        } else {
            const int s = (xs ^ ys) < 0 ? -1 : 1;
            keep = m > t.smag[ly - 1][lx - s] && m > t.smag[ly + 1][lx + s];
        }
    }
    return keep ? m : 0;
}

__global__ __launch_bounds__(256) void canny_nms_kernel(const uint8_t* rgb, int H, int W, int low, int high, uint8_t* map) {
    __shared__ CannyTile t;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int r = canny_ridge(t, rgb, H, W, x0, y0, low);
    const int gx = x0 + threadIdx.x, gy = y0 + threadIdx.y;
    if (gx >= W || gy >= H) return;
    map[(size_t)gy * W + gx] = r > 0 ? (r > high ? 2 : 1) : 0;
}

// ---- edge-budget thresholds: the thresholds are picked per image from the histogram of the ridge magnitudes
constexpr int kBins = 2048;           // ridge magnitudes are 0 .. 2040 (|dx| + |dy|, each <= 4 * 255)
constexpr int kFloor = 16;            // grey levels that differ by +-1 give |dx|, |dy| <= 8: no smaller threshold keeps quantisation noise out
constexpr int kMaxMag = 2040;

// Ridge map + histogram.  A block walks the 32x8 tiles t = blockIdx.x, + gridDim.x, ...: r (u16) of every pixel goes to `ridge`, r > 0 is counted
// in the block's LDS histogram, and the block adds its non-zero bins to `hist` once, at its end.  Integer counts: the order of the adds is free.
__global__ __launch_bounds__(256) void canny_ridge_kernel(const uint8_t* rgb, int H, int W, int tiles_x, int tiles, uint16_t* ridge, unsigned* hist) {
    __shared__ CannyTile t;
    __shared__ unsigned bins[kBins];
    const int tid = threadIdx.y * TX + threadIdx.x;
    for (int i = tid; i < kBins; i += TX * TY) bins[i] = 0;
    __syncthreads();
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int x0 = tx * TX, y0 = ty * TY;
        const int r = canny_ridge(t, rgb, H, W, x0, y0, 0);      // the next tile's first barrier stands between these reads of the tile and its rewrite
        const int gx = x0 + threadIdx.x, gy = y0 + threadIdx.y;
        if (gx < W && gy < H) {
            ridge[(size_t)gy * W + gx] = (uint16_t)r;
            if (r > 0) atomicAdd(&bins[r], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < kBins; i += TX * TY)
        if (bins[i]) atomicAdd(&hist[i], bins[i]);
}

// One block: high = the smallest h in 16 .. 2040 with #{r > h} <= budget, low = high * lo / hi (0 <= lo <= hi, hi > 0) -> pair[0] = low, pair[1] = high.
// Lane i owns bins 8 i .. 8 i + 7; a suffix scan over the 256 lane sums gives every lane the count above its bins.
__global__ __launch_bounds__(256) void canny_select_kernel(const unsigned* hist, long long budget, int lo, int hi, int* pair) {
    __shared__ long long above[256];
    __shared__ int best;
    const int tid = threadIdx.x;
    unsigned c[8];
    long long own = 0;
    for (int j = 0; j < 8; ++j) { c[j] = hist[tid * 8 + j]; own += c[j]; }
    above[tid] = own;
    if (tid == 0) best = kMaxMag;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                        // inclusive suffix sums
        const long long add = tid + d < 256 ? above[tid + d] : 0;
        __syncthreads();
        above[tid] += add;
        __syncthreads();
    }
    long long n = above[tid] - own;                            // #{r > 8 tid + 7}
    int mine = kMaxMag;
    for (int j = 7; j >= 0; --j) {                             // n = #{r > h} for h = 8 tid + j, non-increasing in h
        const int h = tid * 8 + j;
        if (h >= kFloor && h <= kMaxMag && n <= budget) mine = h;
        n += c[j];
    }
    if (mine < kMaxMag) atomicMin(&best, mine);
    __syncthreads();
    if (tid == 0) {
        pair[0] = (int)((long long)best * lo / hi);
        pair[1] = best;
    }
}

// Ridge map -> the label map of canny_nms_kernel under the pair in device memory: r > high -> 2, r > low -> 1, else 0.  A lane takes 8 pixels:
// one 16-byte load, one 8-byte store; the last n % 8 pixels go one by one.
__global__ __launch_bounds__(256) void canny_classify_kernel(const uint16_t* ridge, size_t n, const int* pair, uint8_t* map) {
    const int low = pair[0], high = pair[1];
    auto label = [=](unsigned r) -> unsigned { return (int)r > low ? ((int)r > high ? 2u : 1u) : 0u; };      // low >= 0: r == 0 is never labelled
    const size_t groups = n / 8;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        const uint4 v = reinterpret_cast<const uint4*>(ridge)[g];
        uint2 o;
        o.x = label(v.x & 0xffff) | label(v.x >> 16) << 8 | label(v.y & 0xffff) << 16 | label(v.y >> 16) << 24;
        o.y = label(v.z & 0xffff) | label(v.z >> 16) << 8 | label(v.w & 0xffff) << 16 | label(v.w >> 16) << 24;
        reinterpret_cast<uint2*>(map)[g] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < n - groups * 8) {
        const size_t i = groups * 8 + threadIdx.x;
        map[i] = (uint8_t)label(ridge[i]);
    }
}

constexpr int HT = 32;

__global__ __launch_bounds__(256) void canny_hyst_kernel(uint8_t* map, int H, int W, int* changed) {
    __shared__ uint8_t t[HT + 2][HT + 2 + 2];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * HT, y0 = blockIdx.y * HT;
    for (int i = tid; i < (HT + 2) * (HT + 2); i += 256) {
        const int ly = i / (HT + 2), lx = i - ly * (HT + 2);
        const int gx = x0 + lx - 1, gy = y0 + ly - 1;
        t[ly][lx] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? map[(size_t)gy * W + gx] : 0;
    }
    __syncthreads();
    bool any_local = false;
    for (;;) {
        bool ch = false;
        for (int i = tid; i < HT * HT; i += 256) {
            const int ly = (i >> 5) + 1, lx = (i & 31) + 1;
            if (t[ly][lx] == 1) {
                const bool strong = t[ly - 1][lx - 1] == 2 || t[ly - 1][lx] == 2 || t[ly - 1][lx + 1] == 2 || t[ly][lx - 1] == 2 ||
                                    t[ly][lx + 1] == 2 || t[ly + 1][lx - 1] == 2 || t[ly + 1][lx] == 2 || t[ly + 1][lx + 1] == 2;
                if (strong) {
                    t[ly][lx] = 2;          // monotone 1 -> 2: racing readers see either value, both are valid states
                    ch = true;
                }
            }
        }
        any_local |= ch;
        if (!__syncthreads_or(ch)) break;
    }
    if (any_local) {
        for (int i = tid; i < HT * HT; i += 256) {
            const int ly = (i >> 5) + 1, lx = (i & 31) + 1;
            const int gx = x0 + lx - 1, gy = y0 + ly - 1;
            if (gx < W && gy < H && t[ly][lx] == 2) map[(size_t)gy * W + gx] = 2;
        }
    }
    if (__syncthreads_or(any_local) && tid == 0) atomicOr(changed, 1);
}

__global__ void canny_out_kernel(const uint8_t* map, size_t n, uint8_t* out) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint8_t e = map[i] == 2 ? 255 : 0;
        out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = e;
    }
}

}  // namespace

extern "C" {

int64_t fie_canny_workspace_bytes(int H, int W) { return (int64_t)H * W + 256; }     // the label map + the flag words of a round

// One round of hysteresis = kPasses passes, each with its own flag word: the fixed point is reached when the LAST pass of a round changed nothing.
// (Round 3 read ONE flag per round -- "any of the four passes changed something" -- so an image that needs two passes paid for eight and two read-backs.)
constexpr int kPasses = 4;

static int canny_round(fie_ctx* ctx, uint8_t* map, int H, int W, int* flags) {
    if (hipMemsetAsync(flags, 0, kPasses * sizeof(int), ctx->stream) != hipSuccess) { fie_set_error("fie_canny_rgb_device_u8: memset failed"); return FIE_EHIP; }
    const dim3 hgrid((W + HT - 1) / HT, (H + HT - 1) / HT);
    for (int rep = 0; rep < kPasses; ++rep) fie_launch(ctx, canny_hyst_kernel, hgrid, dim3(256), 0, map, H, W, flags + rep);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

static void canny_out(fie_ctx* ctx, const uint8_t* map, int H, int W, uint8_t* edges_rgb) {
    const size_t n = (size_t)H * W;
    fie_launch(ctx, canny_out_kernel, dim3((unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256)), dim3(256), 0, map, n, edges_rgb);
}

// Asynchronous first half: NMS, `rounds` rounds of hysteresis, the edge map of that state, and the LAST round's flags on their way to `host_flags`
// (kPasses ints of PINNED host memory).  Nothing is waited for: the host goes on with its own work while the device does this.
int fie_canny_rgb_device_begin_u8(fie_ctx* ctx, const uint8_t* rgb, int H, int W, int low, int high, int rounds, void* workspace, uint8_t* edges_rgb,
                                  int* host_flags) {
    FIE_REQUIRE(ctx && rgb && workspace && edges_rgb && host_flags && H > 0 && W > 0 && rounds >= 1 && rounds <= 64, "fie_canny_rgb_device_begin_u8: bad argument");
    if (low > high) { int t = low; low = high; high = t; }
    uint8_t* map = (uint8_t*)workspace;
    int* flags = (int*)(map + (((size_t)H * W + 63) / 64) * 64);
    fie_launch(ctx, canny_nms_kernel, dim3((W + TX - 1) / TX, (H + TY - 1) / TY), dim3(TX, TY), 0, rgb, H, W, low, high, map);
    FIE_LAUNCH_CHECK();
    for (int r = 0; r < rounds; ++r) {
        const int rc = canny_round(ctx, map, H, W, flags);
        if (rc != FIE_OK) return rc;
    }
    canny_out(ctx, map, H, W, edges_rgb);
    FIE_LAUNCH_CHECK();
    if (hipMemcpyAsync(host_flags, flags, kPasses * sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
        fie_set_error("fie_canny_rgb_device_begin_u8: flag copy failed");
        return FIE_EHIP;
    }
    return FIE_OK;
}

// ---- edge-budget thresholds.  Workspace: [label map, H W rounded to 64][256 bytes: 4 flag words, then the pair {low, high}][ridge map u16, 2 H W
// rounded to 64][histogram, 2048 u32] -- map and flags where fie_canny_rgb_device_finish_u8 expects them.
static size_t round64(size_t v) { return (v + 63) / 64 * 64; }

int64_t fie_canny_auto_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31)) return -1;
    const size_t n = (size_t)H * W;
    return (int64_t)(round64(n) + 256 + round64(2 * n) + kBins * sizeof(unsigned));
}

static bool canny_auto_args(int H, int W, int64_t budget, int lo, int hi, const void* workspace) {
    return H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) && budget >= 1 && budget <= (int64_t)H * W && lo >= 0 && hi >= 0 && (lo > 0 || hi > 0) &&
           ((uintptr_t)workspace & 15) == 0;
}

// Clears the histogram, then ridge + select: the ridge map stays in the workspace and {low, high} lands in `pair` (device memory).  No wait.
static int canny_auto_front(fie_ctx* ctx, const uint8_t* rgb, int H, int W, int64_t budget, int lo, int hi, void* workspace, int* pair) {
    if (lo > hi) { int t = lo; lo = hi; hi = t; }
    const size_t n = (size_t)H * W;
    uint16_t* ridge = (uint16_t*)((uint8_t*)workspace + round64(n) + 256);
    unsigned* hist = (unsigned*)((uint8_t*)ridge + round64(2 * n));
    if (hipMemsetAsync(hist, 0, kBins * sizeof(unsigned), ctx->stream) != hipSuccess) { fie_set_error("fie_canny_thresholds_device_u8: memset failed"); return FIE_EHIP; }
    const int tiles_x = (W + TX - 1) / TX, tiles = tiles_x * ((H + TY - 1) / TY);
    const int cap = 4 * (ctx->num_cus > 0 ? ctx->num_cus : 256);                  // a block flushes its histogram once: bound the blocks, not the tiles
    fie_launch(ctx, canny_ridge_kernel, dim3(tiles < cap ? tiles : cap), dim3(TX, TY), 0, rgb, H, W, tiles_x, tiles, ridge, hist);
    fie_launch(ctx, canny_select_kernel, dim3(1), dim3(256), 0, (const unsigned*)hist, (long long)budget, lo, hi, pair);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

int fie_canny_thresholds_device_u8(fie_ctx* ctx, const uint8_t* rgb, int H, int W, int64_t budget, int lo, int hi, void* workspace, int* pair_dev) {
    FIE_REQUIRE(ctx && rgb && workspace && pair_dev && canny_auto_args(H, W, budget, lo, hi, workspace), "fie_canny_thresholds_device_u8: bad argument");
    return canny_auto_front(ctx, rgb, H, W, budget, lo, hi, workspace, pair_dev);
}

// fie_canny_rgb_device_begin_u8 with the thresholds picked on the device: ridge + histogram, select, classify stand where the NMS kernel stood; the
// pair never visits the host on its way to the classify kernel and travels to host_words[4 .. 5] with the flags, to be reported.
int fie_canny_rgb_device_begin_auto_u8(fie_ctx* ctx, const uint8_t* rgb, int H, int W, int64_t budget, int lo, int hi, int rounds, void* workspace,
                                       uint8_t* edges_rgb, int* host_words) {
    FIE_REQUIRE(ctx && rgb && workspace && edges_rgb && host_words && rounds >= 1 && rounds <= 64 && canny_auto_args(H, W, budget, lo, hi, workspace),
                "fie_canny_rgb_device_begin_auto_u8: bad argument");
    const size_t n = (size_t)H * W;
    uint8_t* map = (uint8_t*)workspace;
    int* flags = (int*)(map + round64(n));
    int* pair = flags + kPasses;
    const uint16_t* ridge = (const uint16_t*)(map + round64(n) + 256);
    int rc = canny_auto_front(ctx, rgb, H, W, budget, lo, hi, workspace, pair);
    if (rc != FIE_OK) return rc;
    const size_t groups = (n / 8 + 255) / 256;
    fie_launch(ctx, canny_classify_kernel, dim3((unsigned)(groups > 2048 ? 2048 : (groups ? groups : 1))), dim3(256), 0, ridge, n, (const int*)pair, map);
    FIE_LAUNCH_CHECK();
    for (int r = 0; r < rounds; ++r) {
        rc = canny_round(ctx, map, H, W, flags);
        if (rc != FIE_OK) return rc;
    }
    canny_out(ctx, map, H, W, edges_rgb);
    FIE_LAUNCH_CHECK();
    if (hipMemcpyAsync(host_words, flags, (kPasses + 2) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
        fie_set_error("fie_canny_rgb_device_begin_auto_u8: flag copy failed");
        return FIE_EHIP;
    }
    return FIE_OK;
}

// Second half: waits for the first (SYNCHRONISES the ctx stream); when its last pass still changed something, further rounds until one ends unchanged, and
// the edge map again.  iterations (optional): hysteresis passes launched HERE (0: begin's rounds had reached the fixed point, edges_rgb was final).
int fie_canny_rgb_device_finish_u8(fie_ctx* ctx, int H, int W, void* workspace, uint8_t* edges_rgb, int* host_flags, int* iterations) {
    FIE_REQUIRE(ctx && workspace && edges_rgb && host_flags && H > 0 && W > 0, "fie_canny_rgb_device_finish_u8: bad argument");
    uint8_t* map = (uint8_t*)workspace;
    int* flags = (int*)(map + (((size_t)H * W + 63) / 64) * 64);
    const int max_iters = ((W + HT - 1) / HT) * ((H + HT - 1) / HT) + 2 * kPasses;       // a strong seed can cross every tile at most once
    int iters = 0;
    bool more = false;
    for (;;) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) { fie_set_error("fie_canny_rgb_device_finish_u8: synchronisation failed"); return FIE_EHIP; }
        if (!host_flags[kPasses - 1]) break;
        if (iters > max_iters) { fie_set_error("fie_canny_rgb_device_u8: hysteresis did not converge in %d passes", iters); return FIE_EHIP; }
        more = true;
        const int rc = canny_round(ctx, map, H, W, flags);
        if (rc != FIE_OK) return rc;
        if (hipMemcpyAsync(host_flags, flags, kPasses * sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) {
            fie_set_error("fie_canny_rgb_device_finish_u8: flag copy failed");
            return FIE_EHIP;
        }
        iters += kPasses;
    }
    if (more) {
        canny_out(ctx, map, H, W, edges_rgb);
        FIE_LAUNCH_CHECK();
    }
    if (iterations) *iterations = iters;
    return FIE_OK;
}

int fie_canny_rgb_device_u8(fie_ctx* ctx, const uint8_t* rgb, int H, int W, int low, int high, void* workspace,
                            uint8_t* edges_rgb, int* iterations) {
    FIE_REQUIRE(ctx && rgb && workspace && edges_rgb && H > 0 && W > 0, "fie_canny_rgb_device_u8: bad argument");
    int host_flags[kPasses] = {0, 0, 0, 0};               // pageable: the copy is then synchronous with respect to the host, which this entry is anyway
    int rc = fie_canny_rgb_device_begin_u8(ctx, rgb, H, W, low, high, 1, workspace, edges_rgb, host_flags);
    if (rc != FIE_OK) return rc;
    int more = 0;
    rc = fie_canny_rgb_device_finish_u8(ctx, H, W, workspace, edges_rgb, host_flags, &more);
    if (iterations) *iterations = kPasses + more;
    return rc;
}

}  // extern "C"
