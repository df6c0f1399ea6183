// Growing / shrinking an edit mask by an exact Euclidean disk (include/fie.h: fie_mask_grow_u8).
//   m(q) = (mask_l(q) >= 128), R = |radius|, p and q pixels of the H x W mask only.
//   radius > 0  out(p) = 255 iff some q has m(q) and (px - qx)^2 + (py - qy)^2 <= R^2   (dilation; nothing grows in from outside the image)
//   radius < 0  out(p) = 255 iff every such q has m(q)                                   (erosion; the border does not erode: ~grow(~m, R))
//   radius = 0  out = 255 m.
// Integers only.  One launch, one 256-thread block per 64 x 64 output tile, three phases in LDS:
//   stage   the tile's binary pixels and an R-halo as bytes, out-of-image = 0; for an erosion the in-image pixels complemented (then "outside is
//           not set" is exactly the rule above).  A block whose staged pixels are all 0 stores the constant and leaves;
//   columns one thread per staged column: a downward and an upward scan leave g[y][c], the distance from tile row y to the nearest set pixel
//           of column c, saturated at R + 1 (rows further than R away never matter), in place of the tile rows' staged bytes;
//   rows    a pixel is set iff some k = |dx| in 0 .. R has g[y][x - k] <= lim[k] or g[y][x + k] <= lim[k], lim[k] = floor(sqrt(R^2 - k^2)):
//           g^2 + k^2 <= R^2 on integers.  k runs outwards, so a pixel inside the mask leaves at once.
// LDS accesses are byte accesses of consecutive lanes to consecutive bytes of one row in every phase: four lanes share a dword (a broadcast), no
// two lanes of a group meet in one bank on different dwords.  No workspace, no atomics, no block waits for another.
#include "image_ops.h"

namespace {

constexpr int kGrowTile = 64;              // 64 x 64 output pixels per block, 16 per thread
constexpr int kGrowRows = 8;               // staged rows a wave loads together
constexpr int kGrowMaxRadius = 64;         // LDS: (64 + 2R)^2 staged bytes + the table of R + 1: 36.1 KiB at R = 64

__global__ __launch_bounds__(256) void mask_grow_kernel(const uint8_t* __restrict__ L, int H, int W, int R, int erode, int tiles_x,
                                                        uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mg_smem[];
    const int BW = kGrowTile + 2 * R, BH = kGrowTile + 2 * R;
    uint8_t* bin = mg_smem;                        // [BH][BW]
    uint8_t* lim = bin + BH * BW;                  // [R + 1]
    const int tid = threadIdx.x;
    const int by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int y0 = by * kGrowTile, x0 = (int)(blockIdx.x - (unsigned)by * tiles_x) * kGrowTile;
    const uint8_t on = erode ? 0 : 255, off = 255 - on;

    int any = 0;
    // a wave takes kGrowRows staged rows at a time, a lane one column of each: the loads go to addresses clamped into the image, so that none
    // hangs on a condition and all kGrowRows are in flight together (one after the other, a block alone on its CU waits out each load's
    // latency: at R = 64 that was most of the kernel's time); what lies outside the image, or past the staged rows and columns, is 0
    for (int rb = (tid >> 6) * kGrowRows; rb < BH; rb += 4 * kGrowRows) {
        for (int c = tid & 63; c < BW + 63; c += 64) {
            const int gx = x0 - R + c;
            const int64_t col = min(max(gx, 0), W - 1);
            uint8_t v[kGrowRows];
#pragma unroll
            for (int j = 0; j < kGrowRows; ++j) v[j] = L[(int64_t)min(max(y0 - R + rb + j, 0), H - 1) * W + col];
#pragma unroll
            for (int j = 0; j < kGrowRows; ++j) {
                const int r = rb + j, gy = y0 - R + r;
                if (r < BH && c < BW) {
                    const uint8_t b = (gy >= 0 && gy < H && gx >= 0 && gx < W && ((v[j] >= 128) != (erode != 0))) ? 1 : 0;
                    bin[r * BW + c] = b;
                    any |= b;
                }
            }
        }
    }
    if (tid <= R) {                                // floor(sqrt(R^2 - k^2)): the float root is a first guess, the integers decide
        const int v = R * R - tid * tid;
        int s = (int)sqrtf((float)v);
        while (s * s > v) --s;
        while ((s + 1) * (s + 1) <= v) ++s;
        lim[tid] = (uint8_t)s;
    }
    if (!__syncthreads_or(any)) {                  // nothing set within reach of the tile
        for (int i = tid; i < kGrowTile * kGrowTile; i += 256) {
            const int y = y0 + (i >> 6), x = x0 + (i & 63);
            if (y < H && x < W) out[(int64_t)y * W + x] = off;
        }
        return;
    }

    const int sat = R + 1;
    uint8_t* g = bin + R * BW;                     // [kGrowTile][BW], in place: a column is read and written by its own thread only
    for (int c = tid; c < BW; c += 256) {
        uint8_t* col = bin + c;
        int d = sat;
#pragma unroll 4
        for (int r = 0; r < R + kGrowTile; ++r) {                  // nearest set pixel at or above; a stored 0 still says "set"
            d = col[r * BW] ? 0 : min(d + 1, sat);
            if (r >= R) col[r * BW] = (uint8_t)d;
        }
        d = sat;
        for (int r = BH - 1; r >= R + kGrowTile; --r) d = col[r * BW] ? 0 : min(d + 1, sat);      // at or below: the lower halo, still 0 / 1
#pragma unroll 4
        for (int r = R + kGrowTile - 1; r >= R; --r) {
            const int up = col[r * BW];
            d = up == 0 ? 0 : min(d + 1, sat);
            col[r * BW] = (uint8_t)min(up, d);
        }
    }
    __syncthreads();

    const int tx = tid & 63;
    for (int ty = tid >> 6; ty < kGrowTile; ty += 4) {             // a wave per tile row
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const uint8_t* row = g + ty * BW + R + tx;
        bool hit = false;
        for (int k0 = 0; k0 <= R && !hit; k0 += 4) {               // four distances per look at `hit`: their LDS reads do not wait for each other
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = min(k0 + j, R);
                const int l = lim[k];
                hit |= (row[-k] <= l) | (row[k] <= l);
            }
        }
        out[(int64_t)y * W + x] = hit ? on : off;
    }
}

}  // namespace

extern "C" {

int fie_mask_grow_u8(fie_ctx* ctx, const uint8_t* mask_l, int H, int W, int radius, uint8_t* out) {
    FIE_REQUIRE(ctx && mask_l && out, "fie_mask_grow_u8: NULL argument");
    FIE_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31), "fie_mask_grow_u8: %d x %d outside 1 .. 2^31 - 1 pixels", H, W);
    FIE_REQUIRE(radius >= -kGrowMaxRadius && radius <= kGrowMaxRadius, "fie_mask_grow_u8: radius %d outside [%d, %d]", radius, -kGrowMaxRadius,
                kGrowMaxRadius);
    const int64_t n = (int64_t)H * W;
    FIE_REQUIRE(out + n <= mask_l || mask_l + n <= out, "fie_mask_grow_u8: out overlaps mask_l (blocks read each other's halo)");
    const int R = radius < 0 ? -radius : radius;
    const int B = kGrowTile + 2 * R;
    const unsigned lds = (unsigned)fie_roundup((int64_t)B * B + R + 1, 16);
    const int tiles_x = (W + kGrowTile - 1) / kGrowTile, tiles_y = (H + kGrowTile - 1) / kGrowTile;
    FIE_DESC(ctx, "mask_grow %dx%d r=%d", H, W, radius);
    fie_launch(ctx, mask_grow_kernel, dim3((unsigned)((int64_t)tiles_x * tiles_y)), dim3(256), lds, mask_l, H, W, R, radius < 0 ? 1 : 0, tiles_x, out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
