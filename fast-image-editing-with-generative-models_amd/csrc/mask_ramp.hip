// A level map from a binary mask's outline: the inward distance ramp of a soft mask (include/fie.h: fie_mask_ramp_u8).
//   m(q) = (mask_l(q) >= 128), R = radius in 1 .. 64, p and q pixels of the H x W mask only.
//   D2(p) = min over q with !m(q) of (px - qx)^2 + (py - qy)^2
//   out(p) = 0 where !m(p); 255 where no such q lies within distance < R (a mask of all ones included); else isqrt(65025 D2(p)) / R,
//   which is floor(255 sqrt(D2) / R) < 255.  The image border is not an edge: outside the image counts as set, as for fie_mask_grow_u8's erosion.
// Integers only.  One launch, one 256-thread block per 64 x 64 output tile, csrc/mask_grow.hip's three phases in LDS:
//   stage   the complement of the tile's binary pixels and of an R-halo as bytes (1 = an unset pixel of the image, 0 = set or outside the image).
//           A block with no unset pixel staged stores 255 and leaves; one whose own pixels are all unset stores 0 and leaves;
//   columns one thread per staged column: a downward and an upward scan leave g[y][c], the distance from tile row y to the nearest unset pixel
//           of column c, saturated at R (a pixel R away never lowers a level below 255), in place of the tile rows' staged bytes;
//   rows    D2 = min over k = |dx| in 0 .. R - 1 of min(g[y][x - k], g[y][x + k])^2 + k^2, saturated at R^2.  k runs outwards and the loop leaves
//           once k^2 has reached the minimum so far.
// LDS accesses are byte accesses of consecutive lanes to consecutive bytes of one row in every phase, as in csrc/mask_grow.hip.  No workspace, no
// atomics, no block waits for another.
#include "image_ops.h"

namespace {

constexpr int kRampTile = 64;              // 64 x 64 output pixels per block, 16 per thread
constexpr int kRampRows = 8;               // staged rows a wave loads together
constexpr int kRampMaxRadius = 64;         // LDS: (64 + 2R)^2 staged bytes: 36 KiB at R = 64

__global__ __launch_bounds__(256) void mask_ramp_kernel(const uint8_t* __restrict__ L, int H, int W, int R, int tiles_x, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mr_smem[];
    const int BW = kRampTile + 2 * R, BH = kRampTile + 2 * R;
    uint8_t* bin = mr_smem;                        // [BH][BW]
    const int tid = threadIdx.x;
    const int by = (int)(blockIdx.x / (unsigned)tiles_x);
    const int y0 = by * kRampTile, x0 = (int)(blockIdx.x - (unsigned)by * tiles_x) * kRampTile;

    int unset = 0, set = 0;
    // mask_grow_kernel's staging: a wave takes kRampRows staged rows at a time, a lane one column of each, the loads go to addresses clamped into
    // the image so that all kRampRows are in flight together; what lies outside the image, or past the staged rows and columns, is 0
    for (int rb = (tid >> 6) * kRampRows; rb < BH; rb += 4 * kRampRows) {
        for (int c = tid & 63; c < BW + 63; c += 64) {
            const int gx = x0 - R + c;
            const int64_t col = min(max(gx, 0), W - 1);
            uint8_t v[kRampRows];
#pragma unroll
            for (int j = 0; j < kRampRows; ++j) v[j] = L[(int64_t)min(max(y0 - R + rb + j, 0), H - 1) * W + col];
#pragma unroll
            for (int j = 0; j < kRampRows; ++j) {
                const int r = rb + j, gy = y0 - R + r;
                if (r < BH && c < BW) {
                    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
                    const uint8_t b = (in && v[j] < 128) ? 1 : 0;
                    bin[r * BW + c] = b;
                    unset |= b;
                    set |= (in && !b && r >= R && r < R + kRampTile && c >= R && c < R + kRampTile) ? 1 : 0;
                }
            }
        }
    }
    const int any_unset = __syncthreads_or(unset), any_set = __syncthreads_or(set);
    if (!any_unset || !any_set) {                  // nothing unset within reach of the tile: all 255; nothing set in the tile: all 0
        const uint8_t fill = any_unset ? 0 : 255;
        for (int i = tid; i < kRampTile * kRampTile; i += 256) {
            const int y = y0 + (i >> 6), x = x0 + (i & 63);
            if (y < H && x < W) out[(int64_t)y * W + x] = fill;
        }
        return;
    }

    const int sat = R;
    uint8_t* g = bin + R * BW;                     // [kRampTile][BW], in place: a column is read and written by its own thread only
    for (int c = tid; c < BW; c += 256) {
        uint8_t* col = bin + c;
        int d = sat;
#pragma unroll 4
        for (int r = 0; r < R + kRampTile; ++r) {                  // nearest unset pixel at or above; a stored 0 still says "unset"
            d = col[r * BW] ? 0 : min(d + 1, sat);
            if (r >= R) col[r * BW] = (uint8_t)d;
        }
        d = sat;
        for (int r = BH - 1; r >= R + kRampTile; --r) d = col[r * BW] ? 0 : min(d + 1, sat);      // at or below: the lower halo, still 0 / 1
#pragma unroll 4
        for (int r = R + kRampTile - 1; r >= R; --r) {
            const int up = col[r * BW];
            d = up == 0 ? 0 : min(d + 1, sat);
            col[r * BW] = (uint8_t)min(up, d);
        }
    }
    __syncthreads();

    const int tx = tid & 63, far = R * R;
    for (int ty = tid >> 6; ty < kRampTile; ty += 4) {             // a wave per tile row
        const int y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const uint8_t* row = g + ty * BW + R + tx;
        int best = far;
        for (int k0 = 0; k0 < R && k0 * k0 < best; k0 += 4) {      // four distances per look at `best`: their LDS reads do not wait for each other
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = min(k0 + j, R - 1);
                const int m = min((int)row[-k], (int)row[k]);
                best = min(best, m * m + k * k);
            }
        }
        int v = 255;
        if (best < far) {                          // isqrt(65025 D2) / R: the float root is a first guess, the integers decide
            const int n = 65025 * best;            // < 65025 * 64^2 < 2^31
            int s = (int)sqrtf((float)n);
            while (s * s > n) --s;
            while ((s + 1) * (s + 1) <= n) ++s;
            v = s / R;
        }
        out[(int64_t)y * W + x] = (uint8_t)v;
    }
}

}  // namespace

extern "C" {

int fie_mask_ramp_u8(fie_ctx* ctx, const uint8_t* mask_l, int H, int W, int radius, uint8_t* out_levels) {
    FIE_REQUIRE(ctx && mask_l && out_levels, "fie_mask_ramp_u8: NULL argument");
    FIE_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31), "fie_mask_ramp_u8: %d x %d outside 1 .. 2^31 - 1 pixels", H, W);
    FIE_REQUIRE(radius >= 1 && radius <= kRampMaxRadius, "fie_mask_ramp_u8: radius %d outside [1, %d]", radius, kRampMaxRadius);
    const int64_t n = (int64_t)H * W;
    FIE_REQUIRE(out_levels + n <= mask_l || mask_l + n <= out_levels, "fie_mask_ramp_u8: out_levels overlaps mask_l (blocks read each other's halo)");
    const int B = kRampTile + 2 * radius;
    const unsigned lds = (unsigned)fie_roundup((int64_t)B * B, 16);
    const int tiles_x = (W + kRampTile - 1) / kRampTile, tiles_y = (H + kRampTile - 1) / kRampTile;
    FIE_DESC(ctx, "mask_ramp %dx%d r=%d", H, W, radius);
    fie_launch(ctx, mask_ramp_kernel, dim3((unsigned)((int64_t)tiles_x * tiles_y)), dim3(256), lds, mask_l, H, W, radius, tiles_x, out_levels);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
