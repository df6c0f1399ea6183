// The back end of a tiled edit: ny x nx overlapping tiles blended into one image (include/fie.h: fie_tile_blend_rgb_u8).
//   tile j = iy * nx + ix lies at (xs[ix], ys[iy]); its weight at its own pixel (v, u) is W_j = wy(v) * wx(u) with, per axis,
//   w(u) = min(first tile ? t : u + 1, last tile ? t : t - u)                  the distance to the tile's nearest INTERIOR edge
//   out(y, x, c) = (sum_j W_j tile_j(y - ys, x - xs, c) + (S >> 1)) / S,  S = sum_j W_j  over the tiles that cover (y, x)
// A gather in integers: no atomics, no f32, no workspace.  Positions increase, so the tiles that cover a pixel are a RANGE of columns times
// a range of rows, and S = (sum of wy over the rows) * (sum of wx over the columns).  One launch: blockIdx.y strides over the output rows,
// the threads of a row's blocks are its "slots" as in outpaint.hip -- a row of 3 W bytes starts wherever the row before it ends, so it is a
// head of 0 .. 3 bytes up to the next dword boundary of its ADDRESS, a body of aligned dwords and a tail; slot k < body stores dword k, slot
// k == body the head and the tail by bytes.  A block's 256 dwords span at most 343 pixels of a row: the column range that can cover them is
// resolved once per block (from the positions in LDS) and a thread looks only inside it; the row range is one per output row.  A dword's
// four bytes belong to two neighbouring pixels.  Where both have the same cover -- all but the dwords across a tile's edge -- each covering
// tile contributes the same four consecutive bytes of its row, read through the aligned dwords that hold them (load4); where that cover
// is one tile the dword is a copy: no multiply, no division.  Every byte is written once, by one thread; no store reaches past a row, no
// load past the tiles' first or last byte.
//
// The accumulator.  W_j <= th tw, and a pixel is covered by at most cy row ranges times cx column ranges (cy, cx: the most tiles that share a
// pixel along each axis, found on the host), so S <= B = (cy th) (cx tw) and the numerator sum_j W_j 255 + (S >> 1) < 256 B.  B < 2^24 keeps
// it below 2^32 and the kernel runs on 32-bit unsigned integers (the plans of fie_amd/tiles.py: cy, cx <= 3, th, tw <= 1024 -> B <= 9.5e6;
// the largest numerator those reach is 267 386 880, at three 1024-tiles per axis over 2047 pixels); any other geometry takes the same kernel
// on 64-bit integers.
#include "image_ops.h"

namespace {

using fie_img::load4;
using fie_img::row_split;

constexpr int kTileBlendMaxAxis = 32;
constexpr int kTileBlendRows = 4;          // output rows a thread takes, one after the other

struct TileBlendGeom {
    int nx, ny, th, tw, H, W;
    int xs[kTileBlendMaxAxis], ys[kTileBlendMaxAxis];       // entries past nx / ny are 0
};

// tile i of n along an axis, u pixels from the tile's first
__device__ __forceinline__ int axis_weight(int t, int i, int n, int u) {
    const int a = i == 0 ? t : u + 1, b = i == n - 1 ? t : t - u;
    return a < b ? a : b;
}

// the tiles lo .. hi that cover pixel p of an axis, looked for among clo .. chi (which hold them)
__device__ __forceinline__ void axis_cover(const int* pos, int t, int clo, int chi, int p, int& lo, int& hi) {
    lo = clo;
    while (lo < chi && pos[lo] + t <= p) ++lo;
    hi = chi;
    while (hi > lo && pos[hi] > p) --hi;
}

struct TileRow {              // one output row: which tile rows cover it
    int y, lo, hi;
};

__device__ __forceinline__ int64_t tile_byte(const TileBlendGeom& g, int iy, int ix, int v, int u, int c) {
    return (((int64_t)(iy * g.nx + ix) * g.th + v) * g.tw + u) * 3 + c;
}

// one output byte the general way: the head and the tail of a row, and the dwords across a tile's edge
template <typename Acc>
__device__ __forceinline__ uint8_t blend_byte(const uint8_t* __restrict__ tiles, const TileBlendGeom& g, const int* xs, const int* ys, const TileRow& r,
                                              int x, int c, int clo, int chi) {
    int lo, hi;
    axis_cover(xs, g.tw, clo, chi, x, lo, hi);
    if (lo == hi && r.lo == r.hi) return tiles[tile_byte(g, r.lo, lo, r.y - ys[r.lo], x - xs[lo], c)];
    Acc num = 0, den = 0;
    for (int iy = r.lo; iy <= r.hi; ++iy) {
        const int v = r.y - ys[iy];
        const Acc wy = (Acc)axis_weight(g.th, iy, g.ny, v);
        for (int ix = lo; ix <= hi; ++ix) {
            const int u = x - xs[ix];
            const Acc w = wy * (Acc)axis_weight(g.tw, ix, g.nx, u);
            num += w * (Acc)tiles[tile_byte(g, iy, ix, v, u, c)];
            den += w;
        }
    }
    return (uint8_t)((num + (den >> 1)) / den);
}

template <typename Acc>
__global__ __launch_bounds__(256) void tile_blend_kernel(const uint8_t* __restrict__ tiles, TileBlendGeom g, uint8_t* __restrict__ out) {
    __shared__ int pos[2 * kTileBlendMaxAxis];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kTileBlendMaxAxis; ++k) {
            pos[k] = g.xs[k];
            pos[kTileBlendMaxAxis + k] = g.ys[k];
        }
    }
    __syncthreads();
    const int* xs = pos;
    const int* ys = pos + kTileBlendMaxAxis;
    const int64_t rbytes = (int64_t)g.W * 3;
    const uint8_t* tend = tiles + (int64_t)g.nx * g.ny * g.th * g.tw * 3;
    const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // the block's dwords are bytes head + 1024 b .. head + 1024 b + 1023 of a row, head <= 3: the columns that can cover their pixels
    const int64_t b0 = (int64_t)blockIdx.x * 1024;
    const int64_t last = (int64_t)g.W - 1;
    const int pf = (int)(b0 / 3 < last ? b0 / 3 : last), pl = (int)((b0 + 1026) / 3 < last ? (b0 + 1026) / 3 : last);
    int blo, bhi, unused;
    axis_cover(xs, g.tw, 0, g.nx - 1, pf, blo, unused);
    axis_cover(xs, g.tw, blo, g.nx - 1, pl, unused, bhi);
    for (int y = blockIdx.y; y < g.H; y += gridDim.y) {
        TileRow r;
        r.y = y;
        axis_cover(ys, g.th, 0, g.ny - 1, y, r.lo, r.hi);
        uint8_t* orow = out + (int64_t)y * rbytes;
        int head;
        int64_t body;
        row_split(orow, rbytes, head, body);
        if (slot < body) {
            const int64_t j = head + slot * 4;
            const int x0 = (int)(j / 3), c0 = (int)(j - (int64_t)x0 * 3);       // bytes c0 .. 2 of pixel x0, the rest of pixel x0 + 1
            int l0, h0, l1, h1;
            axis_cover(xs, g.tw, blo, bhi, x0, l0, h0);
            axis_cover(xs, g.tw, blo, bhi, x0 + 1, l1, h1);
            uint32_t d = 0;
            if (l0 != l1 || h0 != h1) {
                int x = x0, c = c0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    d |= (uint32_t)blend_byte<Acc>(tiles, g, xs, ys, r, x, c, blo, bhi) << (8 * k);
                    if (++c == 3) { c = 0; ++x; }
                }
            } else if (l0 == h0 && r.lo == r.hi) {
                d = load4(tiles + tile_byte(g, r.lo, l0, y - ys[r.lo], x0 - xs[l0], c0), tiles, tend);
            } else {
                Acc num[4] = {0, 0, 0, 0}, den0 = 0, den1 = 0;
                for (int iy = r.lo; iy <= r.hi; ++iy) {
                    const int v = y - ys[iy];
                    const Acc wy = (Acc)axis_weight(g.th, iy, g.ny, v);
                    for (int ix = l0; ix <= h0; ++ix) {
                        const int u = x0 - xs[ix];
                        const Acc w0 = wy * (Acc)axis_weight(g.tw, ix, g.nx, u), w1 = wy * (Acc)axis_weight(g.tw, ix, g.nx, u + 1);
                        const uint32_t q = load4(tiles + tile_byte(g, iy, ix, v, u, c0), tiles, tend);
                        den0 += w0;
                        den1 += w1;
#pragma unroll
                        for (int k = 0; k < 4; ++k) num[k] += (Acc)((q >> (8 * k)) & 255u) * (c0 + k < 3 ? w0 : w1);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const Acc den = c0 + k < 3 ? den0 : den1;
                    d |= (uint32_t)((num[k] + (den >> 1)) / den) << (8 * k);
                }
            }
            *reinterpret_cast<uint32_t*>(orow + j) = d;
        } else if (slot == body) {
            for (int64_t j = 0; j < head; ++j) orow[j] = blend_byte<Acc>(tiles, g, xs, ys, r, (int)(j / 3), (int)(j % 3), 0, g.nx - 1);
            for (int64_t j = head + body * 4; j < rbytes; ++j) orow[j] = blend_byte<Acc>(tiles, g, xs, ys, r, (int)(j / 3), (int)(j % 3), 0, g.nx - 1);
        }
    }
}

// the rules of one axis; -> the most tiles that share a pixel along it, 0 when a rule is broken
int axis_check(const int* pos, int n, int t, int S) {
    if (n < 1 || n > kTileBlendMaxAxis || t < 1 || S < 1 || pos[0] != 0 || pos[n - 1] != S - t) return 0;
    for (int i = 0; i + 1 < n; ++i)
        if (pos[i + 1] <= pos[i] || pos[i + 1] > pos[i] + t) return 0;
    int most = 1;
    for (int i = 0; i < n; ++i) {             // the cover grows only where a tile starts
        int c = 0;
        for (int k = 0; k <= i; ++k) c += pos[k] + t > pos[i];
        most = c > most ? c : most;
    }
    return most;
}

}  // namespace

extern "C" {

int fie_tile_blend_rgb_u8(fie_ctx* ctx, const uint8_t* tiles, int nx, int ny, const int* xs, const int* ys, int th, int tw, int H, int W, uint8_t* out) {
    FIE_REQUIRE(ctx && tiles && xs && ys && out, "fie_tile_blend_rgb_u8: NULL argument");
    FIE_REQUIRE(th >= 1 && tw >= 1 && H >= 1 && W >= 1, "fie_tile_blend_rgb_u8: tiles %d x %d, image %d x %d: all at least 1", th, tw, H, W);
    FIE_REQUIRE(nx >= 1 && nx <= kTileBlendMaxAxis && ny >= 1 && ny <= kTileBlendMaxAxis, "fie_tile_blend_rgb_u8: a grid of %d x %d tiles outside 1 .. %d",
                nx, ny, kTileBlendMaxAxis);
    FIE_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "fie_tile_blend_rgb_u8: image %d x %d outside 1 .. 2^31 - 1 pixels", H, W);
    const int cx = axis_check(xs, nx, tw, W), cy = axis_check(ys, ny, th, H);
    FIE_REQUIRE(cx > 0, "fie_tile_blend_rgb_u8: xs: %d positions of %d-wide tiles over %d must start at 0, increase strictly, leave no gap and end at %d", nx,
                tw, W, W - tw);
    FIE_REQUIRE(cy > 0, "fie_tile_blend_rgb_u8: ys: %d positions of %d-high tiles over %d must start at 0, increase strictly, leave no gap and end at %d", ny,
                th, H, H - th);
    const int64_t nt = (int64_t)nx * ny * th * tw * 3, no = (int64_t)H * W * 3;
    FIE_REQUIRE(tiles + nt <= out || out + no <= tiles, "fie_tile_blend_rgb_u8: the output overlaps the tiles");
    TileBlendGeom g = {};
    g.nx = nx; g.ny = ny; g.th = th; g.tw = tw; g.H = H; g.W = W;
    for (int i = 0; i < nx; ++i) g.xs[i] = xs[i];
    for (int i = 0; i < ny; ++i) g.ys[i] = ys[i];
    const int64_t bound = (int64_t)cy * th * cx * tw;              // S <= bound; 32-bit accumulators hold 256 S up to 2^24 - 1 (see the top of the file)
    const int64_t slots = (int64_t)W * 3 / 4 + 1, groups = ((int64_t)H + kTileBlendRows - 1) / kTileBlendRows;
    const dim3 grid((unsigned)((slots + 255) / 256), (unsigned)(groups < 65535 ? groups : 65535));
    FIE_DESC(ctx, "tile_blend %dx%d of %dx%d -> %dx%d%s", ny, nx, th, tw, H, W, bound < (1 << 24) ? "" : " wide");
    if (bound < (1 << 24))
        fie_launch(ctx, tile_blend_kernel<uint32_t>, grid, dim3(256), 0, tiles, g, out);
    else
        fie_launch(ctx, tile_blend_kernel<uint64_t>, grid, dim3(256), 0, tiles, g, out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
