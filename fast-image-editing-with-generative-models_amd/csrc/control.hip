// Control weights (include/fie.h: fie_control_pyramid_u8, fie_control_add): the ControlNet's residuals weighed per latent position.
//   fie_control_pyramid_u8: the edit-size map e (u8 [H, W]; a binary L mask is read as 255 (L >= 128)) -> the f32 weights of 1 .. 3 pyramid levels in
//     one vector.  One block of one wave per 32 x 32-pixel tile: it sums its pixels in integers -- 8-byte loads, a fixed tree through LDS -- into the
//     tile's 4 x 4 positions of level 0, 2 x 2 of level 1 and 1 of level 2, clipped at the image, and divides once per position.  A level's block
//     is the union of the finer level's blocks that exist (H, W are multiples of 8), so the sums are exact and no block waits for another.
//   fie_control_add: out = u + (s w[p]) t for every residual of one evaluation in one launch.  The table of segments travels by value in the kernel
//     arguments; a block finds its segment from the prefix of block counts in it.  A thread owns whole 8-element groups (16-byte accesses for f16), so
//     no element has two writers.  The product and the sum are two roundings (this file is built with -ffp-contract=off): fie_amd/control.py restates
//     both ops to the bit.  Weights are read from device memory at run time: a hipGraph replay reads the weights of the job it replays.
// No atomics, no workspace.
#include "fie_internal.h"

namespace {

constexpr int kTile = 32;                  // edit-size pixels per block side: one position of the coarsest level
constexpr int kAddGroups = 4;              // 8-element groups per thread: a block of 256 threads covers 8192 elements

__global__ __launch_bounds__(64) void control_pyramid_kernel(const uint8_t* __restrict__ e, int H, int W, int levels, int a, int binary,
                                                             float* __restrict__ out) {
    __shared__ int part[kTile][4];         // the sum of 8 pixels: row r of the tile, 8-byte chunk c
    __shared__ int e0[4][4];               // level 0: the tile's 4 x 4 blocks of 8 x 8 pixels
    const int t = (int)threadIdx.x, cx = t & 3;
    const int x = (int)blockIdx.x * kTile + cx * 8;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (t >> 2) + 16 * j, y = (int)blockIdx.y * kTile + r;
        int sum = 0;
        if (y < H && x < W) {              // W % 8 == 0: a chunk is inside the image or outside it
            const uint2 v = *reinterpret_cast<const uint2*>(e + (int64_t)y * W + x);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int px = (int)(((b < 4 ? v.x : v.y) >> (8 * (b & 3))) & 255u);
                sum += binary ? (px >= 128 ? 255 : 0) : px;
            }
        }
        part[r][cx] = sum;
    }
    __syncthreads();
    if (t < 16) {
        int sum = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) sum += part[(t >> 2) * 8 + r][t & 3];
        e0[t >> 2][t & 3] = sum;
    }
    __syncthreads();
    const int h0 = H / 8, w0 = W / 8, h1 = (h0 + 1) / 2, w1 = (w0 + 1) / 2, w2 = (w1 + 1) / 2;
    // thread t < 16: level 0 position t; 16 .. 19: level 1; 20: level 2.  cnt counts the 8 x 8 blocks of the position that lie inside the image
    int lvl, py, px, side;
    if (t < 16) { lvl = 0; py = t >> 2; px = t & 3; side = 1; }
    else if (t < 20) { lvl = 1; py = (t - 16) >> 1; px = (t - 16) & 1; side = 2; }
    else if (t == 20) { lvl = 2; py = 0; px = 0; side = 4; }
    else return;
    if (lvl >= levels) return;
    int E = 0, blocks = 0;
    for (int dy = 0; dy < side; ++dy)
        for (int dx = 0; dx < side; ++dx) {
            const int by = py * side + dy, bx = px * side + dx;
            if ((int)blockIdx.y * 4 + by < h0 && (int)blockIdx.x * 4 + bx < w0) {
                E += e0[by][bx];
                ++blocks;
            }
        }
    if (blocks == 0) return;               // the position lies outside the image
    const int wl = lvl == 0 ? w0 : lvl == 1 ? w1 : w2;
    const int off = lvl == 0 ? 0 : lvl == 1 ? h0 * w0 : h0 * w0 + h1 * w1;
    const int gy = (int)blockIdx.y * (4 / side) + py, gx = (int)blockIdx.x * (4 / side) + px;
    const int den = 255 * 256 * 64 * blocks;                   // <= 255 * 256 * 1024 < 2^31
    const int num = den - (256 - a) * E;
    out[off + gy * wl + gx] = (float)num / (float)den;         // one IEEE division
}

struct AddTable {                          // by value in the kernel arguments: 16 segments, 776 bytes
    const void* u[FIE_CONTROL_MAX_SEGMENTS];
    const void* t[FIE_CONTROL_MAX_SEGMENTS];
    void* out[FIE_CONTROL_MAX_SEGMENTS];
    unsigned cg[FIE_CONTROL_MAX_SEGMENTS];      // C / 8
    unsigned P[FIE_CONTROL_MAX_SEGMENTS];
    unsigned groups[FIE_CONTROL_MAX_SEGMENTS];  // rows * C / 8
    unsigned woff[FIE_CONTROL_MAX_SEGMENTS];
    float s[FIE_CONTROL_MAX_SEGMENTS];
    unsigned blk0[FIE_CONTROL_MAX_SEGMENTS + 1];   // the first block of every segment, and the grid
    int count;
};

template <typename T>
__global__ __launch_bounds__(256) void control_add_kernel(const AddTable tab, const float* __restrict__ w, unsigned p_tot, unsigned rows_per_image) {
    int seg = 0;                           // block-uniform: a scalar scan of the prefix
    while (seg + 1 < tab.count && blockIdx.x >= tab.blk0[seg + 1]) ++seg;
    const T* __restrict__ u = static_cast<const T*>(tab.u[seg]);
    const T* __restrict__ t = static_cast<const T*>(tab.t[seg]);
    T* __restrict__ out = static_cast<T*>(tab.out[seg]);
    const unsigned cg = tab.cg[seg], P = tab.P[seg], groups = tab.groups[seg], woff = tab.woff[seg];
    const float s = tab.s[seg];
    const unsigned g0 = (blockIdx.x - tab.blk0[seg]) * (256 * kAddGroups) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kAddGroups; ++j) {
        const unsigned g = g0 + j * 256;   // consecutive lanes, consecutive 16 / 32 bytes
        if (g >= groups) break;
        const unsigned row = g / cg, b = row / P, p = row - b * P;
        const float c = s * w[(size_t)(b / rows_per_image) * p_tot + woff + p];
        const size_t at = (size_t)g * 8;
        if (c == 0.0f) {                   // u's bits; t is not read
            constexpr int kVec = sizeof(T) * 8 / 16;
#pragma unroll
            for (int v = 0; v < kVec; ++v) reinterpret_cast<uint4*>(out + at)[v] = reinterpret_cast<const uint4*>(u + at)[v];
        } else {
            float x[8], y[8];
            fie_load8(u + at, x);
            fie_load8(t + at, y);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float q = c * y[e];
                x[e] = x[e] + q;
            }
            fie_store8(out + at, x);
        }
    }
}

}  // namespace

extern "C" {

int fie_control_pyramid_u8(fie_ctx* ctx, const uint8_t* e, int H, int W, int levels, int a, int binary, float* out) {
    FIE_REQUIRE(ctx && e && out, "fie_control_pyramid_u8: NULL argument");
    FIE_REQUIRE(H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && H <= 2048 && W <= 2048,
                "fie_control_pyramid_u8: H = %d, W = %d: multiples of 8 in 8 .. 2048", H, W);
    FIE_REQUIRE(levels >= 1 && levels <= FIE_CONTROL_MAX_LEVELS, "fie_control_pyramid_u8: levels = %d outside 1 .. %d", levels, FIE_CONTROL_MAX_LEVELS);
    FIE_REQUIRE(a >= 0 && a <= 255, "fie_control_pyramid_u8: a = %d outside 0 .. 255", a);
    FIE_REQUIRE(binary == 0 || binary == 1, "fie_control_pyramid_u8: binary = %d: 0 (a level map) or 1 (an L mask)", binary);
    FIE_REQUIRE((uintptr_t)e % 8 == 0 && (uintptr_t)out % 4 == 0, "fie_control_pyramid_u8: e must be 8-byte aligned, out 4-byte aligned");
    const dim3 grid((unsigned)((W + kTile - 1) / kTile), (unsigned)((H + kTile - 1) / kTile));
    FIE_DESC(ctx, "control_pyramid %dx%d levels=%d a=%d %s", H, W, levels, a, binary ? "mask" : "levels");
    fie_launch(ctx, control_pyramid_kernel, grid, dim3(64), 0, e, H, W, levels, a, binary, out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

int fie_control_add(fie_ctx* ctx, const fie_control_table* table, const float* w, int64_t p_tot, int rows_per_image, int f32) {
    FIE_REQUIRE(ctx && table && w, "fie_control_add: NULL argument");
    FIE_REQUIRE(table->count >= 1 && table->count <= FIE_CONTROL_MAX_SEGMENTS, "fie_control_add: %d segments outside 1 .. %d", table->count,
                FIE_CONTROL_MAX_SEGMENTS);
    FIE_REQUIRE(p_tot >= 1 && p_tot < ((int64_t)1 << 24), "fie_control_add: p_tot %lld outside 1 .. 2^24 - 1", (long long)p_tot);
    FIE_REQUIRE(rows_per_image >= 1, "fie_control_add: rows_per_image %d < 1", rows_per_image);
    FIE_REQUIRE(f32 == 0 || f32 == 1, "fie_control_add: f32 = %d: 0 (f16) or 1", f32);
    FIE_REQUIRE((uintptr_t)w % 4 == 0, "fie_control_add: w must be 4-byte aligned");
    AddTable tab;
    memset(&tab, 0, sizeof(tab));
    tab.count = table->count;
    int64_t blocks = 0, elems = 0;
    for (int i = 0; i < table->count; ++i) {
        const int64_t C = table->C[i], P = table->P[i], rows = table->rows[i], woff = table->woff[i];
        FIE_REQUIRE(table->u[i] && table->t[i] && table->out[i], "fie_control_add: segment %d: NULL tensor", i);
        FIE_REQUIRE((uintptr_t)table->u[i] % 16 == 0 && (uintptr_t)table->t[i] % 16 == 0 && (uintptr_t)table->out[i] % 16 == 0,
                    "fie_control_add: segment %d: u, t and out must be 16-byte aligned", i);
        FIE_REQUIRE(table->out[i] != table->u[i] && table->out[i] != table->t[i], "fie_control_add: segment %d: out is a tensor of its own", i);
        FIE_REQUIRE(C >= 8 && C % 8 == 0 && C <= (1 << 16), "fie_control_add: segment %d: C = %lld: a multiple of 8 in 8 .. 65536 (C %% 8 == 0)", i, (long long)C);
        FIE_REQUIRE(P >= 1 && rows >= P && rows % P == 0, "fie_control_add: segment %d: rows = %lld is no positive multiple of P = %lld", i,
                    (long long)rows, (long long)P);
        FIE_REQUIRE(rows * (C / 8) < ((int64_t)1 << 31), "fie_control_add: segment %d: %lld x %lld elements are too many", i, (long long)rows, (long long)C);
        FIE_REQUIRE(woff >= 0 && woff + P <= p_tot, "fie_control_add: segment %d: weights %lld .. %lld outside the vector of %lld", i, (long long)woff,
                    (long long)(woff + P), (long long)p_tot);
        FIE_REQUIRE(table->s[i] == table->s[i], "fie_control_add: segment %d: the scale is a NaN", i);
        tab.u[i] = table->u[i]; tab.t[i] = table->t[i]; tab.out[i] = table->out[i];
        tab.cg[i] = (unsigned)(C / 8); tab.P[i] = (unsigned)P; tab.groups[i] = (unsigned)(rows * (C / 8)); tab.woff[i] = (unsigned)woff;
        tab.s[i] = table->s[i];
        tab.blk0[i] = (unsigned)blocks;
        blocks += (rows * (C / 8) + 256 * kAddGroups - 1) / (256 * kAddGroups);
        elems += rows * C;
    }
    FIE_REQUIRE(blocks < ((int64_t)1 << 31), "fie_control_add: %lld blocks are too many for one launch", (long long)blocks);
    for (int i = table->count; i <= FIE_CONTROL_MAX_SEGMENTS; ++i) tab.blk0[i] = (unsigned)blocks;
    FIE_DESC(ctx, "control_add %d segments %lld elements rows_per_image=%d %s", table->count, (long long)elems, rows_per_image, f32 ? "f32" : "f16");
    if (f32)
        fie_launch(ctx, control_add_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, tab, w, (unsigned)p_tot, (unsigned)rows_per_image);
    else
        fie_launch(ctx, control_add_kernel<half_t>, dim3((unsigned)blocks), dim3(256), 0, tab, w, (unsigned)p_tot, (unsigned)rows_per_image);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
