// The canvas of an outpainting edit and its mask (include/fie.h: fie_outpaint_canvas_rgb_u8).
//   Hc = top + H + bottom, Wc = left + W + right
//   canvas(y, x)      = src(clamp(y - top, 0, H - 1), clamp(x - left, 0, W - 1))           the source, its edge pixels replicated outwards
//   canvas_mask(y, x) = 255 outside the source rectangle, mask_l(y - top, x - left) inside it (0 without a mask): greys pass as they are
// Pure data movement.  One launch: blockIdx.y strides over the canvas rows, the threads of a row's blocks are its "slots" -- first the slots of
// the canvas row (3 Wc bytes), then those of the mask row (Wc bytes).  A row of either output starts wherever the rows before it end, so it is
// cut into a head of 0 .. 3 bytes up to the next dword boundary of its ADDRESS, a body of whole aligned dwords and a tail of 0 .. 3 bytes:
// slot k < body stores dword k, slot k == body stores the head and the tail by bytes.  A dword that lies wholly over the source rectangle is
// four consecutive source bytes at some alignment: they are taken from the one or two ALIGNED dwords that cover them (a funnel shift), where
// those lie inside the operand; everywhere else -- the margins, the seam, an operand's first or last bytes -- a dword is assembled from four
// byte loads.  Every byte is written once, by one thread; no dword access is misaligned, no store reaches past a row's last byte, no load
// past an operand's first or last.  No workspace, no atomics, no block waits for another.
#include "image_ops.h"

namespace {

using fie_img::load4;
using fie_img::row_split;

constexpr int kOutpaintMaxMargin = 4096;

constexpr int kOutpaintRows = 4;           // canvas rows a thread takes, one after the other: enough work per wave to pay for its launch

struct OutpaintGeom {
    int H, W, left, top, Hc, Wc;
    unsigned canvas_slots;                 // 3 Wc / 4 + 1: the most dwords a canvas row can hold, and the slot of its head and tail
};

__device__ __forceinline__ uint8_t canvas_byte(const uint8_t* __restrict__ srow, const OutpaintGeom& g, int x, int c) {
    return srow[(int64_t)min(max(x - g.left, 0), g.W - 1) * 3 + c];
}

// mrow: the mask's row under this canvas row, or NULL when the row lies in the top / bottom margin or there is no mask; `inside_y` tells the two apart
__device__ __forceinline__ uint8_t mask_byte(const uint8_t* __restrict__ mrow, bool inside_y, const OutpaintGeom& g, int x) {
    const int sx = x - g.left;
    if (!inside_y || sx < 0 || sx >= g.W) return 255;
    return mrow ? mrow[sx] : (uint8_t)0;
}

__global__ __launch_bounds__(256) void outpaint_canvas_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ mask_l, OutpaintGeom g,
                                                              uint8_t* __restrict__ canvas, uint8_t* __restrict__ canvas_mask) {
    const unsigned slot = blockIdx.x * 256u + threadIdx.x;
    const int64_t cbytes = (int64_t)g.Wc * 3, sbytes = (int64_t)g.W * 3;
    for (int y = blockIdx.y; y < g.Hc; y += gridDim.y) {
        const int sy = min(max(y - g.top, 0), g.H - 1);
        if (slot < g.canvas_slots) {
            const uint8_t* srow = src + (int64_t)sy * g.W * 3;
            uint8_t* crow = canvas + (int64_t)y * cbytes;
            int head;
            int64_t body;
            row_split(crow, cbytes, head, body);
            if (slot < body) {
                const int64_t j = head + (int64_t)slot * 4, s0 = j - (int64_t)g.left * 3;
                uint32_t v = 0;
                if (s0 >= 0 && s0 + 4 <= sbytes) {
                    v = load4(srow + s0, src, src + (int64_t)g.H * sbytes);
                } else {
                    int x = (int)(j / 3), c = (int)(j - (int64_t)x * 3);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v |= (uint32_t)canvas_byte(srow, g, x, c) << (8 * k);
                        if (++c == 3) { c = 0; ++x; }
                    }
                }
                *reinterpret_cast<uint32_t*>(crow + j) = v;
            } else if (slot == body) {
                for (int64_t j = 0; j < head; ++j) crow[j] = canvas_byte(srow, g, (int)(j / 3), (int)(j % 3));
                for (int64_t j = head + body * 4; j < cbytes; ++j) crow[j] = canvas_byte(srow, g, (int)(j / 3), (int)(j % 3));
            }
        } else {
            const unsigned ms = slot - g.canvas_slots;
            const bool inside_y = y >= g.top && y < g.top + g.H;
            const uint8_t* mrow = (mask_l && inside_y) ? mask_l + (int64_t)sy * g.W : nullptr;
            uint8_t* orow = canvas_mask + (int64_t)y * g.Wc;
            int head;
            int64_t body;
            row_split(orow, g.Wc, head, body);
            if (ms < body) {
                const int x = head + (int)ms * 4, s0 = x - g.left;
                uint32_t v = 0;
                if (mrow && s0 >= 0 && s0 + 4 <= g.W) {
                    v = load4(mrow + s0, mask_l, mask_l + (int64_t)g.H * g.W);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v |= (uint32_t)mask_byte(mrow, inside_y, g, x + k) << (8 * k);
                }
                *reinterpret_cast<uint32_t*>(orow + x) = v;
            } else if (ms == body) {
                for (int x = 0; x < head; ++x) orow[x] = mask_byte(mrow, inside_y, g, x);
                for (int x = head + (int)body * 4; x < g.Wc; ++x) orow[x] = mask_byte(mrow, inside_y, g, x);
            }
        }
    }
}

bool disjoint(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb) { return !a || !b || a + na <= b || b + nb <= a; }

}  // namespace

extern "C" {

int fie_outpaint_canvas_rgb_u8(fie_ctx* ctx, const uint8_t* src, const uint8_t* mask_l, int H, int W, int left, int top, int right, int bottom,
                               uint8_t* canvas, uint8_t* canvas_mask) {
    FIE_REQUIRE(ctx && src && canvas && canvas_mask, "fie_outpaint_canvas_rgb_u8: NULL argument");
    FIE_REQUIRE(H >= 1 && W >= 1, "fie_outpaint_canvas_rgb_u8: source %d x %d: both at least 1", H, W);
    const int margins[4] = {left, top, right, bottom};
    for (int m : margins)
        FIE_REQUIRE(m >= 0 && m <= kOutpaintMaxMargin, "fie_outpaint_canvas_rgb_u8: margins (%d, %d, %d, %d) outside 0 .. %d", left, top, right, bottom,
                    kOutpaintMaxMargin);
    FIE_REQUIRE(left || top || right || bottom, "fie_outpaint_canvas_rgb_u8: all four margins are 0");
    const int64_t Hc = (int64_t)top + H + bottom, Wc = (int64_t)left + W + right;
    FIE_REQUIRE(Hc * Wc < ((int64_t)1 << 31), "fie_outpaint_canvas_rgb_u8: canvas %lld x %lld outside 1 .. 2^31 - 1 pixels", (long long)Hc, (long long)Wc);
    const int64_t n = (int64_t)H * W, nc = Hc * Wc;
    FIE_REQUIRE(disjoint(canvas, 3 * nc, src, 3 * n) && disjoint(canvas, 3 * nc, mask_l, n) && disjoint(canvas_mask, nc, src, 3 * n) &&
                    disjoint(canvas_mask, nc, mask_l, n) && disjoint(canvas, 3 * nc, canvas_mask, nc),
                "fie_outpaint_canvas_rgb_u8: an output overlaps an operand or the other output");
    OutpaintGeom g;
    g.H = H; g.W = W; g.left = left; g.top = top; g.Hc = (int)Hc; g.Wc = (int)Wc;
    g.canvas_slots = (unsigned)(Wc * 3 / 4 + 1);
    const int64_t slots = (int64_t)g.canvas_slots + Wc / 4 + 1;
    FIE_DESC(ctx, "outpaint_canvas %dx%d +(%d,%d,%d,%d)", H, W, left, top, right, bottom);
    const int64_t groups = (Hc + kOutpaintRows - 1) / kOutpaintRows;
    fie_launch(ctx, outpaint_canvas_kernel, dim3((unsigned)((slots + 255) / 256), (unsigned)(groups < 65535 ? groups : 65535)), dim3(256), 0, src, mask_l,
               g, canvas, canvas_mask);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // extern "C"
