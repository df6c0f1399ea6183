// K11: RGB -> gray -> Canny(low, high, aperture 3, L1 gradient) on the host, integer exact (include/fie.h:
// fie_canny_rgb_u8).  Replaces cv2.cvtColor(COLOR_RGB2GRAY) + cv2.Canny + 3-channel stack at
// /root/reference/src/pipeline.py:200,205,208.  The reference also runs this step on the host CPU (OpenCV), before
// anything is handed to the device, so this is host logic on both sides of the boundary, not a device fallback.
//
// Algorithm (OpenCV 4.x imgproc semantics): 15-bit fixed-point luma; 3x3 Sobel with replicated
// borders; |dx|+|dy| magnitude with a zero ring; fixed-point tan(22.5 deg) sector test; asymmetric (>, >=)
// non-maximum comparisons; hysteresis as an explicit-stack flood fill from strong pixels.
#include <stdint.h>
#include <stdlib.h>
#include <vector>
#include "fie_internal.h"

namespace {

constexpr int kShift = 15;
constexpr int kTg22 = (int)(0.4142135623730950488016887242097 * (1 << kShift) + 0.5);

inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Gray, Sobel and the L1 magnitudes of an image: dx, dy [H, W]; mag [H + 2, W + 2] with a zero ring.
struct Gradients {
    int MS;
    std::vector<int16_t> dx, dy;
    std::vector<int32_t> mag;
};

Gradients gradients(const uint8_t* rgb, int H, int W) {
    const size_t n = (size_t)H * W;
    std::vector<uint8_t> gray(n);
    for (size_t i = 0; i < n; ++i)
        gray[i] = (uint8_t)((rgb[3 * i] * 9798 + rgb[3 * i + 1] * 19235 + rgb[3 * i + 2] * 3735 + (1 << 14)) >> 15);
    Gradients g{W + 2, std::vector<int16_t>(n), std::vector<int16_t>(n), std::vector<int32_t>((size_t)(H + 2) * (W + 2), 0)};
    for (int y = 0; y < H; ++y) {
        const uint8_t* r0 = &gray[(size_t)clampi(y - 1, 0, H - 1) * W];
        const uint8_t* r1 = &gray[(size_t)y * W];
        const uint8_t* r2 = &gray[(size_t)clampi(y + 1, 0, H - 1) * W];
        for (int x = 0; x < W; ++x) {
            const int xl = clampi(x - 1, 0, W - 1), xr = clampi(x + 1, 0, W - 1);
            const int gx = (r0[xr] + 2 * r1[xr] + r2[xr]) - (r0[xl] + 2 * r1[xl] + r2[xl]);
            const int gy = (r2[xl] + 2 * r2[x] + r2[xr]) - (r0[xl] + 2 * r0[x] + r0[xr]);
            g.dx[(size_t)y * W + x] = (int16_t)gx;
            g.dy[(size_t)y * W + x] = (int16_t)gy;
            g.mag[(size_t)(y + 1) * g.MS + x + 1] = abs(gx) + abs(gy);
        }
    }
    return g;
}

// The non-maximum-suppression direction test of the pixel with magnitude m = mc[x] and gradient (xs, ys); mp, mc, mn: its previous, own and next
// row of the magnitude plane.
inline bool nms_keep(int m, int xs, int ys, const int32_t* mp, const int32_t* mc, const int32_t* mn, int x) {
    const int64_t ax = abs(xs), ay = (int64_t)abs(ys) << kShift;
    const int64_t tg22x = ax * kTg22;
    if (ay < tg22x) return m > mc[x - 1] && m >= mc[x + 1];
    const int64_t tg67x = tg22x + (ax << (kShift + 1));
    if (ay > tg67x) return m > mp[x] && m >= mn[x];
    const int s = (xs ^ ys) < 0 ? -1 : 1;
    return m > mp[x - s] && m > mn[x + s];
}

}  // namespace

extern "C" int fie_canny_rgb_u8(const uint8_t* rgb, int H, int W, int low, int high, uint8_t* edges_rgb) {
    FIE_REQUIRE(rgb && edges_rgb && H > 0 && W > 0, "fie_canny_rgb_u8: bad argument");
    if (low > high) { int t = low; low = high; high = t; }
    const size_t n = (size_t)H * W;
    const Gradients g = gradients(rgb, H, W);
    const int MS = g.MS;
    const std::vector<int16_t>&dx = g.dx, &dy = g.dy;
    const std::vector<int32_t>& mag = g.mag;

    // map: 0 = not an edge, 1 = candidate (weak), 2 = edge
    std::vector<uint8_t> map((size_t)(H + 2) * MS, 0);
    std::vector<int32_t> stack;
    stack.reserve(n / 8 + 16);
    for (int y = 0; y < H; ++y) {
        const int32_t* mp = &mag[(size_t)y * MS + 1];      // previous row
        const int32_t* mc = mp + MS;
        const int32_t* mn = mc + MS;
        uint8_t* mrow = &map[(size_t)(y + 1) * MS + 1];
        for (int x = 0; x < W; ++x) {
            const int m = mc[x];
            if (m <= low) continue;
            const bool keep = nms_keep(m, dx[(size_t)y * W + x], dy[(size_t)y * W + x], mp, mc, mn, x);
            if (!keep) continue;
            if (m > high) {
                mrow[x] = 2;
                stack.push_back((int32_t)((y + 1) * MS + x + 1));
            } else {
                mrow[x] = 1;
            }
        }
    }
    static const int dxy[8][2] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 1}, {1, -1}, {1, 0}, {1, 1}};
    while (!stack.empty()) {
        const int32_t pos = stack.back();
        stack.pop_back();
        for (int k = 0; k < 8; ++k) {
            const int32_t q = pos + dxy[k][0] * MS + dxy[k][1];
            if (map[q] == 1) {
                map[q] = 2;
                stack.push_back(q);
            }
        }
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const uint8_t e = map[(size_t)(y + 1) * MS + x + 1] == 2 ? 255 : 0;
            uint8_t* o = edges_rgb + ((size_t)y * W + x) * 3;
            o[0] = o[1] = o[2] = e;
        }
    return FIE_OK;
}

// Edge-budget thresholds on the host (include/fie.h): the histogram of the ridge magnitudes, high = the smallest h in
// 16 .. 2040 that leaves at most `budget` pixels above it, low = high * lo / hi.  The twin of canny_ridge_kernel + canny_select_kernel.
extern "C" int fie_canny_auto_thresholds_u8(const uint8_t* rgb, int H, int W, int64_t budget, int lo, int hi, int* out) {
    FIE_REQUIRE(rgb && out && H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31) && budget >= 1 && budget <= (int64_t)H * W && lo >= 0 && hi >= 0 &&
                (lo > 0 || hi > 0), "fie_canny_auto_thresholds_u8: bad argument");
    if (lo > hi) { int t = lo; lo = hi; hi = t; }
    const Gradients g = gradients(rgb, H, W);
    std::vector<int64_t> hist(2048, 0);
    for (int y = 0; y < H; ++y) {
        const int32_t* mp = &g.mag[(size_t)y * g.MS + 1];
        const int32_t* mc = mp + g.MS;
        const int32_t* mn = mc + g.MS;
        for (int x = 0; x < W; ++x)
            if (mc[x] > 0 && nms_keep(mc[x], g.dx[(size_t)y * W + x], g.dy[(size_t)y * W + x], mp, mc, mn, x)) ++hist[mc[x]];
    }
    int high = 2040;
    int64_t above = 0;                                      // #{r > h}
    for (int h = 2040; h >= 16 && above <= budget; --h) {
        high = h;
        above += hist[h];
    }
    out[0] = (int)((int64_t)high * lo / hi);
    out[1] = high;
    return FIE_OK;
}
