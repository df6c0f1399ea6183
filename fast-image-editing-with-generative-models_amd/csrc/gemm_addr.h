// The address arithmetic of the GEMM / implicit-GEMM convolution kernels, stated once (gemm_conv.hip, gemm8.hip, gemm_w8.hip, gemm_x8.hip, f32.hip
// and the parity scatter of gemm_common.h's epilogue): which tile a block owns, which input pixel a (output row, tap) of the im2col view reads or
// whether it is padding, and which K-steps a split-K slice runs.  Plain integers only, no builtins: a host compiler builds this header too
// (tests/test_gemm_addr_cpu.py checks every function against a brute-force answer).  What stays in each kernel is what decides its registers and
// schedule: the loops, the per-piece arrays, the byte offsets with the kernel's own element size, kOob and the issue lambdas.
// conv_halo.hip addresses a resident halo, a different scheme, and does not come through here.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FIE_ADDR_FN __host__ __device__ __forceinline__
#else
#define FIE_ADDR_FN inline
#endif

namespace fie_gemm {

// ---- which tile: block id (after the XCD remap) -> first row / column.  order 0: n-tiles fastest, 1: m-tiles fastest (GemmArgs::order).
// (Two functions of one int each: returned as a pair -- a struct by value, or a constructor -- the same arithmetic changed the instruction order of
// GEMM-view kernels, which must keep their text: profiles/gemm_addr_shared.md.  gemm3_kernel spells the two lines out for the same reason.)
template <int BM>
FIE_ADDR_FN int tile_m0(int order, int nbm, int nbn, int bid) { return (order ? bid % nbm : bid / nbn) * BM; }
template <int BN>
FIE_ADDR_FN int tile_n0(int order, int nbm, int nbn, int bid) { return (order ? bid / nbm : bid % nbn) * BN; }

// ---- the im2col view of an NHWC tensor [B, H, W, Cin]: output row m = (b, oh, ow) of a [B, OH, OW] output, K = (tap, channel).
// Tap (ky, kx) of row m reads pixel (oh * stride - pt + ky, ow * stride - pl + kx) of the image -- of its nearest-2x enlargement when ups == 1,
// that is input pixel (ih >> 1, iw >> 1) -- and zero outside it.  taps2: 2x2 taps instead of 3x3 (the parity convs of fie_conv_up2x_nhwc_f16).
struct ConvGeom { int M, OH, OW, H, W, Cin, stride, pt, pl, ups, taps2; };

// output row -> (image, output pixel): the one division of a row number by the image size (the epilogue's parity scatter uses it as it is)
struct OutPixel { int b, oh, ow; };
FIE_ADDR_FN OutPixel out_pixel(int OH, int OW, int m) {
    const int hw = OH * OW;
    const int b = m / hw, rem = m - b * hw;
    const int oh = rem / OW;
    return {b, oh, rem - oh * OW};
}

// output row -> image and top-left input coordinate (tap (0, 0)); ok: the row exists (evaluated first, as the kernels always did: evaluated
// last, 16 conv views order their instructions differently)
struct ConvRow { int b, ih0, iw0; bool ok; };
FIE_ADDR_FN ConvRow conv_row(const ConvGeom& g, int m) {
    const bool ok = m < g.M;
    const OutPixel o = out_pixel(g.OH, g.OW, m);
    return {o.b, o.oh * g.stride - g.pt, o.ow * g.stride - g.pl, ok};
}

// tap number (ky-major) -> (ky, kx); 3x3: tap / 3 as a multiply and a shift, exact for tap <= 9
struct TapYX { int ky, kx; };
FIE_ADDR_FN TapYX tap_yx(const ConvGeom& g, int tap) {
    const int ky = g.taps2 ? tap >> 1 : (tap * 11) >> 5;
    return {ky, g.taps2 ? tap & 1 : tap - 3 * ky};
}

FIE_ADDR_FN int conv_taps(const ConvGeom& g) { return g.taps2 ? 4 : 9; }

// the padding test and the source pixel, separately for the kernels that select between an offset and kOob themselves ...
FIE_ADDR_FN bool conv_inside(const ConvGeom& g, const ConvRow& r, int ky, int kx) {
    const int ih = r.ih0 + ky, iw = r.iw0 + kx;
    return r.ok && ih >= 0 && ih < (g.H << g.ups) && iw >= 0 && iw < (g.W << g.ups);
}
FIE_ADDR_FN int conv_index(const ConvGeom& g, const ConvRow& r, int ky, int kx) {
    return ((r.ih0 + ky) >> g.ups) * g.W + ((r.iw0 + kx) >> g.ups);
}
// ... and as one value: the pixel index inside image r.b, -1 for padding or a row past M
FIE_ADDR_FN int conv_pixel(const ConvGeom& g, const ConvRow& r, int ky, int kx) {
    return conv_inside(g, r, ky, kx) ? conv_index(g, r, ky, kx) : -1;
}

// ---- split-K: slice `slice` of `nsplit` runs K-steps [kbeg, kbeg + nk) of nk_all; conv view with csteps K-steps per tap: it starts at
// tap ftap, channel step cs (in the middle of a tap when cs != 0).  A kernel that never splits K has no slice to pass and starts at (0, 0).
// (A constructor for the reason given at tile_m0: nothing is returned by value.)
struct KSlice {
    int kbeg, nk, ftap, cs;
    FIE_ADDR_FN KSlice(int nk_all, int slice, int nsplit, int csteps)
        : kbeg((int)((int64_t)nk_all * slice / nsplit)), nk((int)((int64_t)nk_all * (slice + 1) / nsplit) - kbeg), ftap(kbeg / csteps), cs(kbeg - ftap * csteps) {}
};

}  // namespace fie_gemm
