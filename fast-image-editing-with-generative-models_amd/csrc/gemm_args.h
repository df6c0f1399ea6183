// The one problem description of the fp16 / fp8 GEMM and 3x3 implicit-GEMM convolution kernels: passed by value to every kernel of gemm_common.h's
// families, and read as it is by the tile selection (gemm_select.h).  No HIP include: the selector and this header are also built by a host compiler
// (tests/test_gemm_select_cpu.py), which must know _Float16 (clang does).
#pragma once
#include <cstdint>

typedef _Float16 half_t;

namespace fie_gemm {

constexpr int BK = 64;

struct GemmArgs {
    const half_t* A1; int64_t lda1; int K1;
    const half_t* A2; int64_t lda2;
    // conv view with 1x1 side inputs (fie_conv3x3_plus_nhwc_f16: a resnet's conv2 + its 1x1 shortcut in one GEMM): after the taps, K-steps
    // C2x / 64 read row m of A2 and C3x / 64 row m of A3 (the shortcut's input, or its two halves [x | skip])
    const half_t* A3; int64_t lda3; int C2x, C3x; int64_t a3_bytes;
    // conv view of A1
    int H, W, Cin, OH, OW, stride, pt, pl, ups;
    const half_t* Wt; int64_t ldw;
    half_t* C; int64_t ldc;
    int M, N, K;
    const half_t* bias;
    const half_t* rowbias; int64_t ld_rowbias; int rows_per_batch;
    const half_t* res; int64_t ldr;
    float scale; int act;
    int nbm, nbn;
    int64_t a1_bytes, a2_bytes, w_bytes;   // operand extents for the v3 buffer descriptors
    // 2x-upsampling conv as four 2x2 convs (fie_conv_up2x_nhwc_f16): taps2 = the conv view has 2x2 taps (K = 4 * Cin) with pt / pl = 1 - parity;
    // oscat = output row m = (b, oh, ow) of the OH x OW view is stored at pixel (2 oh + opy, 2 ow + opx) of the [B, 2 OH, 2 OW] output
    int taps2, oscat, opy, opx;             // oscat 2: all four parities in ONE launch, tile id = 4 * tile + parity (gemm_common.h: take_parity)
    int64_t w_par_stride;                   // oscat 2: elements between the parity weight matrices
    int gn_nch, gn_chunk0;                  // GroupNorm partials: granules per image in the buffer (0: gn_rows / 32) and this launch's first granule
    float* gn_partial; int gn_rows, gn_G, gn_cg;   // GroupNorm statistics of the OUTPUT (fie_gn_stats_target): per image and 32-row granule [b][gn_rows / 32][gn_G][2] = (sum, sum of squares) of the f16-rounded values, gn_cg = N / gn_G in {4, 8, 16} channels per group; NULL: none
    const float* w_scale;                   // fp8 weights (gemm_w8.hip): per-output-channel dequantisation scale [N], applied to the accumulator first; Wt then points at e4m3 bytes and ldw counts bytes
    unsigned* stamps;                       // tile codes 97 / 98: [tile][wave][8] cycle sums of the K-loop segments (fie_debug_gemm_stamps), else NULL
    int epi_prefetch;                       // ring kernels: bias row + residual tile loaded ahead of the K loop (gemm_common.h: EpiPre); 0 = in the epilogue (fie_debug_epilogue_prefetch)
    int probe;                              // timing-only probes (fie_debug_gemm_probe; outputs are wrong): 1 = every DMA load dropped (zero-record descriptors), 2 = every tile fetches tile (0,0)'s operands (all L2 hits), 3 = ring kernels issue no DMA inside the K loop (MFMA + ds_read + barrier floor), 4 = no epilogue (nothing stored)
    // split-K (ring kernels, fie_splitk_workspace): the K-steps of a tile are dealt to `splitk` consecutive blocks (one XCD under the remap); each
    // writes its fp32 partial tile to sk_slabs[tile][slice] (write-through), draws a ticket from sk_tickets[tile]; the block that draws the last
    // ticket sums the slices IN SLICE ORDER (deterministic) and runs the epilogue.  splitk <= 1: off
    int splitk; float* sk_slabs; unsigned* sk_tickets;
    // fp8 activations (gemm_x8.hip, BASELINE config 5): a_scale = dequantisation scale of the e4m3 A operand (0 = none; multiplies the accumulator
    // together with w_scale); out_f8 = the output is written as e4m3 bytes, value * out_inv_scale, saturated to +-448 (C then points at bytes and
    // ldc counts bytes): the consumer GEMM reads it without any conversion
    float a_scale; int out_f8; float out_inv_scale;
    int order;                              // 0: n-tiles fastest (an XCD owns a range of rows), 1: m-tiles fastest (an XCD owns a range of columns)
    // halo-resident conv (conv_halo.hip): a tile is a 16x16 PATCH of one image's output pixels, not 256 consecutive rows.  Fragment j of a wave
    // (16 pixels of one patch row) then starts frag_ld = OW rows after fragment j - 1 instead of 16: the epilogue's row of fragment (wm, j), lane fr
    // is m0 + (wm * FM + j) * frag_ld + fr with m0 = the patch's first pixel.  0 = the ordinary consecutive-row tile (16).
    int frag_ld;
    // LayerNorm folded into the GEMM (fie_gemm_ln_f16; ring tiles 42 / 48 / 96 / 64, LEAN == 2): A1 is the UN-normalised tensor, Wt = W * gamma, and with
    // (mean, rstd) of row m -- summed over the activation fragments on their way to the MFMAs -- C[m, n] = rstd * (acc - mean * ln_tab[n][0]) + ln_tab[n][1],
    // ln_tab[n] = (sum_k Wt[n, k], (W beta)[n] + bias[n]) in fp32 (packed column order).  NULL: none
    const float* ln_tab; float ln_eps;
    const float* gna_tab; int gna_silu;        // conv_halo.hip, GNA: per-(image, channel) GroupNorm coefficients (sc, sh) of the conv's INPUT (fie_groupnorm_coef_f16), applied on the resident halo
};

}  // namespace fie_gemm
