// The fp8 ring tiles, one list per kernel family: X(code, BM, BN, ST, NW).  gemm_w8.hip / gemm_x8.hip generate their attribute setters AND their launch
// switches from these lists (so the two cannot disagree), and the launch table of gemm_select.h checks its fp8 remap columns against them at compile
// time.  A new fp8 tile is one X(...) here plus the w8 / x8 column of the rows of gemm_select.h that should run on it.
#pragma once
// gemm3w8_kernel (fp16 activations x e4m3 weights): 256x128 x 3 stages, 192x128 / 128x128 x 2 stages (8 waves: two and more blocks per CU), 128x64 / 64x64 (4 waves)
#define FIE_W8_TILES(X) X(62, 256, 128, 3, 8) X(54, 192, 128, 2, 8) X(52, 128, 128, 2, 8) X(42, 128, 64, 3, 4) X(43, 64, 64, 3, 4)
// gemm3x8_kernel (e4m3 activations x e4m3 weights): 4-wave tiles with 3 stages, 128x128 / 256x128 with 3 and 128x128 / 192x128 with 2, 256x320 (GEMM view only)
#define FIE_X8_TILES(X) \
    X(42, 128, 64, 3, 4) X(43, 64, 64, 3, 4) X(47, 128, 96, 3, 4) X(51, 128, 128, 3, 8) X(52, 128, 128, 2, 8) X(54, 192, 128, 2, 8) X(62, 256, 128, 3, 8) X(63, 256, 320, 2, 8)

struct fie_f8_tile { int code, bm, bn; };
#define FIE_F8_ROW(code, BM, BN, ST, NW) {code, BM, BN},
constexpr fie_f8_tile kFieW8Tiles[] = {FIE_W8_TILES(FIE_F8_ROW)}, kFieX8Tiles[] = {FIE_X8_TILES(FIE_F8_ROW)};
#undef FIE_F8_ROW
