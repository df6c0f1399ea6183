// Which kernel a GEMM / 3x3 conv launch gets: the launch table's data rows, the encoded choice (tile code, tile order, split-K factor), the
// eligibility predicates of the kernel families, the built-in rule, the tile-order estimate, the split-K fit, the tuner's candidate list and the
// fallback of a remembered choice.  Everything that decides and nothing that launches: plain C++17 on a GemmArgs and a SelectEnv, no HIP include, so a
// host compiler builds it into a stand-alone program (tests/test_gemm_select_cpu.py replays tests/golden/launch_problems.json through it: a rule
// edited here is checked without a GPU).  gemm_conv.hip adds the launchers to the rows and runs the choice; conv_halo.hip / conv_thin.hip ask the
// predicates again before they launch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <iterator>
#include <vector>

#include "../../include/fie.h"
#include "gemm_args.h"
#include "gemm_tiles.h"

namespace fie_gemm {

// ---- the choice: what fie_debug_force_tile / fie_debug_tile_override take, what the tuner remembers and reports, and the code= token of the oplog,
// as one integer = split-K factor * kSplit + (1000: n-tiles fastest / 2000: m-tiles fastest, forced; none: estimated) + tile code.  Nothing else
// takes such an integer apart or puts one together.
struct Choice {
    int code = 0;
    int order = -1;                // 0: n-tiles fastest (an XCD owns a range of activation rows), 1: m-tiles fastest; -1: estimate (tile_order)
    int split = 1;
    static constexpr int kSplit = 10000;        // also the fie_debug_tune_exclude entry that stands for every split-K variant
    constexpr int encode() const { return (split > 1 ? split : 0) * kSplit + (order < 0 ? 0 : order ? 2000 : 1000) + code; }
    static constexpr Choice decode(int v) { return {v % kSplit % 1000, v % kSplit >= 2000 ? 1 : v % kSplit >= 1000 ? 0 : -1, v / kSplit > 1 ? v / kSplit : 1}; }
};

// ---- the launch table: ONE row per tile code.  Everything the host knows about a code is in its row, the arguments its launcher is built from
// included (gemm_conv.hip: kLaunch makes the launchers from the rows, by family); a new tile is one row here (and, for an fp8 kernel, one entry in
// gemm_tiles.h).
enum Family { kGeneric, kRing, kPhased, kHalo, kHaloEdge, kThin };      // kGeneric and kThin serve shapes the LDS-DMA kernels cannot address (no dma_ok needed)
// flags: may split K (ring kernels with <= 16 accumulator fragments per lane, no stamps); writes cycle stamps (fie_debug_gemm_stamps: slower, for
// tools/kstep_stamps.py only; on a ring row also the kernel's STAMP); no conv-view build; has an LN-folded build (LEAN == 2); ring rows: the kernel's PF / ALT
enum : unsigned { kSplitK = 1, kStamps = 2, kGemmOnly = 4, kLnFold = 8, kPF = 16, kAlt = 32 };
struct Tile {
    int code, bm, bn;
    Family family;
    const char* name;               // the kernel family as fie_debug_last_gemm_kernel prints it
    unsigned flags;
    int w8, x8;                     // the code that runs in its place with fp8 weights (gemm_w8.hip) / fp8 activations x weights (gemm_x8.hip); 0 = none
    int p0 = 0, p1 = 0;             // the launcher's own arguments.  Ring rows: ring stages, waves (ST, NW of gemm3_kernel); phased and halo rows: p0 = the variant of fie_launch_gemm8 / fie_launch_conv_halo
};

// Columns: code, bm, bn, family, name, flags, w8, x8, p0, p1.  With fp8 WEIGHTS every code runs on one of the five W8 tiles (its own shape where that
// is built, 256x128 otherwise; the halo rows never get there: their eligibility test refuses fp8 weights first); with fp8 ACTIVATIONS a code without a
// stand-in is refused.
constexpr Tile kTiles[] = {
    {1, 128, 128, kGeneric, "gemm_kernel", 0, 62, 43},      // gemm_kernel: any shape
    {2, 128, 64, kGeneric, "gemm_kernel", 0, 42, 42},
    {3, 64, 64, kGeneric, "gemm_kernel", 0, 43, 43},
    {42, 128, 64, kRing, "gemm3_kernel", kSplitK | kLnFold, 42, 42, 3, 4},      // 128x64 / 64x64, 3 stages, 4 waves (two / three blocks per CU)
    {43, 64, 64, kRing, "gemm3_kernel", kSplitK, 43, 43, 3, 4},
    {44, 128, 64, kRing, "gemm3_kernel", kSplitK, 42, 42, 2, 4},                // the same tiles with 2 stages (three / five blocks per CU)
    {46, 64, 64, kRing, "gemm3_kernel", kSplitK, 43, 43, 2, 4},
    // 128x96, 3 stages, 4 waves: 224 tiles for M 2048 x N 1280 (one per CU, each streaming a 96-row weight tile: the 32x32-latent convs lose nothing
    // on cold weights with it, 7-9 % with 128x128)
    {47, 128, 96, kRing, "gemm3_kernel", kSplitK, 62, 47, 3, 4},
    // 128x80, 3 stages, 4 waves stacked along the rows (wave tile 32x80); M 2048 x N 1280 = 256 tiles, one per CU.  Weight rows past the packed matrix
    // (80 does not divide Npad) read as zero through the descriptor.  (Its LN-folded build returned wrong values in 16-row x 1-column spots on a loaded
    // chip, in every form tried, while 42 / 96 / 64 never did, and is NOT built: profiles/r04_ln_fold_tile48_anomaly.md; tests/test_ops_gpu.py screens the three that ship)
    {48, 128, 80, kRing, "gemm3_kernel", kSplitK, 62, 0, 3, 4},
    {51, 128, 128, kRing, "gemm3_kernel", kSplitK, 62, 51, 3, 8},               // 128x128, 3 stages, 8 waves
    {52, 128, 128, kRing, "gemm3_kernel", kSplitK, 52, 52, 2, 8},               // 128x128 / 192x128, 2 stages, 8 waves: two blocks per CU
    {54, 192, 128, kRing, "gemm3_kernel", kSplitK, 54, 54, 2, 8},
    {61, 256, 256, kRing, "gemm3_kernel", 0, 62, 62, 2, 8},                     // 256x256 x 2 stages / 256x128 x 3 stages, 8 waves
    {62, 256, 128, kRing, "gemm3_kernel", kSplitK, 62, 62, 3, 8},
    // 256x320 x 2 stages, 8 waves (wave tile 128x80): exactly ONE tile per CU for the FF1 projection M 2048 x N 10240 (256 tiles) and two rounds for
    // M 8192 x N 5120; 142 FLOP per staged byte pair against 85 for 256x128
    {63, 256, 320, kRing, "gemm3_kernel", kGemmOnly, 62, 63, 2, 8},
    // 63 with the two wave groups taking turns at a K-step's LDS-DMA refill (kAlt): FF1 56.5 us against 59.5-63.4 (the same idea on 256x128 x 3
    // stages was 3 % SLOWER than 62 and is not built: the barrier still paces both groups by the slower one).  No alternating-refill form of the fp8 kernels
    {64, 256, 320, kRing, "gemm3_kernel", kGemmOnly | kAlt | kLnFold, 62, 63, 2, 8},
    // 51 / 62 with fragment reads one half K-step ahead of the MFMAs (the 4-wave and 2-stage tiles gain nothing from it)
    {95, 128, 128, kRing, "gemm3_kernel+prefetch", kPF | kSplitK, 62, 51, 3, 8},
    {96, 256, 128, kRing, "gemm3_kernel+prefetch", kPF | kSplitK | kLnFold, 62, 62, 3, 8},
    // 62 / 96 / 42 with in-kernel cycle stamps.  97 and 94 do NOT prefetch: their printed name is a misnomer of the old `code >= 90` rule that tests,
    // tools and bench.py parse; fixing it is a change of its own
    {97, 256, 128, kRing, "gemm3_kernel+prefetch", kStamps, 62, 0, 3, 8},
    {98, 256, 128, kRing, "gemm3_kernel+prefetch", kPF | kStamps, 62, 0, 3, 8},
    {94, 128, 64, kRing, "gemm3_kernel+prefetch", kStamps, 62, 0, 3, 4},
    {81, 256, 256, kPhased, "gemm8_kernel", 0, 62, 62, 0},      // gemm8.hip: 256x256 phased
    {82, 256, 256, kPhased, "gemm8_kernel", 0, 62, 0, 1},       // A/B: second DMA piece of each phase inside the MFMA cluster (measured slower)
    // conv_halo.hip: a 16x16 output patch x 128 channels per block, the patch's 18x18 halo resident in LDS per 64-channel chunk, weights through a ring;
    // stride-1 same-size convs with H, W % 16 == 0 only (73: with cycle stamps).  K is summed chunk-major (the im2col kernels: tap-major): equal to the
    // other codes to rounding, not bit for bit
    {71, 256, 128, kHalo, "conv_halo_kernel", 0, 62, 0, 0},
    {73, 256, 128, kHalo, "conv_halo_kernel", kStamps, 62, 0, 1},
    // the same K loop in persistent blocks that prefetch their next tile and defer a tile's stores into the next tile's first chunk (74: with cycle
    // stamps, 76: the 8-byte-store form, A/B); 72 is THE RULE for eligible convs (heuristic_code)
    {72, 256, 128, kHalo, "conv_halo2_kernel", 0, 62, 0, 2},
    {74, 256, 128, kHalo, "conv_halo2_kernel", kStamps, 62, 0, 4},
    {76, 256, 128, kHalo, "conv_halo2_kernel", 0, 62, 0, 5},
    // ... with edge patches: maps whose height or width is not a multiple of 16 (the aspect-ratio buckets); the patch grid is rounded up, stores of pixels
    // outside the image are dropped per lane; no GroupNorm sums.  The rule for eligible convs, under 72's threshold.  Sums chunk-major like 71-76
    {78, 256, 128, kHaloEdge, "conv_halo2_kernel+edge", 0, 62, 0, 6},
    {77, 64, 16, kThin, "conv_thin_kernel", 0, 62, 0},      // conv_thin.hip: at most 16 output channels, by rule; its launcher refuses GEMM arguments itself
};
constexpr const Tile* find_tile(int code) {
    for (const Tile& t : kTiles)
        if (t.code == code) return &t;
    return nullptr;
}
constexpr bool is_family(int code, Family f) { return find_tile(code) && find_tile(code)->family == f; }

// What the tuner times besides the rule's code, in timing order (the order decides ties): plain tile codes (tune_candidates filters them), then the
// split-K choices (split 2..4) of the split lists, offered while the tile's grid stays under per_cu blocks per CU
constexpr int kCandF16[] = {43, 46, 42, 44, 51, 52, 54, 96, 81, 63, 47, 48, 64, 72, 78};      // 47 (128x96): FIE_TUNE_47=0 leaves it out
constexpr int kCandW8[] = {43, 42, 62, 52, 54};
constexpr int kCandX8[] = {43, 42, 47, 51, 52, 54, 62, 63};
struct SplitCand { int code, per_cu; };
constexpr SplitCand kSplitF16[] = {{96, 1}, {95, 1}, {47, 1}, {54, 2}, {52, 2}};
constexpr SplitCand kSplitX8[] = {{62, 1}, {51, 1}, {47, 1}, {54, 2}, {52, 2}};

// ---- the checks the hand-kept lists never had: 0, or the number of the first rule the tables break (rule 4, a missing view is declared, reads the
// launchers and is gemm_conv.hip's)
template <size_t N>
constexpr bool f8_built(const fie_f8_tile (&built)[N], int code) {      // a kernel of that precision with the row's tile shape
    const Tile* t = find_tile(code);
    for (const fie_f8_tile& b : built)
        if (t && b.code == code && b.bm == t->bm && b.bn == t->bn) return true;
    return false;
}
constexpr int table_error() {
    for (const Tile& t : kTiles) {
        int n = 0;
        for (const Tile& u : kTiles) n += u.code == t.code;
        if (n != 1) return 1;                                                                       // codes are unique
        if (!f8_built(kFieW8Tiles, t.w8) || (t.x8 && !f8_built(kFieX8Tiles, t.x8))) return 2;       // a remap target is a row with a kernel of that precision
        if ((t.flags & kSplitK) && t.family != kRing) return 3;                                     // only the ring kernels reduce split K
    }
    for (int c : kCandF16) if (!find_tile(c)) return 5;                                                // every candidate is a row, with a kernel of its precision
    for (int c : kCandW8) if (!f8_built(kFieW8Tiles, c)) return 6;
    for (int c : kCandX8) if (!f8_built(kFieX8Tiles, c)) return 7;
    for (const SplitCand& c : kSplitF16) if (!find_tile(c.code) || !(find_tile(c.code)->flags & kSplitK)) return 8;
    for (const SplitCand& c : kSplitX8) if (!f8_built(kFieX8Tiles, c.code) || !(find_tile(c.code)->flags & kSplitK)) return 9;
    return 0;
}
static_assert(table_error() == 0, "kTiles / candidate lists inconsistent: see table_error for the rule with that number");

// ---- eligibility
// LDS-DMA kernels (codes >= 40): 32-bit buffer offsets (operands < 2 GiB) and K-steps that never straddle a 3x3 tap / the A1|A2 seam
// (A = [A1 | A2]: K1 AND K multiples of 64 -- the last, partial K-step of these kernels is issued from A1's descriptor, which is A2's tail there)
// ... and an epilogue on 32-bit buffer offsets (gemm_common.h): output / residual spans of at most 1 GiB
inline bool dma_ok(const GemmArgs& a, bool conv) {
    const int64_t c_span = ((int64_t)((a.oscat ? 4 * (int64_t)a.M : a.M) - 1) * a.ldc + a.N) * 2, r_span = a.res ? ((int64_t)(a.M - 1) * a.ldr + a.N) * 2 : 0;
    return a.a1_bytes < (1ll << 31) && a.a2_bytes < (1ll << 31) && a.w_bytes < (1ll << 31) && c_span <= (1ll << 30) && r_span <= (1ll << 30) &&
           (conv ? a.Cin % (a.a_scale != 0.f ? 2 * BK : BK) == 0 : (a.K1 == a.K || (a.K1 % BK == 0 && a.K % BK == 0)));
}

constexpr int BNH = 128;        // conv_halo.hip: output channels per block

// Shapes the halo-resident kernel takes: the plain same-size conv (stride 1, zero padding 1, no up-sampling gather, no 1x1 side inputs, fp16
// weights) on maps whose height and width are multiples of 16, Cin % 64 == 0, operands the 32-bit buffer offsets reach (checked by the caller: dma_ok)
inline bool fie_conv_halo_ok(const GemmArgs& a) {
    const bool base = a.stride == 1 && !a.ups && !a.taps2 && !a.oscat && a.pt == 1 && a.pl == 1 && a.H == a.OH && a.W == a.OW && a.OH % 16 == 0 &&
                      a.OW % 16 == 0 && a.Cin % BK == 0 && a.Cin >= BK && !a.w_scale && !a.out_f8 && a.splitk <= 1;
    if (!base) return false;
    if (!a.A2) return !a.A3 && a.K == 9 * a.Cin;
    // 1x1 side inputs (conv2 + shortcut): the persistent form only, so everything that form asks for
    return a.C2x % BK == 0 && a.C3x % BK == 0 && a.C2x > 0 && (a.A3 != nullptr) == (a.C3x > 0) && a.K == 9 * a.Cin + a.C2x + a.C3x && a.Cin >= 2 * BK && a.N % BNH == 0 &&
           !a.res && !a.rowbias && a.act == FIE_ACT_NONE && a.scale == 1.f && a.lda2 * 2 * (int64_t)a.OW * a.OH < (1ll << 31) && a.lda3 * 2 * (int64_t)a.OW * a.OH < (1ll << 31);
}

// Edge patches (tile code 78): the same conv on maps whose height or width is NOT a multiple of 16 (at least one side; maps of whole patches keep
// codes 71-76, so no shape changes kernels), in the persistent form only, so everything that form asks for: Cin >= 128, no activation / scale, row bias
// and residual never together.  N % 64 == 0 (not 128): a wave whose 64 channels lie past N drops its stores per lane like a pixel outside the image;
// its weight rows are the packing's zero rows (Npad = N rounded up to 128), so every DMA piece is a real load.  No GroupNorm sums (their granules are 32-pixel halves of whole patches)
inline bool fie_conv_halo_edge_ok(const GemmArgs& a) {
    const bool base = a.stride == 1 && !a.ups && !a.taps2 && !a.oscat && a.pt == 1 && a.pl == 1 && a.H == a.OH && a.W == a.OW && a.OH > 0 && a.OW > 0 &&
                      (a.OH % 16 != 0 || a.OW % 16 != 0) && a.M % (a.OH * a.OW) == 0 && a.Cin % BK == 0 && a.Cin >= 2 * BK && !a.w_scale && !a.out_f8 &&
                      a.splitk <= 1 && a.N % 64 == 0 && a.ldc >= a.N && !a.gn_partial && !a.gna_tab && a.act == FIE_ACT_NONE && a.scale == 1.f && !(a.rowbias && a.res);
    if (!base) return false;
    if (!a.A2) return !a.A3 && a.K == 9 * a.Cin;
    return a.C2x % BK == 0 && a.C3x % BK == 0 && a.C2x > 0 && (a.A3 != nullptr) == (a.C3x > 0) && a.K == 9 * a.Cin + a.C2x + a.C3x && !a.res && !a.rowbias &&
           a.lda2 * 2 * (int64_t)a.OW * a.OH < (1ll << 31) && a.lda3 * 2 * (int64_t)a.OW * a.OH < (1ll << 31);
}

// 16x16 patches of the output (the row blocks of the halo-resident kernels), partial ones at the edges counted
inline int64_t fie_conv_halo_patches(const GemmArgs& a) {
    if (a.OH <= 0 || a.OW <= 0) return 0;
    return (int64_t)(a.M / (a.OH * a.OW)) * ((a.OH + 15) / 16) * ((a.OW + 15) / 16);
}

// GNA (the input's GroupNorm + SiLU applied on the resident halo): the persistent form, ONE image, GroupNorm sums armed for the output (every resnet conv
// of the VAE has them), no row bias, no side inputs, Cin <= 1024 (an 8 KiB coefficient table behind the dump), as many column tiles as fit the grid
inline bool fie_conv_halo_gna_ok(const GemmArgs& a) {
    if (!fie_conv_halo_ok(a) || a.A2 || a.rowbias) return false;
    const int nbn = (a.N + BNH - 1) / BNH;
    return a.M == a.OH * a.OW && a.Cin >= 2 * BK && a.Cin <= 1024 && a.N % BNH == 0 && nbn <= 64 && a.act == FIE_ACT_NONE && a.scale == 1.f && a.gn_partial != nullptr &&
           (a.gn_cg == 4 || a.gn_cg == 8 || a.gn_cg == 16);
}

// conv_thin.hip (tile code 77): at most 16 output channels, plain bias / SiLU epilogue, f16 weights packed to whole 32-deep K-steps, no side inputs
inline bool fie_conv_thin_ok(const GemmArgs& a) {
    return a.N <= 16 && a.N % 4 == 0 && a.ldc % 4 == 0 && a.Cin % 8 == 0 && !a.ups && !a.taps2 && !a.oscat && !a.A2 && !a.w_scale && !a.rowbias && !a.res &&
           !a.gn_partial && !a.gna_tab && !a.ln_tab && !a.out_f8 && (a.act == FIE_ACT_NONE || a.act == FIE_ACT_SILU) && (a.stride == 1 || a.stride == 2) &&
           a.ldw >= ((int64_t)a.K + 31) / 32 * 32 && a.w_bytes >= 16 * a.ldw * 2;
}

// ---- what the selection reads besides the problem: a plain copy of the context's knobs (gemm_conv.hip: select_env builds it, in one place)
struct SelectEnv {
    int num_cus;
    bool sk_bound;                 // a split-K workspace is bound (fie_splitk_workspace) ...
    int64_t sk_bytes;              // ... of this size
    int splitk_mode;               // fie_debug_splitk: 0 = never split K
    int tune_exclude[16];          // fie_debug_tune_exclude: codes neither the rule (72 / 78 / 77: their A/B switches) nor the tuner may pick; Choice::kSplit = every split-K variant
    bool tune47;                   // FIE_TUNE_47 != "0": the tuner times 128x96
    bool excluded(int c) const { return c != 0 && std::find(std::begin(tune_exclude), std::end(tune_exclude), c) != std::end(tune_exclude); }
};

// ---- the rule.  Heuristic tile code for a shape (the default; the autotuner and the debug hooks can replace it).
inline int heuristic_code(const SelectEnv& env, const GemmArgs& a, bool conv, bool dma) {
    auto blocks = [&](int bm, int bn) { return (int64_t)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn); };
    const int64_t cus = env.num_cus;
    // Selection: tools/tile_table.py (interleaved rounds per shape, profiles/r02_tile_table.md) + tools/tile_trials.py inside the
    // UNet.  The K loop is paced by the per-CU global->LDS issue path (~100 cycles per 1 KiB piece), so a tile's FLOP per
    // staged byte BM*BN/(BM+BN) decides its ceiling -- but only while the grid still fills the CUs: the largest tile that does wins.
    const int64_t b256 = blocks(256, 256), b62 = blocks(256, 128), b51 = blocks(128, 128), b42 = blocks(128, 64);
    int code;
    if (!dma) {
        code = b42 >= cus ? 2 : 3;
    } else if (conv && fie_conv_halo_ok(a) && 4 * (int64_t)(a.M / 256) * ((a.N + 127) / 128) >= 3 * cus && a.C2x + a.C3x <= 4 * BK &&      // (1x1 side inputs: each 64 channels cost a drained K-step: the rule takes few of them, the tuner may take more)
               !env.excluded(72)) {      // fie_debug_tune_exclude("72"): the A/B switch
        // stride-1 same-size convs on maps of whole 16x16 patches with enough (patch, 128-channel) tiles to fill the chip: the halo-resident kernel
        // (conv_halo.hip; persistent, deferred stores).  Measured against every im2col code on the VAE's and the UNet's 64x64 / 128x128-latent
        // shapes: -15 to -35 % (profiles/r04_halo_conv.md)
        code = 72;
    } else if (conv && fie_conv_halo_edge_ok(a) && 4 * fie_conv_halo_patches(a) * ((a.N + 127) / 128) >= 3 * cus && a.C2x + a.C3x <= 4 * BK &&
               !env.excluded(78)) {      // fie_debug_tune_exclude("78"): the A/B switch
        // the same kernel on maps with a side that is not a multiple of 16 (the aspect-ratio buckets: 72x56, 152x104, 38x26, ...): partial patches at
        // the right and bottom edges.  Measured against every im2col code on the buckets' UNet maps (profiles/resolution_buckets.md): 0.84-0.86x the
        // best on the 640-channel maps, 0.97-0.98x on the 320-channel ones; 1.07-1.14x on the 1280-channel maps, which have 120 tiles and stay under
        // this threshold (so the rule keeps their im2col code)
        code = 78;
    } else if (conv) {
        if (!a.A2 && ((b256 >= cus && (a.N % 256 == 0 || (a.N % 128 != 0 && a.K >= 5760))) ||        // 256x256 phased: VAE 256/512-ch maps, 128x128-latent convs into 320 ch (not with 1x1 side inputs: ring kernels only)
            (a.N % 256 == 0 && a.K >= 8192 && 2 * b256 >= cus))) code = 81;                  // ... and the long-K upsampling convs of the 32x32 level
        else if (a.N % 128 == 0 && b62 >= 150) code = 96;
        else if (a.N % 128 == 0 && a.K >= 5760 && b51 >= 100) code = 51;                     // 32x32-latent convs: 160 x (128x128), 8 waves
        else if (2 * b42 < 3 * cus) code = 43;                                               // stride-2 convs and other small grids
        else code = 42;
    } else if (a.N % 320 == 0 && a.N >= 5120 && 4 * blocks(256, 320) >= 3 * cus) {
        // the FF1 projections (M 2048 x N 10240: 256 tiles of 256x320 = one per CU; M 8192 x N 5120: two exact rounds): tile 64 measured 52-58 us
        // on every box of round 3 against 65-80 us for 96 -- but the cold-timed tuner, starting from 96 as the rule, kept 96 on some boxes (one
        // profile run of round 4: 79.7 us x 112 launches = +2.4 ms per edit).  As the RULE it needs a 3 % better challenger to be displaced.
        code = 64;
    } else if (a.N % 256 == 0 && a.K >= 4096 && b256 >= cus) {
        code = 81;
    } else if (a.N % 128 == 0 && b62 >= 150 && (a.N >= 1536 || a.K >= 2048 || a.M >= 16384)) {
        code = 96;
    } else if (a.N >= 2048 && a.K >= 1024 && b51 >= cus) {
        code = 51;
    } else if (a.K <= 640 && a.N <= 640) {
        code = 43;                                                                           // 64x64 / 128x128-latent projections: many small tiles
    } else if (b42 >= cus * 7 / 2 || a.K >= 4096 || (a.K >= 1024 && b42 >= cus)) {
        code = 42;
    } else {
        code = 43;
    }
    return code;
}

// What a launch runs when nothing is pinned or remembered.  The three families with no choice to make come first; `forced`: the code of
// fie_debug_force_tile (the LN-folded GEMM honours it where it names an LN build); `thin`: the caller allows the thin-conv rule (nothing pinned, no probe)
inline Choice rule(const SelectEnv& env, const GemmArgs& a, bool conv, bool dma, int forced = 0, bool thin = true) {
    if (conv && a.gna_tab) return {72};      // the input's GroupNorm applied on the resident halo: one kernel family
    if (!conv && a.ln_tab) {
        // LayerNorm folded in: four tiles, chosen by rule (no tuner: the choice among them does not change the sums, every one adds K in the same order)
        auto blocks = [&](int bm, int bn) { return (int64_t)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn); };
        int code;
        if (a.act == FIE_ACT_GEGLU) code = 64;
        else if (a.N % 128 == 0 && blocks(256, 128) >= 150 && (a.N >= 1536 || a.M >= 16384)) code = 96;
        else code = 42;
        if (forced && find_tile(forced) && (find_tile(forced)->flags & kLnFold) && (forced == 64) == (a.act == FIE_ACT_GEGLU)) code = forced;
        return {code};
    }
    // at most 16 output channels (conv_out of the VAE / UNet, the conditioning embedding's first convs): the direct-load strip kernel of conv_thin.hip,
    // by rule and without the tuner (one kernel family; profiles/r04_conv_thin.md).  fie_debug_tune_exclude("77") is the A/B switch.
    if (conv && thin && fie_conv_thin_ok(a) && a.M >= 131072 && !env.excluded(77)) return {77, 0, 1};      // (the 128x128-latent conv_outs, K 2880 / 4608 on few strips: the ring tiles are faster)
    return {heuristic_code(env, a, conv, dma)};
}

// tuner keys carry neither the map's height and width nor the epilogue: one key covers 144x112 and 168x96 (M 16128), and 78 refuses GroupNorm
// sums and activations.  A remembered halo-resident code the launch is not eligible for (72 met on a map of whole patches, then the same key
// on a bucket map; 78 met without sums, then with them) falls back to the rule instead of failing; a pinned choice is run (and refused) as it is
inline Choice eligible_or_rule(const SelectEnv& env, const GemmArgs& a, bool conv, bool dma, Choice c, bool pinned) {
    if (conv && !pinned && ((is_family(c.code, kHalo) && !fie_conv_halo_ok(a)) || (is_family(c.code, kHaloEdge) && !fie_conv_halo_edge_ok(a)))) return {heuristic_code(env, a, conv, dma)};
    return c;
}

// ---- tile order = which operand an XCD re-streams past its 4 MiB L2.  Consecutive tile ids run on one XCD (xcd_remap), so an
// XCD owns T/8 consecutive tiles: with n fastest that is `dm` row blocks x up to all column tiles, with m fastest the
// transpose.  Fabric bytes per XCD ~ (row blocks touched) x (A bytes per row block) + (column tiles touched) x (W bytes per
// column tile); pick the smaller (FF1 at M 2048: 8 XCDs x all 26 MB of W with n fastest, 247 MB measured by PMC in round 1,
// against 8 x (3.3 MB of W + all 5.2 MB of A) with m fastest).  The 3x3 im2col view re-reads an input row block ~once.
struct XcdSpan { int64_t slow, fast; };       // distinct slow-index / fast-index values among an XCD's tiles
inline XcdSpan xcd_span(int64_t per_xcd, int64_t fast, int64_t slow) {       // `fast` tiles per row of the id space
    const int64_t rows = (per_xcd + fast - 1) / fast;                        // slow-index values an XCD touches
    return {rows < slow ? rows : slow, per_xcd < fast ? per_xcd : fast};
}
inline int tile_order(const GemmArgs& a, const Tile& t, bool conv) {
    const int64_t nbm = (a.M + t.bm - 1) / t.bm, nbn = (a.N + t.bn - 1) / t.bn;
    const int64_t per_xcd = (nbm * nbn + 7) / 8;
    const double a_tile = (double)t.bm * a.K * 2 * (conv ? 1.0 / 9 : 1.0), w_tile = (double)t.bn * a.K * 2;
    auto fabric = [&](int64_t fast, int64_t slow, double fast_tile, double slow_tile) {
        const XcdSpan s = xcd_span(per_xcd, fast, slow);
        return (double)s.slow * slow_tile + (double)s.fast * fast_tile;
    };
    return fabric(nbm, nbn, a_tile, w_tile) < fabric(nbn, nbm, w_tile, a_tile) ? 1 : 0;
}

// ---- split-K
constexpr int64_t kSkTickets = 4096;        // arrival counters at the head of the split-K workspace

// Largest usable split for a tile: a row that may split K (kSplitK), at least 4 K-steps per slice, counters and slabs inside the bound
// workspace.  Returns 1 when split-K cannot run.
inline int splitk_fit(const SelectEnv& env, const GemmArgs& a, const Tile& t, int want) {
    const int bm = t.bm, bn = t.bn;
    if (want <= 1 || !(t.flags & kSplitK) || !env.sk_bound || !env.splitk_mode || (a.w_scale && a.a_scale == 0.f)) return 1;
    const int64_t tiles = (int64_t)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn) * (a.oscat == 2 ? 4 : 1);
    const int nk = (a.K + BK - 1) / BK / (a.a_scale != 0.f ? 2 : 1);      // fp8 activations: 128 k-values per K-step
    int s = want;
    while (s > 1 && (nk / s < 4 || tiles > kSkTickets || (int64_t)(kSkTickets * 4 + tiles * s * bm * bn * 4) > env.sk_bytes)) --s;
    return s;
}

// ---- what the tuner times besides the rule's code `guess` (kCandF16 / kCandW8 / kCandX8 and the split lists above, filtered), as encoded choices:
// autotune (gemm_conv.hip) times exactly this list; fie_debug_tune_candidates reports it (tests/test_launch_table_gpu.py runs every entry at the
// product's shapes).  The only allocating function here: it runs while tuning or reporting, never on a launch that knows its choice.
inline std::vector<int> tune_candidates(const SelectEnv& env, const GemmArgs& a, bool conv, int guess) {
    std::vector<int> out;
    auto blocks = [&](int bm, int bn) { return (int64_t)((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn); };
    const bool x8 = a.w_scale && a.a_scale != 0.f;
    const int* cand = x8 ? kCandX8 : a.w_scale ? kCandW8 : kCandF16;
    const size_t ncand = x8 ? std::size(kCandX8) : a.w_scale ? std::size(kCandW8) : std::size(kCandF16);
    for (size_t i = 0; i < ncand; ++i) {
        const int c = cand[i];
        if (c == guess || env.excluded(c)) continue;
        if ((c == 43 || c == 46) && blocks(64, 64) > 64 * env.num_cus) continue;       // tens of thousands of tiny tiles: never wins
        if ((c == 81 || c == 96 || c == 62) && 2 * blocks(256, 128) < env.num_cus) continue;
        if ((c == 63 || c == 64) && (conv || a.N % 320 != 0 || 2 * blocks(256, 320) < env.num_cus)) continue;
        if (c == 47 && !env.tune47) continue;
        if (c == 48 && (a.N % 80 != 0 || blocks(128, 80) > 2 * env.num_cus)) continue;      // the exact-fit tile of the N = 1280 projections: small grids only
        if (x8 && conv && c == 63) continue;
        if (x8 && (c == 62 || c == 51) && 2 * blocks(c == 62 ? 256 : 128, 128) < env.num_cus) continue;
        if (c == 81 && conv && a.A2) continue;            // side inputs: ring kernels only
        if (c == 72 && (!conv || !fie_conv_halo_ok(a) || 2 * (int64_t)(a.M / 256) * ((a.N + 127) / 128) < env.num_cus)) continue;
        if (c == 78 && (!conv || !fie_conv_halo_edge_ok(a) || 2 * fie_conv_halo_patches(a) * ((a.N + 127) / 128) < env.num_cus)) continue;
        out.push_back(Choice{c}.encode());
    }
    // split-K: big tiles whose grid leaves CUs idle (the M = 2048 class: 80 tiles of 256x128 on 256 CUs) with the K-steps of a tile dealt
    // to 2-4 blocks, reduced in the launch (gemm_common.h: splitk_reduce).  Changes the fp32 summation order, so unlike the tile choice
    // it is visible in the last bit of some f16 outputs; fixed per (shape, choice), hence deterministic within a process.
    if ((!a.w_scale || x8) && env.sk_bound && env.splitk_mode && !env.excluded(Choice::kSplit)) {
        const SplitCand* sc = x8 ? kSplitX8 : kSplitF16;
        const size_t nsc = x8 ? std::size(kSplitX8) : std::size(kSplitF16);
        for (size_t i = 0; i < nsc; ++i) {
            const SplitCand& c = sc[i];
            if (env.excluded(c.code)) continue;
            const Tile& t = *find_tile(c.code);
            const int64_t nb = blocks(t.bm, t.bn) * (a.oscat == 2 ? 4 : 1);
            if (nb >= env.num_cus * c.per_cu) continue;                 // the grid already fills the chip
            for (int sp = 2; sp <= 4; ++sp) {
                if (nb * sp > (int64_t)env.num_cus * c.per_cu * 21 / 20) break;
                if (splitk_fit(env, a, t, sp) != sp) continue;
                out.push_back(Choice{c.code, -1, sp}.encode());
            }
        }
    }
    return out;
}

}  // namespace fie_gemm
