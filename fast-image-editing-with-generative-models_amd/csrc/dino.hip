// DINO structure distance on the device (include/fie.h: fie_dino_patches_u8_*, fie_selfsim_mse_*): what stands between the u8
// image and the ViT tower, and between the tower's layer-11 keys and the number.
//   patches   fie_dino_patches_u8_*: torchvision's `Resize(R, antialias=True)` on the float image -- ATen's separable antialias triangle filter, fp32, the
//             horizontal pass first -- then (x - mean) / std, patchify and cast.  Taps and bounds come from the host (fie_amd/resize.py:
//             aa_coefficients).  Launch 1: the horizontal pass of u8 / 255 into an fp32 [n, H, OW, 3] scratch image.  Launch 2: vertical pass,
//             normalisation, patchify and cast in one; its work item is 16 contiguous output bytes, as in fie_clip_patches_u8_*, and its rows are in
//             the same K order (csrc/image_ops.h: patch_item, one decode for both).  Up-scaling and the identity size run through the same tables (identity: taps {1, 0}, exact).
//   selfsim   fie_selfsim_mse_*: mean over T x T of (S_b - S_a)^2 with S = K K^T / max(|k_i| |k_j|, 1e-8), the T x T matrices never stored.
//             Launch 1: row norms, one wave per key row, fp32 sums in a fixed order.  Launch 2: one block per 64 x 64 tile (i <= j: S is symmetric,
//             tiles above the diagonal count twice) of one pair; each of its four waves owns 32 x 32 entries of BOTH Gram tiles as 2 x 2 MFMA
//             fragments with fp32 accumulators.  A key row is at once the A operand's row and the B operand's column, and a lane's share of either is
//             contiguous in k, so fragments are loaded straight from global memory (the 2.4 MB of a pair's keys stay in L2); there is nothing
//             to stage in LDS.  The epilogue divides by the clamped norm products, squares the difference, masks rows / columns >= T and adds in
//             fp64: lanes by a shuffle tree, the four waves in wave order -> ONE partial per block, an ordinary store.  Launch 3: one block per pair adds
//             the partials in tile order in fp64 and divides by T^2.  No atomics: a pair's bits depend neither on n nor on its position; both
//             Gram tiles run the same instruction sequence, so an identical pair gives exactly 0.
#include "gemm_common.h"
#include "image_ops.h"

namespace {

using fie_gemm::static_for;
using namespace fie_img;

// items: (image, y, ox, c) of the scratch image [n, H, OW, 3]
__global__ __launch_bounds__(256) void dino_hpass_kernel(const uint8_t* __restrict__ src, int H, int W, int OW, const float* __restrict__ wx,
                                                         const int* __restrict__ bx, int ksx, float* __restrict__ tmp, int64_t total) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        const int64_t p = i / 3;
        const int ox = (int)(p % OW);
        const int64_t row = p / OW;                                          // image * H + y
        const int x0 = bx[ox * 2], cnt = min(bx[ox * 2 + 1], ksx);
        const uint8_t* s = src + row * W * 3 + c;
        const float* w = wx + (int64_t)ox * ksx;
        float t = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float v = (float)s[(int64_t)min(x0 + j, W - 1) * 3] / 255.0f;
            t = j == 0 ? v * w[0] : t + v * w[j];
        }
        tmp[i] = t;
    }
}

// items: (row = image * P + patch, 16-byte chunk of the row)
template <typename T>
__global__ __launch_bounds__(256) void dino_vpass_patches_kernel(const float* __restrict__ tmp, int H, int OW, const float* __restrict__ wy,
                                                                 const int* __restrict__ by, int ksy, int grid_w, int P, int ps, ChannelNorm nm,
                                                                 T* __restrict__ out, int64_t total) {
    constexpr int E = 16 / (int)sizeof(T);
    const int K = 3 * ps * ps, nch = K / E;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const PatchItem it = patch_item<E>(i, nch, P, grid_w, ps);
        const int b = it.b, c = it.c, oy = it.gy * ps + it.py, ox = it.gx * ps + it.px;
        const int y0 = by[oy * 2], cnt = min(by[oy * 2 + 1], ksy);
        const float* w = wy + (int64_t)oy * ksy;
        const float mean = channel_pick(nm.mean[0], nm.mean[1], nm.mean[2], c), std = channel_pick(nm.std[0], nm.std[1], nm.std[2], c);
        float t[E];
        for (int j = 0; j < cnt; ++j) {
            const float* s = tmp + (((int64_t)b * H + min(y0 + j, H - 1)) * OW + ox) * 3 + c;
            const float wj = w[j];
            static_for([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                t[e] = j == 0 ? s[e * 3] * wj : t[e] + s[e * 3] * wj;
            }, std::make_integer_sequence<int, E>{});
        }
        alignas(16) T v[E];
        static_for([&](auto ec) {
            constexpr int e = decltype(ec)::value;
            v[e] = (T)(((cnt > 0 ? t[e] : 0.f) - mean) / std);
        }, std::make_integer_sequence<int, E>{});
        *reinterpret_cast<uint4*>(out + it.row * K + it.k0) = *reinterpret_cast<const uint4*>(v);
    }
}

// ---------------------------------------------------------------------------------------------------------------- self-similarity MSE
constexpr int kTile = 64;                  // entries of S per block edge; a wave owns 32 x 32 of them

// one wave per key row (rows of both sides of all pairs: grid = 2 * n * T / 4 blocks of 4 waves); norms [2][n * T]
template <typename T>
__global__ __launch_bounds__(256) void selfsim_norm_kernel(const T* __restrict__ ka, const T* __restrict__ kb, int64_t ld, int64_t rows, int C,
                                                           float* __restrict__ norms) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= 2 * rows) return;
    const T* k = r < rows ? ka + r * ld : kb + (r - rows) * ld;
    float s = 0.f;
    for (int j = lane; j < C; j += 64) {
        const float x = (float)k[j];
        s += x * x;
    }
    s = wave_sum(s);
    if (lane == 0) norms[r] = sqrtf(s);
}

// The MFMA operands of 16 key rows at k-chunk k0.  f16 (v_mfma_f32_16x16x32_f16): lane l holds row l & 15, k = k0 + 8 (l >> 4) + 0..7 -- one 16-byte
// load, a chunk is 32 wide.  f32 (v_mfma_f32_16x16x4_f32): lane l holds row l & 15 and ONE k per instruction; it loads k0 + 4 (l >> 4) + 0..3 at once and
// feeds element s to instruction s of the chunk (16 wide).  Which k an instruction sums is the same on the A and on the B side, which is all a dot product needs.
template <typename T> struct Frag;
template <> struct Frag<half_t> {
    static constexpr int kChunk = 32;
    f16x8 v;
    __device__ __forceinline__ void load(const half_t* row, int k0, int lane) { v = *reinterpret_cast<const f16x8*>(row + k0 + 8 * (lane >> 4)); }
    static __device__ __forceinline__ f32x4 mma(const Frag& a, const Frag& b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v, b.v, c, 0, 0, 0); }
};
template <> struct Frag<float> {
    static constexpr int kChunk = 16;
    f32x4 v;
    __device__ __forceinline__ void load(const float* row, int k0, int lane) { v = *reinterpret_cast<const f32x4*>(row + k0 + 4 * (lane >> 4)); }
    static __device__ __forceinline__ f32x4 mma(const Frag& a, const Frag& b, f32x4 c) {
        static_for([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[s], b.v[s], c, 0, 0, 0);
        }, std::make_integer_sequence<int, 4>{});
        return c;
    }
};

// grid (nt (nt + 1) / 2, n): block x = the x-th tile (ti <= tj) in row-major order of the upper triangle
template <typename T>
__global__ __launch_bounds__(256) void selfsim_tile_kernel(const T* __restrict__ ka, const T* __restrict__ kb, int64_t ld, int n, int Tn, int C, int nt,
                                                           const float* __restrict__ norms, double* __restrict__ partial) {
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.y;
    int ti = 0, rest = blockIdx.x;
    while (rest >= nt - ti) { rest -= nt - ti; ++ti; }
    const int tj = ti + rest;
    const int i0 = ti * kTile + (wave >> 1) * 32, j0 = tj * kTile + (wave & 1) * 32;
    const T* base[2] = {ka + (int64_t)pair * Tn * ld, kb + (int64_t)pair * Tn * ld};
    // rows past T are read as row T - 1 (in bounds) and masked in the epilogue
    const T* ri[2][2];
    const T* rj[2][2];
    static_for([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        static_for([&](auto fc) {
            constexpr int f = decltype(fc)::value;
            ri[s][f] = base[s] + (int64_t)min(i0 + f * 16 + (lane & 15), Tn - 1) * ld;
            rj[s][f] = base[s] + (int64_t)min(j0 + f * 16 + (lane & 15), Tn - 1) * ld;
        }, std::make_integer_sequence<int, 2>{});
    }, std::make_integer_sequence<int, 2>{});

    f32x4 acc[2][2][2];                     // [side][row fragment][column fragment]
    static_for([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        acc[q >> 2][(q >> 1) & 1][q & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }, std::make_integer_sequence<int, 8>{});

    for (int k0 = 0; k0 < C; k0 += Frag<T>::kChunk) {
        Frag<T> fi[2][2], fj[2][2];
        static_for([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            fi[q >> 1][q & 1].load(ri[q >> 1][q & 1], k0, lane);
            fj[q >> 1][q & 1].load(rj[q >> 1][q & 1], k0, lane);
        }, std::make_integer_sequence<int, 4>{});
        static_for([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int s = q >> 2, a = (q >> 1) & 1, b = q & 1;
            acc[s][a][b] = Frag<T>::mma(fi[s][a], fj[s][b], acc[s][a][b]);
        }, std::make_integer_sequence<int, 8>{});
    }

    // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register
    const float* na = norms + (int64_t)pair * Tn;
    const float* nb = norms + (int64_t)(n + pair) * Tn;
    double sum = 0.0;
    static_for([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        constexpr int a = q >> 1, b = q & 1;
        const int j = j0 + b * 16 + (lane & 15);
        const int jc = min(j, Tn - 1);
        const float naj = na[jc], nbj = nb[jc];
        static_for([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            const int i = i0 + a * 16 + 4 * (lane >> 4) + r;
            const int ic = min(i, Tn - 1);
            const float sa = acc[0][a][b][r] / fmaxf(na[ic] * naj, 1e-8f);
            const float sb = acc[1][a][b][r] / fmaxf(nb[ic] * nbj, 1e-8f);
            const float d = sb - sa;
            if (i < Tn && j < Tn) sum += (double)d * (double)d;
        }, std::make_integer_sequence<int, 4>{});
    }, std::make_integer_sequence<int, 4>{});

    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        const double s = ((red[0] + red[1]) + red[2]) + red[3];
        partial[(int64_t)pair * gridDim.x + blockIdx.x] = ti == tj ? s : 2.0 * s;
    }
}

// one block per pair: thread t adds partials t, t + 256, ... in that order, then a fixed tree
__global__ __launch_bounds__(256) void selfsim_final_kernel(const double* __restrict__ partial, int tiles, int Tn, double* __restrict__ out) {
    __shared__ double rs[256];
    const int tid = threadIdx.x;
    const double* p = partial + (int64_t)blockIdx.x * tiles;
    double s = 0.0;
    for (int i = tid; i < tiles; i += 256) s += p[i];
    rs[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) rs[tid] += rs[tid + o];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = rs[0] / ((double)Tn * (double)Tn);
}

inline int tiles_of(int T) { return (T + kTile - 1) / kTile; }
inline int64_t tri_of(int T) { return (int64_t)tiles_of(T) * (tiles_of(T) + 1) / 2; }
inline int64_t partial_bytes(int n, int T) { return (int64_t)n * tri_of(T) * (int64_t)sizeof(double); }

template <typename T>
int dino_patches_t(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int OH, int OW, const float* wx, const int* bx, int ksx, const float* wy,
                   const int* by, int ksy, int patch, const float* mean, const float* std, float* tmp, void* out) {
    FIE_REQUIRE(ctx && src && wx && bx && wy && by && mean && std && tmp && out, "fie_dino_patches_u8: NULL argument");
    FIE_REQUIRE(n > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && ksx > 0 && ksy > 0, "fie_dino_patches_u8: bad shape");
    FIE_REQUIRE(patch > 0 && patch % 8 == 0 && OH % patch == 0 && OW % patch == 0,
                "fie_dino_patches_u8: resized size %d x %d / patch size %d: the patch size must divide both edges and be a multiple of 8", OH, OW, patch);
    FIE_REQUIRE((uintptr_t)out % 16 == 0 && (uintptr_t)tmp % 4 == 0, "fie_dino_patches_u8: the output must be 16-byte aligned");
    ChannelNorm nm;
    if (const int rc = channel_norm("fie_dino_patches_u8", mean, std, &nm)) return rc;
    const int gw = OW / patch, P = (OH / patch) * gw;
    const int64_t t1 = (int64_t)n * H * OW * 3;
    const int64_t t2 = (int64_t)n * P * (3 * patch * patch / (16 / (int)sizeof(T)));
    FIE_DESC(ctx, "dino_hpass n=%d %dx%d -> width %d taps=%d", n, H, W, OW, ksx);
    fie_launch(ctx, dino_hpass_kernel, dim3(grid_1d(t1, kPatchBlocks)), dim3(256), 0, src, H, W, OW, wx, bx, ksx, tmp, t1);
    FIE_LAUNCH_CHECK();
    FIE_DESC(ctx, "dino_vpass_patches n=%d %dx%d -> %dx%d taps=%d patch=%d", n, H, OW, OH, OW, ksy, patch);
    fie_launch(ctx, dino_vpass_patches_kernel<T>, dim3(grid_1d(t2, kPatchBlocks)), dim3(256), 0, (const float*)tmp, H, OW, wy, by, ksy, gw, P, patch, nm, (T*)out, t2);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

template <typename T>
int selfsim_mse_t(fie_ctx* ctx, const void* keys_a, const void* keys_b, int64_t ld, int n, int Tn, int C, void* workspace, double* out) {
    FIE_REQUIRE(ctx && keys_a && keys_b && workspace && out, "fie_selfsim_mse: NULL argument");
    FIE_REQUIRE(n > 0 && n <= 65535 && Tn > 0 && C > 0 && ld >= C, "fie_selfsim_mse: bad shape (n=%d, T=%d, C=%d, row stride %lld)", n, Tn, C, (long long)ld);
    FIE_REQUIRE(C % Frag<T>::kChunk == 0, "fie_selfsim_mse: C=%d must be a multiple of %d (one MFMA k-chunk)", C, Frag<T>::kChunk);
    FIE_REQUIRE(((uintptr_t)keys_a | (uintptr_t)keys_b) % 16 == 0 && (ld * (int64_t)sizeof(T)) % 16 == 0,
                "fie_selfsim_mse: key rows must be 16-byte aligned (base pointers and row stride %lld)", (long long)ld);
    FIE_REQUIRE(((uintptr_t)workspace | (uintptr_t)out) % 8 == 0, "fie_selfsim_mse: workspace and out must be 8-byte aligned");
    const int nt = tiles_of(Tn);
    const int64_t tri = tri_of(Tn), rows = (int64_t)n * Tn;
    FIE_REQUIRE(tri <= 0x7fffffff && (2 * rows + 3) / 4 <= 0x7fffffff, "fie_selfsim_mse: n=%d pairs of %d rows exceed the launch grid", n, Tn);
    double* partial = (double*)workspace;
    float* norms = (float*)((char*)workspace + partial_bytes(n, Tn));
    FIE_DESC(ctx, "selfsim_norms n=%d T=%d C=%d", n, Tn, C);
    fie_launch(ctx, selfsim_norm_kernel<T>, dim3((unsigned)((2 * rows + 3) / 4)), dim3(256), 0, (const T*)keys_a, (const T*)keys_b, ld, rows, C, norms);
    FIE_LAUNCH_CHECK();
    FIE_DESC(ctx, "selfsim_tiles n=%d T=%d C=%d tiles=%lld", n, Tn, C, (long long)tri);
    fie_launch(ctx, selfsim_tile_kernel<T>, dim3((unsigned)tri, n), dim3(256), 0, (const T*)keys_a, (const T*)keys_b, ld, n, Tn, C, nt, (const float*)norms, partial);
    FIE_LAUNCH_CHECK();
    FIE_DESC(ctx, "selfsim_final n=%d tiles=%lld", n, (long long)tri);
    fie_launch(ctx, selfsim_final_kernel, dim3(n), dim3(256), 0, (const double*)partial, (int)tri, Tn, out);
    FIE_LAUNCH_CHECK();
    return FIE_OK;
}

}  // namespace

extern "C" {

int fie_dino_patches_u8_f16(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int OH, int OW, const float* wx, const int* bx, int ksx, const float* wy,
                            const int* by, int ksy, int patch, const float* mean, const float* std, float* tmp, void* out) {
    return dino_patches_t<half_t>(ctx, src, n, H, W, OH, OW, wx, bx, ksx, wy, by, ksy, patch, mean, std, tmp, out);
}
int fie_dino_patches_u8_f32(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int OH, int OW, const float* wx, const int* bx, int ksx, const float* wy,
                            const int* by, int ksy, int patch, const float* mean, const float* std, float* tmp, void* out) {
    return dino_patches_t<float>(ctx, src, n, H, W, OH, OW, wx, bx, ksx, wy, by, ksy, patch, mean, std, tmp, out);
}

int64_t fie_selfsim_workspace_bytes(int n, int T) {
    if (n <= 0 || T <= 0) return -1;
    return partial_bytes(n, T) + (int64_t)2 * n * T * (int64_t)sizeof(float);
}
int fie_selfsim_mse_f16(fie_ctx* ctx, const void* keys_a, const void* keys_b, int64_t ld, int n, int T, int C, void* workspace, double* out) {
    return selfsim_mse_t<half_t>(ctx, keys_a, keys_b, ld, n, T, C, workspace, out);
}
int fie_selfsim_mse_f32(fie_ctx* ctx, const void* keys_a, const void* keys_b, int64_t ld, int n, int T, int C, void* workspace, double* out) {
    return selfsim_mse_t<float>(ctx, keys_a, keys_b, ld, n, T, C, workspace, out);
}

}  // extern "C"
