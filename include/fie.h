/*
 * fie.h -- C ABI of the MI355X (gfx950) hot-path library `libfie_hip.so`.
 *
 * The reference (/root/reference) is pure Python and has NO FFI of its own: every multiply-add of its hot call
 * `self.pipe(...)` (src/pipeline.py:261-272) runs inside diffusers/transformers/torch/OpenCV.  This header is
 * therefore the boundary a maintainer would bind from Python (ctypes stub in INTEGRATION.md) to replace those
 * upstream internals.  Each entry names the reference call site / upstream module it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  Every function returns 0 on success or a
 *     negative FIE_E* code; `fie_last_error()` returns a thread-local message for the last failure.
 *   - All device pointers are owned by the caller (PyTorch-ROCm allocations: tensor.data_ptr()).  The library never
 *     allocates device memory; kernels that need scratch take a caller-provided workspace.
 *   - Every launch is asynchronous on the ctx's stream and never synchronises (hipGraph-capturable).
 *   - fp16 storage ("f16" = IEEE binary16), fp32 accumulation.  Activations are NHWC; a tensor with C channels
 *     has C % 8 == 0 (3/4-channel images and latents are stored zero-padded to 8 channels unless stated).
 *   - One ctx per (thread, device); a ctx is not thread-safe; distinct ctxs are independent.
 */
#ifndef FIE_H_
#define FIE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIE_OK 0
#define FIE_EINVAL (-1)   /* bad argument / unsupported shape */
#define FIE_EHIP (-2)     /* HIP runtime error */
#define FIE_ENODEV (-3)   /* no gfx950 device */

/* Device-side failures cannot return a code from an asynchronous launch: a kernel that has to give up (today: the bounded spin of the
 * in-launch barrier of fie_time_embed_f16) stores one of these into the word bound with fie_ctx_error_flag, and the host reads that word
 * at its next synchronisation (fie_amd: after the D2H copy of every edit; non-zero raises).  The word is sticky until the host clears it. */
#define FIE_DEVERR_TIME_EMBED_BARRIER 1u

/* epilogue activations (applied to acc + bias [+ rowbias]) */
#define FIE_ACT_NONE 0
#define FIE_ACT_SILU 1
#define FIE_ACT_GELU 2        /* exact erf GELU */
#define FIE_ACT_QUICK_GELU 3  /* x * sigmoid(1.702 x), CLIP-L */
#define FIE_ACT_GEGLU 4       /* weight rows interleaved (value, gate): out[j] = v_j * gelu(g_j); N counts both */
#define FIE_ACT_RELU 5        /* max(x, 0): fie_gemm_f32 and fie_conv3x3_nhwc_f32 only (the LPIPS tower); every f16 / f8 entry refuses it */

typedef struct fie_ctx fie_ctx;

int fie_version(void);
const char* fie_last_error(void);
/* stream: hipStream_t (0 = default stream).  Replaces: nothing in the reference (torch owns streams there). */
int fie_ctx_create(int device, void* stream, fie_ctx** out);
int fie_ctx_set_stream(fie_ctx* ctx, void* stream);
int fie_ctx_error_flag(fie_ctx* ctx, void* device_word);    /* caller-owned, zero-initialised uint32 in device memory (NULL: none); see FIE_DEVERR_* */
int fie_ctx_destroy(fie_ctx* ctx);

/* ---- Graph-level entries: the upstream calls they replace are the model forwards inside the diffusers pipeline call
 * at /root/reference/src/pipeline.py:261-272 -- UNet2DConditionModel.forward, ControlNetModel.forward,
 * AutoencoderKL.encode / .decode, CLIPTextModel(.WithProjection).forward.
 *
 * Mechanism: LAUNCH PROGRAMS.  The host walks a graph once, with the device buffers it will keep using (weights, static
 * input / output / scratch tensors), between fie_program_begin and fie_program_end: every kernel launch the op entries below
 * issue meanwhile EXECUTES as usual and is ALSO appended to the program (kernel, grid, block, LDS bytes, argument values).
 * fie_program_run re-issues the whole list on the ctx stream from C++: no host-side shape logic, no Python, asynchronous and
 * hipGraph-capturable like any single op.  New inputs = new CONTENTS of the same input buffers.  The caller keeps every buffer
 * the program references alive and destroys programs it created.
 * ORDERING CONTRACT (round 4).  A program's launches carry FROZEN pointers: its static buffers and the split-K workspace
 * (fie_splitk_workspace) that was bound to the ctx while it was recorded -- arrival counters and partial-tile slabs included.  Therefore
 *   (1) a program must never be in flight twice.  fie_program_run enforces this for eager runs: the recording pass and every run record
 *       an event, and a run on a DIFFERENT stream than the previous pass first makes that stream wait for it (same stream: stream order).
 *       Under stream capture nothing is ordered by the library: a captured graph that contains the program inherits the rule (do not
 *       replay it while another copy of the program, captured or eager, is running);
 *   (2) nothing else may use that split-K workspace concurrently: record a program with a workspace of its OWN bound
 *       (fie_amd/hip.py: Context.record() allocates one per program and restores the previous binding afterwards);
 *   (3) the buffers' producers are the caller's to order: make the run's stream wait for whatever wrote the inputs.
 * A caller that breaks (1) / (2) gets undefined sums from the overlapping launches, but no lasting damage: the arrival counters are
 * self-healing (every S-th arrival takes S off the counter; csrc/gemm_common.h: splitk_reduce).
 * What the five NAMED entries (fie_unet_forward ...) are NOT: a C++ implementation of the model graphs.  They are REPLAY HANDLES for a launch list
 * a host walk recorded, with every pointer frozen in.  The C++ implementations are the *_f16 forwards below (round 3).  The product path
 * (hipGraph replay of the Python walk, which takes more fusions) goes through neither; tests/test_programs_gpu.py covers both.
 *   fie_graph_register binds a program to one of the names "unet_forward", "controlnet_forward", "vae_encode", "vae_decode",
 *   "clip_text_forward"; the five named entries run the program bound to their name (FIE_EINVAL if none). */
/* ---- Graph-level forwards that ARE forwards (round 3, csrc/graphs.cpp): the five model calls inside the pipeline call at
 * /root/reference/src/pipeline.py:261-272 sequenced in C++ over the op entries below, on weights registered once by name -- tensor arguments in
 * and out, no Python graph code, no recorded launch list; what a non-Python host binds.
 *   fie_weights_register(name, ptr, n, ld): name = "<prefix><diffusers parameter name>" (prefix = the `prefix` argument of the forward, "" for the
 *     VAE).  "<conv>.weight" = fie_pack_conv3x3_f16 output (n = Cout, ld = ldw), "<linear>.weight" = fie_pack_rows_f16 output (n = N), biases /
 *     norm gains as plain f16 vectors (ld = 0).  Fused matrices (rows concatenated, then packed; biases likewise): "...attn1.to_qkv",
 *     "...attn2.to_kv", "...self_attn.qkv_proj" (CLIP), "<vae>.mid_block.attentions.0.to_qkv", "time_emb_proj_all" (every resnet's time_emb_proj
 *     in walk order: down, mid, up); "...ff.net.0.proj" in the GEGLU layout (fie_pack_rows_f16 with geglu: value / gate rows interleaved, bias
 *     likewise); "post_quant_conv.{weight,bias}" zero-padded to the 8-channel latent layout; CLIP: "zero_row" = `hidden` zeros.
 *   Workspaces: ONE caller-provided device buffer per call, >= the matching *_workspace_bytes(cfg) (the walk's allocation sequence replayed
 *     without launching: exact).  Asynchronous on the ctx stream, hipGraph-capturable, no allocation, no synchronisation.
 *     The walks' GEMMs / convs split K where the tuner chose so, on the split-K workspace currently bound to the ctx (fie_splitk_workspace):
 *     bind the workspace of the stream you are about to issue on BEFORE calling a forward (fie_amd/cabi.py does, per (stream, slot)).
 *   Same kernels and order as the Python walks (fie_amd/{clip,vae,nn}.py) apart from fusions those take and these do not (GroupNorm sums from the
 *     producing epilogue, 2x2-parity up-samplers, conv2 + shortcut as one GEMM, the one-launch timestep embedding, zero convs adding into the UNet's
 *     skips): results agree to rounding (tests/test_programs_gpu.py: <= 3e-3 of the output's max against the Python walk at full size).
 *   Layouts: activations NHWC f16; images and latents 8-channel zero-padded ([B, H, W, 8]); eps / VAE pixels 4-channel ([.., 4], 3 or 4 real). */
typedef struct fie_vae_config {
    int latent_h, latent_w;
    int num_blocks;                /* len(block_out_channels), <= 8 */
    int block_out_channels[8];     /* encoder order, e.g. 128, 256, 512, 512 */
    int layers_per_block;          /* 2: the decoder runs layers_per_block + 1 resnets per up block */
    int norm_num_groups;           /* 32 */
    float norm_eps;                /* 1e-6 */
    int out_channels;              /* 3 */
    const char* prefix;            /* the weights were registered as "<prefix>encoder....", "<prefix>post_quant_conv", ...; NULL: no prefix */
} fie_vae_config;
typedef struct fie_clip_config {
    int batch, tokens;             /* ids: int32 [batch * tokens] on the device */
    int hidden, heads, layers, intermediate;
    int projection_dim;            /* 0: no text_projection (CLIP-L as SDXL uses it): the last layer is not run */
    int quick_gelu;                /* 1: quick_gelu (CLIP-L), 0: gelu (OpenCLIP bigG) */
    float eps;                     /* 1e-5 */
} fie_clip_config;
typedef struct fie_unet_config {   /* UNet2DConditionModel (SDXL family) and the ControlNetModel built on its encoder */
    int batch;                     /* rows of x (CFG rows included) */
    int latent_h, latent_w;        /* multiples of 2^(num_blocks - 1) */
    int text_len;                  /* text rows per batch row (77) */
    int num_blocks;                /* <= 4 */
    int block_out_channels[4];     /* 320, 640, 1280 */
    int layers_per_block;          /* 2 (<= 3) */
    int down_attn[4][4];           /* transformer depth behind resnet j of down block i (0: none) */
    int up_attn[4][4];             /* likewise for the layers_per_block + 1 resnets of up block i (UNet only) */
    int mid_attn;                  /* depth of the mid-block transformer (0: none) */
    int mid_resnets;               /* 2: resnet, transformer, resnet;  1: one resnet */
    int head_dim;                  /* 64 */
    int norm_num_groups;           /* 32 */
    float norm_eps;                /* 1e-5 */
    int cross_attention_dim;       /* 2048 */
    int addition_time_embed_dim;   /* 256 */
    int pooled_dim;                /* 1280: add_embedding.linear_1 reads pooled_dim + 6 * addition_time_embed_dim columns */
    int num_cond_channels;         /* ControlNet only: len(conditioning_embedding_out_channels), <= 8; cond is [B, h * 2^(n-1), w * 2^(n-1), 8] */
    int cond_channels[8];          /* 16, 32, 96, 256 */
} fie_unet_config;
int fie_weights_register(fie_ctx* ctx, const char* name, const void* ptr, int64_t n, int64_t ld);
int fie_weights_clear(fie_ctx* ctx);
int fie_weights_clear_prefix(fie_ctx* ctx, const char* prefix);     /* forgets every name that starts with prefix (a model that goes away) */
/* AutoencoderKL.decode(latents / scaling_factor): z [1, h, w, 8] -> out [1, 8 h, 8 w, 4];  names "post_quant_conv", "decoder...." */
int64_t fie_vae_decode_workspace_bytes(const fie_vae_config* cfg, int latent_h, int latent_w);
int fie_vae_decode_f16(fie_ctx* ctx, const fie_vae_config* cfg, const void* z, void* out, void* workspace, int64_t workspace_bytes);
/* AutoencoderKL.encode(x).latent_dist parameters: x [1, 8 h, 8 w, 8] in [-1, 1] -> moments [h * w, 8] (mean | logvar);  names "encoder....", "quant_conv" */
int64_t fie_vae_encode_workspace_bytes(const fie_vae_config* cfg);
int fie_vae_encode_f16(fie_ctx* ctx, const fie_vae_config* cfg, const void* x, void* moments, void* workspace, int64_t workspace_bytes);
/* CLIPTextModel(.WithProjection)(ids, output_hidden_states=True): penultimate = hidden_states[-2] [batch * tokens, hidden]; pooled (projection_dim > 0
 * and pooled != NULL) = text_projection(final_layer_norm(last)[eos_rows]) [batch, projection_dim]; eos_rows: int32 [batch] ROW indices b * tokens + eos */
int64_t fie_clip_text_workspace_bytes(const fie_clip_config* cfg);
int fie_clip_text_forward_f16(fie_ctx* ctx, const fie_clip_config* cfg, const char* prefix, const int32_t* ids, const int32_t* eos_rows, void* penultimate,
                              void* pooled, void* workspace, int64_t workspace_bytes);
/* UNet2DConditionModel.forward(sample, t, encoder_hidden_states, added_cond_kwargs = {text_embeds, time_ids}, down_block_additional_residuals,
 * mid_block_additional_residual): x [B, h, w, 8], t f32 [B], text [B * text_len, cross_attention_dim], pooled [B, pooled_dim], time_ids f32 [B, 6]
 * (all on the device) -> eps [B, h, w, 4].  down_residuals: fie_unet_num_residuals(cfg) device pointers in skip order (conv_in output first), or NULL. */
int fie_unet_num_residuals(const fie_unet_config* cfg);
int64_t fie_unet_workspace_bytes(const fie_unet_config* cfg);
int fie_unet_forward_f16(fie_ctx* ctx, const fie_unet_config* cfg, const char* prefix, const void* x, const float* t, const void* text, const void* pooled,
                         const float* time_ids, const void* const* down_residuals, const void* mid_residual, void* eps_out, void* workspace,
                         int64_t workspace_bytes);
/* ControlNetModel.forward(sample, t, encoder_hidden_states, controlnet_cond, conditioning_scale, added_cond_kwargs): cond [B, H, W, 8] in [0, 1] ->
 * down_out[i] (shapes of the UNet's skips), mid_out: the zero-conv outputs times conditioning_scale, as upstream returns them */
int64_t fie_controlnet_workspace_bytes(const fie_unet_config* cfg);
int fie_controlnet_forward_f16(fie_ctx* ctx, const fie_unet_config* cfg, const char* prefix, const void* x, const float* t, const void* text, const void* pooled,
                               const float* time_ids, const void* cond, float conditioning_scale, void* const* down_out, void* mid_out, void* workspace,
                               int64_t workspace_bytes);
/* Step cache (optional): what a UNet / ControlNet forward computes from inputs that do NOT change over the denoising steps of one image -- the cross-
 * attention K / V of the text in every transformer block (upstream attention_processor.py: to_k / to_v of encoder_hidden_states) and the ControlNet's
 * conditioning embedding of the edge map -- kept in a caller-owned device buffer bound to the context under the model's prefix.  The first
 * fie_unet_forward_f16 / fie_controlnet_forward_f16 with that prefix after a bind or a reset FILLS the buffer (and ignores nothing: results are the
 * same bits), every later one READS it and skips those launches (SSD-1B: ~60 small GEMMs per UNet call, seven convs per ControlNet call).  The host
 * resets at every new image (new text / edge map); text, cond and the batch must stay what they were at the fill.  The decision is taken on the host when
 * the call is issued, so a hipGraph captured over a whole edit (reset, N x forwards) replays correctly.  Without a bound cache every call computes them. */
int64_t fie_unet_step_cache_bytes(const fie_unet_config* cfg, int controlnet);
int fie_step_cache_bind(fie_ctx* ctx, const char* prefix, void* ptr, int64_t bytes);     /* ptr NULL: unbind */
int fie_step_cache_reset(fie_ctx* ctx, const char* prefix);
/* the two element-wise helpers the walks need (also plain ops): out = a + b over n f16 values (n % 8 == 0); a strided row copy (cols % 8 == 0) */
int fie_add_f16(fie_ctx* ctx, const void* a, const void* b, void* out, int64_t n);
int fie_copy_rows_f16(fie_ctx* ctx, const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int rows, int cols);

typedef struct fie_program fie_program;
int fie_program_begin(fie_ctx* ctx, fie_program** out);
int fie_program_end(fie_ctx* ctx);
int fie_program_launches(const fie_program* p);             /* number of recorded launches (-1: NULL) */
int fie_program_run(fie_ctx* ctx, fie_program* p);          /* see ORDERING CONTRACT above */
int fie_program_destroy(fie_ctx* ctx, fie_program* p);      /* also drops its name bindings on ctx (ctx may be NULL) */
int fie_graph_register(fie_ctx* ctx, const char* name, fie_program* p);
int fie_unet_forward(fie_ctx* ctx);
int fie_controlnet_forward(fie_ctx* ctx);
int fie_vae_encode(fie_ctx* ctx);
int fie_vae_decode(fie_ctx* ctx);
int fie_clip_text_forward(fie_ctx* ctx);

/* ---- K2 GEMM (Linear / 1x1 conv).  Replaces torch.nn.Linear / 1x1 Conv2d dispatched by upstream
 * diffusers models/attention.py, transformer_2d.py, resnet.py (conv_shortcut), controlnet.py (zero convs),
 * embeddings.py (TimestepEmbedding), transformers modeling_clip.py -- all reached from src/pipeline.py:261.
 *   C[m, n] = epi( sum_k A[m, k] * W[n, k] ),  A = [A1 | A2] column-concatenated (A2 may be NULL; K1 = K then)
 *   epi(v) = act(v + bias[n] + rowbias[m / rows_per_batch, n]) * scale + residual[m, n]
 * W is the PACKED weight: [Npad][Kpad] f16, Kpad = roundup(K, 64), Npad = roundup(N, 128), zero filled (see
 * fie_pack_rows).  lda*, ldc, ldr in elements, multiples of 8 (ldc, ldr: multiples of 4).  K1 % 8 == 0, K % 8 == 0.
 * For FIE_ACT_GEGLU the output has N/2 columns. */
int fie_gemm_f16(fie_ctx* ctx, const void* A1, int64_t lda1, int K1, const void* A2, int64_t lda2,
                 const void* Wpacked, int64_t ldw, void* C, int64_t ldc, int M, int N, int K,
                 const void* bias, const void* rowbias, int64_t ld_rowbias, int rows_per_batch,
                 const void* residual, int64_t ldr, float scale, int act);

/* ---- LayerNorm folded into its consumer GEMM.  Replaces the pair nn.LayerNorm -> nn.Linear of upstream diffusers models/attention.py
 * BasicTransformerBlock (norm1 -> attn1.to_q/k/v, norm2 -> attn2.to_q, norm3 -> ff.net.0.proj), reached from src/pipeline.py:261.
 *   C[m, n] = act( sum_k LN(X)[m, k] * W[n, k] + bias[n] ),  LN(x) = (x - mean) * rsqrt(var + eps) * gamma + beta over the K columns of row m
 * computed WITHOUT ever forming LN(X):  = rstd[m] * (sum_k X[m, k] * Wf[n, k] - mean[m] * ln_tab[n][0]) + ln_tab[n][1]  with
 *   Wfolded = pack(W * gamma) (f16, the packed layout of fie_gemm_f16),  ln_tab[n] = (sum_k Wfolded[n, k], sum_k W[n, k] * beta[k] + bias[n]) in fp32,
 * in the PACKED column order (GEGLU: value / gate interleaved as fie_pack_rows_f16 with interleave2).  The row statistics are summed (fp32) from the
 * activation fragments on their way to the MFMAs; var = E[x^2] - mean^2, clamped at 0.  X: [M, K] f16 un-normalised (ldx elements), K % 64 == 0;
 * act = FIE_ACT_NONE or FIE_ACT_GEGLU (N % 320 == 0: the 256x320 tile; output has N/2 columns).  Differences from the two-launch sequence: the
 * normalised activation is not rounded to f16, W * gamma is (once, at load). */
int fie_gemm_ln_f16(fie_ctx* ctx, const void* X, int64_t ldx, const void* Wfolded, int64_t ldw, const float* ln_tab, float eps, void* C, int64_t ldc,
                    int M, int N, int K, int act);

/* ---- K1 3x3 convolution, NHWC, implicit GEMM on fp16 MFMA.  Replaces torch Conv2d(3x3) dispatched by upstream
 * resnet.py / downsampling.py / upsampling.py / vae.py / controlnet.py conditioning embedding.
 *   X: [B, H, W, Cin] f16 (Cin % 8 == 0).  If upsample2x != 0 the conv sees nearest-2x upsampled X (never stored).
 *   pad_mode 0: symmetric padding 1.  pad_mode 1: pad (right, bottom) only -- the VAE encoder's F.pad(0,1,0,1) + pad 0.
 *   Y: [B, OH, OW, ldc] with OH = (Hin + pads - 3)/stride + 1.  Wpacked: [Npad][Kpad], k = (ky*3 + kx)*Cin + ci.
 *   epilogue as fie_gemm_f16 with rows_per_batch = OH*OW (rowbias = per-image time-embedding projection). */
int fie_conv3x3_nhwc_f16(fie_ctx* ctx, const void* X, int B, int H, int W, int Cin, int upsample2x, int stride,
                         int pad_mode, const void* Wpacked, int64_t ldw, void* Y, int64_t ldc, int Cout,
                         const void* bias, const void* rowbias, int64_t ld_rowbias,
                         const void* residual, int64_t ldr, float scale, int act);

/* ---- K3/K3v/K4 + CLIP attention: softmax(scale * Q K^T [+ causal mask]) V, online softmax, one kernel family.
 * Replaces F.scaled_dot_product_attention reached via upstream attention_processor.py (UNet/ControlNet attn1/attn2,
 * VAE mid-block attention) and modeling_clip.py self-attention.
 *   element (b, t, h, d) of Q lives at Q[(b*Tq + t)*ldq + h*D + d]; K/V likewise with Tk, ldk, ldv; O with ldo.
 *   D in {64, 512}.  kv_batch_stride_zero != 0 broadcasts one K/V over the batch. */
int fie_attention_f16(fie_ctx* ctx, const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                      int64_t ldv, void* O, int64_t ldo, int B, int H, int Tq, int Tk, int D, float scale,
                      int causal);

/* ---- K5 GroupNorm (+SiLU), NHWC, fp32 statistics.  Replaces torch GroupNorm + SiLU in resnet.py /
 * transformer_2d.py / vae.py.  Input is the channel concatenation [X1 (C1) | X2 (C2)] (X2 may be NULL): this
 * is how the UNet up blocks' torch.cat([x, skip]) is consumed without materialising the concat.
 *   workspace: fie_groupnorm_workspace_bytes(B, rows, G) bytes of device scratch. */
int64_t fie_groupnorm_workspace_bytes(int B, int64_t rows_per_image, int groups);
int fie_groupnorm_nhwc_f16(fie_ctx* ctx, const void* X1, int C1, const void* X2, int C2, void* Y, int B,
                           int64_t rows_per_image, int groups, const void* gamma, const void* beta, float eps,
                           int silu, void* workspace);

/* ---- K6 LayerNorm over the last dim (affine).  Replaces torch LayerNorm in attention.py / modeling_clip.py. */
int fie_layernorm_f16(fie_ctx* ctx, const void* X, int64_t ldx, void* Y, int64_t ldy, int64_t rows, int C,
                      const void* gamma, const void* beta, float eps);

/* ---- K7 sinusoidal embeddings.  Replaces embeddings.py::get_timestep_embedding (flip_sin_to_cos, shift 0).
 *   out[b, i*dim .. (i+1)*dim) = [cos(v f), sin(v f)] for each of the `nvals` scalars v of row b; out row
 *   stride ld_out, column offset col0 (so the 6 add_time_ids land behind the pooled text embedding). */
int fie_sinusoid_f16(fie_ctx* ctx, const float* vals, int B, int nvals, int dim, void* out, int64_t ld_out,
                     int col0);

/* ---- K7 fused: the whole per-step timestep path in ONE launch (sinusoid -> Linear -> SiLU -> Linear -> + text-time embedding ->
 * the SiLU in front of every resnet's time projection).  Replaces Timesteps + TimestepEmbedding of embeddings.py and the
 * `emb = emb + aug_emb` / `nonlinearity(temb)` steps of unet_2d_condition.py / resnet.py for the M = batch rows of one step.
 *   t: f32 [B] on the device; W1 [E][C0], W2 [E][E] plain row-major f16 (NOT packed), b1, b2 [E]; add: [B][ld_add] f16 or NULL;
 *   out[b, n] = silu(W2 silu(W1 [cos(t f) | sin(t f)] + b1) + b2 + add[b, n]).  B <= 4, C0 % 32 == 0, E % 64 == 0.
 *   workspace: fie_time_embed_workspace_bytes(E) bytes, ZERO-filled once by the caller (hidden vector + the two counters of the
 *   in-launch barrier between the layers; the kernel leaves the counters at zero; the third counter word is a sticky "a workgroup's
 *   bounded spin expired: the output of that launch is not valid" flag, mirrored into the fie_ctx_error_flag word).  One workspace per
 *   (stream, model): launches that may run concurrently must not share one. */
int64_t fie_time_embed_workspace_bytes(int E);
int fie_time_embed_f16(fie_ctx* ctx, const float* t, int B, int C0, int E, const void* W1, const void* b1, const void* W2,
                       const void* b2, const void* add, int64_t ld_add, void* out, int64_t ld_out, void* workspace);

/* ---- K12 token + position embedding gather (CLIPTextEmbeddings). ids: int32 [B*T] on device. */
int fie_clip_embed_f16(fie_ctx* ctx, const int32_t* ids, int B, int T, int C, const void* tok_table,
                       const void* pos_table, void* out);

/* ---- K10 pixels.  Replaces image_processor.py::VaeImageProcessor.preprocess / postprocess.
 *   in : u8 HWC (3 ch) -> f16 NHWC padded to 8 ch; normalize != 0: x/255*2-1, else x/255; `copies` batch copies.
 *   out: f16 NHWC (ld_in channels, first 3 used) -> u8 HWC: round(clamp(x/2+0.5, 0, 1) * 255), evaluated in fp32 as written (x/2+0.5, the
 *        clamp, the product, each rounded once) and rounded half to even.  +Inf -> 255, -Inf -> 0, NaN -> 0 (the clamp's max takes the 0).
 *        For every finite f16 x this is the byte exact arithmetic gives; an fp32 x (fie_pixels_out_f32_u8) within 2^-22 of a rounding
 *        tie (k + 0.5) / 255 * 2 - 1 gets the byte of the fp32 evaluation (tests/pointwise_check.py: pixels_out_expect). */
int fie_pixels_in_u8_f16(fie_ctx* ctx, const uint8_t* src, int H, int W, int normalize, void* dst, int copies);
int fie_pixels_out_f16_u8(fie_ctx* ctx, const void* src, int64_t ld_in, int H, int W, uint8_t* dst);

/* ---- K9 latent prep.  Replaces DiagonalGaussianDistribution.sample, * scaling_factor, LCMScheduler.add_noise.
 *   moments: f16 [H*W, 8] (mean 0..3, logvar 4..7); eps_post, noise: f32 [4, H*W] (NCHW draw order, as torch.randn
 *   of shape [1,4,H,W]); latents_out: f32 [H*W, 4]; model_in: f16 [copies, H*W, 8] (zero padded). */
int fie_latent_prep(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW,
                    float scaling_factor, float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in,
                    int copies);

/* ---- K8 CFG combine + LCMScheduler.step.  Replaces pipeline CFG line + scheduling_lcm.py::step.
 *   eps: f16 [nb, H*W, ld_eps] (nb = 2 when guidance is applied: [uncond, cond]); latents: f32 [H*W, 4] (in/out);
 *   noise: f32 [4, H*W] or NULL on the last step; model_in as in fie_latent_prep; denoised_out may be NULL. */
int fie_lcm_step(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents,
                 const float* noise, int64_t HW, float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out,
                 float sqrt_ab_prev, float sqrt_1mab_prev, void* model_in, int copies, float inv_scaling,
                 void* decode_in);

/* ---- weight repack (one-time, on device): src [N][K] f16 row-major (ld_src) -> dst [Npad][Kpad] zero padded.
 *   conv: src is OIHW [Cout][Cin][3][3]; dst k-order (ky, kx, ci) with Cin padded to cin_pad.
 *   interleave2 != 0: rows (j, j + N/2) become adjacent (GEGLU value/gate pairing). */
int fie_pack_rows_f16(fie_ctx* ctx, const void* src, int64_t ld_src, int N, int K, void* dst, int64_t ldw,
                      int Npad, int interleave2);
int fie_pack_conv3x3_f16(fie_ctx* ctx, const void* src_oihw, int Cout, int Cin, int cin_pad, void* dst,
                         int64_t ldw, int Npad);

/* ---- fp8 (OCP e4m3) WEIGHTS on the fp8 MFMA: BASELINE.json config 5, the low-precision stretch beside the precision choice at
 * /root/reference/src/pipeline.py:67-71 (`FastEditor(..., weight_dtype="f8e4m3")`, additive).  Weights are e4m3 with one fp32
 * scale per output channel (scale[n] = max_k |W[n,k]| / 448); activations stay fp16 in HBM and are converted to e4m3 per fragment
 * in registers (saturating RNE, scale 1) for v_mfma_f32_16x16x32_fp8_fp8; fp32 accumulation;  epi(v) takes v * scale[n].
 *   fie_pack_rows_f8 / fie_pack_conv3x3_f8: as their _f16 twins, dst = [Npad][ldw] BYTES (ldw % 64 == 0), scales = [Npad] fp32 (out).
 *   fie_gemm_w8_f16 / fie_conv3x3_w8_nhwc_f16: as fie_gemm_f16 / fie_conv3x3_nhwc_f16 with (W8packed, ldw in bytes, w_scale).
 *   Shapes must be eligible for the LDS-DMA kernels (operands < 2 GiB, Cin % 64 == 0, K1 == K, or K1 % 64 == 0 and K % 64 == 0), else FIE_EINVAL. */
int fie_pack_rows_f8(fie_ctx* ctx, const void* src, int64_t ld_src, int N, int K, void* dst, int64_t ldw, int Npad, float* scales,
                     int interleave2);
int fie_pack_conv3x3_f8(fie_ctx* ctx, const void* src_oihw, int Cout, int Cin, int cin_pad, void* dst, int64_t ldw, int Npad,
                        float* scales);
int fie_gemm_w8_f16(fie_ctx* ctx, const void* A1, int64_t lda1, int K1, const void* A2, int64_t lda2, const void* W8packed,
                    int64_t ldw, const float* w_scale, void* C, int64_t ldc, int M, int N, int K, const void* bias,
                    const void* rowbias, int64_t ld_rowbias, int rows_per_batch, const void* residual, int64_t ldr, float scale,
                    int act);
int fie_conv3x3_w8_nhwc_f16(fie_ctx* ctx, const void* X, int B, int H, int W, int Cin, int upsample2x, int stride, int pad_mode,
                            const void* W8packed, int64_t ldw, const float* w_scale, void* Y, int64_t ldc, int Cout,
                            const void* bias, const void* rowbias, int64_t ld_rowbias, const void* residual, int64_t ldr,
                            float scale, int act);

/* ---- fp8 (OCP e4m3) ACTIVATIONS as well (config 5, round 3): the transformer-block projections of the UNet / ControlNet (upstream
 * attention.py BasicTransformerBlock: to_q/k/v, to_out, GEGLU proj, FF out) read e4m3 activations written by their PRODUCER -- LayerNorm
 * (fie_layernorm_f16_o8), attention (fie_attention_f16_o8), the FF1 GEGLU epilogue (fie_gemm_x8_f16 with out_f8) -- and multiply them with
 * e4m3 weights on the block-scaled MFMA v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales: twice the fp16 MFMA rate and half the
 * operand bytes.  Quantisation: value * inv_scale, round to nearest even, finite values saturated to +-448; a NaN is written as the e4m3 NaN
 * and +-Inf as NaN too (a blow-up upstream stays visible: the consuming MFMA spreads it); the consumer multiplies the fp32 accumulator by
 * a_scale (= 1 / inv_scale of its input, one per tensor) * w_scale[n].  inv_scale is the caller's: 1 clips activations beyond +-448 without
 * a signal, so a host calibrates it -- fie_amax_f16 folds max |x| of a tensor into a device float (atomic max; the caller zeroes it), run over
 * one representative edit with f16 activations, and inv_scale = 2^-k with k = ceil(log2(amax * margin / 448)) per quantised tensor (a power of
 * two: scaling is exact in both directions; fie_amd/pipe.py::calibrate_fp8 does this with margin 2).  The residual stream, q/k/v and every
 * GEMM output that is not a GEMM input stay fp16.
 *   fie_gemm_x8_f16: A8 [M, K] e4m3 bytes (row stride lda BYTES, K % 16 == 0, lda % 16 == 0); W8packed / w_scale from fie_pack_rows_f8 with
 *     ldw % 128 == 0; epilogue as fie_gemm_f16; out_f8 != 0: C is e4m3 bytes (value * out_inv_scale; ldc in BYTES; GEGLU: N / 2 bytes per row;
 *     no residual), else f16 (ldc in elements).
 *   fie_quantize_f8: plain f16 -> e4m3 conversion of a [rows, C] tensor (tests; producers without a fused form). */
int fie_gemm_x8_f16(fie_ctx* ctx, const void* A8, int64_t lda, const void* W8packed, int64_t ldw, const float* w_scale, float a_scale, void* C, int64_t ldc,
                    int M, int N, int K, const void* bias, const void* rowbias, int64_t ld_rowbias, int rows_per_batch, const void* residual, int64_t ldr,
                    float scale, int act, int out_f8, float out_inv_scale);
int fie_layernorm_f16_o8(fie_ctx* ctx, const void* X, int64_t ldx, void* Y8, int64_t ldy8, int64_t rows, int C, const void* gamma, const void* beta,
                         float eps, float inv_scale);
int fie_attention_f16_o8(fie_ctx* ctx, const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv, void* O8, int64_t ldo8,
                         int B, int H, int Tq, int Tk, int D, float scale, int causal, float inv_scale);
int fie_quantize_f8(fie_ctx* ctx, const void* X, int64_t ldx, void* Y8, int64_t ldy, int64_t rows, int C, float inv_scale);
int fie_amax_f16(fie_ctx* ctx, const void* X, int64_t ldx, int64_t rows, int C, float* amax);
/* The resnet convs of an fp8 model (upstream resnet.py: GroupNorm -> SiLU -> conv): GroupNorm writes e4m3 (the _o8 twins of fie_groupnorm_nhwc_f16 /
 * fie_groupnorm_stats_nhwc_f16; Y8 = [B, rows, C] bytes) and fie_conv3x3_x8_nhwc_f16 runs the conv view of the same block-scaled MFMA kernel: X8 NHWC
 * e4m3 with Cin % 128 == 0 (a K-step is 128 channels of one tap), W8packed from fie_pack_conv3x3_f8 with cin_pad == Cin; output f16.  Conv + 1x1 side
 * inputs and the 2x2 parity up-samplers have no fp8-activation form (their other inputs are the fp16 residual stream). */
int fie_groupnorm_nhwc_f16_o8(fie_ctx* ctx, const void* X1, int C1, const void* X2, int C2, void* Y8, int B, int64_t rows_per_image, int groups,
                              const void* gamma, const void* beta, float eps, int silu, void* workspace, float inv_scale);
int fie_groupnorm_stats_nhwc_f16_o8(fie_ctx* ctx, const void* X, int C, void* Y8, int B, int64_t rows_per_image, int groups, const void* gamma,
                                    const void* beta, float eps, int silu, const void* partial, void* workspace, int partial_groups, float inv_scale);
int fie_conv3x3_x8_nhwc_f16(fie_ctx* ctx, const void* X8, int B, int H, int W, int Cin, int upsample2x, int stride, int pad_mode, const void* W8packed,
                            int64_t ldw, const float* w_scale, float a_scale, void* Y, int64_t ldc, int Cout, const void* bias, const void* rowbias,
                            int64_t ld_rowbias, const void* residual, int64_t ldr, float scale, int act);

/* ---- fp32 path (`FastEditor(use_full_precision=True)`, run_batch.py --full_precision / --quality_mode; reference:
 * src/pipeline.py:67-71,94-99).  Same graphs, fp32 storage, exact fp32 arithmetic on v_mfma_f32_16x16x4_f32.
 *   fie_gemm_f32: as fie_gemm_f16 with plain (unpacked) weights W [N][ldw] -- or [K][ldw] when w_is_kn -- and a two-level
 *     batch (z1 < nb1, z2 < nb2; element strides sA*, sW*, sC*) that serves the attention products over (image, head).
 *   fie_conv3x3_nhwc_f32: weights [Cout][(ky, kx, ci)] (ldw >= 9*Cin).
 *   These two also take act = FIE_ACT_RELU (max(x, 0), in the epilogue's usual place: bias -> act -> scale -> residual).
 *   fie_softmax_rows_f32: in-place softmax(scale * S) per row, keys > (row % tq) masked when causal.
 *   the *_f32 norm / element-wise entries mirror their f16 twins with fp32 tensors. */
int fie_gemm_f32(fie_ctx* ctx, const float* A1, int64_t lda1, int K1, const float* A2, int64_t lda2, const float* W,
                 int64_t ldw, int w_is_kn, float* C, int64_t ldc, int M, int N, int K, const float* bias,
                 const float* rowbias, int64_t ld_rowbias, int rows_per_batch, const float* residual, int64_t ldr,
                 float scale, int act, int nb1, int nb2, int64_t sA1, int64_t sA2, int64_t sW1, int64_t sW2, int64_t sC1,
                 int64_t sC2);
int fie_conv3x3_nhwc_f32(fie_ctx* ctx, const float* X, int B, int H, int W, int Cin, int upsample2x, int stride, int pad_mode,
                         const float* Wkc, int64_t ldw, float* Y, int64_t ldc, int Cout, const float* bias,
                         const float* rowbias, int64_t ld_rowbias, const float* residual, int64_t ldr, float scale, int act);
int fie_softmax_rows_f32(fie_ctx* ctx, float* S, int64_t rows, int cols, int64_t ld, float scale, int causal, int tq);
int fie_groupnorm_nhwc_f32(fie_ctx* ctx, const void* X1, int C1, const void* X2, int C2, void* Y, int B,
                           int64_t rows_per_image, int groups, const void* gamma, const void* beta, float eps,
                           int silu, void* workspace);
int fie_layernorm_f32(fie_ctx* ctx, const void* X, int64_t ldx, void* Y, int64_t ldy, int64_t rows, int C,
                      const void* gamma, const void* beta, float eps);
int fie_sinusoid_f32(fie_ctx* ctx, const float* vals, int B, int nvals, int dim, void* out, int64_t ld_out, int col0);
int fie_clip_embed_f32(fie_ctx* ctx, const int32_t* ids, int B, int T, int C, const void* tok_table,
                       const void* pos_table, void* out);
int fie_pixels_in_u8_f32(fie_ctx* ctx, const uint8_t* src, int H, int W, int normalize, void* dst, int copies);
int fie_pixels_out_f32_u8(fie_ctx* ctx, const void* src, int64_t ld_in, int H, int W, uint8_t* dst);
int fie_latent_prep_f32(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW,
                        float scaling_factor, float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in,
                        int copies);
int fie_lcm_step_f32(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents,
                     const float* noise, int64_t HW, float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out,
                     float sqrt_ab_prev, float sqrt_1mab_prev, void* model_in, int copies, float inv_scaling,
                     void* decode_in);

/* ---- tuning / test hooks (not part of the drop-in surface).  Tile hooks are PER CTX: nothing process-global sits on the
 * launch path.  Tile codes: 1/2/3 register-staged 128x128 / 128x64 / 64x64 (any shape); 41/42/43 LDS-DMA ring 128x128 /
 * 128x64 / 64x64; 51 ring 128x128 x 8 waves; 61/62 ring 256x256 / 256x128 x 8 waves; 81 phased 256x256 (gemm8.hip); 71-76 the
 * halo-resident 3x3 conv on maps whose sides are multiples of 16 (conv_halo.hip; 72 = the rule's); 77 the thin conv (<= 16 output channels);
 * 78 the halo-resident conv with edge patches: stride-1 same-size 3x3 convs whose height or width is NOT a multiple of 16 (the aspect-ratio
 * buckets), Cin % 64 == 0, Cin >= 128, N % 64 == 0, no activation / scale, no GroupNorm sums; partial 16x16 patches at the right / bottom edges,
 * per-pixel store masks; sums K chunk-major like 71-76 (equal to the im2col codes to rounding; bit for bit on integer data).
 * + 1000 / + 2000: force n-tiles / m-tiles fastest tile order (plain codes estimate the order that re-streams fewer bytes).  A code the shape is not eligible for returns FIE_EINVAL from the op. */
int fie_debug_force_tile(fie_ctx* ctx, int tile);                  /* 0 = heuristic */
int fie_debug_tile_override(fie_ctx* ctx, const char* spec);       /* "mode,M,N,K=code;..." (mode 0 GEMM, 1 conv); NULL clears; returns the count */
/* Per-shape tile autotune.  on = 1: the first EAGER launch of every GEMM / 3x3-conv problem (M, N, K, geometry, weight type) times
 * the eligible tile kernels on a scratch output (the caller's C is written once, by the winner), each launch with the weights
 * cold (a 384 MB flush) and the activations warm, as a layer inside the network sees them, and the context remembers the
 * fastest; launches under stream capture or program recording never tune, they use what is remembered, else the built-in rule.
 * Every tile accumulates K in the same order, so the choice does not change results.  on = 2 keeps using what is remembered but
 * tunes nothing new and frees the scratch (0.4 GB + one output); on = 0 returns to the built-in rule.  fie_gemm_autotune_report writes one "gemm|conv M= N= K= K1= geom= w8= -> code" line per remembered problem
 * into buf (NUL-terminated, truncated to cap) and returns the number of problems. */
/* A resnet's second conv together with its 1x1 shortcut (upstream models/resnet.py ResnetBlock2D.forward: conv2(h) + conv_shortcut(input))
 * as ONE GEMM: Y = conv3x3(X) + [X2 | X3] W1x1^T (+ bias, row bias, activation), Wpacked rows = [9 * Cin taps | C2 | C3] (the conv's packed
 * matrix with the shortcut's columns appended; bias = the two biases added).  X [B, H, W, Cin]; X2 [B*H*W, C2] and the optional X3
 * [B*H*W, C3] (row strides ld2 / ld3) are the shortcut's input, or its two halves when that is a concat [x | skip]; Cin, C2, C3 % 64 == 0.
 * The shortcut GEMM, its [M, Cout] output and the residual read disappear; the sum is rounded once. */
int fie_conv3x3_plus_nhwc_f16(fie_ctx* ctx, const void* X, int B, int H, int W, int Cin, const void* Wpacked, int64_t ldw, void* Y, int64_t ldc, int Cout,
                              const void* bias, const void* rowbias, int64_t ld_rowbias, float scale, int act, const void* X2, int64_t ld2, int C2,
                              const void* X3, int64_t ld3, int C3);

/* conv3x3 on the nearest-2x upsampled input (upstream models/upsampling.py Upsample2D: F.interpolate(scale_factor=2, mode="nearest") then
 * conv) computed as four 2x2 convs on the input itself, one per output parity, with the weights of the taps that coincide on one input
 * pixel summed beforehand: the same sums (zero padding included) from 4 instead of 9 multiply-adds per output.  W4 = the four packed
 * matrices [py * 2 + px][Npad][ldw] with K index (a * 2 + b) * Cin + ci (fie_amd/hip.py: pack_conv_up2x builds them from the OIHW
 * weights).  X [B, H, W, Cin] (Cin % 64 == 0) -> Y [B, 2H, 2W, ldc]; epilogue options as fie_conv3x3_nhwc_f16 without a residual; an
 * armed fie_gn_stats_target (rows_per_image = 4 H W) is honoured.  Differs from the 9-tap form by the f16 rounding of the summed weights. */
int fie_conv_up2x_nhwc_f16(fie_ctx* ctx, const void* X, int B, int H, int W, int Cin, const void* W4, int64_t ldw, int Npad, void* Y, int64_t ldc,
                           int Cout, const void* bias, const void* rowbias, int64_t ld_rowbias, float scale, int act);

/* GroupNorm statistics from the producer's epilogue (upstream: the first of the three passes torch.nn.GroupNorm makes over the tensor,
 * models/resnet.py norm1 / norm2, models/autoencoders/vae.py).  fie_gn_stats_target arms the NEXT fie_gemm_f16 / fie_conv3x3_nhwc_f16
 * launch on this context (one shot): besides its output [M, N] it writes, per image (rows_per_image rows, a multiple of 32), per 32-row
 * granule and per group, the sum and the sum of squares of the f16-ROUNDED outputs: partial[B][rows_per_image / 32][groups][2] floats
 * (fie_gn_stats_bytes).  N / groups must be 4, 8 or 16 channels (the SDXL VAE's 128 / 256 / 512-channel maps with 32 groups); no GEGLU.
 * Every slot has one writer: deterministic.  fie_groupnorm_stats_nhwc_f16 is fie_groupnorm_nhwc_f16 for such a tensor: it reduces the
 * partials (fp64) and applies, reading X once instead of twice; workspace as for fie_groupnorm_nhwc_f16.
 * Group widths that are not 4 / 8 / 16 but a multiple of 4 (the UNet's 20 / 40 channels per group at 640 / 1280 channels): arm the producer
 * with groups = N / 4 (it then writes one slot per 4-channel QUAD, which is all a lane of the MFMA layout can sum without crossing a group
 * border) and pass partial_groups = N / 4 to fie_groupnorm_stats_nhwc_f16, which sums the N / 4 / groups quads of each real group
 * (partial_groups 0 or == groups: slots are groups, as above). */
int fie_gn_stats_target(fie_ctx* ctx, void* partial, int64_t rows_per_image, int groups);
/* GroupNorm (+ SiLU) FUSED INTO THE CONSUMING 3x3 CONV (round 4; upstream models/resnet.py: norm1 -> nonlinearity -> conv1, norm2 -> nonlinearity -> conv2).
 * fie_groupnorm_coef_f16 finishes the statistics a producer's epilogue left (as fie_groupnorm_stats_nhwc_f16 does) but writes, instead of a normalised
 * tensor, coef[B][C][2] floats: (sc, sh) = (rstd * gamma, beta - mean * rstd * gamma).  fie_conv3x3_gn_nhwc_f16 is the same-size stride-1 3x3 conv of
 * silu(X * sc + sh) (silu optional): the halo-resident kernel applies the expression to every 64-channel chunk of a 16x16 patch's halo while it sits in LDS,
 * behind the MFMAs of the chunk before; padding pixels stay zero (the conv pads the NORMALISED tensor).  Same fp32 expression as the apply kernel: the
 * result has the bits of fie_groupnorm_stats_nhwc_f16 followed by fie_conv3x3_nhwc_f16 on tile code 72, without the read + write of the normalised tensor.
 * Built for what fie_conv3x3_gn_ok returns 1 for (one image, H, W % 16 == 0, Cin in whole 64-channel chunks from 128 to 1024, Cout % 128 == 0) WITH a
 * fie_gn_stats_target armed for the OUTPUT at 4 / 8 / 16 channels per group (out_groups) -- every resnet conv of the VAE; elsewhere the caller keeps the two
 * launches.  workspace as for fie_groupnorm_nhwc_f16.  X [B, rows, C] is the tensor the sums were taken of: a group whose mean lies beyond 8 sigma takes its
 * variance from X itself (the raw fp32 sums of y^2 have lost it), here and in fie_groupnorm_stats_nhwc_f16. */
int fie_groupnorm_coef_f16(fie_ctx* ctx, const void* X, int C, int B, int64_t rows_per_image, int groups, const void* gamma, const void* beta, float eps,
                           const void* partial, void* workspace, int partial_groups, float* coef);
int fie_conv3x3_gn_ok(fie_ctx* ctx, int B, int H, int W, int Cin, int Cout, int out_groups);
int fie_conv3x3_gn_nhwc_f16(fie_ctx* ctx, const void* X, int B, int H, int W, int Cin, const float* coef, int silu, const void* Wpacked, int64_t ldw, void* Y,
                            int64_t ldc, int Cout, const void* bias, const void* residual, int64_t ldr);
int64_t fie_gn_stats_bytes(int B, int64_t rows_per_image, int groups);
int fie_groupnorm_stats_nhwc_f16(fie_ctx* ctx, const void* X, int C, void* Y, int B, int64_t rows_per_image, int groups, const void* gamma,
                                 const void* beta, float eps, int silu, const void* partial, void* workspace, int partial_groups);

/* Touches one dword of every 128-byte line of [ptr, ptr + bytes) with `blocks` small workgroups on `stream` (NULL: the context's): pulls a
 * weight matrix from HBM into the Infinity Cache ahead of the kernel that will stream it.  Reads only; no result. */
int fie_prefetch(fie_ctx* ctx, const void* ptr, int64_t bytes, void* stream, int blocks);
/* Split-K for the GEMM / conv ring kernels (M = 2048-class problems whose big tiles leave most CUs idle): binds a caller-owned device
 * workspace to the context -- 16 KiB of arrival counters that MUST be zero when bound (every launch leaves them zero again) followed by
 * the fp32 partial-tile slabs.  Launches that run concurrently (different streams) need different workspaces: bind the stream's own
 * before issuing on it -- that holds for the op entries, for the *_forward_f16 walks and for recorded programs / captured graphs, which
 * keep the workspace that was bound when they were recorded (see ORDERING CONTRACT at fie_program_run).  NULL unbinds (no launch splits
 * K then).  The counters are self-healing (a launch takes its arrivals off again with one atomic subtract), so a violation of the rule
 * corrupts only the overlapping launches' sums, never later ones.  A launch splits only where the autotuner measured it faster, or an
 * override asks (tile codes: split factor * 10000 + code); it falls back to the unsplit kernel when the workspace is too small.
 * Determinism: slices are summed in slice order by the block that arrives last, so results do not depend on timing. */
int fie_splitk_workspace(fie_ctx* ctx, void* workspace, int64_t bytes);
int fie_debug_splitk(fie_ctx* ctx, int mode);                       /* 0 = never split K, 1 = default */
int fie_gemm_autotune(fie_ctx* ctx, int on);
int fie_gemm_autotune_report(fie_ctx* ctx, char* buf, int cap);
/* Remembered choices from a report's text (the inverse of fie_gemm_autotune_report; unknown lines are skipped): a host saves the report of a
 * tuned process and loads it into the next one -- no timing launches at start-up and the same kernels on every box (a split-K choice moves
 * the last f16 bit).  FIE_TUNE_TABLE=<file> makes fie_amd load it into every context.  Returns the number of problems loaded. */
int fie_gemm_autotune_load(fie_ctx* ctx, const char* text);
int fie_debug_tune_exclude(fie_ctx* ctx, const char* codes);        /* A/B hook (tools/tuner_ab.py): comma-separated tile codes the tuner must not offer (10000 = every split-K variant; NULL / "" = none); forgets every remembered choice; returns the number of codes parsed */
int fie_debug_gemm_probe(fie_ctx* ctx, int mode);                  /* TIMING-ONLY probes of the LDS-DMA kernels (outputs are wrong): 0 off, 1 = DMA loads dropped by the descriptor, 2 = every tile loads tile (0,0), 3 = ring kernels: no DMA issued in the K loop, 4 = no epilogue */
int fie_debug_epilogue_prefetch(fie_ctx* ctx, int on);            /* A/B switch (default on): the ring GEMM / conv kernels load the bias row and the residual tile BEFORE the K loop; results are identical either way */
int fie_debug_gemm_stamps(fie_ctx* ctx, void* buf);                  /* device buffer for the stamped ring kernels (tile codes 97 / 98): per tile and wave 8 uint32 cycle sums -- [0] drain + barrier, [1]/[4] DMA issue, [2]/[5] fragment reads, [3]/[6] MFMA issue (code 98: [0] = whole K-steps); NULL detaches */
const char* fie_debug_last_gemm_kernel(fie_ctx* ctx);              /* kernel / tile of the last fie_gemm_f16 / fie_conv3x3_nhwc_f16 launch */
int fie_debug_oplog(fie_ctx* ctx, int on);                         /* launch log for the per-shape profile (tools/shape_profile.py): while on, every launch appends "kernel symbol|blocks|threads|LDS bytes|op description (shape, tile code, algorithmic flop / bytes)" */
int fie_debug_oplog_mark(fie_ctx* ctx, const char* text);           /* appends "#text" (a stage boundary) when the log is on */
int64_t fie_debug_oplog_read(fie_ctx* ctx, char* buf, int64_t cap);  /* newline-joined log into buf when it fits; returns its length (cap 0: size query) */
int fie_debug_tune_candidates(fie_ctx* ctx, int on);               /* while on, every GEMM / conv launch the tuner could decide appends "gemm|conv M= N= K= K1= geom= w8= rule=<code> cands=<c>,..." (exactly the list autotune times besides the rule; split-K as code + 10000 * s) and runs the rule's code (tests/test_launch_table_gpu.py) */
int64_t fie_debug_tune_candidates_read(fie_ctx* ctx, char* buf, int64_t cap);  /* newline-joined lines into buf when they fit; returns their length (cap 0: size query) */
int fie_debug_attn_variant(fie_ctx* ctx, int variant);   /* per context; 0 = default kernel, 1 = first-generation kernel, 2 / 3 = 128 / 64 queries per block forced, 4 = 64 queries per block as two waves x 32 (A/B benchmarking) */
int fie_debug_gn_onepass(fie_ctx* ctx, int enable);      /* per context; 1 = default (single-pass GroupNorm on small maps), 0 = always partial/finalize/apply */

/* ---- K11 Canny on the host (integer exact).  Replaces cv2.cvtColor(RGB2GRAY) + cv2.Canny at
 * src/pipeline.py:200,205 and the 3-channel stack at :208.  rgb, edges_rgb: host u8 [H, W, 3]. */
int fie_canny_rgb_u8(const uint8_t* rgb, int H, int W, int low, int high, uint8_t* edges_rgb);

/* ---- K11 on the device: same integer-exact result as fie_canny_rgb_u8, on a u8 HWC image already in HBM.
 *   workspace: fie_canny_workspace_bytes(H, W) bytes.  The hysteresis fixed point reads a flag back, so this entry
 *   SYNCHRONISES the ctx stream (it runs in the host-side preparation of an edit, never inside the captured graph).
 *   iterations (optional, host int): hysteresis passes launched. */
int64_t fie_canny_workspace_bytes(int H, int W);
int fie_canny_rgb_device_u8(fie_ctx* ctx, const uint8_t* rgb, int H, int W, int low, int high, void* workspace,
                            uint8_t* edges_rgb, int* iterations);
/* The same in two halves, so that the host need not wait for the hysteresis flag before it goes on: begin launches NMS, `rounds` rounds of four
 * hysteresis passes, the edge map of that state and an asynchronous copy of the LAST round's four flag words into host_flags (4 ints of PINNED host
 * memory) and returns without waiting; finish synchronises the stream, runs further rounds only if that round's last pass still changed something
 * (a weak chain that crosses more than 4 * rounds - 1 tiles of 32x32), rewrites the edge map then, and reports the passes IT launched (0: the map begin
 * wrote was final).  fie_amd's FastEditor.edit() begins with 4 rounds, issues the whole edit behind it and calls finish at the edit's own final
 * synchronisation: no host wait at all in the common case, a repeated device job in the rare one.  Same result as the one-call form. */
int fie_canny_rgb_device_begin_u8(fie_ctx* ctx, const uint8_t* rgb, int H, int W, int low, int high, int rounds, void* workspace, uint8_t* edges_rgb,
                                  int* host_flags);
int fie_canny_rgb_device_finish_u8(fie_ctx* ctx, int H, int W, void* workspace, uint8_t* edges_rgb, int* host_flags, int* iterations);

/* ---- Edge-budget Canny: the thresholds are picked per image, on the device, so that at most `budget` pixels are strong
 * edge seeds.  r[p] = the L1 magnitude of p where p passes the non-maximum-suppression direction test, else 0 (threshold free, 0 .. 2040);
 * high = the smallest h in 16 .. 2040 with #{p : r[p] > h} <= budget; low = high * lo / hi with (lo, hi) the caller's thresholds, swapped when
 * lo > hi: they give only the ratio.  The edge map is Canny(low, high).  Arguments: 1 <= budget <= H W < 2^31, 0 <= lo, hi, not both 0, workspace
 * 16-byte aligned; anything else is FIE_EINVAL.
 *   fie_canny_auto_workspace_bytes: label map and flag words where fie_canny_rgb_device_finish_u8 expects them (that entry finishes this form
 *     too), the pair, the u16 ridge map and the 2048-bin histogram; -1 for a bad size.
 *   fie_canny_rgb_device_begin_auto_u8: fie_canny_rgb_device_begin_u8 with ridge + histogram, select and classify kernels in place of the NMS
 *     kernel.  Nothing is waited for and the pair reaches the classify kernel through device memory; host_words: 6 ints of PINNED host
 *     memory, the 4 flag words, then low and high (valid once the stream has drained).
 *   fie_canny_thresholds_device_u8: ridge + select alone, {low, high} into pair_dev (2 ints of device memory); does not synchronise.
 *   fie_canny_auto_thresholds_u8: the same pair on the host (rgb: host memory; out: 2 ints). */
int64_t fie_canny_auto_workspace_bytes(int H, int W);
int fie_canny_rgb_device_begin_auto_u8(fie_ctx* ctx, const uint8_t* rgb, int H, int W, int64_t budget, int lo, int hi, int rounds, void* workspace,
                                       uint8_t* edges_rgb, int* host_words);
int fie_canny_thresholds_device_u8(fie_ctx* ctx, const uint8_t* rgb, int H, int W, int64_t budget, int lo, int hi, void* workspace, int* pair_dev);
int fie_canny_auto_thresholds_u8(const uint8_t* rgb, int H, int W, int64_t budget, int lo, int hi, int* out);

/* ---- K13 LANCZOS resize on the device, bit-exact with Pillow's 8-bit resample.  Replaces
 * `image.resize((1024, 1024), Image.LANCZOS)` at src/pipeline.py:251 (the PIL image is uploaded at its own size instead).
 *   src u8 [H, W, 3] -> dst u8 [OH, OW, 3] on the device; kx/ky: int32 [OW|OH, ks] 22-bit fixed-point taps, bx/by: int32
 *   [OW|OH, 2] = (first input index, tap count) -- Pillow's precompute_coeffs / normalize_coeffs_8bpc, restated in
 *   fie_amd/resize.py; a table may be NULL when that axis keeps its size.  tmp: u8 [H, OW, 3] scratch (both axes change).
 *   Asynchronous on the ctx stream. */
int fie_resize_rgb_u8(fie_ctx* ctx, const uint8_t* src, int H, int W, uint8_t* dst, int OH, int OW, const int* kx,
                      const int* bx, int ksx, const int* ky, const int* by, int ksy, uint8_t* tmp);

/* ---- K13 on one band: LANCZOS resize of a u8 [H, W] mode-L image (an edit mask), bit-exact with Pillow's
 *   `mask.convert("L").resize(..., Image.LANCZOS)`; arguments and coefficient tables as fie_resize_rgb_u8, tmp [H, OW]. */
int fie_resize_l_u8(fie_ctx* ctx, const uint8_t* src, int H, int W, uint8_t* dst, int OH, int OW, const int* kx,
                    const int* bx, int ksx, const int* ky, const int* by, int ksy, uint8_t* tmp);

/* ---- Mask-restricted edits.  In an edit, in order:
 *   1. fie_resize_l_u8 (when the mask is not at the edit size), then fie_mask_prep: mask_l u8 [H, W] (white = edit) ->
 *      mask_px f32 [H, W] (L >= 128 as 0 / 1, feathered by a separable Gaussian when radius > 0) and mask_lat u8 [H/8 * W/8]
 *      (mask_lat[y][x] = binary mask at [8y][8x]).  taps: f32 [2 * radius + 1], the normalised Gaussian of sigma r sampled at
 *      -R .. R (radius R = ceil(3r) <= 64; {1.0f} with radius 0); borders clamp to the edge.  One launch.
 *   2. fie_latent_prep_src in place of fie_latent_prep: also stores the clean source latent z0_out f32 [H*W, 4] (latent pixels).
 *   3. fie_lcm_step_masked in place of fie_lcm_step, every step: after the step, latent pixels where mask_lat == 0 take
 *      sqrt_ab_prev * z0 + sqrt_1mab_prev * noise_init (noise_init: the init noise of fie_latent_prep, f32 [4, H*W]), or z0 on
 *      the last step (noise == NULL); model_in / decode_in are written from the blended latents.
 *   4. fie_pixels_out_composite_* in place of fie_pixels_out_* (paste-back; without it keep fie_pixels_out_*): source u8
 *      [H, W, 3] (the resized source image) where mask == 0, the decoded byte where mask == 1, rint(m d + (1 - m) source)
 *      between, d the unrounded clamp(x / 2 + 0.5, 0, 1) * 255.  mask: fie_mask_prep's mask_px (16-byte aligned). */
int fie_mask_prep(fie_ctx* ctx, const uint8_t* mask_l, int H, int W, const float* taps, int radius, float* mask_px,
                  uint8_t* mask_lat);
int fie_latent_prep_src(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW,
                        float scaling_factor, float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in,
                        int copies, float* z0_out);
int fie_latent_prep_src_f32(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW,
                            float scaling_factor, float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in,
                            int copies, float* z0_out);
int fie_lcm_step_masked(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents,
                        const float* noise, int64_t HW, float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out,
                        float sqrt_ab_prev, float sqrt_1mab_prev, void* model_in, int copies, float inv_scaling,
                        void* decode_in, const uint8_t* mask_lat, const float* z0, const float* noise_init);
int fie_lcm_step_masked_f32(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents,
                            const float* noise, int64_t HW, float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out,
                            float sqrt_ab_prev, float sqrt_1mab_prev, void* model_in, int copies, float inv_scaling,
                            void* decode_in, const uint8_t* mask_lat, const float* z0, const float* noise_init);
int fie_pixels_out_composite_f16_u8(fie_ctx* ctx, const void* src, int64_t ld_in, int H, int W, const uint8_t* source,
                                    const float* mask, uint8_t* dst);
int fie_pixels_out_composite_f32_u8(fie_ctx* ctx, const void* src, int64_t ld_in, int H, int W, const uint8_t* source,
                                    const float* mask, uint8_t* dst);

/* ---- Masked-content modes of a mask-restricted edit: what the model starts from inside the mask.
 *   fie_mask_fill_rgb_u8    src u8 [H, W, 3], mask_l u8 [H, W] (hole = L >= 128), any H, W >= 1 with H * W <= 2^24.
 *      out (optional) u8 [H, W, 3]: src with the hole replaced by a smooth continuation of its surroundings, known pixels byte-identical.
 *      The fill is a push-pull pyramid in integer arithmetic, exact to the bit (DESIGN.md section 14 defines it; tests/masked_content_oracle.py
 *      restates it in numpy): per level the sums of the known pixels and their count over 2x2 children, sides ceil-halved to 1x1; from the top
 *      down a cell with known pixels is their mean in 1/256 units, one without the 9-3-3-1 bilinear tap of the level above (32768 at the top).
 *      ctl_in / ctl_out (optional, a pair) u8 [H, W, 3]: the ControlNet's edge map with every pixel of the hole set to 0.  With out == NULL
 *      the op only clears the edge map (one launch; src and workspace may be NULL).  out may be src, ctl_out may be ctl_in.
 *      workspace: fie_mask_fill_workspace_bytes(H, W) bytes (-1 for sizes the op refuses), 16-byte aligned: the pyramid above the image.
 *      Launches: one per level below the first of <= 1024 cells in each direction, one single-block kernel for that level and all above
 *      it, one for the image (11 at 1024 x 1024).  Asynchronous on the ctx stream; no block waits for another, no atomics.
 *   fie_latent_prep_src_content   fie_latent_prep_src, then for FIE_CONTENT_LATENT_NOISE / _NOTHING a select over the latent pixels with
 *      mask_lat != 0: latents_out = noise (the init noise itself), or sqrt_1mab * noise (add_noise of the zero latent, one f32 product);
 *      model_in is cast from the selected value; z0_out and every value outside the mask keep fie_latent_prep_src's bits.
 *      FIE_CONTENT_ORIGINAL / _FILL: fie_latent_prep_src alone (the fill acts on the image in front of the VAE encode). */
#define FIE_CONTENT_ORIGINAL 0
#define FIE_CONTENT_FILL 1
#define FIE_CONTENT_LATENT_NOISE 2
#define FIE_CONTENT_LATENT_NOTHING 3
int64_t fie_mask_fill_workspace_bytes(int H, int W);
int fie_mask_fill_rgb_u8(fie_ctx* ctx, const uint8_t* src, const uint8_t* mask_l, int H, int W, void* workspace, uint8_t* out,
                         const uint8_t* ctl_in, uint8_t* ctl_out);
int fie_latent_prep_src_content(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW,
                                float scaling_factor, float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in,
                                int copies, float* z0_out, const uint8_t* mask_lat, int mode);
int fie_latent_prep_src_content_f32(fie_ctx* ctx, const void* moments, const float* eps_post, const float* noise, int64_t HW,
                                    float scaling_factor, float sqrt_ab, float sqrt_1mab, float* latents_out, void* model_in,
                                    int copies, float* z0_out, const uint8_t* mask_lat, int mode);

/* ---- One-sided multi-band paste-back of a mask-restricted edit: the seam of a masked edit without a wide alpha ramp.
 *   fie_multiband_blend_rgb_u8   edit u8 [H, W, 3] (A: what fie_pixels_out_* wrote), source u8 [H, W, 3] (S: the resized source), mask_l u8 [H, W]
 *      (m = L >= 128), any H, W >= 1 with H * W <= 2^24, levels L in 1 .. 6.  out u8 [H, W, 3] (aliases no operand).
 *      Signed 32-bit integers, >> floors; level k has sides h_k+1 = (h_k + 1) >> 1.  D_0 = 16 (A - S), G_0 = 256 m; D_k+1 = reduce(D_k),
 *      G_k+1 = reduce(G_k), reduce = the 5x5 binomial [1 4 6 4 1]^2 at (2Y, 2X), indices clamped, (sum + 128) >> 8.  expand(g) at index i per
 *      axis: parents (i >> 1) - 1, i >> 1, (i >> 1) + 1 (clamped) weighted 1 6 1 for even i, 0 4 4 for odd; the 2-D sum (+ 32) >> 6.
 *      W_k = max(0, 2 G_k - 256).  C_L = (W_L D_L + 128) >> 8; C_k = ((W_k (D_k - expand(D_k+1)) + 128) >> 8) + expand(C_k+1);
 *      B = clamp(S + ((C_0 + 8) >> 4), 0, 255).  Exact to the bit (tests/multiband_oracle.py restates it in numpy).
 *      alpha == NULL: out = B.  Otherwise alpha is f32 [H, W] (fie_mask_prep's mask_px) and out = source where alpha <= 0, B where alpha >= 1,
 *      rint(alpha B + (1 - alpha) source) between, in f32 without fused multiply-adds.
 *      workspace: fie_multiband_workspace_bytes(H, W, levels) bytes (-1 for what the op refuses), 16-byte aligned: levels 1 .. L of D, G and C;
 *      level 0 is recomputed from the images.  Every byte the op reads from it, it has written before.
 *      Launches: 2 L (8 at L = 4) -- one reduce per level (three difference channels and the mask in one pass), one collapse per level from the
 *      top down, the last over the image.  Asynchronous on the ctx stream; no block waits for another, no atomics. */
int64_t fie_multiband_workspace_bytes(int H, int W, int levels);
int fie_multiband_blend_rgb_u8(fie_ctx* ctx, const uint8_t* edit, const uint8_t* source, const uint8_t* mask_l, const float* alpha, int H,
                               int W, int levels, void* workspace, uint8_t* out);

/* ---- Growing or shrinking an edit mask by an exact Euclidean disk: in front of everything else that reads the mask.
 *   fie_mask_grow_u8   mask_l u8 [H, W], any H, W >= 1 with H * W < 2^31 (a source-size mask of 12 MP and more; the 2^24 of the fill and the blend
 *      is an edit-size bound and does not apply), radius in -64 .. 64.  out u8 [H, W], every byte written, 0 or 255; it overlaps no byte of mask_l
 *      (blocks read each other's halo).  With m(q) = (mask_l(q) >= 128), R = |radius| and p, q pixels of the H x W mask only:
 *        radius > 0   out(p) = 255 iff some q has m(q) and (px - qx)^2 + (py - qy)^2 <= R^2: nothing grows in from outside the image;
 *        radius < 0   out(p) = 255 iff m(q) for every q with (px - qx)^2 + (py - qy)^2 <= R^2: the image border does not erode a mask that
 *                     touches it; grow(m, -k) = ~grow(~m, k);
 *        radius == 0  out = 255 m, the binarised mask.
 *      Integer comparisons only, exact (tests/mask_grow_oracle.py restates it in numpy).  FIE_EINVAL for anything else, NULL operands included.
 *      One launch of one block per 64 x 64 tile: the tile's binary pixels and an R-halo in LDS ((64 + 2R)^2 + R + 1 bytes), a column scan for the
 *      distance to the nearest set pixel of each column, a row pass against floor(sqrt(R^2 - dx^2)).  Asynchronous on the ctx stream; no
 *      workspace, no atomics, no block waits for another. */
int fie_mask_grow_u8(fie_ctx* ctx, const uint8_t* mask_l, int H, int W, int radius, uint8_t* out);

/* ---- Soft masks: the mask's grey level as a per-pixel strength.  A level map V is u8, 0 = never edited, 255 = edited as
 * a binary mask's white; its support S = 255 (V > 0) is what every other reader of a mask takes in the mask's place.
 *   fie_lcm_step_levels[_f32]   fie_lcm_step_masked with lvl_lat u8 [H*W] (latent pixels, levels 0 .. 255) in place of mask_lat and the step's place:
 *      steps = K in 1 .. 255, the number of steps of the edit, and step = j in 0 .. K - 1.  After step j a latent pixel of level v is inside
 *      iff v K > 255 (K - 1 - j): it is edited for the last (v K + 254) / 255 of the K steps -- 0 for v = 0, 1 for v = 1, K for v = 255.  An
 *      inside pixel keeps the bits fie_lcm_step writes, an outside one takes what fie_lcm_step_masked gives it.  fie_lcm_step_masked is the
 *      case of levels 0 / 1 with K = 1, j = 0; a 0 / 255 map is the binary masked edit at every K.
 *   fie_mask_levels_u8   levels_e u8 [H, W] (the level map at the edit size), mask_lat u8 [H/8 * W/8] (fie_mask_prep's, of the support); H, W
 *      positive multiples of 8.  lvl_lat[y][x] = mask_lat[y][x] ? max(levels_e[8y][8x], 1) : 0: the latent support is mask_lat's bit for bit.
 *      One launch.
 *   fie_mask_support_u8  levels u8 [n], n >= 1 -> out u8 [n] = 255 where levels > 0, else 0 (out may be levels).  One launch.
 *   fie_mask_ramp_u8     a level map from a binary mask's outline.  mask_l u8 [H, W], any H, W >= 1 with H * W < 2^31, radius r in 1 .. 64;
 *      out_levels u8 [H, W], every byte written; it overlaps no byte of mask_l (blocks read each other's halo).  With m(q) = (mask_l(q) >= 128)
 *      and D2(p) the smallest (px - qx)^2 + (py - qy)^2 over the pixels q of the image with !m(q):
 *        out(p) = 0 where !m(p); 255 where no such q lies within distance < r (a mask of all ones included);
 *        else isqrt(65025 D2(p)) / r = floor(255 sqrt(D2(p)) / r).
 *      The image border is not an edge (fie_mask_grow_u8's rule for the erosion); every set pixel gets at least 255 / r >= 3, so the map's support
 *      is the binarised mask.  Integers only, exact (fie_amd/mask.py: ramp_numpy restates it).  FIE_EINVAL for anything else.  One launch of one
 *      block per 64 x 64 tile, staged and scanned as fie_mask_grow_u8's ((64 + 2r)^2 bytes of LDS); the row pass takes the minimum of
 *      g^2 + dx^2 over the column distances g.  Asynchronous on the ctx stream; no workspace, no atomics, no block waits for another. */
int fie_lcm_step_levels(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents,
                        const float* noise, int64_t HW, float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out,
                        float sqrt_ab_prev, float sqrt_1mab_prev, void* model_in, int copies, float inv_scaling,
                        void* decode_in, const uint8_t* lvl_lat, const float* z0, const float* noise_init, int steps, int step);
int fie_lcm_step_levels_f32(fie_ctx* ctx, const void* eps, int64_t ld_eps, int nb, float guidance, float* latents,
                            const float* noise, int64_t HW, float sqrt_ab_t, float sqrt_1mab_t, float c_skip, float c_out,
                            float sqrt_ab_prev, float sqrt_1mab_prev, void* model_in, int copies, float inv_scaling,
                            void* decode_in, const uint8_t* lvl_lat, const float* z0, const float* noise_init, int steps, int step);
int fie_mask_levels_u8(fie_ctx* ctx, const uint8_t* levels_e, const uint8_t* mask_lat, int H, int W, uint8_t* lvl_lat);
int fie_mask_support_u8(fie_ctx* ctx, const uint8_t* levels, int64_t n, uint8_t* out);
int fie_mask_ramp_u8(fie_ctx* ctx, const uint8_t* mask_l, int H, int W, int radius, uint8_t* out_levels);

/* ---- The canvas of an outpainting edit: the source made larger by four margins, and the mask that selects what is new.
 *   fie_outpaint_canvas_rgb_u8   src u8 [H, W, 3], mask_l u8 [H, W] or NULL, H, W >= 1; left, top, right, bottom in 0 .. 4096, not all 0.  With
 *      Hc = top + H + bottom, Wc = left + W + right and Hc * Wc < 2^31:
 *        canvas      u8 [Hc, Wc, 3]   canvas(y, x) = src(clamp(y - top, 0, H - 1), clamp(x - left, 0, W - 1)): the source's bytes inside the source
 *                                     rectangle, its nearest edge pixel outside (a replicate, not zeros: the VAE encoder's receptive field mixes the
 *                                     border into the latents next to the seam);
 *        canvas_mask u8 [Hc, Wc]      255 outside the source rectangle; inside it mask_l(y - top, x - left) as passed, greys included, or 0 when
 *                                     mask_l is NULL.
 *      Every byte of both outputs is written; no output overlaps an operand or the other output.  FIE_EINVAL for anything else, NULL src / canvas /
 *      canvas_mask included.  Exact (tests/outpaint_oracle.py restates it in numpy).  One launch at any size: both outputs are stored as aligned
 *      dwords with the 0 .. 3 bytes in front of and behind them in each row stored as bytes (rows of 3 Wc and Wc bytes start at any address); over the
 *      source rectangle the operands are read as aligned dwords too, by bytes elsewhere; no access is misaligned, none leaves its tensor; 64-bit
 *      indexing.  Asynchronous on the ctx stream; no workspace, no atomics, no block waits for another. */
int fie_outpaint_canvas_rgb_u8(fie_ctx* ctx, const uint8_t* src, const uint8_t* mask_l, int H, int W, int left, int top, int right, int bottom,
                               uint8_t* canvas, uint8_t* canvas_mask);

/* ---- Tiled edits: ny x nx overlapping tiles of one size blended into one H x W image.
 *   tiles u8 [ny * nx, th, tw, 3]: tile j = iy * nx + ix (row-major) lies at (xs[ix], ys[iy]).  xs [nx], ys [ny]: HOST arrays (they travel as kernel
 *   arguments); nx, ny in 1 .. 32.  th, tw, H, W: any values >= 1, H * W < 2^31.  Per axis the positions start at 0, increase strictly, leave no gap
 *   (p[i + 1] <= p[i] + t) and end at S - t.  out u8 [H, W, 3], at any address, overlapping nothing of tiles.
 *   With w(u) = min(t if the tile is the first of its axis else u + 1, t if it is the last else t - u) -- the distance to the tile's nearest INTERIOR
 *   edge: the image border fades nothing --, W_j = wy(y - ys[iy]) * wx(x - xs[ix]) and S = sum_j W_j over the tiles that cover (y, x):
 *       out(y, x, c) = (sum_j W_j * tile_j(y - ys[iy], x - xs[ix], c) + (S >> 1)) / S
 *   a linear crossfade over each overlap, exact in integers (fie_amd/tiles.py: blend_numpy restates it): where one tile covers a pixel the output is
 *   that tile's byte, the blend of a source's own crops is the source, the output lies between the covering tiles' minimum and maximum.
 *   FIE_EINVAL for anything else, NULL pointers included.  One launch at any size: a gather, no atomics, no f32, no workspace; 32-bit accumulators where
 *   the geometry bounds the numerator below 2^32 (every plan of fie_amd/tiles.py), 64-bit ones otherwise; the output is stored as aligned dwords with
 *   the 0 .. 3 bytes in front of and behind them in each row stored as bytes, the tiles are read as aligned dwords wherever those lie inside them; no
 *   access is misaligned, none leaves its tensor.  Asynchronous on the ctx stream. */
int fie_tile_blend_rgb_u8(fie_ctx* ctx, const uint8_t* tiles, int nx, int ny, const int* xs, const int* ys, int th, int tw, int H, int W, uint8_t* out);

/* ---- Full-resolution back end of an edit: the edit-size result at the source's size, composited against the
 * source's own bytes.  res: u8 [h, w, 3], the edit-size result.  The output is H x W: up = Pillow's 8-bit LANCZOS resize of res to
 * (W, H), bit-exact (kx / bx / ksx, ky / by / ksy: the tables of fie_resize_rgb_u8 for w -> W and h -> H; a table is NULL on an axis
 * that keeps its size).  mask_l == NULL: dst = up.  Otherwise mask_l is u8 H x W (white = edit, rows mask_pitch bytes apart) and, with
 * M = (mask_l >= 128) feathered as fie_mask_prep feathers it (taps: f32 [2 * radius + 1], radius <= 64; {1.0f} with radius 0; same
 * passes, same summation order, clamp-to-edge at the borders of the H x W image), dst = source where M <= 0, up where M >= 1,
 * rint(M up + (1 - M) source) between.  source, dst: u8 H x W x 3 with rows source_pitch / dst_pitch bytes apart (>= 3 W; any value,
 * any base alignment): a caller composites a region in place inside a larger image by pointing both at the region's first pixel
 * with the image's pitch -- no byte outside the H x W x 3 region is read or written, and dst may be source.  tmp: u8 [h, W, 3]
 * scratch, needed when w != W.  Two launches (one when w == W), asynchronous on the ctx stream: the horizontal resample into tmp, then
 * one kernel per 64 x 16 output tile that stages the binary mask and its halo in LDS, feathers it, resamples its columns of tmp
 * vertically, blends and stores.  No H x W f32 mask and no H x W resized image is written to memory; a tile whose mask, halo included,
 * is all zero copies the source bytes. */
int fie_fullres_paste_rgb_u8(fie_ctx* ctx, const uint8_t* res, int h, int w, const uint8_t* source, int64_t source_pitch,
                             const uint8_t* mask_l, int64_t mask_pitch, int H, int W, const int* kx, const int* bx, int ksx,
                             const int* ky, const int* by, int ksy, const float* taps, int radius, uint8_t* dst, int64_t dst_pitch,
                             uint8_t* tmp);

/* ---- Edit metrics on the device: SSE and SSIM of n pairs of u8 images in one pass.
 *   a, b: u8 [n, H, W, 3] (H, W >= 11: the 11-tap window's reflect padding); mask: NULL, or u8 [n, H, W] with non-zero = edited region.
 *   result: n rows of four 8-byte fields (8-byte aligned), written by the device:
 *       [0] uint64 sse          sum over pixels and channels of (a - b)^2 on the u8 values, exact
 *       [1] double ssim_sum     sum of the SSIM map over the channels and the (H - 10) x (W - 10) positions whose 11x11 window lies inside
 *                               the image (oracle/metrics.py: the reflect-padded border is cropped from the map again); Gaussian sigma 1.5,
 *                               images / 255, c1 = 1e-4, c2 = 9e-4; fp32 moments, summed in fp64
 *       [2] uint64 bg_sse       } the same two for the BACKGROUND pair: both images with every pixel of the edited region set to 0
 *       [3] double bg_ssim_sum  } in all channels first, sums over the same (H - 10) x (W - 10) positions; both 0 when mask is NULL
 *   MSE = sse / (255^2 * 3HW), PSNR = 10 log10(1 / MSE), SSIM = ssim_sum / (3 (H - 10) (W - 10)) are the host's to form (in double: no device rounding
 *   in MSE / PSNR at all).  workspace: fie_metrics_workspace_bytes(n, H, W) bytes (-1 for sizes the op refuses), 8-byte aligned; one
 *   partial per 32x32 tile.  Two launches, asynchronous on the ctx stream, never synchronises.  Deterministic: no atomics, partials are
 *   added in tile order, so a pair's row has the same bits in every run and at every position of every batch. */
int64_t fie_metrics_workspace_bytes(int n, int H, int W);
int fie_metrics_pairs_u8(fie_ctx* ctx, const uint8_t* a, const uint8_t* b, const uint8_t* mask, int n, int H, int W, void* result,
                         void* workspace, int64_t workspace_bytes);

/* ---- CLIP score on the device: the pieces around the ViT image tower, which itself runs on fie_gemm_* / fie_layernorm_* /
 * fie_attention_f16.  All asynchronous on the ctx stream, none synchronises, none uses atomics.
 *   fie_clip_mask_rgb_u8     the "edited" variant of n u8 [H, W, 3] images: pixels outside the edited region set to 0.  mask: u8 [n, MH, MW], L >= 128 =
 *                            edited; when (MH, MW) != (H, W) it is sampled through ytab int32 [H] / xtab int32 [W], the source indices of Pillow's
 *                            NEAREST resize (fie_amd/resize.py: nearest_indices; a table may be NULL when that axis keeps its size).  dst may be src.
 *   fie_clip_patches_u8_*    src: u8 [n, H, W, 3], the images after the processor's resize.  Crops size x size at (top, left), x / 255, (x - mean[c]) /
 *                            std[c] (mean, std: 3 HOST floats each) and writes the patch rows [n * (size / patch)^2, 3 patch^2], k = (c patch + py) patch
 *                            + px: the K order of the patch-embedding weight [C, 3, patch, patch] viewed as a matrix.  patch % 8 == 0; out 16-byte aligned.
 *                            f32: every value is the fp32 expression above; f16: its round-to-nearest-even.
 *   fie_vit_embed_*          out [n, 1 + P, C]: row 0 = cls + pos[0], row 1 + i = patches[n, i] + pos[1 + i] (patches [n * P, C]: the patch GEMM's
 *                            output; cls [C]; pos [1 + P, C]).  C % 8 == 0, operands 16-byte aligned.
 *   fie_clip_score_*         img, txt: [n, P] embeddings (row strides ld_img / ld_txt in elements); out f32 [n, 2] = (100 cos, max(100 cos, 0)).  One wave per
 *                            pair, fp32 sums in a fixed order: a pair's bits depend neither on n nor on its position.  A zero norm gives 0. */
int fie_clip_mask_rgb_u8(fie_ctx* ctx, const uint8_t* src, const uint8_t* mask, int n, int H, int W, int MH, int MW, const int* ytab, const int* xtab,
                         uint8_t* dst);
int fie_clip_patches_u8_f16(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int top, int left, int size, int patch, const float* mean,
                            const float* std, void* out);
int fie_clip_patches_u8_f32(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int top, int left, int size, int patch, const float* mean,
                            const float* std, void* out);
int fie_vit_embed_f16(fie_ctx* ctx, const void* patches, const void* cls, const void* pos, int n, int P, int C, void* out);
int fie_vit_embed_f32(fie_ctx* ctx, const void* patches, const void* cls, const void* pos, int n, int P, int C, void* out);
int fie_clip_score_f16(fie_ctx* ctx, const void* img, int64_t ld_img, const void* txt, int64_t ld_txt, int n, int P, float* out);
int fie_clip_score_f32(fie_ctx* ctx, const void* img, int64_t ld_img, const void* txt, int64_t ld_txt, int n, int P, float* out);

/* ---- DINO structure distance on the device: the pieces around the ViT tower, which itself runs on fie_gemm_* / fie_layernorm_* /
 * fie_attention_f16 and fie_vit_embed_*.  All asynchronous on the ctx stream, none synchronises, none uses atomics.
 *   fie_dino_patches_u8_*    src: u8 [n, H, W, 3].  x / 255, then torch's `interpolate(mode="bilinear", antialias=True, align_corners=False)` to OH x OW
 *                            in fp32 -- the horizontal pass first, into tmp (f32 [n, H, OW, 3], the caller's scratch), then the vertical one --, (x -
 *                            mean[c]) / std[c] (3 HOST floats each) and the patch rows [n * (OH / patch) * (OW / patch), 3 patch^2] in the K order of
 *                            fie_clip_patches_u8_*.  wx f32 [OW, ksx] / bx int32 [OW, 2] = (first input index, tap count) and wy / by / ksy likewise:
 *                            DEVICE tables of the antialias triangle filter (fie_amd/resize.py: aa_coefficients); input indices are clamped to the image.
 *                            patch % 8 == 0 and divides OH and OW; out 16-byte aligned.  f16: the round-to-nearest-even of the f32 value.  Two launches.
 *   fie_selfsim_mse_*        keys_a, keys_b: [n, T, C] key matrices of n pairs, row stride ld elements (ld >= C: a column range of a fused qkv output),
 *                            rows 16-byte aligned; C % 32 == 0 (f16) / C % 16 == 0 (f32).  out: double [n] = mean over the T x T entries of
 *                            (S_b - S_a)^2, S = K K^T / max(|k_i| |k_j|, 1e-8) (the PRODUCT of the norms is clamped: a zero row gives S = 0).  Both Gram
 *                            tiles of a 64 x 64 tile come from MFMA with fp32 accumulators and never reach memory; only tiles on and above the
 *                            diagonal are computed, the latter counted twice.  Row norms: fp32, one wave per row.  workspace:
 *                            fie_selfsim_workspace_bytes(n, T) bytes (-1 for shapes the op refuses), 8-byte aligned: one fp64 partial per tile, then the
 *                            norms.  Three launches.  Deterministic: partials are added in tile order in fp64, so a pair's bits depend neither on n nor on
 *                            its position, and an identical pair gives exactly 0. */
int fie_dino_patches_u8_f16(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int OH, int OW, const float* wx, const int* bx, int ksx,
                            const float* wy, const int* by, int ksy, int patch, const float* mean, const float* std, float* tmp, void* out);
int fie_dino_patches_u8_f32(fie_ctx* ctx, const uint8_t* src, int n, int H, int W, int OH, int OW, const float* wx, const int* bx, int ksx,
                            const float* wy, const int* by, int ksy, int patch, const float* mean, const float* std, float* tmp, void* out);
int64_t fie_selfsim_workspace_bytes(int n, int T);
int fie_selfsim_mse_f16(fie_ctx* ctx, const void* keys_a, const void* keys_b, int64_t ld, int n, int T, int C, void* workspace, double* out);
int fie_selfsim_mse_f32(fie_ctx* ctx, const void* keys_a, const void* keys_b, int64_t ld, int n, int T, int C, void* workspace, double* out);

/* ---- LPIPS (SqueezeNet 1.1) on the device: what stands around the Fire modules, which run on fie_gemm_f32 / fie_conv3x3_nhwc_f32
 * with FIE_ACT_RELU.  fp32 only, in every context.  All asynchronous on the ctx stream, none synchronises, none uses atomics.
 *   fie_lpips_stem_u8_f32    src: u8 [n, H, W, 3]; mask: NULL or u8 [n, H, W], a pixel with a non-zero byte counts as bytes (0, 0, 0).  lut f32 [3][256]:
 *                            byte -> scaled input per channel (fie_amd/lpips.py: input_lut); w f32 [27][64], k = (ky * 3 + kx) * 3 + ci; bias f32 [64].
 *                            out f32 [n, OH, OW, 64] = relu(conv k3 stride 2 without padding), OH = (H - 3) / 2 + 1, OW likewise.  H, W >= 3; out, w,
 *                            bias 16-byte aligned.  One launch.
 *   fie_maxpool3s2_nhwc_f32  x f32 [n, H, W, C] -> y f32 [n, OH, OW, C], MaxPool2d(3, stride 2, ceil_mode=True): OH = ceil((H - 3) / 2) + 1, windows
 *                            clipped at the far edge, bit-equal to ATen's.  H, W >= 2, C % 4 == 0, 16-byte aligned.  One launch.
 *   fie_lpips_layer_f32      fa, fb f32 [P, HW, C] contiguous: one tap of P pairs.  out[p * ld_out] = mean over the HW pixels of
 *                            sum_c w[c] (fa / sqrt(1e-8 + sum_c fa^2) - fb / sqrt(1e-8 + sum_c fb^2))^2 as a double.  C % 64 == 0, C <= 512; P <= 65535.
 *                            workspace: fie_lpips_layer_workspace_bytes(P, HW) bytes (-1 for shapes the op refuses), 8-byte aligned: one fp64
 *                            partial per block of 64 pixels.  Two launches.  Deterministic: a pair's bits depend neither on P nor on its position, an
 *                            identical pair gives exactly 0, an all-zero pixel contributes 0. */
int fie_lpips_stem_u8_f32(fie_ctx* ctx, const uint8_t* src, const uint8_t* mask, int n, int H, int W, const float* lut, const float* w, const float* bias,
                          float* out);
int fie_maxpool3s2_nhwc_f32(fie_ctx* ctx, const float* x, int n, int H, int W, int C, float* y);
int64_t fie_lpips_layer_workspace_bytes(int P, int HW);
int fie_lpips_layer_f32(fie_ctx* ctx, const float* fa, const float* fb, int P, int HW, int C, const float* w, void* workspace, double* out, int64_t ld_out);

/* ---- Strength sweeps: the winner among k finished variants of one edit, picked and copied on the device.
 *   imgs: a HOST array of k device pointers (they travel as kernel arguments: no pointer table in memory), 1 <= k <= 16, each to `bytes` bytes of
 *   u8 at ANY address, 1 <= bytes <= 2^31; variants come strongest first.  rows: the k result rows of fie_metrics_pairs_u8 on the device.
 *   clip_or_null: f32 [k, 2] on the device, the rows of fie_clip_score_* (the score is column 1); needed by rule 1 only.
 *   With sums[i] = the double in field 1 of row i (ssim_sum), or field 3 (bg_ssim_sum) when bg == 1, and ok[i] = sums[i] >= floor (`floor` is in
 *   the same raw units: min SSIM * 3 (H - 10) (W - 10), or -inf; a NaN never passes):
 *       nobody passes   the index of the largest non-NaN sums[i], ties to the larger index; k - 1 when all are NaN
 *       rule 0          the smallest passing index ("strongest": the most editing the preservation budget allows)
 *       rule 1          the passing index with the largest clip[i][1], ties to the larger index (the weaker edit); a NaN score never wins; when
 *                       all are NaN the largest passing index
 *   float64 and float32 compares only (fie_amd/sweep.py: select_numpy restates it).  out_img: `bytes` bytes at any address, overlapping no
 *   image; receives imgs[winner].  out_idx: one int32 on the device; receives the winner.  Nothing else is written.  FIE_EINVAL ("bad argument")
 *   for anything else, NULL pointers included.  One launch, asynchronous on the ctx stream: every block evaluates the rule for itself and copies
 *   its share -- aligned 16-byte stores, 16-byte loads where the source is congruent to the output mod 16 and aligned dwords otherwise, the up to
 *   15 bytes in front of and behind them by bytes.  No atomics, no workspace, no block waits for another. */
int fie_sweep_select_u8(fie_ctx* ctx, const void* const* imgs, int k, int64_t bytes, const int64_t* rows, const float* clip_or_null, int rule,
                        double floor, int bg, void* out_img, int32_t* out_idx);

/* ---- Prompt emphasis: the text's cross-attention V rows scaled by one weight per text row, in front of the denoising loop.
 *   A weight behind the softmax, out = sum_j p_j w_j v_j, is cross-attention on a V whose row j is scaled by w_j; the text's K | V is projected once
 *   per image and net, so the whole control is this one launch on that result.
 *   X: row-major [rows, ld], f16 (f32 = 0) or f32 (f32 = 1), 16-byte aligned, ld % 8 == 0, ld >= ncols; ncols % 8 == 0 (so every block's c % 8 == 0).
 *   w: f32 [rows] ON THE DEVICE (a graph replay reads the weights of the job it replays).  vflags: u8 [ncols / 8] on the device, non-zero where the
 *   8 columns [8 g, 8 g + 8) are V columns.  For every row r with w[r] != 1 and every flagged g:
 *       X[r, 8 g + e] = round(f32(X[r, 8 g + e]) * w[r])        one fp32 multiply; f16: one rounding to nearest even (beyond 65504: an infinity)
 *   A row with w[r] == 1.0f is neither read nor written; unflagged columns, the columns ncols .. ld and everything outside X keep their bits.
 *   fie_amd/emphasis.py: kv_emphasis_numpy restates it to the bit.  FIE_EINVAL for anything else.  One launch, 16-byte accesses, no atomics, no
 *   workspace, no block waits for another. */
int fie_kv_emphasis(fie_ctx* ctx, void* X, int64_t ld, int64_t rows, int64_t ncols, const float* w, const uint8_t* vflags, int f32);

/* ---- Control weights: the ControlNet's residuals weighed per latent position, so that a mask can let go of the edge map.
 *   fie_control_pyramid_u8   e u8 [H, W] on the device, 8-byte aligned: the edit-ness of every edit-size pixel -- binary = 1: an L mask, read as
 *      255 (e >= 128); binary = 0: a level map, read as it is.  H, W multiples of 8 in 8 .. 2048; levels in 1 .. 3; a in 0 .. 255.
 *      Level l has h_l x w_l positions, h_0 = H / 8, h_{l+1} = ceil(h_l / 2) (w alike), and blocks of side s = 8 * 2^l pixels clipped at the image:
 *      E = the integer sum of e over the block, cnt = its pixels,
 *          out[off_l + y w_l + x] = (float)(255 cnt 256 - (256 - a) E) / (float)(255 cnt 256)      off_l = sum of h_k w_k over k < l
 *      one IEEE f32 division of two int32 converted to f32.  out: f32 [sum h_l w_l], every element written.  One launch, integer sums in a fixed
 *      order, no atomics, no workspace.  fie_amd/control.py: weights_numpy(pyramid_numpy(...)) restates it to the byte.
 *   fie_control_add   all residuals of one evaluation in ONE launch.  The table (read on the host when the call is issued, passed to the kernel
 *      by value) holds `count` in 1 .. 16 segments: u, t, out row-major [rows, C] f16 (f32 = 0) or f32 (f32 = 1), contiguous, 16-byte aligned, out
 *      a tensor of its own; C % 8 == 0; rows = B * P: B batch rows of P latent positions; woff: where the segment's level starts in the weights;
 *      s: its scale.  w: f32 [images, p_tot] ON THE DEVICE (a graph replay reads the weights of the job it replays); batch row b belongs to image
 *      b / rows_per_image.  For every element of row r = b P + p:
 *          c = s * w[(b / rows_per_image) p_tot + woff + p]                f32
 *          out = c == 0 ? u : round(f32(u) + c * f32(t))                   product and sum rounded separately; f16: one conversion, nearest even
 *      Where c == 0, out holds u's bits and t is not read.  The caller keeps b / rows_per_image below the images of w.  fie_amd/control.py:
 *      add_numpy restates it to the bit.  One launch, 16-byte accesses, one writer per element, no atomics, no workspace.
 *   FIE_EINVAL for anything else, before any launch. */
#define FIE_CONTROL_MAX_SEGMENTS 16
#define FIE_CONTROL_MAX_LEVELS 3
typedef struct fie_control_table {
    int count;
    int C[16], P[16], woff[16];
    int64_t rows[16];
    float s[16];
    const void* u[16];
    const void* t[16];
    void* out[16];
} fie_control_table;
int fie_control_pyramid_u8(fie_ctx* ctx, const uint8_t* e, int H, int W, int levels, int a, int binary, float* out);
int fie_control_add(fie_ctx* ctx, const fie_control_table* table, const float* w, int64_t p_tot, int rows_per_image, int f32);

#ifdef __cplusplus
}
#endif
#endif /* FIE_H_ */
