"""`FastEditor` -- drop-in replacement for /root/reference/src/pipeline.py:17-293 on MI355X.

Same constructor, `MODEL_CONFIGS`, `edit()` / `preprocess_image()` / `clear_memory()` / `get_memory_usage()`
signatures, defaults, attributes and error behaviour; `self.pipe` is an `fie_amd.pipe.HipImg2ImgPipeline`
(hand-written HIP kernels behind a C ABI) instead of the diffusers pipeline.  There is no CPU fallback: a missing
HIP library or GPU raises.  Additive: `set_in_flight(n)` / `worker_slot(i)` (several edits in flight from worker threads), and keyword-only knobs: `weights_dir`, `seed_weights`, `noise_dtype`, `weight_dtype` ("f8e4m3": fp8 UNet / ControlNet weights, BASELINE config 5), `broadcast_weights`
(under torch.distributed with world_size > 1, rank 0's synthetic weights are broadcast over RCCL instead of regenerated), `clip_score_dir` (a local
transformers CLIPModel directory: `edit(..., metrics=True)` then also returns the CLIP score of the edit), `dino_dir` (a local
transformers ViTModel directory: `edit(..., metrics=True)` then also returns the DINO structure distance of the edit),
`lpips_dir` (a local directory with the LPIPS SqueezeNet weights: `edit(..., metrics=True)` then also returns the LPIPS of the edit, DESIGN.md
section 19), and `edit_sweep(...)`: edit() at several strengths as one device job, scored on the device, the winner picked there (DESIGN.md
section 20).
"""
import os
import threading

import numpy as np
import torch
from PIL import Image

import fie_amd  # noqa: F401  (alias loader for the hyphenated package directory)
from fie_amd import buckets, hip, stack
from fie_amd import canny_auto as hcanny
from fie_amd import mask as hmask
from fie_amd import metrics as hmetrics
from fie_amd import region as hregion
from fie_amd import tiles as htiles
from fie_amd.pipe import DeviceOutput, HipImg2ImgPipeline, MaskLevels


class FastEditor:
    """SDXL / SSD-1B + Canny ControlNet + LCM few-step image editor."""

    # reference: src/pipeline.py:30-43
    MODEL_CONFIGS = {
        "sdxl": {
            "base_model": "stabilityai/stable-diffusion-xl-base-1.0",
            "lcm_lora": "latent-consistency/lcm-lora-sdxl",
            "use_full_lcm": False,
            "description": "Full SDXL (highest quality, ~6GB VRAM)",
        },
        "ssd-1b": {
            "base_model": "segmind/SSD-1B",
            "lcm_model": "latent-consistency/lcm-ssd-1b",
            "use_full_lcm": True,
            "description": "SSD-1B distilled (50% smaller, 60% faster, ~4GB VRAM)",
        },
    }
    _EXTRA_STACKS = ("tiny", "tiny-nomid")      # test-only topologies (not advertised in MODEL_CONFIGS)

    def __init__(self, model_name="sdxl", device="cuda", dtype=torch.float16, enable_cpu_offload=True,
                 use_full_precision=False, use_full_controlnet=False, *, weights_dir=None, seed_weights=1234,
                 noise_dtype=None, broadcast_weights=True, weight_dtype="f16", clip_score_dir=None, dino_dir=None, dino_layer=11,
                 lpips_dir=None, canny_density=None, prompt_emphasis=None, control_weights=None):
        if model_name not in self.MODEL_CONFIGS and model_name not in self._EXTRA_STACKS:
            raise ValueError(f"Unknown model: {model_name}. Choose from {list(self.MODEL_CONFIGS.keys())}")
        # [additive] set_control_weights() from the start: a dict of its keywords; FIE_CONTROL_WEIGHTS ("layers=prompt;steps=0:0.5;in_mask=0") serves run_batch.py
        from fie_amd import control as hctl
        if control_weights is None and os.environ.get("FIE_CONTROL_WEIGHTS"):
            try:
                control_weights = hctl.parse_env(os.environ["FIE_CONTROL_WEIGHTS"])
            except ValueError as e:
                raise ValueError(f"FIE_CONTROL_WEIGHTS: {e}") from None
        if control_weights is not None and not (isinstance(control_weights, dict) and set(control_weights) <= {"layers", "steps", "in_mask"}):
            raise ValueError(f"control_weights={control_weights!r}: None, or a dict of set_control_weights()'s keywords layers, steps, in_mask")
        cn_cfg = stack.stack_configs(model_name, use_full_controlnet)["controlnet"]
        self._ctl_n_out = 2 + sum(cn_cfg["layers_per_block"] + (i != len(cn_cfg["block_out_channels"]) - 1) for i in range(len(cn_cfg["block_out_channels"])))
        self.set_control_weights(**(control_weights or {}))
        if canny_density is None and os.environ.get("FIE_CANNY_DENSITY"):     # [additive] set_canny_density() from the start; the switch serves run_batch.py
            try:
                canny_density = float(os.environ["FIE_CANNY_DENSITY"])
            except ValueError:
                raise ValueError(f"FIE_CANNY_DENSITY={os.environ['FIE_CANNY_DENSITY']!r}: a number in [0.001, 0.25]") from None
        self.set_canny_density(canny_density)
        if prompt_emphasis is None and os.environ.get("FIE_PROMPT_EMPHASIS"):  # [additive] set_prompt_emphasis() from the start; the switch serves run_batch.py
            try:
                prompt_emphasis = float(os.environ["FIE_PROMPT_EMPHASIS"])
            except ValueError:
                raise ValueError(f"FIE_PROMPT_EMPHASIS={os.environ['FIE_PROMPT_EMPHASIS']!r}: a number in [0, 8]") from None
        self.set_prompt_emphasis(prompt_emphasis)
        self.model_name = model_name
        self.device = device
        self.dtype = torch.float32 if use_full_precision else dtype
        self.enable_cpu_offload = enable_cpu_offload
        self.use_full_controlnet = use_full_controlnet
        self.config = self.MODEL_CONFIGS.get(model_name, {"description": f"{model_name} (test stack)"})
        log = lambda m: print(f"[FastEditor] {m}")
        if use_full_precision:
            log("Full precision mode enabled (fp32)")
        log(f"Initializing with {model_name.upper()}")
        log(self.config["description"])
        log(f"Device: {device}, Dtype: {self.dtype}")
        log(f"CPU offload: {'enabled' if enable_cpu_offload else 'disabled'}")
        if not str(device).startswith("cuda"):
            raise RuntimeError(f"device={device!r}: the MI355X build runs the hot path in HIP kernels only "
                               "(the CPU restatement lives in oracle/ and is test infrastructure)")
        if self.dtype not in (torch.float16, torch.float32):
            raise NotImplementedError(f"dtype {self.dtype}: the HIP path is built for float16 and float32")
        dev_index = torch.device(device).index
        if dev_index is None:
            dev_index = torch.cuda.current_device() if torch.cuda.is_available() else 0
        if torch.cuda.is_available():
            torch.cuda.set_device(dev_index)      # the C-ABI launches go to the calling thread's current HIP device
        ctx = hip.context(dev_index, self.dtype)
        weights_dir = weights_dir or os.environ.get("FIE_WEIGHTS_DIR")
        log(f"Loading ControlNet (Canny) - {'FULL SIZE' if use_full_controlnet else 'small variant'}...")
        log("Loading VAE (fp32 for maximum quality)..." if self.dtype == torch.float32 else "Loading VAE (fp16-fix)...")
        toks = None
        if weights_dir:
            log(f"Loading weights from {weights_dir}")
            cfgs, sds, toks = stack.directory_stack(weights_dir, model_name, use_full_controlnet,
                                                         variant="fp16" if self.dtype == torch.float16 else None)
        else:
            log(f"No weights directory given: seeded synthetic weights (seed {seed_weights}) for preset "
                f"{stack.stack_configs(model_name, use_full_controlnet)['unet']['name']}")
            cfgs = sds = None
            if broadcast_weights and torch.distributed.is_available() and torch.distributed.is_initialized() \
                    and torch.distributed.get_world_size() > 1:
                try:      # rank 0 generates, one bucketed RCCL broadcast over xGMI feeds the other ranks
                    cfgs, sds = stack.broadcast_stack(model_name, use_full_controlnet, device=ctx.device, dtype=self.dtype, seed=seed_weights)
                    log("Weights broadcast from rank 0")
                except Exception as e:  # a broken fabric must not take the job down: every rank can regenerate from the seed
                    log(f"weight broadcast failed ({type(e).__name__}: {e}); regenerating locally from the seed")
                    cfgs = sds = None
            if sds is None:
                cfgs, sds = stack.synthetic_stack(model_name, use_full_controlnet, device=ctx.device, dtype=self.dtype, seed=seed_weights)
        self.presets = {k: c["name"] for k, c in cfgs.items()}
        log("Setting LCM scheduler...")
        if weight_dtype != "f16":
            log(f"UNet / ControlNet weights: {weight_dtype} with per-channel scales on the fp8 MFMA (BASELINE config 5)")
        self.weight_dtype = weight_dtype
        self.pipe = HipImg2ImgPipeline(ctx, cfgs, sds, tokenizers=toks, noise_dtype=noise_dtype or self.dtype, weight_dtype=weight_dtype)
        self.pipe.prompt_emphasis = self.prompt_emphasis
        self.controlnet = self.pipe.controlnet
        self._ctl_n_out = self.controlnet.n_out            # the loaded net's own count (a weights directory brings its config)
        self.set_control_weights(**(self.control_weights or {}))
        self._tls = threading.local()          # .slot: graph slot of the calling worker thread (set_in_flight)
        self._fullres_out = {}                 # (slot, image) -> flat u8 buffer on the device, grown to the largest source: the full-resolution back end's output (output_size="source")
        self._tile_bufs = {}                   # (slot, tiles, th, tw) -> u8 [tiles, th, tw, 3] on the device: where the tile results of a tiled edit meet (tiles=...)
        self._metric_rows = {}                 # (slot, images) -> pinned int64 [images, 4]: where an edit's metric rows land (metrics=True)
        self._sweep_out = {}                   # slot -> flat u8 buffer on the device, grown to the largest image: where a sweep's winner lands (edit_sweep(select=...))
        self._sweep_idx = {}                   # slot -> pinned int32 [1]: where a sweep's winning index lands
        self.clip_scorer = None                # fie_amd.clip_score.ClipScorer: only from a directory, never a made-up number
        self._clip_rows = {}                   # (slot, rows) -> pinned f32 [rows, 2]: where an edit's CLIP score rows land
        if clip_score_dir:
            from fie_amd import clip_score as hclip
            log(f"Loading the CLIP score model from {clip_score_dir}")
            self.clip_scorer = hclip.load(clip_score_dir, ctx)
        self.dino_scorer = None                # fie_amd.dino.DinoScorer: only from a directory, never a made-up number
        self._dino_rows = {}                   # (slot, rows) -> pinned f64 [rows]: where an edit's structure distances land
        if dino_dir:
            from fie_amd import dino as hdino
            log(f"Loading the DINO structure distance model from {dino_dir}")
            self.dino_scorer = hdino.load(dino_dir, ctx, layer=dino_layer)
        self.lpips_scorer = None               # fie_amd.lpips.LpipsScorer: only from a directory, never a made-up number
        self._lpips_rows = {}                  # (slot, images, columns) -> pinned f64 [images, columns]: where an edit's LPIPS layer values land
        if lpips_dir:
            from fie_amd import lpips as hlpips
            log(f"Loading the LPIPS model from {lpips_dir}")
            self.lpips_scorer = hlpips.load(lpips_dir, ctx)
        del sds
        log("Enabling memory optimizations...")
        # 288 GB of HBM: offload / slicing flags are accepted and ignored (reference toggles them at :165-179)
        log("  - CPU offload " + ("requested: ignored on MI355X (models stay resident)" if enable_cpu_offload
                                  else "disabled (faster, needs more VRAM)"))
        log("Initialization complete!")

    CANNY_ROUNDS = 4            # hysteresis rounds (of four passes) edit() launches without looking at the flags: weak chains across <= 15 tiles of 32x32

    def _canny_device(self, image, low_threshold, high_threshold, size=None, wait=True, original=None, density=None):
        """PIL -> (u8 HWC source on the device, u8 HWC edge map on the device): gray, Sobel, NMS and hysteresis run in HIP
        kernels (csrc/canny_device.hip), integer exact.  `size` = (width, height): LANCZOS-resize first, as
        `image.resize(size, Image.LANCZOS)` does -- on the device for RGB images, through PIL for any other mode.
        wait=False: returns (source, edge map, finish) with the kernels still in flight (NMS + CANNY_ROUNDS hysteresis rounds); finish()
        -- called once the stream has drained -- returns True when those rounds had NOT reached the fixed point: it has then run the
        remaining ones and rewritten the edge map, and whatever was computed from the map must be computed again.
        `original`: a list that receives the source as uploaded, before the resize (what an inline metric scores against).
        `image` may also be a u8 [H, W, 3] tensor already on the device (an outpainting canvas): it is taken as the upload.
        `density`: None, or the `canny_density` of an edge-budget Canny: the thresholds are picked on the device from the
        image the Canny sees -- behind the resize -- and the two given ones are their ratio; the pair that was used is `ctx.canny_pair` behind a
        waiting call and `finish.pair` once finish() has run."""
        if torch.is_tensor(image):
            src = image
        else:
            if size is not None and image.size != tuple(size) and image.mode != "RGB":
                if original is not None:                # the one case in which the upload below is not the original: score what evaluate.py would
                    original.append(torch.from_numpy(np.array(image.convert("RGB"))).to(self.pipe.ctx.device))
                image = image.resize(size, Image.LANCZOS)
            arr = np.array(image)
            if arr.ndim == 2:
                arr = np.stack([arr] * 3, axis=2)
            src = torch.from_numpy(np.ascontiguousarray(arr[..., :3])).to(self.pipe.ctx.device)
        if original is not None and not original:
            original.append(src)
        if size is not None and (src.shape[1], src.shape[0]) != tuple(size):
            src = self.pipe.ctx.resize_lanczos(src, size[1], size[0])
        ctx = self.pipe.ctx
        budget = None if density is None else hcanny.budget(src.shape[0] * src.shape[1], density)
        if not wait:
            edges, state = ctx.canny_begin(src, low_threshold, high_threshold, rounds=self.CANNY_ROUNDS, budget=budget)

            def finish():
                with self.pipe.eager_lock:                 # the context's stream binding is shared by the threads of in-flight edits
                    ctx.canny_finish(state)
                    if budget is not None:
                        finish.pair = ctx.canny_pair
                    return ctx.canny_more > 0
            return src, edges, finish
        return src, ctx.canny_device(src, low_threshold, high_threshold, budget=budget)

    canny_density = None        # set_canny_density(): None, or the fraction of the pixels that may be strong edge seeds

    def set_canny_density(self, canny_density):
        """[additive] An edge-budget Canny for every later edit(), edit_batch() and edit_sweep() of this editor; None (the
        default) switches it off again.  `canny_density` is a float in [0.001, 0.25]: about that fraction of the pixels may be strong edge seeds,
        and the two thresholds follow per image, on the device -- a hazy photograph whose gradients stay under 200 still gets an edge map, a noisy one
        is not nailed to its noise.  Exactly: with r the gradient magnitude of every pixel that passes the Canny's non-maximum suppression (0
        elsewhere), N the pixels of the image the Canny sees -- behind the resize and the outpaint canvas -- and budget = max(1, N * round(10^6 d) //
        10^6), `high` is the smallest h in 16 .. 2040 with at most budget pixels of r > h and `low` = high * lo // hi, (lo, hi) = the call's
        `canny_low_threshold`, `canny_high_threshold` (swapped when lo > hi; integers >= 0, not both 0: a ValueError of the call otherwise), which
        give only the ratio; the edge map is that of the two.  A call returns what it returns without the setting for `canny_low_threshold=low,
        canny_high_threshold=high` with (low, high) = `canny_thresholds(...)`.  A region takes the statistics of its crop; a tiled edit takes ONE
        pair from the whole source at its own size in front of the first tile job (one read-back of 8 bytes), so that the edge density does not
        jump at a tile seam; edit_batch gives every image its own pair, edit_sweep has one.  With `metrics=True` the dict gains `canny_low` and
        `canny_high`.  Three more launches in front of the job, no additional host wait (except the tiled edit's).  The setting belongs to the
        editor, not to a thread: set it before the worker threads of `set_in_flight` start.  Returns the value it replaces."""
        before, self.canny_density = self.canny_density, hcanny.check_density(canny_density)
        return before

    prompt_emphasis = None      # set_prompt_emphasis(): None, or the weight of the words a prompt marks with [...]

    def set_prompt_emphasis(self, prompt_emphasis):
        """[additive] Prompt emphasis for every later edit(), edit_batch() and edit_sweep() of this editor; None (the default)
        switches it off again: prompts then go to the tokenizers as they are, brackets included.  `prompt_emphasis` is a float in [0, 8].  With it
        set, prompt and negative prompt are read for marks: `[words]` -- how PIE-Bench writes the words an edit changes -- gives its words that
        weight, `(words:1.3)` the written number (at most 8); the marks themselves are stripped before the tokenizers see the prompt, a `[` or `]`
        that belongs to no mark is a ValueError of the call, parentheses in any other form are text.  Every cross-attention of the UNet and the
        ControlNet then multiplies the softmax probability of a weighted token by its weight, without renormalising (Prompt-to-Prompt's
        re-weighting): exactly, the token's row of each block's `attn2.to_v` output is scaled by the weight, once per image and net, in front of the
        denoising loop (one launch per net).  A weight above 1 strengthens a word, below 1 weakens it, 0 removes its value.  A prompt whose
        weights are all 1 -- the setting 1.0, or no marks -- is the stripped prompt under None: the same job, graph and bytes.  The CLIP score
        keeps reading the prompt as passed.  The setting belongs to the editor, not to a thread: set it before the worker threads of `set_in_flight`
        start.  Returns the value it replaces."""
        from fie_amd import emphasis as hemph
        before, self.prompt_emphasis = self.prompt_emphasis, hemph.check(prompt_emphasis)
        if getattr(self, "pipe", None) is not None:
            self.pipe.prompt_emphasis = self.prompt_emphasis
        return before

    control_weights = None      # set_control_weights(): None, or the dict of its three keywords as normalised

    def set_control_weights(self, layers=None, steps=None, in_mask=None):
        """[additive] Control weights for every later edit(), edit_batch() and edit_sweep() of this editor: how much of the
        ControlNet's edge guidance reaches the UNet, per residual, per step and inside the mask.  All three at None (the default) switch it off.
        `layers`: one factor in [0, 2] on top of `controlnet_conditioning_scale` for each of the ControlNet's residuals -- 10 for SDXL / SSD-1B:
        the nine skip tensors, finest first, and the mid block's last -- or a preset: "balanced" (all 1), "prompt" (0.825 ** (9 - i): the front
        ends' "My prompt is more important") or "guess" (10 ** (-1 + i / 9): diffusers' guess_mode ramp).  A factor of 0 skips that zero-conv.
        `steps`: (start, end) in [0, 1], diffusers' control_guidance_start / control_guidance_end over the K loop steps that run after
        `strength`: step k keeps the ControlNet unless k / K < start or (k + 1) / K > end; a dropped step runs no ControlNet kernel at all.  It
        does not combine with edit_sweep (a ValueError there: the variants share their loop steps, the rule counts each variant's own).
        `in_mask`: a number in [0, 1] that scales the residuals inside the mask relative to outside -- 0 lets go of the edge map where the edit
        happens and keeps it everywhere else.  A latent position's weight is 1 - (1 - in_mask) * the mean of the mask over its pixels (a level map's
        greys count as fractions), per resolution level, made on the device from the mask behind `mask_grow` / `mask_ramp`; a call without a
        mask has nothing to weigh and runs as without `in_mask`.  Neutral values -- all layers 1, steps (0, 1), in_mask 1 -- are None: the same
        job, graph and bytes.  fp16, fp32 and fp8-weight editors alike (the zero-convs write fp16 there too); the C-ABI model forwards do not
        read the setting.  No preset, window or `in_mask` value has been tried on real checkpoints.  With `metrics=True` the dict gains
        `control_steps_kept`.  The setting belongs to the editor, not to a thread: set it before the worker threads of `set_in_flight` start.
        Returns the setting it replaces: None, or a dict of the three keywords."""
        from fie_amd import control as hctl
        new = hctl.check(layers, steps, in_mask, self._ctl_n_out)
        before, self.control_weights = self.control_weights, None if new is None else new._asdict()
        if getattr(self, "pipe", None) is not None:
            self.pipe.control_weights = new
        return before

    _ctl_n_out = 10             # the ControlNet's residuals (SDXL / SSD-1B and the test stacks: 9 skips + mid); __init__ reads the model's own

    def _with_control(self, dicts, kw, strength=None):
        """The metric dicts with `control_steps_kept` -- the loop steps of the edit that ran the ControlNet -- while control weights are set.  kw: the
        scalar keywords of the call (_scalars); `strength`: one variant's, for a sweep."""
        ctl = self.control_weights
        if ctl is not None:
            from fie_amd import control as hctl
            steps = len(self.pipe.scheduler.plan(kw["num_inference_steps"], kw["strength"] if strength is None else strength))
            live = any(s != 0 for s in hctl.layer_scales(kw["controlnet_conditioning_scale"], ctl["layers"], self._ctl_n_out))
            for d in dicts:
                d["control_steps_kept"] = sum(hctl.keep(steps, ctl["steps"])) if live else 0
        return dicts

    def last_canny_thresholds(self):
        """[additive] Per image of the calling thread's last edit(), edit_batch() or edit_sweep(): the (low, high) its edge-budget Canny picked, or
        None where the editor had no `canny_density` set.  Costs nothing: the pairs came to the host with the edit's result."""
        return list(getattr(self._tls, "canny_pairs", []))

    def preprocess_image(self, image, low_threshold=100, high_threshold=200, canny_density=None):
        """PIL RGB -> 3-channel PIL Canny edge map (reference :183-210).  [additive] `canny_density`: as edit()'s, on the image as passed."""
        density = hcanny.check(canny_density, low_threshold, high_threshold)
        return Image.fromarray(self._canny_device(image, low_threshold, high_threshold, density=density)[1].cpu().numpy())

    def canny_thresholds(self, image, canny_density, canny_low_threshold=100, canny_high_threshold=200, resolution=None, outpaint=None, mask=None, *,
                         tiles=None):
        """[additive] The (low, high) that `edit(image, ...)` with these arguments hands its Canny after `set_canny_density(canny_density)` (DESIGN.md
        section 22), as two Python ints.  The statistics are taken on the image the Canny sees: the outpaint canvas when there is one, LANCZOS-resized
        to the edit size of `resolution`; with `tiles` (any value but None) the source at its own size, as a tiled edit takes them.  `mask` is
        checked and otherwise unused (the mask's interior counts like the rest).  One upload, the ridge + histogram and select kernels and one
        synchronising read-back of 8 bytes: for tests and tools, not for the hot path."""
        density = hcanny.check(canny_density, canny_low_threshold, canny_high_threshold)
        if density is None:
            raise ValueError("canny_thresholds: canny_density=None: a number in [0.001, 0.25]")
        margins = hmask.check_outpaint(outpaint)
        if tiles is not None and (resolution is not None or margins is not None):
            raise ValueError("canny_thresholds: tiles with resolution or outpaint (a tiled edit takes neither)")
        mask_l = hmask.to_l_array(mask, image.size) if mask is not None else None
        size = None if tiles is not None else buckets.target_size(resolution, hmask.canvas_size(image.size, margins))
        ctx = self.pipe.ctx
        with self.pipe.eager_lock, torch.cuda.stream(self.pipe.slot_stream(getattr(self._tls, "slot", 0))):
            if margins is not None:
                src = self._outpaint_device(image, mask_l, margins)[0]
            else:
                src = torch.from_numpy(np.array(image if image.mode == "RGB" else image.convert("RGB"))).to(ctx.device)
            if size is not None and (src.shape[1], src.shape[0]) != tuple(size):
                src = ctx.resize_lanczos(src, size[1], size[0])
            return ctx.canny_thresholds(src.contiguous(), hcanny.budget(src.shape[0] * src.shape[1], density), canny_low_threshold,
                                        canny_high_threshold)

    def edit(self, image, prompt, negative_prompt="", strength=0.80, num_inference_steps=4, guidance_scale=1.5,
             controlnet_conditioning_scale=0.5, canny_low_threshold=100, canny_high_threshold=200, seed=None, mask=None, mask_blur=0,
             paste_back=True, *, resolution=None, metrics=False, output_size=None, region=None, region_padding=32, masked_content="original",
             blend="alpha", blend_levels=4, mask_grow=0, outpaint=None, tiles=None, tile_overlap=128, tile_batch=4, mask_mode="binary",
             mask_ramp=0):
        """Edit `image` (PIL RGB) following `prompt`, structure preserved through Canny edges (reference :212-274).
        [additive] `mask` (a PIL image or a uint8 / bool [H, W] array of the image's size, white = edit): only that region changes -- the
        latents outside it follow the source's trajectory and, with `paste_back` (default), the output outside it is the resized source byte
        for byte; `mask_blur` r > 0 feathers the paste-back seam with a Gaussian of sigma r.
        [additive] `resolution`: the size the edit runs at and returns -- None / "square" 1024x1024 (the reference's), "auto" the SDXL
        aspect-ratio bucket nearest the source's, or (width, height) (fie_amd/buckets.py).  Source, edge map and mask are
        LANCZOS-resized to it; resizing the result back to the source's size is the caller's choice.
        [additive] `metrics=True`: returns (image, dict) with `ssim`, `psnr`, `mse` of the edit (and `bg_ssim`, `bg_psnr`, `bg_mse` with a mask),
        scored on the device behind the edit: the pair is the ORIGINAL source and the u8 result, each LANCZOS-resized to 512x512 -- what
        evaluate.py would score had the result been saved losslessly.  No additional host wait.  With
        `FastEditor(clip_score_dir=...)` the dict also holds `clip_score` (the result against `prompt`) and, with a mask,
        `clip_score_edited` (the result zeroed outside the edited region).  With `FastEditor(dino_dir=...)` the dict also holds `dino_distance`: the
        structure distance between the ORIGINAL source and the result; None when the source or the result is not square.
        With `FastEditor(lpips_dir=...)` the dict also holds `lpips` (SqueezeNet LPIPS of source and result at 512x512)
        and, with a mask, `bg_lpips` (both images zeroed inside the edited region, as bg_ssim).
        [additive] `output_size`: None / "edit" returns the result at the edit size (above); "source" returns it at the source image's own
        (width, height): the u8 result LANCZOS-resized on the device, bit-exact with `result.resize(image.size, Image.LANCZOS)`, and -- with a mask
        and `paste_back` -- composited THERE against the source as uploaded: the caller's own bytes where the feathered mask is 0, the resized
        result where it is 1, the rounded blend between (csrc/fullres.hip).  `mask_blur` is in pixels of the image the composite
        runs on: the output image here, the edit-size image without `output_size`.  The latent blending is unchanged.  With `metrics=True` the
        scored pair is the original source and this source-size output.
        [additive] `region`: None edits the whole image; "mask" (needs a mask) or an explicit (l, t, r, b) box in source pixels runs the edit on
        that crop of the source alone -- the model sees the region at its native size -- and returns the source-size image with the crop composited
        in: exactly the source converted to RGB with `edit(image.crop(box), prompt, mask=mask.crop(box), output_size="source", ...)` pasted at the
        box's corner.  The box of "mask" is the selection's bounding box grown by `region_padding` pixels and to the target's aspect
        (fie_amd/region.py: mask_box).  A region implies output_size="source" (output_size="edit" with one is a ValueError).  With `metrics=True`
        the scored pair is the region crop and its output, `bg_*` through the crop's mask: outside the region the output IS the source, so
        whole-image numbers would only dilute the edit's by the region's share of the area.
        [additive] `masked_content` (needs a mask): what the model starts from inside the mask.  "original" (default) the source, as ever; "fill"
        the source with the hole replaced by a smooth continuation of its surroundings before the encode (object removal); "latent_noise" pure
        noise; "latent_nothing" the zero latent plus noise.  The three new modes also clear the ControlNet's edge map inside the mask, so the old
        outline is not redrawn.  They act on the edit-size source inside the device job; paste-back, the source-size composite and the metrics
        still use the original source.
        [additive] `blend` (needs a mask and `paste_back`): how the edited region meets the source.  "alpha" (default) the paste-back as ever: one
        ramp (`mask_blur`) for all frequencies.  "multiband" a one-sided multi-band blend over `blend_levels` (1..6, default 4) pyramid levels, run at
        the edit size inside the device job: inside the mask the edit keeps all of its detail while its low-frequency difference to the source
        (brightness, white balance, a slow gradient) fades to nothing towards the seam, over about 2^blend_levels pixels; outside the mask the
        output stays the source's bytes, and `mask_blur`, the source-size composite, regions and the metrics take the blended image in place of
        the decoded one.  A region smaller than about 2^(blend_levels + 2) pixels keeps less of its own low frequencies.
        [additive] `mask_grow` (an integer in -64..64; a non-zero value needs a mask): moves the mask's outline before anything else looks at the
        mask.  r > 0 grows it by the exact Euclidean disk of r pixels (what a tight segmenter mask needs for object removal: the rim and the
        shadow fall inside the hole), r < 0 shrinks it by |r|; pixels of the mask as passed, that is of the source image.  Nothing grows in from
        outside the image and the image border does not erode.  The call returns exactly what it returns for the grown mask passed in: the latent
        mask, the feather, the fill, the blend, the source-size composite, `bg_*` / `clip_score_edited` and the box of region="mask" all see the
        grown mask, and a region crops it after it has grown.  One HIP op on the device; a mask shrunk to nothing returns
        the source; 0 (default) launches nothing.
        [additive] `outpaint` (None, or (left, top, right, bottom): integers in 0..4096, at least one > 0): outpainting.  The picture is made larger
        by that many pixels on each side and the model invents what lies in the new border.  The call returns exactly what
        `edit(C, prompt, mask=M, ...)` returns with the same other arguments, where C is the canvas -- `image` (converted to RGB) with its edge
        pixels replicated into the margins -- and M the canvas mask: 255 in the margins, `mask` as passed (or 0) over the source
        (`outpaint_canvas()` returns the pair).  So the keyword counts as a mask for `mask_grow` (r > 0 grows the border r pixels into the source:
        the seam is regenerated), `mask_blur`, `masked_content`, `blend` and region="mask"; `resolution="auto"` picks the bucket of the canvas;
        output_size="source" returns the canvas's size with the caller's bytes wherever the mask is 0; an explicit `region` box is in canvas
        coordinates.  With masked_content="original" the model starts from the replicated streaks and the edge map keeps their edges: "fill" or
        "latent_noise" with mask_grow=8..32 is the usual recipe.  Source and mask are uploaded at their own size and the canvas is built by one
        HIP op on the device in front of the job; None (default) launches nothing.
        [additive] `tiles` (None, "auto", (tw, th) or "WxH"), `tile_overlap` (0..256, default 128), `tile_batch` (1..16, default 4): a tiled edit, for
        images above 1024^2 pixels.  The image is covered by overlapping tiles of one legal edit size (fie_amd/tiles.py: plan -- "auto" picks per
        axis the smallest size that still overlaps by `tile_overlap`), every tile is edited at its native size, `tile_batch` tiles per device job,
        and the results are crossfaded across their overlaps into one image of the source's size.  Exactly: with (tw, th, xs, ys) the plan and the
        tiles' crops of `image.convert("RGB")` in tile order, the call returns `tiles.blend_numpy(R, xs, ys, H, W)` where R is the concatenation,
        over `tiles.chunks(n, tile_batch)`, of `edit_batch(crops, [prompt] * len(crops), resolution=(tw, th), masks=the mask's crops, ...)`; every
        tile carries `seed`.  The mask keywords apply per tile through the mask's crop (`mask_grow` grows the mask first and crops it second); with
        a mask and `paste_back` every byte outside the mask is the source's.  `metrics=True` scores (source, output).  Source and mask are
        uploaded once, the tiles are device slices, the blend is one HIP op behind the last job (csrc/tile_blend.hip) and the only image that
        crosses to the host is the result.  `resolution`, `region`, `outpaint` and output_size="edit" with tiles are a
        ValueError; None (default) changes nothing.
        [additive] `mask_mode` ("binary" / "levels") and `mask_ramp` (an integer in 0..64); both need a mask: a soft mask, the mask's grey level
        as a per-pixel strength.  With "levels" the mask's greys V are read as they are: 255 is edited as a binary mask's
        white, 0 never, and a pixel of level v between is held on the source's trajectory and released into the edit for the last
        (v K + 254) // 255 of the edit's K steps only -- a face and its background, or an object and its shadow, get different strengths inside
        one image, and the seam of the edit stops being a step in latent space.  Only the latent steps read the levels; the paste-back and its
        feather, `masked_content`, `blend`, output_size="source", the box of region="mask", `bg_*` / `clip_score_edited` / `bg_lpips` read the
        support 255 (V > 0) where they read the mask, each by its own rule.  `mask_ramp` = r >= 1 builds V from a binary mask's outline on the
        device: 0 outside the mask, floor(255 d / r) clipped to 255 inside, d the distance to the nearest pixel outside the mask -- the ramp runs
        inward, the image border is not an edge, and `mask_grow=r` in front of it (grown first, ramped second) moves it outward.  r counts pixels
        of the mask as passed, that is of the source image, as `mask_grow` does: on a large source the edit runs at a fraction of that size and the
        recipe is region="mask", so that the ramp spans more than a latent pixel or two.  "levels" with `mask_ramp` or with `mask_grow` is a
        ValueError (both work on the outline and would discard the greys).  A region and tiles ramp the whole mask first and crop second.  The
        defaults launch nothing and change nothing.
        [additive] `set_canny_density(d)` in front of the call: an edge-budget Canny; the two thresholds are then picked per
        image on the device and `canny_low_threshold` / `canny_high_threshold` give only their ratio.  Without it nothing changes."""
        tiles, tile_overlap, tile_batch = htiles.check(tiles, tile_overlap, tile_batch)
        scalars = self._scalars(strength, num_inference_steps, guidance_scale, controlnet_conditioning_scale, canny_low_threshold,
                                canny_high_threshold, seed)
        density = self._density(scalars)
        if tiles is not None:
            self._check_tiled(resolution, region, outpaint, output_size)
        full = hregion.check_output(output_size, region)
        margins = hmask.check_outpaint(outpaint)
        masked = mask is not None or margins is not None          # the new border is a mask of its own
        spec = hmask.MaskSpec.check(mask_blur, paste_back, masked_content, blend, blend_levels, mask_grow, mask_mode, mask_ramp, have_mask=masked)
        mask_l = hmask.to_l_array(mask, image.size) if mask is not None else None
        if tiles is not None:
            pair = None
            if density is not None:                       # one pair from the whole source, handed to every tile job as explicit thresholds
                pair = self.canny_thresholds(image, density, canny_low_threshold, canny_high_threshold, tiles=tiles)
                scalars = dict(scalars, canny_density=None, canny_low_threshold=pair[0], canny_high_threshold=pair[1])
            res = self._edit_tiled(image, prompt, negative_prompt, htiles.plan(image.size, tiles, tile_overlap), tile_batch, mask_l, spec, metrics,
                                   scalars)
            if metrics and pair is not None:
                res[1].update(canny_low=pair[0], canny_high=pair[1])
            if metrics:
                self._with_control([res[1]], scalars)
            self._tls.canny_pairs = [pair]
            return res
        if region is not None and margins is not None:            # a region crops on the host: the canvas comes back once, the rest is the call on it
            canvas, canvas_mask = self._outpaint_host(image, mask_l, margins)
            return self.edit(Image.fromarray(canvas), prompt, negative_prompt, **scalars, mask=canvas_mask, **spec.keywords(),
                             resolution=resolution, metrics=metrics, output_size=output_size, region=region, region_padding=region_padding)
        if region is not None:
            if spec.grow:   # grown first, cropped second: the box of "mask" is the grown mask's, and pixels outside an explicit box reach into it
                mask_l = self._grow_host(mask_l, spec.grow)
            if spec.ramp:   # ramped whole, cropped second: the crop carries its levels, and the box of "mask" comes from their support
                mask_l = self._ramp_host(mask_l, spec.ramp)
            box = hregion.resolve(region, image.size, hmask.support_numpy(mask_l) if spec.soft else mask_l, region_padding, resolution)
            res = self.edit(image.crop(box), prompt, negative_prompt, **scalars, mask=None if mask_l is None else mask_l[box[1]:box[3], box[0]:box[2]],
                            **spec.prepared().keywords(), resolution=resolution, metrics=metrics, output_size="source")
            if metrics:
                return hregion.paste(image, res[0], box), res[1]
            return hregion.paste(image, res, box)
        res = self._single_job(image, prompt, negative_prompt, 1, resolution, mask_l, margins, spec, metrics, full, scalars)
        self._tls.canny_pairs = [res.canny_pair]
        if not metrics:
            return res.images[0]
        return res.images[0], self._with_control(self._with_pair(self._scores(res.extra, [masked]), [res.canny_pair]), scalars)[0]

    @staticmethod
    def _scalars(strength, num_inference_steps, guidance_scale, controlnet_conditioning_scale, canny_low_threshold, canny_high_threshold, seed):
        """The scalar keywords of edit() under their own names: what its tails read and its re-entries pass on."""
        return dict(strength=strength, num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                    controlnet_conditioning_scale=controlnet_conditioning_scale, canny_low_threshold=canny_low_threshold,
                    canny_high_threshold=canny_high_threshold, seed=seed)

    def _density(self, kw):
        """The density of a device job's Canny: the editor's setting (set_canny_density), checked with the call's pair, which is then its ratio.
        The tile jobs of a tiled edit carry `canny_density=None` in kw: their thresholds are the pair picked from the whole source."""
        if "canny_density" in kw:
            return kw["canny_density"]
        return hcanny.check(self.canny_density, kw["canny_low_threshold"], kw["canny_high_threshold"])

    @staticmethod
    def _with_pair(dicts, pairs):
        """The metric dicts with `canny_low` / `canny_high` where an image's Canny picked its own thresholds (pairs[i] not None)."""
        for d, pair in zip(dicts, pairs):
            if pair is not None:
                d.update(canny_low=pair[0], canny_high=pair[1])
        return dicts

    def _single_job(self, image, prompt, negative_prompt, k, resolution, mask_l, margins, spec, metrics, full, kw, select=None):
        """The tail of edit() and edit_sweep() behind their argument checks: ONE device job on one image with k rows -- edit(): 1 and
        kw["strength"] a float; edit_sweep(): its variants and kw["strength"] their list of strengths.  mask_l: None or the uint8 [H, W] mask;
        margins: check_outpaint()'s tuple or None; spec: the call's MaskSpec; kw: the scalar keywords of edit() (_scalars).  `select`: None, or
        (rule, floor, bg) of the selector that wraps the scorer (_selector).  Hooks, outermost first: _fullres, _selector, _scorer.
        -> the pipeline's result."""
        size = buckets.target_size(resolution, hmask.canvas_size(image.size, margins))
        generator = None
        if kw["seed"] is not None:
            generator = torch.Generator(device=self.device).manual_seed(kw["seed"])
        # same data flow as the reference (:251-272) with the images kept in HBM: the LANCZOS resize to 1024x1024 (:251) runs
        # on the device (bit-exact with Pillow, csrc/resize.hip) on the uploaded original, and preprocess_image()'s PIL round
        # trip (D2H of the edge map + H2D again inside the pipeline) is skipped
        slot = getattr(self._tls, "slot", 0)
        # the Canny kernels (NMS + a fixed number of hysteresis rounds) are launched and NOT waited for: the whole edit is issued behind them on
        # the same stream, and whether the rounds had reached the fixed point is read when the result is on the host (the flags travelled
        # with it).  Common case: no host wait in front of the edit.  Rare case (a weak chain across more than 15 tiles): the remaining rounds
        # run and the device job is repeated on the final edge map -- same result as preprocess_image() + the pipeline call, always
        origs, omasks = ([], []) if metrics or full else (None, None)
        with self.pipe.eager_lock, torch.cuda.stream(self.pipe.slot_stream(slot)):
            if margins is not None:         # from here on the canvas and its mask stand where the image and the mask stood, already on the device
                image, mask_l = self._outpaint_device(image, mask_l, margins)
            source_dev, control_dev, finish = self._canny_device(image, kw["canny_low_threshold"], kw["canny_high_threshold"], size=size, wait=False,
                                                                 original=origs, density=self._density(kw))
            mask_dev = self._mask_device(mask_l, size, spec, original=omasks)
        hook = None
        if metrics:
            keep = {} if select is not None else None
            hook = self._scorer(slot, origs * k, omasks * k, [prompt] * k, keep=keep)
            if select is not None:
                hook = self._selector(slot, hook, keep, *select)
        if full:        # the edit-size job runs with its own paste-back off: the composite happens at the source's size, behind it, for all k rows
            hook = self._fullres(slot, origs * k, (omasks if spec.paste_back else [None]) * k, spec.blur, hook)
        res = self.pipe(slot=slot, prompt=prompt, negative_prompt=negative_prompt, image=source_dev, control_image=control_dev,
                        generator=generator, post_check=finish, mask_image=mask_dev, after_device=hook, **self._job_keywords(kw, spec, full))
        res.canny_pair = getattr(finish, "pair", None)    # an edge-budget Canny's (low, high): they came to the host with the flags
        return res

    @staticmethod
    def _job_keywords(kw, spec, full):
        """The pipeline's keywords of a device job: the scalars it reads, and the spec of a mask that _mask_device has grown and ramped already,
        with `full` in front of the source-size back end."""
        spec = (spec.behind_fullres() if full else spec).prepared()
        return dict({k: kw[k] for k in ("strength", "num_inference_steps", "guidance_scale", "controlnet_conditioning_scale")}, **spec.keywords())

    def _fullres(self, slot, origs, omasks, blur, then=None):
        """The `after_device` hook of an edit with output_size="source": queues, on the edit's stream behind its result and outside its graph, the
        full-resolution back end of every image of the job (hip.Context.fullres_paste: two launches each, into a buffer of the slot) and hands its
        output to the pipeline's final device-to-host copy in place of the edit-size image.  `origs`: the sources as uploaded; `omasks`: the masks
        as uploaded (None: that image is a pure resize); `then`: the scorer of metrics=True, which then scores the source-size outputs."""
        ctx = self.pipe.ctx

        def backend(out_u8):
            batch = out_u8.dim() == 4
            outs = []
            with self.pipe.eager_lock:                    # the context's stream binding is shared by the threads of in-flight edits
                for i, (o, src, m) in enumerate(zip(list(out_u8) if batch else [out_u8], origs, omasks)):
                    buf = self._fullres_out.get((slot, i))           # grown, never shrunk: source sizes follow the caller's images
                    if buf is None or buf.numel() < src.numel():
                        buf = self._fullres_out[(slot, i)] = torch.empty(src.numel(), device=src.device, dtype=torch.uint8)
                    outs.append(ctx.fullres_paste(o.contiguous(), src, m, blur if m is not None else 0.0, out=buf[:src.numel()].view(src.shape)))
            extra = then(outs if batch else outs[0]) if then is not None else None
            if isinstance(extra, DeviceOutput):           # `then` chose what travels itself (edit_sweep's selector: the winner alone)
                return extra
            return DeviceOutput(outs if batch else outs[0], extra)
        return backend

    def _selector(self, slot, scorer, keep, rule, floor, bg):
        """The `after_device` hook of edit_sweep(select=...): runs `scorer` (the _scorer hook, whose device rows arrive in `keep`) on the k variants,
        then queues ONE fie_sweep_select_u8 launch behind it on the same stream: the winner's bytes go into a buffer of the slot and take the final
        device-to-host copy in place of the k images; the index rides with the rows into pinned host memory.  -> DeviceOutput([winner], (the
        scorer's result, the int32 [1] index on the host))."""
        ctx = self.pipe.ctx

        def pick(out_u8):
            outs = list(out_u8) if isinstance(out_u8, list) or out_u8.dim() == 4 else [out_u8]
            extra = scorer(out_u8)
            with self.pipe.eager_lock:                    # the context's stream binding is shared by the threads of in-flight edits
                n = outs[0].numel()
                buf = self._sweep_out.get(slot)           # grown, never shrunk: with output_size="source" the size follows the caller's images
                if buf is None or buf.numel() < n:
                    buf = self._sweep_out[slot] = torch.empty(n, device=ctx.device, dtype=torch.uint8)
                win, idx = ctx.sweep_select([o.contiguous() for o in outs], keep["rows"], keep.get("clip"), rule, floor, bg,
                                            out=buf[:n].view(outs[0].shape))
            ihost = self._sweep_idx.get(slot)
            if ihost is None:
                ihost = self._sweep_idx[slot] = torch.empty(1, dtype=torch.int32).pin_memory()
            ihost.copy_(idx, non_blocking=True)
            return DeviceOutput([win], (extra, ihost))
        return pick

    def edit_sweep(self, image, prompt, negative_prompt="", strengths="all", num_inference_steps=4, guidance_scale=1.5,
                   controlnet_conditioning_scale=0.5, canny_low_threshold=100, canny_high_threshold=200, seed=None, mask=None, mask_blur=0,
                   paste_back=True, *, resolution=None, output_size=None, region=None, tiles=None, masked_content="original", blend="alpha",
                   blend_levels=4, mask_grow=0, outpaint=None, select=None, min_ssim=None, mask_mode="binary", mask_ramp=0):
        """[additive] edit() at several strengths as ONE device job, scored on the device, optionally with the winner picked there (DESIGN.md
        section 20).  `strength` only decides how many of the `num_inference_steps` LCM steps an edit runs, so the distinct edits are those of the
        distinct step counts m = min(int(N * s), N): `strengths` is "all" (one variant per m = 1 .. N) or a list of floats in [0, 1]; strengths with
        the same m are one variant (fie_amd/sweep.py: variants; at most 16).  Variants are ordered strongest first.  Upload, resize, Canny map, text
        encoders, mask preparation, fill, VAE encode and edge-map embedding run once; the UNet and the ControlNet run each loop step on the
        variants that have joined by then; with `seed`, variant i is what edit(..., strength=s_i, seed=seed) returns up to fp16 tiling effects
        (the bound of edit_batch against serial edits).  A soft mask (`mask_mode` / `mask_ramp`) is prepared once: its support does not depend
        on the step count, and every variant releases a level by its own number of steps.  The other keywords are edit()'s (`metrics` is always on; `region` and `tiles` are a
        ValueError).  With `set_canny_density(d)` the Canny map is shared, so the sweep has ONE pair and every variant's dict reports it.
        select=None: returns (images, variants): variants[i] = {"strength": [the requested strengths of the variant], "steps": m, and the
        metrics dict edit(..., strength=s_i, metrics=True) reports}.
        select="strongest" (needs `min_ssim`): the strongest variant whose SSIM against the source -- `bg_ssim` with a mask -- is at least
        `min_ssim`: the most editing the preservation budget allows.  select="clip_score" (needs FastEditor(clip_score_dir=...)): the variant
        with the best CLIP score, among those that pass `min_ssim` when one is given; ties go to the weaker edit.  When no variant passes, the
        one with the highest SSIM wins (fie_amd/sweep.py: select_numpy is the rule, word for word).  Both return (image, info): info holds
        `index`, `strength`, `steps`, the winner's metrics, `variants` as above and `rows` / `clip_rows` (the raw rows the rule read).  The rule runs
        in one HIP op behind the scorer (fie_sweep_select_u8): only the winner's image crosses to the host -- with output_size="source" one
        source-size image instead of k -- behind one synchronisation."""
        from fie_amd import sweep as hsweep
        if region is not None:
            raise ValueError("edit_sweep with a region: a sweep runs on the whole image")
        if tiles is not None:
            raise ValueError("edit_sweep with tiles: a sweep runs as one device job")
        if select not in (None, "clip_score", "strongest"):
            raise ValueError(f"select={select!r}: None, 'clip_score' or 'strongest'")
        if select == "clip_score" and self.clip_scorer is None:
            raise ValueError("select='clip_score' needs a CLIP model: FastEditor(clip_score_dir=...)")
        if select == "strongest" and min_ssim is None:
            raise ValueError("select='strongest' needs min_ssim: the SSIM every candidate must keep")
        if min_ssim is not None:
            if select is None:
                raise ValueError("min_ssim without select: 'clip_score' or 'strongest'")
            if isinstance(min_ssim, bool) or not isinstance(min_ssim, (int, float)) or not -1.0 <= float(min_ssim) <= 1.0:
                raise ValueError(f"min_ssim={min_ssim!r}: a number in [-1, 1]")
        vs = hsweep.variants(num_inference_steps, strengths)
        full = hregion.check_output(output_size, None)
        margins = hmask.check_outpaint(outpaint)
        masked = mask is not None or margins is not None
        spec = hmask.MaskSpec.check(mask_blur, paste_back, masked_content, blend, blend_levels, mask_grow, mask_mode, mask_ramp, have_mask=masked)
        mask_l = hmask.to_l_array(mask, image.size) if mask is not None else None
        k = len(vs)
        scalars = self._scalars([v[1][0] for v in vs], num_inference_steps, guidance_scale, controlnet_conditioning_scale, canny_low_threshold,
                                canny_high_threshold, seed)
        self._density(scalars)
        rule = None if select is None else (select, hsweep.ssim_floor(min_ssim, hmetrics.TARGET[1], hmetrics.TARGET[0]), masked)
        res = self._single_job(image, prompt, negative_prompt, k, resolution, mask_l, margins, spec, True, full, scalars, select=rule)
        self._tls.canny_pairs = [res.canny_pair]
        extra, ihost = res.extra if select is not None else (res.extra, None)
        variants = [{"strength": list(v[1]), "steps": v[0], **d}
                    for v, d in zip(vs, self._with_pair(self._scores(extra, [masked] * k), [res.canny_pair] * k))]
        for v, d in zip(vs, variants):                    # control weights: a sweep has no window, every variant keeps all of its own steps
            self._with_control([d], scalars, strength=v[1][0])
        if select is None:
            return res.images, variants
        index = int(ihost[0])
        rows = (extra[0] if isinstance(extra, tuple) else extra).numpy().copy()
        clip_rows = extra[1].numpy()[:k].copy() if isinstance(extra, tuple) and extra[1] is not None else None
        info = dict(variants[index], index=index, variants=variants, rows=rows, clip_rows=clip_rows)
        return res.images[0], info

    def _scorer(self, slot, origs, omasks, prompts=None, keep=None):
        """The `after_device` hook of an edit with metrics=True: queues, on the edit's stream behind its result, the LANCZOS resizes to
        512x512 (sources, results, masks), ONE fie_metrics_pairs_u8 launch pair for all images of the job and the copy of the 32-byte result
        rows into pinned host memory of the slot.  The edit's own final synchronisation (the image's D2H) completes them.  With a CLIP model
        (`clip_scorer`) the hook also queues the CLIP score of every result against its prompt (cached text embedding, one batched pass of the
        image tower, the masked variants in the same pass) and returns (metric rows, CLIP rows, which (image, masked) each CLIP row is).  With a DINO
        model (`dino_scorer`) it queues, behind those, the structure distance of every (original source, result) pair of square images -- one batched
        pass of the tower per (source size, result size) -- and the tuple grows by (distance rows, which image each row is).  With the LPIPS
        weights (`lpips_scorer`) it queues the LPIPS layer values of every pair on the 512x512 tensors and the binary masks it has already built
        (the background variant where an image has a mask), and the tuple's sixth entry is their rows.  `keep`: a dict that receives the DEVICE
        tensors of the metric rows ("rows") and of the CLIP rows ("clip"), for work queued behind the scorer (edit_sweep's selector)."""
        ctx = self.pipe.ctx
        th, tw = hmetrics.TARGET[1], hmetrics.TARGET[0]
        to512 = lambda t: t if tuple(t.shape[:2]) == (th, tw) else ctx.resize_lanczos(t.contiguous(), th, tw)
        stack = lambda ts: ts[0][None] if len(ts) == 1 else torch.stack(ts)

        def score(out_u8):
            outs = list(out_u8) if isinstance(out_u8, list) or out_u8.dim() == 4 else [out_u8]
            with self.pipe.eager_lock:                    # the context's stream binding is shared by the threads of in-flight edits
                a = stack([to512(o) for o in origs])
                b = stack([to512(o) for o in outs])
                mk = None
                if any(m is not None for m in omasks):
                    zero = lambda: torch.zeros((th, tw), device=ctx.device, dtype=torch.uint8)
                    mk = stack([zero() if m is None else hmetrics.binary_mask_device(ctx, m) for m in omasks])
                rows = ctx.metrics_pairs(a, b, mk)
                if keep is not None:
                    keep["rows"] = rows
            host = self._metric_rows.get((slot, len(outs)))
            if host is None:
                host = self._metric_rows[(slot, len(outs))] = torch.empty((len(outs), 4), dtype=torch.int64).pin_memory()
            host.copy_(rows, non_blocking=True)
            if self.lpips_scorer is not None:
                return self._with_lpips(score_more(outs, host), self._lpips_queue(slot, a, b, mk, [m is not None for m in omasks]))
            return score_more(outs, host)

        def score_more(outs, host):
            if self.clip_scorer is None and self.dino_scorer is None:
                return host
            if self.clip_scorer is None:
                return (host, None, ()) + self._dino_queue(slot, origs, outs)
            clip = self.clip_scorer
            items = [(i, False) for i in range(len(outs))] + [(i, True) for i, m in enumerate(omasks) if m is not None]
            with self.pipe.eager_lock:
                txts = [clip.text_embedding(prompts[i]) for i, _ in items]
                emb = clip.image_embeddings([outs[i] for i, _ in items], [omasks[i] if masked else None for i, masked in items])
                crow = clip.score_rows(emb, txts[0] if len(txts) == 1 else torch.cat(txts))
                if keep is not None:
                    keep["clip"] = crow
            chost = self._clip_rows.get((slot, len(items)))
            if chost is None:
                chost = self._clip_rows[(slot, len(items))] = torch.empty((len(items), 2), dtype=torch.float32).pin_memory()
            chost.copy_(crow, non_blocking=True)
            if self.dino_scorer is not None:
                return (host, chost, items) + self._dino_queue(slot, origs, outs)
            return host, chost, items
        return score

    @staticmethod
    def _with_lpips(extra, lpips_rows):
        """The scorer's result with the LPIPS rows as its sixth entry."""
        return ((tuple(extra) if isinstance(extra, tuple) else (extra, None, ())) + (None, ()))[:5] + (lpips_rows,)

    def _lpips_queue(self, slot, a, b, mk, has_mask):
        """Queues the LPIPS layer values of the pairs (a[i], b[i]) -- u8 [n, 512, 512, 3] -- and, where has_mask[i], of their background variants
        under the 0 / 1 masks mk u8 [n, 512, 512], on the current stream, and the copy of the rows into pinned host memory of the slot.
        -> f64 [n, 7] (no mask at all) or [n, 14] on the host."""
        n = a.shape[0]
        with self.pipe.eager_lock:
            rows = self.lpips_scorer.scores(list(a), list(b), None if mk is None else [mk[i] if has_mask[i] else None for i in range(n)])
        lhost = self._lpips_rows.get((slot, n, rows.shape[1]))
        if lhost is None:
            lhost = self._lpips_rows[(slot, n, rows.shape[1])] = torch.empty(tuple(rows.shape), dtype=torch.float64).pin_memory()
        lhost.copy_(rows, non_blocking=True)
        return lhost

    def _dino_queue(self, slot, origs, outs):
        """Queues the structure distances of the square (original, result) pairs on the current stream and the copy of their 8 bytes each into pinned
        host memory of the slot.  -> (f64 rows on the host or None, the image index of every row)."""
        from fie_amd import dino as hdino
        groups = {}
        for i, (a, b) in enumerate(zip(origs, outs)):
            if hdino.supported_size(*a.shape[:2]) and hdino.supported_size(*b.shape[:2]):
                groups.setdefault((tuple(a.shape[:2]), tuple(b.shape[:2])), []).append(i)
        order = [i for g in groups.values() for i in g]
        if not order:
            return None, ()
        ctx = self.pipe.ctx
        rows = torch.empty(len(order), device=ctx.device, dtype=torch.float64)
        r0 = 0
        with self.pipe.eager_lock:
            for g in groups.values():
                self.dino_scorer.distances([origs[i] for i in g], [outs[i] for i in g], out=rows[r0:r0 + len(g)])
                r0 += len(g)
        dhost = self._dino_rows.get((slot, len(order)))
        if dhost is None:
            dhost = self._dino_rows[(slot, len(order))] = torch.empty(len(order), dtype=torch.float64).pin_memory()
        dhost.copy_(rows, non_blocking=True)
        return dhost, tuple(order)

    def _scores(self, extra, has_mask):
        lpips_rows = extra[5] if isinstance(extra, tuple) and len(extra) > 5 else None
        host_rows, clip_rows, items, dino_rows, dino_items = (tuple(extra) + (None, ()))[:5] if isinstance(extra, tuple) else (extra, None, (), None, ())
        out = hmetrics.rows_to_dicts(host_rows.numpy().copy(), hmetrics.TARGET[1], hmetrics.TARGET[0], has_mask)
        for (i, masked), row in zip(items, clip_rows.numpy().copy() if clip_rows is not None else ()):
            out[i]["clip_score_edited" if masked else "clip_score"] = float(row[1])
        if self.dino_scorer is not None:
            for m in out:
                m["dino_distance"] = None
            for i, v in zip(dino_items, dino_rows.numpy().copy() if dino_rows is not None else ()):
                out[i]["dino_distance"] = float(v)
        if lpips_rows is not None:
            from fie_amd import lpips as hlpips
            for m, row, masked in zip(out, lpips_rows.numpy().copy(), has_mask):
                m["lpips"] = hlpips.total(row[:7])
                if masked:
                    m["bg_lpips"] = hlpips.total(row[7:14])
        return out

    def _grow_host(self, mask_l, grow):
        """uint8 [H, W] mask -> the mask grown by `grow` (fie_mask_grow_u8), back on the host: what a region edit crops.  One upload, one launch
        and one synchronising copy of H * W bytes on the calling thread's slot stream."""
        with self.pipe.eager_lock, torch.cuda.stream(self.pipe.slot_stream(getattr(self._tls, "slot", 0))):
            return self.pipe.ctx.mask_grow(torch.from_numpy(mask_l).to(self.pipe.ctx.device), grow).cpu().numpy()

    def _ramp_host(self, mask_l, ramp):
        """uint8 [H, W] mask -> its level map under `mask_ramp` (fie_mask_ramp_u8), back on the host: what a region edit crops.  As _grow_host()."""
        with self.pipe.eager_lock, torch.cuda.stream(self.pipe.slot_stream(getattr(self._tls, "slot", 0))):
            return self.pipe.ctx.mask_ramp(torch.from_numpy(mask_l).to(self.pipe.ctx.device), ramp).cpu().numpy()

    def _outpaint_device(self, image, mask_l, margins):
        """PIL image, uint8 [H, W] mask or None, check_outpaint()'s margins -> (canvas u8 [Hc, Wc, 3], canvas mask u8 [Hc, Wc]) on the device:
        source and mask are uploaded at their own size, the canvas is one launch (fie_outpaint_canvas_rgb_u8) on the current stream.  An image of
        another mode than RGB goes through `.convert("RGB")`."""
        dev = self.pipe.ctx.device
        src = torch.from_numpy(np.array(image if image.mode == "RGB" else image.convert("RGB"))).to(dev)
        return self.pipe.ctx.outpaint_canvas(src, None if mask_l is None else torch.from_numpy(mask_l).to(dev), margins)

    def _outpaint_host(self, image, mask_l, margins):
        """_outpaint_device(), back on the host as two numpy arrays: what a region edit crops.  One synchronising copy of the canvas and its mask
        on the calling thread's slot stream."""
        with self.pipe.eager_lock, torch.cuda.stream(self.pipe.slot_stream(getattr(self._tls, "slot", 0))):
            canvas, canvas_mask = self._outpaint_device(image, mask_l, margins)
            return canvas.cpu().numpy(), canvas_mask.cpu().numpy()

    def outpaint_canvas(self, image, outpaint, mask=None):
        """[additive] What `edit(image, ..., mask=mask, outpaint=outpaint)` runs on: (canvas, canvas mask) as PIL images of modes RGB and L, built
        by the device op.  edit(canvas, ..., mask=canvas mask) is that call."""
        margins = hmask.check_outpaint(outpaint)
        if margins is None:
            raise ValueError("outpaint_canvas: outpaint=None: (left, top, right, bottom)")
        canvas, canvas_mask = self._outpaint_host(image, hmask.to_l_array(mask, image.size) if mask is not None else None, margins)
        return Image.fromarray(canvas), Image.fromarray(canvas_mask)

    def _mask_device(self, mask_l, size, spec=hmask.MaskSpec(), original=None):
        """uint8 [H, W] mode-L mask (or None) -> u8 [size[1], size[0]] on the device: LANCZOS-resized as the source is (fie_resize_l_u8,
        bit-exact with `mask.convert("L").resize(size, Image.LANCZOS)`).  `mask_l` may also be a u8 [H, W] tensor already on the device (an
        outpainting canvas's mask): it is taken as the upload.  Under `spec` the upload is grown first (fie_mask_grow_u8), and a soft mask
         comes back as MaskLevels(support, levels): the level map V is the grown mask ramped (fie_mask_ramp_u8) or, with
        "levels", the upload itself, and its support S and V are resized separately.  `original`: a list that receives the mask every later
        reader takes as the uploaded one, the grown mask or S (or None)."""
        if mask_l is None:
            if original is not None:
                original.append(None)
            return None
        m = mask_l if torch.is_tensor(mask_l) else torch.from_numpy(mask_l).to(self.pipe.ctx.device)
        if spec.grow:
            m = self.pipe.ctx.mask_grow(m, spec.grow)
        v = self.pipe.ctx.mask_ramp(m.contiguous(), spec.ramp) if spec.ramp else m.contiguous() if spec.mode == "levels" else None
        if v is not None:
            m = self.pipe.ctx.mask_support(v)
        if original is not None:
            original.append(m)
        if (m.shape[1], m.shape[0]) != tuple(size):
            m = self.pipe.ctx.resize_lanczos(m, size[1], size[0])
            if v is not None:
                v = self.pipe.ctx.resize_lanczos(v, size[1], size[0])
        return m if v is None else MaskLevels(m, v)

    def edit_batch(self, images, prompts, negative_prompts=None, strength=0.80, num_inference_steps=4, guidance_scale=1.5,
                   controlnet_conditioning_scale=0.5, canny_low_threshold=100, canny_high_threshold=200, seed=None, masks=None, mask_blur=0,
                   paste_back=True, *, resolution=None, metrics=False, output_size=None, region=None, region_padding=32, masked_content="original",
                   blend="alpha", blend_levels=4, mask_grow=0, outpaint=None, tiles=None, tile_overlap=128, tile_batch=4, mask_mode="binary",
                   mask_ramp=0):
        """[additive] edit() for a list of images in ONE device job (UNet / ControlNet / CLIP at batch n x CFG; the
        BASELINE "batch=8" configuration).  Every image gets its own generator seeded with `seed`, exactly as n serial
        edit(..., seed=seed) calls would, so image i of the batch equals the serial result up to fp16 tiling effects.
        `masks`: None, or one mask per image as edit()'s `mask` (None in the list: that image is edited everywhere).
        `resolution`: as edit()'s, per image.  Images of different target sizes ("auto" on mixed aspect ratios) run as one device job per
        size, in the order of each size's first image; the results come back in input order.
        `metrics=True`: returns (images, [dict per image]) as edit() does; all images of a device job are scored in one launch.
        `output_size` / `region` / `region_padding`: as edit()'s; every image comes back at its own source's size, the back end queued per image
        behind the job.  `region` may also be a LIST with one entry per image (None, "mask" or a box): each image gets its own box, images are
        grouped by the target size of their crops, and an image whose entry is None is edited whole and returned at its source's size.
        `masked_content`: as edit()'s, one value for the whole call; an image whose mask is None is edited as without it.
        `blend` / `blend_levels`: as edit()'s, one value for the whole call; an image whose mask is None comes out as without them.
        `mask_grow`: as edit()'s, one radius for the whole call; an image whose mask is None is untouched.
        `mask_mode` / `mask_ramp`: as edit()'s, one value for the whole call; an image whose mask is None is untouched.
        `outpaint`: as edit()'s -- one (left, top, right, bottom) tuple for the whole call, or a LIST with one entry (a tuple or None) per image; an
        image whose entry is None is treated as without the keyword, one with margins counts as masked.  Images group by the target size of their
        canvases.
        `tiles` / `tile_overlap` / `tile_batch`: as edit()'s; every image is tiled on its own (its tiles alone fill its device jobs) and the results
        come back in input order.
        With `set_canny_density(d)` every image gets its own pair of thresholds from its own statistics."""
        if len(images) != len(prompts) or not images:
            raise ValueError("images and prompts must be non-empty lists of one length")
        if masks is not None and len(masks) != len(images):
            raise ValueError(f"{len(masks)} masks for {len(images)} images: one mask (or None) per image")
        tiled = htiles.check(tiles, tile_overlap, tile_batch)[0] is not None
        if tiled:
            self._check_tiled(resolution, region, outpaint, output_size)
        if isinstance(outpaint, list) and len(outpaint) != len(images):
            raise ValueError(f"{len(outpaint)} outpaint entries for {len(images)} images: one (left, top, right, bottom) or None per image")
        margins = [hmask.check_outpaint(o) for o in outpaint] if isinstance(outpaint, list) else [hmask.check_outpaint(outpaint)] * len(images)
        outpainted = any(o is not None for o in margins)
        has_mask = [(masks is not None and masks[i] is not None) or o is not None for i, o in enumerate(margins)]
        spec = hmask.MaskSpec.check(mask_blur, paste_back, masked_content, blend, blend_levels, mask_grow, mask_mode, mask_ramp,
                                    have_mask=any(has_mask))
        scalars = self._scalars(strength, num_inference_steps, guidance_scale, controlnet_conditioning_scale, canny_low_threshold,
                                canny_high_threshold, seed)
        self._density(scalars)
        if tiled:
            negs = list(negative_prompts) if isinstance(negative_prompts, (list, tuple)) else [negative_prompts or ""] * len(images)
            if len(negs) != len(images):
                raise ValueError(f"{len(negs)} negative prompts for {len(images)} images")
            res, pairs = [], []
            for i, (im, p, neg, masked) in enumerate(zip(images, prompts, negs, has_mask)):
                res.append(self.edit(im, p, neg, **scalars, mask=masks[i] if masked else None, **(spec if masked else spec.unmasked()).keywords(),
                                     metrics=metrics, output_size=output_size, tiles=tiles, tile_overlap=tile_overlap, tile_batch=tile_batch))
                pairs += self._tls.canny_pairs
            self._tls.canny_pairs = pairs
            return ([r[0] for r in res], [r[1] for r in res]) if metrics else res
        regions = list(region) if isinstance(region, list) else [region] * len(images)
        if len(regions) != len(images):
            raise ValueError(f"{len(regions)} regions for {len(images)} images: one region (or None) per image")
        has_region = any(r is not None for r in regions)
        full = hregion.check_output(output_size, "mask" if has_region else None)
        if has_region and outpainted:       # regions crop on the host: the canvases come back once (edit()), the rest is the call on them
            canvases, cmasks = list(images), list(masks) if masks is not None else [None] * len(images)
            for i, o in enumerate(margins):
                if o is not None:
                    c, m = self._outpaint_host(images[i], hmask.to_l_array(cmasks[i], images[i].size) if cmasks[i] is not None else None, o)
                    canvases[i], cmasks[i] = Image.fromarray(c), m
            return self.edit_batch(canvases, prompts, negative_prompts, **scalars, masks=cmasks, **spec.keywords(), resolution=resolution,
                                   metrics=metrics, output_size=output_size, region=region, region_padding=region_padding)
        if has_region:
            mls = [hmask.to_l_array(m, im.size) if m is not None else None for m, im in zip(masks or [None] * len(images), images)]
            if spec.grow:   # grown first, cropped second (edit())
                mls = [m if m is None else self._grow_host(m, spec.grow) for m in mls]
            if spec.ramp:   # ramped whole, cropped second (edit())
                mls = [m if m is None else self._ramp_host(m, spec.ramp) for m in mls]
            boxes = [hregion.resolve(r, im.size, hmask.support_numpy(m) if spec.soft and m is not None else m, region_padding, resolution)
                     for r, im, m in zip(regions, images, mls)]
            cut = lambda a, b: a if a is None or b is None else a[b[1]:b[3], b[0]:b[2]]
            res = self.edit_batch([im if b is None else im.crop(b) for im, b in zip(images, boxes)], prompts, negative_prompts, **scalars,
                                  masks=None if masks is None else [cut(m, b) for m, b in zip(mls, boxes)], **spec.prepared().keywords(),
                                  resolution=resolution, metrics=metrics, output_size="source")
            outs = [o if b is None else hregion.paste(im, o, b) for im, o, b in zip(images, res[0] if metrics else res, boxes)]
            return (outs, res[1]) if metrics else outs
        sizes = [buckets.target_size(resolution, hmask.canvas_size(im.size, o)) for im, o in zip(images, margins)]
        groups = {}
        for i, sz in enumerate(sizes):
            groups.setdefault(sz, []).append(i)
        if len(groups) > 1:
            out, mets, pairs = [None] * len(images), [None] * len(images), [None] * len(images)
            pick = lambda seq, idx: None if seq is None else seq if isinstance(seq, str) else [seq[i] for i in idx]
            for sz, idx in groups.items():
                res = self.edit_batch([images[i] for i in idx], [prompts[i] for i in idx], pick(negative_prompts, idx), **scalars,
                                      masks=pick(masks, idx), **(spec if any(has_mask[i] for i in idx) else spec.unmasked()).keywords(),
                                      resolution=sz, metrics=metrics, output_size=output_size,
                                      outpaint=[margins[i] for i in idx] if outpainted else None)
                res, ms = res if metrics else (res, [None] * len(idx))
                for i, r, m, pair in zip(idx, res, ms, self._tls.canny_pairs):
                    out[i], mets[i], pairs[i] = r, m, pair
            self._tls.canny_pairs = pairs
            return (out, mets) if metrics else out
        mask_ls = [hmask.to_l_array(m, im.size) if m is not None else None for m, im in zip(masks, images)] if masks is not None else None
        if outpainted and mask_ls is None:
            mask_ls = [None] * len(images)
        res, omasks = self._batch_job(images, prompts, negative_prompts, sizes[0], mask_ls, margins if outpainted else None, spec, metrics, full,
                                      scalars)
        self._tls.canny_pairs = res.canny_pairs
        if not metrics:
            return res.images
        return res.images, self._with_control(self._with_pair(self._scores(res.extra, [m is not None for m in omasks]), res.canny_pairs), scalars)

    def _batch_job(self, images, prompts, negative_prompts, size, mask_ls, margins, spec, metrics, full, kw, after=None):
        """The single-size tail of edit_batch(): ONE device job for images that share the target `size`.  images: PIL images, or u8 [H, W, 3] tensors
        already on the device (the tiles of a tiled edit: slices of one upload); mask_ls: None, or one uint8 [H, W] array / device tensor / None per
        image; margins: None, or check_outpaint()'s tuple / None per image; spec: the call's MaskSpec; kw: the scalar keywords of edit().  `after`: an `after_device` hook that
        stands in place of the scorer and the full-resolution back end (metrics and full are then False).  -> (the pipeline's result, the masks as
        uploaded)."""
        gens = None
        if kw["seed"] is not None:
            gens = [torch.Generator(device=self.device).manual_seed(kw["seed"]) for _ in images]
        slot = getattr(self._tls, "slot", 0)
        srcs, ctls, pairs = [], [], []
        density = self._density(kw)
        origs, omasks = ([], []) if metrics or full else (None, None)
        with self.pipe.eager_lock, torch.cuda.stream(self.pipe.slot_stream(slot)):
            if margins is not None:         # the canvases and their masks stand where the images and the masks stood, already on the device
                images = list(images)
                for i, o in enumerate(margins):
                    if o is not None:
                        images[i], mask_ls[i] = self._outpaint_device(images[i], mask_ls[i], o)
            for im in images:
                one = [] if metrics or full else None
                s_dev, c_dev = self._canny_device(im, kw["canny_low_threshold"], kw["canny_high_threshold"], size=size, original=one,
                                                  density=density)
                srcs.append(s_dev)
                ctls.append(c_dev)
                pairs.append(None if density is None else self.pipe.ctx.canny_pair)
                if one is not None:
                    origs.append(one[0])
            mask_devs = [self._mask_device(m, size, spec, original=omasks) for m in mask_ls] if mask_ls is not None else None
        if (metrics or full) and mask_ls is None:
            omasks = [None] * len(images)
        hook = after
        if metrics:
            hook = self._scorer(slot, origs, omasks, list(prompts))
        if full:
            hook = self._fullres(slot, origs, omasks if spec.paste_back else [None] * len(images), spec.blur, hook)
        res = self.pipe(slot=slot, prompt=list(prompts), negative_prompt=negative_prompts, image=srcs, control_image=ctls, generator=gens,
                        mask_image=mask_devs, after_device=hook, **self._job_keywords(kw, spec, full))
        res.canny_pairs = pairs                           # per image: an edge-budget Canny's (low, high), or None
        return res, omasks

    def _check_tiled(self, resolution, region, outpaint, output_size):
        """What a tiled edit cannot be combined with: the tiles ARE the edit size and the output IS the source's size."""
        if resolution is not None:
            raise ValueError(f"tiles with resolution={resolution!r}: the tile size is the edit size (tiles=(tw, th))")
        if region is not None:
            raise ValueError("tiles with a region: a region edit runs on one crop")
        if outpaint is not None:
            raise ValueError("tiles with outpaint: build the canvas first (outpaint_canvas()) and tile that")
        hregion.check_output(output_size, None)
        if output_size == "edit":
            raise ValueError("tiles with output_size='edit': a tiled edit returns the source-size image (output_size='source')")

    def _edit_tiled(self, image, prompt, negative_prompt, plan, tile_batch, mask_l, spec, metrics, kw):
        """edit(..., tiles=...) behind its argument checks (the docstring of edit() defines the result).  plan: tiles.plan()'s (tw, th, xs, ys);
        mask_l: None or the uint8 [H, W] mask; spec: the call's MaskSpec; kw: the scalar keywords of edit().  Source and mask go up once and the
        mask is grown and ramped there, whole; the tiles of a device job are contiguous copies of their boxes; each job's `after_device` hook copies its u8
        results into their rows of the slot's [n, th, tw, 3] buffer and keeps them off the host; the hook of the last job queues the blend (and,
        with metrics, the scorer behind it) and hands the H x W x 3 image to the pipeline's device-to-host copy."""
        tw, th, xs, ys = plan
        W, H = image.size
        ctx, slot = self.pipe.ctx, getattr(self._tls, "slot", 0)
        n = len(xs) * len(ys)
        with self.pipe.eager_lock, torch.cuda.stream(self.pipe.slot_stream(slot)):
            src = torch.from_numpy(np.array(image if image.mode == "RGB" else image.convert("RGB"))).to(ctx.device)
            mask_dev = levels_dev = None
            if mask_l is not None:
                mask_dev = torch.from_numpy(mask_l).to(ctx.device)
                if spec.grow:
                    mask_dev = ctx.mask_grow(mask_dev, spec.grow)
                if spec.soft:                             # ramped whole, once; the tiles carry crops of the levels, the scorer reads the support
                    levels_dev = ctx.mask_ramp(mask_dev, spec.ramp) if spec.ramp else mask_dev
                    mask_dev = ctx.mask_support(levels_dev)
            key = (slot, n, th, tw)
            if key not in self._tile_bufs:
                self._tile_bufs = {k: v for k, v in self._tile_bufs.items() if k[0] != slot}          # one plan's buffer per slot
                self._tile_bufs[key] = torch.empty((n, th, tw, 3), device=ctx.device, dtype=torch.uint8)
            buf = self._tile_bufs[key]
            out = self._fullres_out.get((slot, 0))           # the source-size output shares the full-resolution back end's buffer
            if out is None or out.numel() < src.numel():
                out = self._fullres_out[(slot, 0)] = torch.empty(src.numel(), device=ctx.device, dtype=torch.uint8)
            out = out[:src.numel()].view(src.shape)
        scorer = self._scorer(slot, [src], [mask_dev], [prompt]) if metrics else None
        jobs = htiles.chunks(n, tile_batch)
        boxes = htiles.boxes(tw, th, xs, ys)
        cut = lambda t, b: t[b[1]:b[3], b[0]:b[2]].contiguous()
        res = None
        for c in jobs:
            def collect(out_u8, c=c):
                with self.pipe.eager_lock:                # the context's stream binding is shared by the threads of in-flight edits
                    buf[c[0]:c[0] + len(c)].copy_(out_u8 if out_u8.dim() == 4 else out_u8[None])
                    if c[-1] != n - 1:
                        return DeviceOutput([])           # nothing of this job crosses to the host
                    ctx.tile_blend(buf, xs, ys, H, W, out=out)
                return DeviceOutput([out], scorer(out) if scorer is not None else None)
            with self.pipe.eager_lock, torch.cuda.stream(self.pipe.slot_stream(slot)):
                crops = [cut(src, boxes[j]) for j in c]
                mcrops = [cut(levels_dev if levels_dev is not None else mask_dev, boxes[j]) for j in c] if mask_dev is not None else None
            res, _ = self._batch_job(crops, [prompt] * len(c), [negative_prompt or ""] * len(c), (tw, th), mcrops, None, spec.prepared(), False, False,
                                     kw, after=collect)
        if not metrics:
            return res.images[0]
        return res.images[0], self._scores(res.extra, [mask_dev is not None])[0]

    def calibrate_fp8(self, image, prompt, negative_prompt="", strength=0.80, num_inference_steps=4, guidance_scale=1.5,
                      controlnet_conditioning_scale=0.5, canny_low_threshold=100, canny_high_threshold=200, seed=0, margin=2.0):
        """[additive] FastEditor(weight_dtype="f8e4m3") only: measure the activation scales of the fp8 configuration on ONE representative edit
        (same arguments as edit(); fie_amd/pipe.py: calibrate_fp8 -- per-tensor max |x| -> power-of-two scale with `margin` head-room).  Without it the
        scales are 1 and activations beyond +-448 clip.  Returns the {layer: scales} dict; `self.pipe.load_fp8_scales(d)` restores a stored one."""
        with self.pipe.eager_lock:
            src, ctl = self._canny_device(image, canny_low_threshold, canny_high_threshold, size=(1024, 1024))
        return self.pipe.calibrate_fp8(prompt=prompt, image=src, control_image=ctl, margin=margin, negative_prompt=negative_prompt, strength=strength,
                                       num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                       controlnet_conditioning_scale=controlnet_conditioning_scale,
                                       generator=torch.Generator(device=self.device).manual_seed(seed))

    def set_in_flight(self, n):
        """[additive] allow `n` edits in flight on this GPU: edit() may then be called from up to n worker threads (see
        `worker_slot`); each thread replays its own hipGraph slot on its own stream.  Measured on MI355X: 2 in flight =
        +17 % images/s (the 32x32-latent kernels of one edit leave CUs idle that the other edit fills)."""
        self.in_flight = max(1, int(n))
        if self.in_flight > 1:
            self.pipe.use_graph = True

    def calibrate_in_flight(self, image, prompt, **edit_kwargs):
        """[additive] after set_in_flight(n): make sure the n slot streams really overlap on this GPU.  Which hardware queue a
        stream gets depends on the order of stream creation in the process; when two slots share a queue the edits serialise
        and the in-flight gain is lost.  Prepares one job per slot from (image, prompt), times concurrent replays on the current
        slot streams and on a few freshly drawn sets, and keeps the fastest (HipImg2ImgPipeline.calibrate_streams)."""
        if self.in_flight <= 1:
            return
        kw = dict(strength=0.80, num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5,
                  canny_low_threshold=100, canny_high_threshold=200)
        kw.update(edit_kwargs)
        seed = kw.pop("seed", None)
        lo, hi = kw.pop("canny_low_threshold"), kw.pop("canny_high_threshold")
        kw.pop("negative_prompt", None)
        with self.pipe.eager_lock:
            src, ctl = self._canny_device(image, lo, hi, size=(1024, 1024))
            jobs = [self.pipe.prepare(prompt, "", src, ctl, kw["strength"], kw["num_inference_steps"], kw["guidance_scale"],
                                      kw["controlnet_conditioning_scale"],
                                      torch.Generator(device="cpu").manual_seed(seed if seed is not None else 0))
                    for _ in range(self.in_flight)]
            streams = self.pipe.calibrate_streams(jobs, [self.pipe.slot_stream(i) for i in range(self.in_flight)], tries=6)
            for i, st in enumerate(streams):
                self.pipe._slot_streams[i] = st

    def worker_slot(self, slot):
        """Bind the calling thread to graph slot `slot` (0 <= slot < in_flight)."""
        self._tls.slot = int(slot)

    def clear_memory(self):
        if self.device == "cuda":
            torch.cuda.empty_cache()

    def get_memory_usage(self):
        if self.device == "cuda":
            gb = 1024 ** 3
            return {"allocated_gb": torch.cuda.memory_allocated() / gb, "reserved_gb": torch.cuda.memory_reserved() / gb}
        return {"allocated_gb": 0, "reserved_gb": 0}
