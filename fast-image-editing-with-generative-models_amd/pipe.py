"""The object `FastEditor` stores in ``self.pipe``: same call signature as the diffusers
StableDiffusionXLControlNetImg2ImgPipeline call at /root/reference/src/pipeline.py:261-272, but every stage
(CLIP text, VAE encode, ControlNet + UNet evaluations, CFG + LCM step, VAE decode, pixel conversion) runs in the
hand-written HIP kernels of csrc/ (call order: SURVEY.md 3.2 steps 1-9)."""
import gc
import itertools
import os
import threading
import types

import numpy as np
import torch
from PIL import Image

from . import cabi, hip
from . import control as hctl
from . import emphasis as hemph
from . import mask as hmask
from .clip import ClipText, eos_positions
from .lcm import LCMSchedule
from .nn import ControlNet, UNet, passed_through
from .presets import LCM_SCHED
from .tokenizer import StandInTokenizer
from .vae import VAE

F16 = torch.float16
_PIPE_SEQ = itertools.count()


class DeviceOutput:
    """What an `after_device` hook returns when the work it queued REPLACES the image the call returns: `out` (a u8 device tensor, or a list of
    them -- one per image of a batch call, of any sizes) goes to the host instead of the edit-size result, `extra` comes back as `.extra`."""
    __slots__ = ("out", "extra")

    def __init__(self, out, extra=None):
        self.out, self.extra = out, extra


class MaskLevels:
    """A soft mask at the edit size as the pair its readers take: `levels` u8 [H, W], what the latent step reads through
    fie_mask_levels_u8, and `support` u8 [H, W], what every other reader of a mask reads by its own rule.  A caller that resizes a level map
    resizes the two separately (FastEditor); passed as `mask_image` with mask_mode="levels"."""
    __slots__ = ("support", "levels")

    def __init__(self, support, levels):
        self.support, self.levels = support, levels


def _latent_prep(ctx, job, moments, noises, first_step, latents, rows, z0, image, sf):
    """The latent prep of one image (or sweep variant) of `job`: plain; with a mask the one that keeps z0; with a latent
    content mode (section 14) that one and the mode's select.  noises: (posterior draw, init noise); rows: the image's model_in rows; image: its
    place among the job's masks."""
    head = (moments, noises[0], noises[1], latents.shape[0], sf, first_step["sqrt_ab"], first_step["sqrt_1mab"], latents, rows)
    if job.get("mask_lat") is None:
        ctx.latent_prep(*head)
    elif job.get("content_lat") is None:
        ctx.latent_prep_src(*head, z0)
    else:
        ctx.latent_prep_src_content(*head, z0, job["content_lat"][image], job["content"])


def _lcm_step(ctx, job, eps_rows, st, z, noise_init, latents, rows, decode_row, z0, image, sf):
    """The LCM step `st` of one image (or sweep variant) of `job`: plain; with a mask the one that blends towards z0 at the step's noise level;
    with a soft mask the one that compares the latent levels with the step's place st["index"] among st["count"]."""
    head = (eps_rows, job["nb"], job["guidance"], latents, z, latents.shape[0], st["sqrt_ab"], st["sqrt_1mab"], st["c_skip"], st["c_out"],
            st["sqrt_ab_prev"], st["sqrt_1mab_prev"], rows, 1.0 / sf, decode_row)
    if job.get("mask_lat") is None:
        ctx.lcm_step(*head)
    elif job.get("lvl_lat") is None:
        ctx.lcm_step_masked(*head, job["mask_lat"][image], z0, noise_init)
    else:
        ctx.lcm_step_levels(*head, job["lvl_lat"][image], z0, noise_init, st["count"], st["index"])


class HipImg2ImgPipeline:
    # [additive] Prompt emphasis: None (off: prompts are tokenised as they are), or the weight in [0, 8] of the words a prompt
    # marks with [...]; `(words:1.3)` then carries its own.  Read on the host when a job is prepared (FastEditor.set_prompt_emphasis sets it).
    prompt_emphasis = None
    # [additive] Control weights: None (off: the ControlNet's residuals are added at `controlnet_conditioning_scale`, at
    # every step, everywhere), or a fie_amd/control.py Setting (layers, steps, in_mask) as check() returns it.  Read on the host when a job is
    # prepared (FastEditor.set_control_weights sets it).
    control_weights = None

    def __init__(self, ctx, cfgs, sds, tokenizers=None, sched_cfg=None, noise_dtype=None, weight_dtype="f16"):
        """cfgs / sds: dicts with keys unet, controlnet, vae, clip_l, clip_g (configs / diffusers-named state dicts).
        weight_dtype "f8e4m3" (BASELINE config 5): the Linear / conv weights of the UNet and the ControlNet are stored as fp8 e4m3
        with per-output-channel scales (csrc/gemm_w8.hip); the 1280-wide 3x3 convs, VAE, text encoders, embedding MLPs and the few convs
        the LDS-DMA kernels cannot address (Cin % 64 != 0) stay fp16.  ACTIVATIONS: the transformer-block projections and the resnet convs read e4m3
        written by LayerNorm / attention / the GEGLU epilogue / GroupNorm (value / s, saturating at +-448, NaN kept) and run the block-scaled fp8
        MFMA (csrc/gemm_x8.hip) with s folded into the weight scale; every other fp8-weight GEMM / conv rounds its fp16 activations to e4m3 per
        fragment in registers.  So this configuration is W8A8 (not "fp8 weights only").  The per-tensor scales s are 1 until calibrate_fp8() has
        measured them on one edit (powers of two; load_fp8_scales() takes a stored set): on real checkpoints, activations beyond +-448 clip
        without that step.  Parity: SSIM vs the fp16 pipeline and an evaluation against the oracle on the dequantised weights
        (tests/test_fp8_gpu.py, tests/test_sdxl_gpu.py)."""
        if weight_dtype not in ("f16", "f8e4m3"):
            raise ValueError(f"weight_dtype {weight_dtype!r}: 'f16' or 'f8e4m3'")
        if weight_dtype != "f16" and ctx.f32:
            raise ValueError("fp8 weights belong to the fp16 path")
        self.ctx, self.cfgs, self.weight_dtype = ctx, cfgs, weight_dtype
        ctx.w8 = weight_dtype == "f8e4m3"
        try:
            self.unet = UNet(ctx, cfgs["unet"], sds["unet"])
            self.controlnet = ControlNet(ctx, cfgs["controlnet"], sds["controlnet"])
        finally:
            ctx.w8 = False
        self.vae = VAE(ctx, cfgs["vae"], sds["vae"])
        self.clip_l = ClipText(ctx, cfgs["clip_l"], sds["clip_l"])
        self.clip_g = ClipText(ctx, cfgs["clip_g"], sds["clip_g"])
        # The VAE and the two text encoders run through the C++ graph walks of the library (include/fie.h: fie_vae_encode_f16, fie_vae_decode_f16,
        # fie_clip_text_forward_f16; csrc/graphs.cpp) -- bit-identical to the Python walks of vae.py / clip.py (tests/test_cabi_graphs_gpu.py), which stay as
        # the weight packers and the A/B (FIE_CPP_WALKS=0).  Weights are registered under a prefix of this pipeline's own: contexts are shared.
        self.weight_prefix = f"pipe{next(_PIPE_SEQ)}."
        self.cpp_walks = (not ctx.f32) and ctx.device.type == "cuda" and os.environ.get("FIE_CPP_WALKS", "1") != "0"
        if self.cpp_walks:
            cabi.register_vae(self.vae, self.weight_prefix)
            cabi.register_clip(self.clip_l, self.weight_prefix + "text_encoder.")
            cabi.register_clip(self.clip_g, self.weight_prefix + "text_encoder_2.")
        self.tok_l, self.tok_g = tokenizers or (StandInTokenizer(cfgs["clip_l"]["pad_token_id"]),
                                                StandInTokenizer(cfgs["clip_g"]["pad_token_id"]))
        self.scheduler = LCMSchedule(**(sched_cfg or LCM_SCHED))
        self.noise_dtype = noise_dtype or ctx.dtype        # upstream randn_tensor draws in the pipeline dtype
        self.progress = {}
        self.last_stats = {}
        self.timing = None         # set to [] to collect per-stage HIP-event timings in run_device()
        self.use_graph = os.environ.get("FIE_NO_GRAPH", "0") != "1"
        # GEMM / conv tile selection by measurement: the eager warm-up in front of every capture meets each shape once
        # (include/fie.h: fie_gemm_autotune); FIE_AUTOTUNE=0 keeps the built-in rule
        self.autotune = ctx.device.type == "cuda" and os.environ.get("FIE_AUTOTUNE", "1") != "0"
        ctx.autotune(2 if self.autotune else 0)     # shapes are tuned during the eager warm-up of a capture only (_capture)
        # hipGraph cache, bounded: key = (size, CFG batch, step plan, guidance, control scale, slot, images); at most MAX_GRAPHS
        # keys are captured (insertion-ordered dict, least recently used first); a key beyond the cap runs EAGERLY instead of
        # evicting -- destroying a graph and capturing another one was measured to give a slow graph (121 vs 81 ms), and a
        # parameter sweep must not grow HBM without bound.  All graphs of a slot share one capture memory pool (a slot
        # replays one graph at a time and its output is consumed before the next replay), so k keys cost one pool, not k.
        self._graphs = {}
        self._pools = {}
        self.max_graphs = int(os.environ.get("FIE_MAX_GRAPHS", "12"))
        self.eager_overflow = 0     # calls served eagerly because the cache was full
        self._job_consts = {}       # (size, CFG batch, step plan) -> device tensors every job of that shape shares (time ids, timesteps)
        self.repeated_jobs = 0      # device jobs run a second time because a post_check said their inputs had changed (see __call__)
        self._side = None
        self._slot_streams = {}
        self._n_forked = 0
        self._fork_override = None
        self._host_out = {}
        self.eager_lock = threading.RLock()
        self.fork_streams = os.environ.get("FIE_NO_FORK", "0") != "1"
        # Which hardware queue a stream lands on depends on the order in which streams are first used, and two edits in flight
        # only overlap when their streams (and their graphs' branch streams) sit on different queues: creating the slot streams
        # HERE, before any graph, was measured to lose the whole in-flight gain (12.5 instead of 14.4 images/s).  They are
        # created lazily instead, and calibrate_streams() below re-draws streams when a measured pair does not overlap.
        if ctx.device.type == "cuda" and os.environ.get("FIE_EAGER_STREAMS") == "1":    # reproducer of a bad queue mapping (tests of calibrate_streams)
            warm = [self.slot_stream(0), self.slot_stream(1)] + ([self._side_stream()] if self.fork_streams else [])
            for st in warm:
                with torch.cuda.stream(st):
                    torch.zeros(1, device=ctx.device)
            torch.cuda.synchronize(ctx.device)

    def __del__(self):
        try:                       # the registry holds raw pointers into this pipeline's weight tensors: forget them with the pipeline
            if getattr(self, "cpp_walks", False) and self.ctx.h:
                hip.lib().fie_weights_clear_prefix(self.ctx.h, self.weight_prefix.encode())
        except Exception:
            pass

    # -- diffusers API surface the reference touches
    def set_progress_bar_config(self, **kw):          # run_batch.py:157-158
        self.progress.update(kw)

    def _randn(self, shape, generator):
        """diffusers utils/torch_utils.py::randn_tensor: a CPU generator draws on the host and the result is moved;
        a device generator draws on the device.  Drawn in `noise_dtype` (the pipeline dtype upstream)."""
        gdev = generator.device.type if generator is not None else self.ctx.device.type
        if gdev == "cpu":
            x = torch.randn(shape, generator=generator, device="cpu", dtype=self.noise_dtype).to(self.ctx.device)
        else:
            x = torch.randn(shape, generator=generator, device=self.ctx.device, dtype=self.noise_dtype)
        return x.float().contiguous()

    def encode_prompt(self, texts):
        """texts: list of strings -> ([len*77, Dl+Dg] f16, pooled [len, P] f16)."""
        pl, _ = self.clip_l(self.tok_l(texts))
        pg, pooled = self.clip_g(self.tok_g(texts))
        return torch.cat([pl, pg], dim=1), pooled

    def prepare(self, prompt, negative_prompt="", image=None, control_image=None, strength=0.8,
                num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5, generator=None,
                mask_image=None, mask_blur=0, paste_back=True, *, masked_content="original", blend="alpha", blend_levels=4, paste_later=False,
                mask_grow=0, mask_mode="binary", mask_ramp=0):
        """`image` / `control_image`: PIL images, or u8 [H, W, 3] tensors already on the device (FastEditor.edit keeps the
        resized source and its device-side Canny map in HBM instead of bouncing them through PIL).  `mask_image` (additive, diffusers'
        name): restricts the edit to its white region -- a PIL image, a uint8 / bool [H, W] array, or a u8 [H, W]
        device tensor, at the image's size; `mask_blur` feathers and `paste_back` (default) enables the paste-back of the source.
        `masked_content` (additive; needs a mask): what the model starts from inside the mask -- "original" the source, "fill" a smooth
        continuation of the surroundings, "latent_noise" pure noise, "latent_nothing" the zero latent plus noise.
        `blend` (additive; needs a mask and the paste-back): "alpha" the paste-back as ever, "multiband" the one-sided multi-band blend over
        `blend_levels` (1..6) pyramid levels -- the decoded image's low-frequency difference to the source fades out towards the seam, outside the
        mask the output stays the source's bytes.  `paste_later`: the caller composites the result itself behind the job
        (FastEditor's source-size back end): a "multiband" job with paste_back=False then returns the blended image B uncomposited.
        `mask_grow` (additive; a non-zero value needs a mask): the mask grown (> 0) or shrunk (< 0) by the exact Euclidean disk of that many of its
        pixels, -64 .. 64, on the device before anything else reads it: the call equals the one with the grown mask passed in (DESIGN.md section
        16).  0 launches nothing and passes the mask on as it is.
        `mask_mode` / `mask_ramp` (additive; both need a mask): a soft mask.  "levels" reads the mask's greys as a
        per-pixel strength V: a latent pixel of level v is held on the source's trajectory and released into the edit for the last
        (v K + 254) // 255 of the edit's K steps -- 255 is edited as a binary mask's white, 0 never; everything else that reads a mask (the
        paste-back and its feather, `masked_content`, `blend`) reads the support 255 (V > 0) in its place.  `mask_ramp` = r in 1..64 builds V
        from the binary mask's outline on the device (after `mask_grow`): 0 outside, floor(255 d / r) up to 255 inside, d the distance to the
        nearest pixel outside the mask, in pixels of the mask as passed.  The two do not combine, nor does "levels" with `mask_grow`.  A
        `MaskLevels(support, levels)` pair of u8 [H, W] device tensors is taken as it is (FastEditor resizes the two separately)."""
        spec = hmask.MaskSpec.check(mask_blur, paste_back, masked_content, blend, blend_levels, mask_grow, mask_mode, mask_ramp,
                                    have_mask=mask_image is not None, paste_later=paste_later)
        return self._prepare(prompt, negative_prompt, image, control_image, strength, num_inference_steps, guidance_scale,
                             controlnet_conditioning_scale, generator, mask_image, spec)

    def _mask_job(self, mask_image, spec, h, w, ctl_a=None):
        """Mask tensors of one image under its MaskSpec: (mask_lat u8 [1, h/8 * w/8], mask_px f32 [1, h, w] or None without paste-back, the
        edit-size L mask u8 [1, h, w], lvl_lat u8 [1, h/8 * w/8] or None), made on the device on the current stream, in front of the job:
        the optional grow (fie_mask_grow_u8), a soft mask's level map V -- the mask itself ("levels"), fie_mask_ramp_u8 of the grown mask, or a
        MaskLevels pair's -- and its support, which is the L mask returned, then fie_mask_prep on that; lvl_lat holds V's latent levels
        (fie_mask_levels_u8), which the latent step alone reads (DESIGN.md sections 8, 16, 21).  `ctl_a`: None, or the integer of the control
        weights' `in_mask`: a fifth entry then holds the weights of every latent position of every pyramid level, f32
        [1, P_tot], made by fie_control_pyramid_u8 from the level map, or from the L mask behind the grow."""
        if mask_image is None:
            return (None,) * (4 if ctl_a is None else 5)
        pair = isinstance(mask_image, MaskLevels)         # support and levels as the caller resized them: nothing to grow, ramp or derive
        if pair:
            if spec.mode != "levels":
                raise ValueError("a MaskLevels pair is a level map: it needs mask_mode='levels'")
            for t in (mask_image.support, mask_image.levels):
                if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != (h, w):
                    raise ValueError(f"a MaskLevels pair holds two u8 [{h}, {w}] tensors")
            lm, lv = (t.to(self.ctx.device).contiguous() for t in (mask_image.support, mask_image.levels))
        elif torch.is_tensor(mask_image):
            if mask_image.dim() != 2 or mask_image.dtype != torch.uint8:
                raise ValueError("a mask tensor must be u8 [H, W]")
            if tuple(mask_image.shape) != (h, w):
                raise ValueError(f"mask size {(mask_image.shape[1], mask_image.shape[0])} differs from the image size {(w, h)}")
            lm = mask_image.to(self.ctx.device).contiguous()
        else:
            lm = torch.from_numpy(hmask.to_l_array(mask_image, (w, h))).to(self.ctx.device)
        with self.eager_lock:                             # the context's stream binding is shared by the threads of in-flight edits
            if spec.grow:
                lm = self.ctx.mask_grow(lm, spec.grow)
            if not pair:
                lv = self.ctx.mask_ramp(lm, spec.ramp) if spec.ramp else lm if spec.mode == "levels" else None
                if lv is not None:
                    lm = self.ctx.mask_support(lv)
            m_px, m_lat = self.ctx.mask_prep(lm, spec.blur)
            lvl = self.ctx.mask_levels(lv, m_lat) if lv is not None else None
            if ctl_a is not None:                         # after grow and ramp: the control map moves with the mask
                ctl_w = self.ctx.control_pyramid(lm if lv is None else lv, ctl_a, binary=lv is None, levels=self._ctl_levels())
        out = m_lat[None], (m_px[None] if spec.paste_back else None), lm[None], None if lvl is None else lvl[None]
        return out if ctl_a is None else out + (ctl_w[None],)

    def _ctl_levels(self):
        """The pyramid levels of the ControlNet's residuals; more than the weight pyramid has is a ValueError."""
        levels = max(self.controlnet.residual_levels()) + 1
        if levels > hctl.MAX_LEVELS:
            raise ValueError(f"control weights: `in_mask` serves ControlNets of up to {hctl.MAX_LEVELS} resolution levels, this one has {levels}")
        return levels

    def _ctl_job(self, cn_scale, steps, ctl_w=None):
        """The job entries of the control weights; none with the setting at None, whose job is what it was.  ctl_layers: the
        scale of every residual; ctl_keep: whether each loop step runs the ControlNet (no step does when every scale is 0); ctl_w: with `in_mask`
        and a mask, the weights of the latent positions, f32 [1, P_tot]."""
        ctl = self.control_weights
        if ctl is None:
            return {}
        scales = hctl.layer_scales(cn_scale, ctl.layers, self.controlnet.n_out)
        live = any(s != 0 for s in scales)
        out = dict(ctl_layers=scales, ctl_keep=tuple(k and live for k in hctl.keep(len(steps), ctl.steps)))
        if ctl_w is not None:
            out["ctl_w"] = ctl_w
        return out

    def _prepare(self, prompt, negative_prompt, image, control_image, strength, num_inference_steps, guidance_scale,
                 controlnet_conditioning_scale, generator, mask_image, spec):
        """Host side of one call: image and size checks, tokenisation, RNG draws (in upstream order: posterior sample, init
        noise, one per non-final step) and the H2D copies.  `spec`: the call's checked MaskSpec.  Returns the device-resident job for
        run_device()."""
        ctx = self.ctx
        if image is None or control_image is None:
            raise ValueError("`image` and `control_image` are both required")
        if strength < 0 or strength > 1:
            raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        size_of = lambda im: (im.shape[1], im.shape[0]) if torch.is_tensor(im) else im.size
        if size_of(image) != size_of(control_image):
            raise ValueError("image and control_image must have the same size")
        w, h = size_of(image)
        if h % 8 or w % 8:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {h} and {w}.")
        ctl, ctl_w = self.control_weights, None
        if ctl is not None and ctl.in_mask is not None and mask_image is not None:     # `in_mask` without a mask has nothing to weigh: the scalar job
            mask_lat, mask_px, mask_l, lvl_lat, ctl_w = self._mask_job(mask_image, spec, h, w, hctl.mask_a(ctl.in_mask))
        else:
            mask_lat, mask_px, mask_l, lvl_lat = self._mask_job(mask_image, spec, h, w)
        steps = self.scheduler.plan(num_inference_steps, strength)
        if not steps:
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of "
                             f"pipeline steps is 0 which is < 1 and not appropriate for this pipeline.")
        do_cfg = guidance_scale > 1.0
        dev = ctx.device
        texts = [negative_prompt or "", prompt] if do_cfg else [prompt]
        lh, lw = h // 8, w // 8
        u8 = lambda im: im.to(dev).contiguous() if torch.is_tensor(im) else torch.from_numpy(np.array(im.convert("RGB"))).to(dev)
        n_noise = 2 + sum(1 for st in steps if not st["last"])
        nb = 2 if do_cfg else 1
        # prompt emphasis: None reads no marks -- the prompts go to the tokenizers as they are; a setting tokenises the
        # prompts with their marks stripped and gives every text row a weight, `emph` f32 [nb * 77], or None when all of them are 1
        emph = None
        if self.prompt_emphasis is None:
            ids_g, ids_l = self.tok_g(texts), self.tok_l(texts)
        else:
            setting = hemph.check(self.prompt_emphasis)
            (ids_g, w_g), (ids_l, w_l) = self.tok_g.weighted(texts, setting), self.tok_l.weighted(texts, setting)
            if not np.array_equal(w_g, w_l):          # one weight per text row serves the concatenated embedding: both encoders tokenise alike
                raise ValueError("prompt emphasis: the two tokenizers split the prompt differently")
            emph = hemph.row_weights(w_l)
        eos = eos_positions(ids_g, self.cfgs["clip_g"]["eos_token_id"])                 # pooled-token column per row
        # the three prompt-dependent int32 tensors travel in ONE host-to-device copy (each pageable copy is a host-synchronous ~40 us); what depends on
        # the size and the step plan only (time ids, timesteps) is uploaded once per (size, plan) and shared by every later job
        ids_l = ids_l.to(torch.int32)
        ids_g32 = ids_g.to(torch.int32)
        eos_rows = (torch.arange(nb) * ids_g.shape[1] + eos).to(torch.int32)
        parts = [ids_l.reshape(-1), ids_g32.reshape(-1), eos_rows.reshape(-1)]
        if emph is not None:                              # the weights ride in the same copy, bit-cast
            parts.append(torch.from_numpy(emph.view(np.int32)))
        packed = torch.cat(parts).to(dev)
        n_l, n_g = ids_l.numel(), ids_g32.numel()
        ckey = (h, w, nb, tuple(float(st["t"]) for st in steps), str(dev))
        const = self._job_consts.get(ckey)
        if const is None:
            if len(self._job_consts) > 64:
                self._job_consts.clear()
            const = self._job_consts[ckey] = (torch.tensor([[h, w, 0, 0, h, w]], dtype=torch.float32).repeat(nb, 1).to(dev),
                                              [torch.full((nb, 1), float(st["t"]), dtype=torch.float32).to(dev) for st in steps])
        return dict(
            ids_l=packed[:n_l].view(ids_l.shape), ids_g=packed[n_l:n_l + n_g].view(ids_g32.shape), eos_rows=packed[n_l + n_g:n_l + n_g + nb],
            **({} if emph is None else dict(emph=packed[n_l + n_g + nb:].view(torch.float32))),     # none: the job is what it was
            img_u8=u8(image), ctl_u8=u8(control_image), hw=(h, w), steps=steps, nb=nb,
            guidance=float(guidance_scale), cn_scale=float(controlnet_conditioning_scale),
            time_ids=const[0], t_dev=const[1],
            noises=[self._randn((1, 4, lh, lw), generator) for _ in range(n_noise)],
            mask_lat=mask_lat, mask_px=mask_px, mask_cfg=None if mask_lat is None else (spec.blur, spec.paste_back),
            **({} if lvl_lat is None else dict(lvl_lat=lvl_lat)),         # a soft mask's latent levels; none: the job is what it was
            **self._content_job(spec, mask_l, mask_lat), **self._blend_job(spec, mask_l),
            **self._ctl_job(controlnet_conditioning_scale, steps, ctl_w))   # control weights; none: the job is what it was

    @staticmethod
    def _blend_job(spec, blend_l):
        """The job entries of blend="multiband" (DESIGN.md section 15); none with "alpha", whose job is what it was.  `blend_l`: the edit-size L
        mask u8 [1, h, w] that the blend reads inside the device job -- the image's own mask, or all 255 for an image of a batch that has none
        (everything is inside: the blend returns the decoded bytes)."""
        return {} if spec.blend == "alpha" else dict(blend=(spec.blend, spec.blend_levels), blend_l=blend_l)

    @staticmethod
    def _content_job(spec, mask_l, content_lat):
        """The job entries of a masked-content mode; none with "original", whose job is what it was.  `mask_l`: the edit-size
        L mask u8 [1, h, w], read inside the device job by the fill and the edge-map clear; `content_lat`: u8 [1, h/8 * w/8], where the latent
        modes replace the initial latents -- the image's mask_lat, or zeros for an image of a batch that has no mask of its own."""
        content = spec.content
        if content == "original":
            return {}
        out = dict(content=content, mask_l=mask_l)
        if content in ("latent_noise", "latent_nothing"):
            out["content_lat"] = content_lat
        return out

    def prepare_batch(self, prompts, negative_prompts, images, control_images, strength=0.8, num_inference_steps=4,
                      guidance_scale=1.5, controlnet_conditioning_scale=0.5, generators=None, mask_image=None, mask_blur=0,
                      paste_back=True, *, masked_content="original", blend="alpha", blend_levels=4, paste_later=False, mask_grow=0,
                      mask_mode="binary", mask_ramp=0):
        """[additive] n independent edits as ONE device job (BASELINE config "batch=8"): the UNet / ControlNet / CLIP run
        at batch n * nb, the VAE per image.  Rows are image-major ([img0 uncond, img0 cond, img1 uncond, ...]); each
        image keeps its own generator, so image i of a batch draws exactly the noise a single call with that generator
        draws (upstream: a list of generators, one per prompt).  `mask_image`: None, or one mask per image (None in the
        list = edit everywhere).  `masked_content`: one mode for the call (prepare()); an image without a mask is edited as ever.  `blend` / `blend_levels` /
        `paste_later`: prepare()'s, one value for the call; an image without a mask comes out as without the keyword.  `mask_grow`: prepare()'s, one
        radius for the call; an image without a mask is untouched.  `mask_mode` / `mask_ramp`: prepare()'s, one value for the call; an image without a
        mask is untouched (its latent levels are 255 everywhere)."""
        n = len(prompts)
        masks = list(mask_image) if mask_image is not None else [None] * n
        masked = any(m is not None for m in masks)
        spec = hmask.MaskSpec.check(mask_blur, paste_back, masked_content, blend, blend_levels, mask_grow, mask_mode, mask_ramp,
                                    have_mask=masked, paste_later=paste_later)
        if not (n == len(images) == len(control_images)) or n == 0:
            raise ValueError("prompts, images and control_images must be non-empty lists of one length")
        if len(masks) != n:
            raise ValueError(f"{len(masks)} masks for {n} images: one mask (or None) per image")
        negative_prompts = negative_prompts or [""] * n
        generators = generators or [None] * n
        jobs = [self._prepare(prompts[i], negative_prompts[i], images[i], control_images[i], strength, num_inference_steps,
                              guidance_scale, controlnet_conditioning_scale, generators[i], masks[i],
                              spec if masks[i] is not None else spec.unmasked()) for i in range(n)]
        if any(j["hw"] != jobs[0]["hw"] for j in jobs):
            raise ValueError("all images of a batch must have one size")
        if masked:                                        # an image without a mask edits everywhere: an all-ones mask
            h, w = jobs[0]["hw"]
            for j in jobs:
                if j["mask_lat"] is None:
                    j["mask_lat"] = torch.ones((1, (h // 8) * (w // 8)), device=self.ctx.device, dtype=torch.uint8)
                    j["mask_px"] = torch.ones((1, h, w), device=self.ctx.device, dtype=torch.float32) if spec.paste_back else None
                    j["mask_cfg"] = (spec.blur, spec.paste_back)
                    if spec.soft:
                        j["lvl_lat"] = torch.full((1, (h // 8) * (w // 8)), 255, device=self.ctx.device, dtype=torch.uint8)
                    # no mask of its own: an empty hole -- nothing filled, no edge cleared, no latent replaced
                    j.update(self._content_job(spec, torch.zeros((1, h, w), device=self.ctx.device, dtype=torch.uint8),
                                               torch.zeros((1, (h // 8) * (w // 8)), device=self.ctx.device, dtype=torch.uint8)))
                    j.update(self._blend_job(spec, torch.full((1, h, w), 255, device=self.ctx.device, dtype=torch.uint8)))
        if n == 1:
            return jobs[0]                                # the single-image job (and its graph)
        nb, t77 = jobs[0]["nb"], jobs[0]["ids_g"].shape[1]
        job = dict(jobs[0])
        job["n"] = n
        for k in ("ids_l", "ids_g", "time_ids"):
            job[k] = torch.cat([j[k] for j in jobs], dim=0)
        job["eos_rows"] = torch.cat([j["eos_rows"] + i * nb * t77 for i, j in enumerate(jobs)])
        if any(j.get("emph") is not None for j in jobs):  # prompt emphasis: every image its own weights; an image without a weighted token has ones
            ones = torch.ones(nb * t77, device=self.ctx.device, dtype=torch.float32)
            job["emph"] = torch.cat([j["emph"] if j.get("emph") is not None else ones for j in jobs])
        if any(j.get("ctl_w") is not None for j in jobs):  # control weights: every image its own mask's; an image without a mask has ones
            ones = torch.ones_like(next(j["ctl_w"] for j in jobs if j.get("ctl_w") is not None))
            job["ctl_w"] = torch.cat([j["ctl_w"] if j.get("ctl_w") is not None else ones for j in jobs])
        job["img_u8"] = torch.stack([j["img_u8"] for j in jobs])
        job["ctl_u8"] = torch.stack([j["ctl_u8"] for j in jobs])
        job["t_dev"] = [t.repeat(n, 1) for t in jobs[0]["t_dev"]]
        job["noises"] = [z for j in jobs for z in j["noises"]]          # image-major: image i owns [i*k, (i+1)*k)
        for k in self._MASK_KEYS:
            if job.get(k) is not None:
                job[k] = torch.cat([j[k] for j in jobs], dim=0)
        return job

    def prepare_sweep(self, prompt, negative_prompt="", image=None, control_image=None, strengths="all", num_inference_steps=4,
                      guidance_scale=1.5, controlnet_conditioning_scale=0.5, generator=None, mask_image=None, mask_blur=0, paste_back=True, *,
                      masked_content="original", blend="alpha", blend_levels=4, paste_later=False, mask_grow=0, mask_mode="binary", mask_ramp=0):
        """[additive] A strength sweep as ONE device job: one image, one prompt pair, and the k variants of
        fie_amd/sweep.py: variants(num_inference_steps, strengths) as the k "images" of the job, strongest first.  Everything that does not depend
        on the strength runs once (tokenisation, both text encoders, the mask preparation, the fill, the VAE encode, the edge-map embedding); the
        UNet and the ControlNet run each loop step on the rows of the variants that have joined the loop by then -- a leading slice, rows being
        image-major as in prepare_batch().  One generator: variant i consumes the noise a single call with that generator and strength draws (its
        stream is a prefix of the longest variant's).  A soft mask's level map is shared: its support does not depend on the step count, and every
        variant releases a level by its own K.  The other arguments are prepare()'s.  A sweep of ONE variant is the single-image job.
        Control weights: `layers` and `in_mask` work, every variant reading the image's one weight vector; a `steps`
        window is a ValueError here -- the variants share their loop steps, and diffusers' rule counts each variant's own."""
        if self.control_weights is not None and self.control_weights.steps is not None:
            raise ValueError(f"control weights: steps={self.control_weights.steps} does not combine with a strength sweep (the variants share "
                             "their loop steps, the window counts each variant's own)")
        spec = hmask.MaskSpec.check(mask_blur, paste_back, masked_content, blend, blend_levels, mask_grow, mask_mode, mask_ramp,
                                    have_mask=mask_image is not None, paste_later=paste_later)
        from . import sweep as hsweep
        vs = hsweep.variants(num_inference_steps, strengths)
        job = self._prepare(prompt, negative_prompt, image, control_image, vs[0][1][0], num_inference_steps, guidance_scale,
                            controlnet_conditioning_scale, generator, mask_image, spec)
        if len(vs) == 1:
            return job                                    # the single-image job (and its graph)
        plans = [self.scheduler.plan(num_inference_steps, v[1][0]) for v in vs]
        assert [len(p) for p in plans] == [m for m, _ in vs] and plans[0] == job["steps"] and len(job["noises"]) == hsweep.noise_count(plans)
        job["sweep"] = tuple(m for m, _ in vs)
        job["plans"] = plans
        job["sched"] = hsweep.schedule(plans)
        job["t_dev"] = [t.repeat(len(row), 1) for t, row in zip(job["t_dev"], job["sched"])]       # one timestep for the rows active at that step
        return job

    def _side_stream(self):
        """Second stream for the independent branches of one edit (CLIP beside the VAE encode, UNet encoder beside the
        ControlNet trunk).  `fork_streams = False` keeps the whole edit on one stream.  Overlap between the branches
        (and between edits in flight) needs the streams to land on different hardware queues: see GPU_MAX_HW_QUEUES in
        fie_amd.py."""
        if not (self.fork_streams if self._fork_override is None else self._fork_override):
            return torch.cuda.current_stream(self.ctx.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.ctx.device)
        return self._side

    def _mark(self, name):
        self.ctx.oplog_mark(name)
        if self.timing is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.timing.append((name, ev))

    @torch.no_grad()
    def run_device(self, job):
        """Device side: everything between the H2D and D2H copies.  Returns the u8 HWC image on the device."""
        if job.get("sweep"):                              # a strength sweep's ragged job (prepare_sweep)
            return self._run_sweep(job)
        ctx, dev = self.ctx, self.ctx.device
        h, w = job["hw"]
        nb, steps = job["nb"], job["steps"]
        lh, lw = h // 8, w // 8
        hw = lh * lw
        self._mark("start")
        main = torch.cuda.current_stream(dev)
        side = self._side_stream()
        # 1-2. text encoders (negative prompt "" is really encoded: SURVEY 0 item 4).  Independent of the VAE encode:
        # issued on a second HIP stream so the latency-bound 77-token GEMMs hide under the VAE's large convs.
        n = job.get("n", 1)                               # images in this job (prepare_batch); rows are image-major
        imgs = job["img_u8"] if n > 1 else job["img_u8"][None]
        ctls = job["ctl_u8"] if n > 1 else job["ctl_u8"][None]
        srcs = imgs                                       # what the VAE encodes; `imgs` keeps feeding the composites
        content = job.get("content")                      # a masked-content mode other than "original" 
        if content is not None:
            # inside the job, on the main stream in front of the fork: a replay (and a job repeated on a finished edge map) recomputes the filled
            # source and the cleared edge map from its own buffers; the side stream's wait below orders its edge-map embedding behind them
            pre = [ctx.mask_fill(imgs[i], job["mask_l"][i], ctls[i], fill=content == "fill") for i in range(n)]
            ctls = [c for _, c in pre]
            if content == "fill":
                srcs = [f for f, _ in pre]
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if self.cpp_walks:
                pl, _ = cabi.clip_forward(self.clip_l, self.weight_prefix + "text_encoder.", job["ids_l"])
                pg, pooled = cabi.clip_forward(self.clip_g, self.weight_prefix + "text_encoder_2.", job["ids_g"], job["eos_rows"])
            else:
                pl, _ = self.clip_l(job["ids_l"])
                pg, pooled = self.clip_g(job["ids_g"], eos_rows=job["eos_rows"])
            text = torch.cat([pl, pg], dim=1)
            # 6. per-image invariants: nothing here depends on the latents, so the whole block rides on the side stream beside the VAE
            # encode (text-time addition embeddings, the ControlNet's edge-map embedding, the first step's timestep projections)
            self.unet.begin_image(pooled, job["time_ids"], emph=job.get("emph"))       # emph: prompt emphasis, the weight of every text row
            # control weights: ctl_keep says which steps run the ControlNet; None: all of them, as ever
            ctl_s, ctl_keep = job.get("ctl_layers"), job.get("ctl_keep")
            if ctl_keep is None or any(ctl_keep):
                self.controlnet.begin_image(pooled, job["time_ids"], emph=job.get("emph"))
                # the edge-map embedding is the same for the CFG rows of an image: computed once per image, then repeated (upstream runs
                # it on the duplicated batch; the values are identical)
                conds = [ctx.pixels_in(ctls[i], False) for i in range(n)]
                cond_emb = self.controlnet.cond_embedding(conds[0] if n == 1 else torch.cat(conds, dim=0))
                if nb > 1:
                    cond_emb = cond_emb.repeat_interleave(nb, dim=0)
            tb0 = (self.unet.time_rowbias(job["t_dev"][0]), self.controlnet.time_rowbias(job["t_dev"][0]) if ctl_keep is None or ctl_keep[0] else None)
        text_len = text.shape[0] // (n * nb)
        # 3. pixels, 5. prepare_latents: VAE posterior sample (draw #1), init noise (draw #2), add_noise -- per image (the
        # 1024^2 VAE tensors of a batch would cross the 2 GiB operand limit of the buffer-load kernels, and gain nothing)
        per = len(job["noises"]) // n                     # noise tensors per image
        mask_lat, mask_px = job.get("mask_lat"), job.get("mask_px")     # a masked edit
        latents = torch.empty((n, hw, 4), device=dev, dtype=torch.float32)
        z0 = torch.empty((n, hw, 4), device=dev, dtype=torch.float32) if mask_lat is not None else None
        model_in = torch.empty((n * nb, lh, lw, 8), device=dev, dtype=ctx.dtype)
        sf = self.cfgs["vae"]["scaling_factor"]
        for i in range(n):
            x_img = ctx.pixels_in(srcs[i], True)
            moments = cabi.vae_encode(self.vae, x_img) if self.cpp_walks else self.vae.encode_moments(x_img)[0]
            _latent_prep(ctx, job, moments, job["noises"][i * per:i * per + 2], steps[0], latents[i], model_in[i * nb:(i + 1) * nb],
                         None if z0 is None else z0[i], i, sf)
        next_noise = 2
        main.wait_stream(side)
        self._mark("clip+vae_encode")
        decode_in = torch.empty((n, lh, lw, 8), device=dev, dtype=ctx.dtype)
        self._mark("cond_embed")
        # 7. denoising loop
        for k, (st, t_dev) in enumerate(zip(steps, job["t_dev"])):
            cn_on = ctl_keep is None or ctl_keep[k]       # a dropped step issues nothing of the ControlNet: no time projections, no trunk, no fork
            tb_u, tb_c = tb0 if k == 0 else (self.unet.time_rowbias(t_dev), self.controlnet.time_rowbias(t_dev) if cn_on else None)
            self._mark("embed")
            # UNet encoder and ControlNet trunk are independent until the zero-conv adds: two HIP streams, so their
            # small-grid kernels (32x32 latent level: <= 1 block per CU each) share the 256 CUs
            if cn_on:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    c_skips, c_mid = self.controlnet.encode_cond(model_in, cond_emb, tb_c, text, text_len)
            skips, mid = self.unet.encode(self.unet.conv_in(ctx, model_in), tb_u, text, text_len)
            if cn_on:
                main.wait_stream(side)
            self._mark("unet_enc+controlnet")
            if ctl_s is None:
                skips, mid = self.controlnet.add_residuals(c_skips, c_mid, job["cn_scale"], skips, mid)
            elif cn_on:
                skips, mid = self.controlnet.add_residuals_weighted(c_skips, c_mid, ctl_s, skips, mid, w=job.get("ctl_w"), rows_per_image=nb)
            else:                                         # the UNet decodes on its own skips
                skips, mid = [passed_through(s) for s in skips], passed_through(mid)
            eps = self.unet.decode(mid, skips, tb_u, text, text_len)
            self._mark("unet_dec")
            for i in range(n):
                z = None if st["last"] else job["noises"][i * per + next_noise]
                _lcm_step(ctx, job, eps[i * nb:(i + 1) * nb], st, z, job["noises"][i * per + 1], latents[i], model_in[i * nb:(i + 1) * nb],
                          decode_in[i:i + 1], None if z0 is None else z0[i], i, sf)
            next_noise += 1
            self._mark("lcm_step")
        # 8-9. decode + postprocess
        dec = (lambda z: cabi.vae_decode(self.vae, z)) if self.cpp_walks else self.vae.decode
        if job.get("blend"):                              # the one-sided multi-band paste-back: B takes the decoded image's place
            outs = [ctx.multiband_blend(ctx.pixels_out(dec(decode_in[i:i + 1])), imgs[i], job["blend_l"][i],
                                        None if mask_px is None else mask_px[i], job["blend"][1]) for i in range(n)]
        elif mask_px is None:
            outs = [ctx.pixels_out(dec(decode_in[i:i + 1])) for i in range(n)]
        else:                                             # paste-back of the source outside the (feathered) mask
            outs = [ctx.pixels_out_composite(dec(decode_in[i:i + 1]), imgs[i], mask_px[i]) for i in range(n)]
        out_u8 = outs[0] if n == 1 else torch.stack(outs)
        self._mark("vae_decode")
        self.last_stats = dict(unet_evals=len(steps), cfg_batch=nb, latent_hw=(lh, lw), images=n)
        if ctl_keep is not None:
            self.last_stats["control_steps_kept"] = sum(ctl_keep)
        self._latents = latents
        job["_result"] = dict(stats=dict(self.last_stats), latents=latents)     # what THIS job produced (graph entries keep theirs)
        if z0 is not None:
            job["_result"]["z0"] = z0                     # a masked edit's clean source latents (its blend target)
        return out_u8

    @torch.no_grad()
    def _run_sweep(self, job):
        """run_device() of a strength sweep (prepare_sweep): k variants of ONE image, variant i joining the loop at step M - m_i.  Same stages, marks
        and streams as run_device().  Once per sweep: the text encoders, begin_image, the fill, the edge-map embedding, the VAE encode.  Per variant:
        latent_prep on the one moments tensor with its own first-step scalars, lcm_step with its own step record, the decode and the paste-back.  Per
        loop step the two networks run on the leading act * nb rows.  The per-job state -- add_emb, the text and with it the text K/V caches of
        the transformer blocks, the edge-map embedding -- covers all k * nb rows from the start (the FIRST step runs the fewest rows and fills the
        caches), and a step reads their leading rows.  Returns u8 [k, h, w, 3], strongest variant first."""
        ctx, dev = self.ctx, self.ctx.device
        h, w = job["hw"]
        nb, plans, sched = job["nb"], job["plans"], job["sched"]
        k = len(plans)
        lh, lw = h // 8, w // 8
        hw = lh * lw
        self._mark("start")
        main = torch.cuda.current_stream(dev)
        side = self._side_stream()
        img, ctl = job["img_u8"], job["ctl_u8"]
        src = img                                         # what the VAE encodes; `img` keeps feeding the composites
        content = job.get("content")
        if content is not None:
            filled, ctl = ctx.mask_fill(img, job["mask_l"][0], ctl, fill=content == "fill")
            if content == "fill":
                src = filled
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if self.cpp_walks:
                pl, _ = cabi.clip_forward(self.clip_l, self.weight_prefix + "text_encoder.", job["ids_l"])
                pg, pooled = cabi.clip_forward(self.clip_g, self.weight_prefix + "text_encoder_2.", job["ids_g"], job["eos_rows"])
            else:
                pl, _ = self.clip_l(job["ids_l"])
                pg, pooled = self.clip_g(job["ids_g"], eos_rows=job["eos_rows"])
            # one prompt pair: its nb rows stand for every variant (torch copies, as the CFG repeat of the edge-map embedding is)
            text = torch.cat([pl, pg], dim=1).repeat(k, 1)
            emph = None if job.get("emph") is None else job["emph"].repeat(k)     # prompt emphasis: the one prompt pair's weights, as its text rows
            # control weights: the scales, and whether the ControlNet runs at all (a sweep has no window: every scale 0 or none)
            ctl_s, ctl_keep = job.get("ctl_layers"), job.get("ctl_keep")
            cn_on = ctl_keep is None or any(ctl_keep)
            for net in (self.unet, self.controlnet) if cn_on else (self.unet,):
                net.begin_image(pooled, job["time_ids"], emph=emph)
                net.add_emb = net.add_emb.repeat(k, 1)
            if cn_on:
                cond_emb = self.controlnet.cond_embedding(ctx.pixels_in(ctl, False)).repeat_interleave(k * nb, dim=0)
            tb0 = (self.unet.time_rowbias(job["t_dev"][0]), self.controlnet.time_rowbias(job["t_dev"][0]) if cn_on else None)
        text_len = text.shape[0] // (k * nb)
        mask_lat, mask_px = job.get("mask_lat"), job.get("mask_px")
        latents = torch.empty((k, hw, 4), device=dev, dtype=torch.float32)
        z0 = torch.empty((hw, 4), device=dev, dtype=torch.float32) if mask_lat is not None else None
        model_in = torch.empty((k * nb, lh, lw, 8), device=dev, dtype=ctx.dtype)
        sf = self.cfgs["vae"]["scaling_factor"]
        noises = job["noises"]
        x_img = ctx.pixels_in(src, True)
        moments = cabi.vae_encode(self.vae, x_img) if self.cpp_walks else self.vae.encode_moments(x_img)[0]
        for i, p in enumerate(plans):                     # z0 does not depend on the variant: every variant writes the same values
            rows = model_in[i * nb:(i + 1) * nb]
            _latent_prep(ctx, job, moments, noises[:2], p[0], latents[i], rows, z0, 0, sf)
        main.wait_stream(side)
        self._mark("clip+vae_encode")
        decode_in = torch.empty((k, lh, lw, 8), device=dev, dtype=ctx.dtype)
        self._mark("cond_embed")
        for step, (active, t_dev) in enumerate(zip(sched, job["t_dev"])):
            r = len(active) * nb                          # the rows of this step: the variants that have joined the loop
            tb_u, tb_c = tb0 if step == 0 else (self.unet.time_rowbias(t_dev), self.controlnet.time_rowbias(t_dev) if cn_on else None)
            self._mark("embed")
            if cn_on:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    c_skips, c_mid = self.controlnet.encode_cond(model_in[:r], cond_emb[:r], tb_c, text, text_len)
            skips, mid = self.unet.encode(self.unet.conv_in(ctx, model_in[:r]), tb_u, text, text_len)
            if cn_on:
                main.wait_stream(side)
            self._mark("unet_enc+controlnet")
            if ctl_s is None:
                skips, mid = self.controlnet.add_residuals(c_skips, c_mid, job["cn_scale"], skips, mid)
            elif cn_on:                                   # every variant is the one image: all rows read its one weight vector
                skips, mid = self.controlnet.add_residuals_weighted(c_skips, c_mid, ctl_s, skips, mid, w=job.get("ctl_w"), rows_per_image=k * nb)
            else:
                skips, mid = [passed_through(s) for s in skips], passed_through(mid)
            eps = self.unet.decode(mid, skips, tb_u, text, text_len)
            self._mark("unet_dec")
            for i, st, zi in active:
                z = None if zi is None else noises[zi]
                # st is the variant's own step record: with a soft mask it releases a level by its own step count
                _lcm_step(ctx, job, eps[i * nb:(i + 1) * nb], st, z, noises[1], latents[i], model_in[i * nb:(i + 1) * nb], decode_in[i:i + 1], z0, 0, sf)
            self._mark("lcm_step")
        dec = (lambda z: cabi.vae_decode(self.vae, z)) if self.cpp_walks else self.vae.decode
        if job.get("blend"):
            outs = [ctx.multiband_blend(ctx.pixels_out(dec(decode_in[i:i + 1])), img, job["blend_l"][0],
                                        None if mask_px is None else mask_px[0], job["blend"][1]) for i in range(k)]
        elif mask_px is None:
            outs = [ctx.pixels_out(dec(decode_in[i:i + 1])) for i in range(k)]
        else:
            outs = [ctx.pixels_out_composite(dec(decode_in[i:i + 1]), img, mask_px[0]) for i in range(k)]
        out_u8 = torch.stack(outs)
        self._mark("vae_decode")
        self.last_stats = dict(unet_evals=len(sched), cfg_batch=nb, latent_hw=(lh, lw), images=k, sweep=job["sweep"])
        self._latents = latents
        job["_result"] = dict(stats=dict(self.last_stats), latents=latents)
        if z0 is not None:
            job["_result"]["z0"] = z0
        return out_u8

    def _run_eager(self, job):
        """run_device() with the tuner meeting new shapes (as the eager warm-up of a capture does): an eager call and a graph replay of
        the same job then use the same kernels.  That matters since round 3: a split-K choice changes the fp32 summation order, so
        unlike the tile choice it can move the last bit of an f16 output (eager == replay is asserted bit for bit by the tests)."""
        with self.eager_lock:
            self.ctx.autotune(self._tune_mode())
            try:
                return self.run_device(job)
            finally:
                self.ctx.autotune(2 if self.autotune else 0)

    # ------------------------------------------------------------------------------------------------ fp8 activation scales (config 5)
    def _fp8_layers(self):
        """(name, layer) of every layer that reads e4m3 activations: the transformer blocks (six tensors each) and the fp8-activation resnets (two)."""
        out = []
        for mname, net in (("unet", self.unet), ("controlnet", self.controlnet)):
            for i, t in enumerate(net.transformers()):
                out += [(f"{mname}.transformer{i}.block{k}", b) for k, b in enumerate(t.blocks) if b.a8]
            out += [(mname + "." + p.rstrip("."), r) for p, r in net.temb_names if r.c1.a8 or (r.c2.a8 and r.wp_plus is None)]
        return out

    def calibrate_fp8(self, prompt, image, control_image, margin=2.0, **edit_kw):
        """One-pass activation-scale calibration of the fp8 configuration (weight_dtype="f8e4m3"; include/fie.h: fie_amax_f16).  Runs ONE eager edit
        with the fp8-activation layers on f16 activations, folding max |x| of every tensor they would have quantised into a device float; then
        sets, per tensor, the power-of-two scale s = 2^ceil(log2(amax * margin / 448)) -- the producer writes value / s as e4m3, the consumer folds
        s into its per-channel weight scale.  A tensor beyond +-448 is no longer clipped, a small one uses the upper binades of e4m3 instead of its
        subnormals.  Captured graphs hold the old scales and are dropped.  Returns {layer name: [scales]} (load_fp8_scales takes it back)."""
        import math
        if self.weight_dtype != "f8e4m3":
            raise ValueError("calibrate_fp8: the pipeline was not built with weight_dtype='f8e4m3'")
        layers = self._fp8_layers()
        for _, l in layers:
            l.amax = torch.zeros(len(l.s8), device=self.ctx.device, dtype=torch.float32)
        graph, self.use_graph, self.ctx.calib = self.use_graph, False, True
        try:
            self(prompt=prompt, image=image, control_image=control_image, **edit_kw)
        finally:
            self.use_graph, self.ctx.calib = graph, False
        torch.cuda.synchronize(self.ctx.device)
        scales = {}
        for name, l in layers:
            am = l.amax.cpu().tolist()
            l.amax = None
            l.s8 = [2.0 ** math.ceil(math.log2(a * margin / 448.0)) if a > 0 else 1.0 for a in am]
            scales[name] = list(l.s8)
        self._drop_graphs()
        return scales

    def _drop_graphs(self):
        """Captured graphs hold the scales (and kernels) of their capture: forget them AND their memory pools (a pool whose graphs are all gone cannot
        take a new capture: torch's allocator asserts on its use count)."""
        self._graphs.clear()
        self._pools.clear()
        self._n_forked = 0

    def load_fp8_scales(self, scales):
        """Scales from an earlier calibrate_fp8 of the same model (a JSON-able dict); unknown / missing layer names raise."""
        layers = dict(self._fp8_layers())
        if set(scales) != set(layers):
            raise ValueError(f"load_fp8_scales: layer names differ ({len(set(scales) ^ set(layers))} unmatched)")
        for name, sc in scales.items():
            if len(sc) != len(layers[name].s8) or any(not (v > 0) for v in sc):
                raise ValueError(f"load_fp8_scales: bad scales for {name}")
            layers[name].s8 = [float(v) for v in sc]
        self._drop_graphs()

    def _tune_mode(self):
        """fie_gemm_autotune mode of a pass that may meet new shapes: 1 (time them), or 2 (remembered choices only) when the context's choices
        are frozen to a loaded table (FIE_TUNE_TABLE + FIE_TUNE_FROZEN=1: the test session), 0 with FIE_AUTOTUNE=0."""
        return 0 if not self.autotune else 2 if self.ctx.tune_frozen else 1

    MAX_FORKED_GRAPHS = 6

    _TENSOR_KEYS = ("ids_l", "ids_g", "eos_rows", "img_u8", "ctl_u8", "time_ids")
    # mask_l, content_lat: a masked-content mode's; blend_l: the multi-band blend's (section 15)
    # lvl_lat: a soft mask's latent levels (section 21)
    _MASK_KEYS = ("mask_lat", "mask_px", "mask_l", "content_lat", "blend_l", "lvl_lat")

    @staticmethod
    def _graph_base(job, slot):
        """What of a job decides which graph replays it: the graph key without the fork flag."""
        base = (job["hw"], job["nb"], tuple(st["t"] for st in job["steps"]), job["guidance"], job["cn_scale"], slot, job.get("n", 1))
        if job.get("mask_lat") is not None:              # masked: (masked, mask_blur, paste_back); an unmasked key is what it was
            # + the masked-content mode, unless "original"; + ("multiband", levels), unless the blend is "alpha"; + "levels" for a soft mask
            base = base + ((True,) + job["mask_cfg"] + ((job["content"],) if job.get("content") else ()) + ((job["blend"],) if job.get("blend") else ())
                           + (("levels",) if job.get("lvl_lat") is not None else ()),)
        if job.get("sweep"):                             # a strength sweep: + the step counts of its variants
            base = base + (("sweep", job["sweep"]),)
        if job.get("emph") is not None:                  # prompt emphasis: + one flag (the weights are graph inputs); an un-weighted key is what it was
            base = base + ("emph",)
        if job.get("ctl_layers") is not None:            # control weights: + the scales and the kept steps (the position weights are graph inputs)
            base = base + (("ctl", job["ctl_layers"], job["ctl_keep"], job.get("ctl_w") is not None),)
        return base

    def run_device_graphed(self, job, slot=0):
        """run_device() replayed from a hipGraph: the ~2 500 launches of one edit are captured once per
        (size, CFG batch, step plan, scales) and replayed with the job's inputs copied into the graph's static buffers.
        The returned u8 image is the graph's static output buffer (consume it before the next replay).
        `slot` selects an independent graph instance (own static buffers / scratch) so that several edits can be in
        flight on different streams of one GPU."""
        base = self._graph_base(job, slot)
        # A forked graph owns extra runtime streams; past ~8 such graphs in one process new ones start sharing hardware queues
        # with their own launch stream and replay 50 % slower (measured: 82 -> 125 ms, tools/edit_ab.py).  Beyond the budget a
        # new key is captured on one stream instead (87 ms): slower than a healthy forked graph, never pathological.
        fork = self.fork_streams and ((base, True) in self._graphs or self._n_forked < self.MAX_FORKED_GRAPHS)
        key = (base, fork)
        entry = self._graphs.get(key)
        if entry is None:
            with self.eager_lock:                       # eager launches + capture go through the one C-ABI context
                entry = self._graphs.get(key)
                if entry is None:
                    if len(self._graphs) >= self.max_graphs:
                        self.eager_overflow += 1
                        # cache full: serve this parameter set eagerly (see __init__) -- with the SLOT's workspaces (GroupNorm scratch,
                        # split-K slabs, the timestep-embedding barrier counters are keyed by (stream, ws_tag)): another slot's graph may
                        # be replaying on its own stream meanwhile
                        self.ctx.ws_tag = slot
                        try:
                            return self._run_eager(job)
                        finally:
                            self.ctx.ws_tag = 0
                    self._fork_override = fork           # read by _side_stream() during this capture only
                    try:
                        entry = self._capture(key, job, slot)
                    finally:
                        self._fork_override = None
                    self._n_forked += int(fork)
        else:
            self._graphs[key] = self._graphs.pop(key)    # most recently used last
        graph, static, out = entry
        if static is not job:
            for k in self._tensor_keys(job):
                static[k].copy_(job[k], non_blocking=True)
            for d, s_ in zip(static["noises"], job["noises"]):
                d.copy_(s_, non_blocking=True)
        graph.replay()
        job["_result"] = static["_result"]               # the replayed entry's own latents buffer / stats
        self.last_stats = dict(static["_result"]["stats"])
        return out

    def _tensor_keys(self, job):
        """The job tensors a graph reads from its static buffers: the mask tensors of a masked job, the weights of an emphasised prompt and the control
        weights of a mask join them."""
        return self._TENSOR_KEYS + tuple(k for k in self._MASK_KEYS + ("emph", "ctl_w") if job.get(k) is not None)

    def _capture(self, key, job, slot):
        static = dict(job)
        for k in self._tensor_keys(job):
            static[k] = job[k].clone()
        static["noises"] = [n.clone() for n in job["noises"]]
        static["t_dev"] = [t.clone() for t in job["t_dev"]]
        timing, self.timing = self.timing, None
        self.ctx.ws_tag = slot
        self.ctx.autotune(self._tune_mode())
        self.run_device(static)                     # eager warm-up: lazy workspaces / function attributes, tile autotune
        torch.cuda.synchronize()
        self.ctx.autotune(2 if self.autotune else 0)   # frees the tuner's scratch; the capture below uses what it remembered
        graph = torch.cuda.CUDAGraph()
        pool = self._pools.get(slot)
        if pool is None:
            pool = self._pools[slot] = torch.cuda.graph_pool_handle()
        # The capture stream is ours (created here, where torch would create its default one: same first-use order of streams) so that
        # its split-K workspace can be bound BEFORE the capture: allocated inside, its torch.zeros became a 96 MB memset node that every
        # replay of the slot's first graph re-ran
        cap = self.ctx.capture_stream()
        # No pass of Python's cycle collector inside the capture.  A capturing thread may not call the runtime's unsafe entries (free, event query,
        # synchronise), and a collector pass that starts between two launches runs the finalisers of whatever dead cycles the process has
        # gathered -- device and pinned buffers, events, launch programs of objects long out of use -- from this very thread; an error raised in
        # such a finaliser ends the process (seen once: "Fatal Python error: Aborted ... Garbage-collecting" under hip.py: attention, in this
        # captured pass).  torch.cuda.graph() used to collect on entry and, since 2.10, no longer does (torch.compiler.config.force_cudagraph_gc).
        # So: collect here, in front of the capture, and keep the collector off until it has ended.  Reference counts free as ever.
        gc_was_on = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            # thread_local: other worker threads keep replaying / allocating on their own streams during this capture
            with torch.cuda.graph(graph, pool=pool, stream=cap, capture_error_mode="thread_local"):
                out = self.run_device(static)
        finally:
            if gc_was_on:
                gc.enable()
        self.ctx.ws_tag = 0
        self.timing = timing
        self._graphs[key] = (graph, static, out)
        return self._graphs[key]

    def stage_ms(self):
        """Per-stage device milliseconds of the last run_device() (needs `self.timing = []` before the call)."""
        torch.cuda.synchronize()
        out = {}
        for (_, e0), (name, e1) in zip(self.timing[:-1], self.timing[1:]):
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out

    def new_slot_stream(self, slot, equal_priority=False):
        """A stream for graph slot `slot`.  Odd slots take a high-priority stream: ROCm keeps separate hardware queues per
        priority, so slots 0 and 1 can never be dealt onto one queue (which would serialise the two edits), and with worker
        threads (PIL in -> PIL out) the priority split measures best: 13.3 vs 12.9 images/s.  `equal_priority` is for a caller
        that replays device-resident jobs back to back (bench.py's timed loop: 14.1 vs 13.8 images/s) and needs >= 8 hardware
        queues (fie_amd.py sets 16) for the streams to stay on separate queues."""
        few_queues = int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 8
        return torch.cuda.Stream(device=self.ctx.device, priority=0 if equal_priority and not few_queues else -(slot % 2))

    def calibrate_streams(self, jobs, streams, tries=4, log=None):
        """Pick launch streams on which `len(jobs)` edits really overlap.  jobs[i] is replayed on slot i (its graph must exist or
        is captured here); candidates are `streams` and up to `tries - 1` freshly drawn sets; each is timed with two rounds of
        concurrent replays and the fastest set is returned.  Replay is stream-agnostic, so no graph is re-captured."""
        def timed(strs):
            torch.cuda.synchronize(self.ctx.device)
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(2):
                for i, (job, st) in enumerate(zip(jobs, strs)):
                    with torch.cuda.stream(st):
                        self.run_device_graphed(job, slot=i)
            torch.cuda.synchronize(self.ctx.device)
            t1.record()
            torch.cuda.synchronize(self.ctx.device)
            return t0.elapsed_time(t1)

        for i, (job, st) in enumerate(zip(jobs, streams)):          # captures (if needed) + first replays: untimed
            with torch.cuda.stream(st):
                self.run_device_graphed(job, slot=i)
        best, best_ms = list(streams), timed(streams)
        first_ms = best_ms
        for _ in range(tries - 1):
            cand = [self.new_slot_stream(i, equal_priority=all(s.priority == 0 for s in streams)) for i in range(len(jobs))]
            ms = timed(cand)
            if ms < best_ms:
                best, best_ms = cand, ms
        if log:
            log(f"stream calibration: first set {first_ms:.1f} ms, chosen {best_ms:.1f} ms for 2 rounds of {len(jobs)} edits in flight")
        return best

    def slot_stream(self, slot):
        """Stream of graph slot `slot`.  Every slot, slot 0 included, owns a stream: replaying an edit's graph on the legacy
        null stream costs +30 ms per edit once other streams exist in the process (measured, 92 vs 122 ms end to end)."""
        if slot not in self._slot_streams:
            self._slot_streams[slot] = self.new_slot_stream(slot)
        return self._slot_streams[slot]

    def __call__(self, prompt, negative_prompt="", image=None, control_image=None, strength=0.8,
                 num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5, generator=None,
                 output_type="pil", slot=0, post_check=None, mask_image=None, mask_blur=0, paste_back=True, after_device=None, *,
                 masked_content="original", blend="alpha", blend_levels=4, paste_later=False, mask_grow=0, mask_mode="binary", mask_ramp=0,
                 **unused):
        """`slot` (additive): independent hipGraph instance + stream, so that several calls may be in flight from different
        host threads on one GPU (graph mode only).  `post_check` (additive): a callable run after the result has reached the host
        (the stream is idle then); when it returns True the device-resident inputs have changed meanwhile and the device job is run
        again.  FastEditor.edit() passes the second half of its asynchronous device Canny: the edge map is computed with a fixed
        number of hysteresis rounds in front of the edit, and whether they had reached the fixed point is only looked at here --
        no host wait in front of the edit, a repeated job in the rare case that they had not.  `mask_image` / `mask_blur` / `paste_back`
        (additive): a mask-restricted edit (prepare(); a list of masks for a batch call); `masked_content`: what it starts from inside the mask
        (prepare()); `blend` / `blend_levels` / `paste_later`: how the paste-back meets the source (prepare()); `mask_grow`: the mask grown or
        shrunk by an exact disk before anything reads it (prepare()); `mask_mode` / `mask_ramp`: a soft mask, the greys as per-pixel strength
        (prepare()).  `after_device` (additive): a callable given the u8 result
        while it is still on the device, on the slot's stream behind the device job and outside its graph; it may queue more work there (FastEditor
        scores the edit) and whatever it returns comes back as `.extra`, complete once the image has reached the host.  A hook that returns a
        `DeviceOutput` replaces the image: its tensor(s) take the final device-to-host copy (FastEditor's full-resolution back end).
        `strength` (additive): a list of strengths or "all" makes the call a strength sweep (prepare_sweep): `.images` holds one image per distinct
        step count, strongest first, and the hooks see u8 [k, h, w, 3] as they do for a batch."""
        have_mask = any(m is not None for m in mask_image) if isinstance(mask_image, (list, tuple)) else mask_image is not None
        spec = hmask.MaskSpec.check(mask_blur, paste_back, masked_content, blend, blend_levels, mask_grow, mask_mode, mask_ramp,
                                    have_mask=have_mask, paste_later=paste_later)
        if slot and not self.use_graph:
            raise ValueError("slots > 0 need hipGraph replay (the eager path shares per-image state)")
        caller, st = torch.cuda.current_stream(self.ctx.device), self.slot_stream(slot)
        st.wait_stream(caller)                           # device-resident inputs may still be in flight on the caller's stream
        with torch.cuda.stream(st):
            out = self._call(prompt, negative_prompt, image, control_image, strength, num_inference_steps, guidance_scale,
                             controlnet_conditioning_scale, generator, output_type, slot, post_check, mask_image, spec, after_device)
        caller.wait_stream(st)
        return out

    def _to_host(self, out_u8, slot, varying=False):
        """D2H of the u8 result through a pinned staging buffer of the slot (a pageable `.cpu()` costs ~3x as much), then one
        host memcpy so the caller owns its array.  Synchronises the current stream only.  A list of tensors (a DeviceOutput of a batch call) comes
        back as a list of arrays behind the one synchronisation.  `varying`: the shapes follow the caller's images (a DeviceOutput), so the staging
        buffers are kept per image position and grown, not per shape."""
        outs = out_u8 if isinstance(out_u8, (list, tuple)) else [out_u8]
        hosts = []
        for i, o in enumerate(outs):
            if varying:
                key, n = (slot, "varying", i), o.numel()
                flat = self._host_out.get(key)
                if flat is None or flat.numel() < n:
                    flat = self._host_out[key] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
                host = flat[:n].view(o.shape)
            else:
                key = (slot, tuple(o.shape))
                host = self._host_out.get(key)
                if host is None:
                    host = self._host_out[key] = torch.empty(o.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(o, non_blocking=True)
            hosts.append(host)
        self.ctx.fetch_device_errors()                   # 16 bytes behind the image: a kernel that had to give up does not stay silent
        torch.cuda.current_stream(self.ctx.device).synchronize()
        self.ctx.check_device_errors(fetch=False)
        if isinstance(out_u8, (list, tuple)):
            return [h.numpy().copy() for h in hosts]
        return hosts[0].numpy().copy()

    def _call(self, prompt, negative_prompt, image, control_image, strength, num_inference_steps, guidance_scale,
              controlnet_conditioning_scale, generator, output_type, slot, post_check=None, mask_image=None, spec=hmask.MaskSpec(), after_device=None):

        def run(job):
            """One device job, the caller's after_device hook behind it, then the result on the host: -> (u8 array, hook's return)."""
            out_u8 = self.run_device_graphed(job, slot) if self.use_graph else self._run_eager(job)
            extra = after_device(out_u8) if after_device is not None else None
            if isinstance(extra, DeviceOutput):             # the hook's own output travels instead of the edit-size image
                return self._to_host(extra.out, slot, varying=True), extra.extra
            return self._to_host(out_u8, slot), extra       # device -> host sync, as `.images[0]` implies upstream

        if isinstance(strength, (list, tuple, str)):     # [additive] a strength sweep: one image, one variant per distinct step count (prepare_sweep)
            if isinstance(prompt, (list, tuple)):
                raise ValueError("a strength sweep runs on one image: `strength` is a list and `prompt` is one too")
            job = self.prepare_sweep(prompt, negative_prompt, image, control_image, strength, num_inference_steps, guidance_scale,
                                     controlnet_conditioning_scale, generator, mask_image, **spec.keywords())
            arr, extra = run(job)
            if post_check is not None and post_check():
                self.repeated_jobs += 1
                arr, extra = run(job)
            if not isinstance(arr, list):
                arr = [arr] if arr.ndim == 3 else list(arr)
            return types.SimpleNamespace(images=arr if output_type == "np" else [Image.fromarray(a) for a in arr], extra=extra)
        if isinstance(prompt, (list, tuple)):            # [additive] a batch: lists of prompts / images / generators
            job = self.prepare_batch(list(prompt), negative_prompt if isinstance(negative_prompt, (list, tuple)) else None,
                                     list(image), list(control_image), strength, num_inference_steps, guidance_scale,
                                     controlnet_conditioning_scale, generator if isinstance(generator, (list, tuple)) else None, mask_image,
                                     **spec.keywords())
            arr, extra = run(job)
            if post_check is not None and post_check():
                arr, extra = run(job)
            if not isinstance(arr, list):
                arr = arr[None] if arr.ndim == 3 else arr
            if output_type == "np":
                return types.SimpleNamespace(images=list(arr), extra=extra)
            return types.SimpleNamespace(images=[Image.fromarray(a) for a in arr], extra=extra)
        job = self.prepare(prompt, negative_prompt, image, control_image, strength, num_inference_steps,
                           guidance_scale, controlnet_conditioning_scale, generator, mask_image, **spec.keywords())
        if output_type == "latent":
            self.run_device_graphed(job, slot) if self.use_graph else self._run_eager(job)
            res = job["_result"]
            lh, lw = res["stats"]["latent_hw"]
            return types.SimpleNamespace(images=[res["latents"].view(lh, lw, 4).clone()])
        arr, extra = run(job)
        if post_check is not None and post_check():
            self.repeated_jobs += 1
            arr, extra = run(job)
        if output_type == "np":
            return types.SimpleNamespace(images=[arr], extra=extra)
        return types.SimpleNamespace(images=[Image.fromarray(arr)], extra=extra)
