"""CLIP score of an edit on the device (kernels: csrc/clip_score.hip, towers: clip.py).

The number is the reference's `CLIPScore(model_name_or_path="openai/clip-vit-base-patch16")` on one image and one text
(reference src/metrics.py:184-186, 271-289): `max(100 * cos(image_emb, text_emb), 0)` with
  image_emb = visual_projection(post_layernorm(CLS)) of the processor's output: Pillow BICUBIC resize of the u8 image (shortest edge ->
              224, the other `int(224 * long / short)`), centre crop, /255, (x - mean) / std;
  text_emb  = text_projection of the final-LN state at the EOS token; the prompt truncated to the tower's max_position_embeddings.
`load(dir, ctx)` reads a transformers `CLIPModel` directory; there is no scorer without one (a made-up number stays forbidden).
The host-side arithmetic of this module (sizes, crop origins, the preprocessor's settings) is device-free and tested on the CPU."""
import json
import os

import torch

DEFAULT_MEAN = (0.48145466, 0.4578275, 0.40821073)
DEFAULT_STD = (0.26862954, 0.26130258, 0.27577711)
DIR_ENV = "FIE_CLIP_SCORE_DIR"


def resolve_dir(clip_dir=None):
    """The CLIPModel directory: the argument, else FIE_CLIP_SCORE_DIR, else <FIE_WEIGHTS_DIR>/clip_score when that exists, else None."""
    if clip_dir:
        return str(clip_dir)
    if os.environ.get(DIR_ENV):
        return os.environ[DIR_ENV]
    root = os.environ.get("FIE_WEIGHTS_DIR")
    if root and os.path.isdir(os.path.join(root, "clip_score")):
        return os.path.join(root, "clip_score")
    return None


def resized_size(h, w, short):
    """(height, width) after the processor's resize: the shortest edge becomes `short`, the other `int(short * long / short_edge)`."""
    if w <= h:
        return int(short * h / w), short
    return short, int(short * w / h)


def crop_origin(h, w, crop):
    """(top, left) of the centre crop of a resized h x w image."""
    return (h - crop) // 2, (w - crop) // 2


def preprocessor(cfg=None, image_size=224):
    """preprocessor_config.json's dict (None: CLIPImageProcessor's defaults) -> dict(short, crop, mean, std).  Settings the device path does not
    restate (another resample filter, a switched-off step, a crop that is not the tower's input) raise."""
    cfg = cfg or {}
    for k in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
        if cfg.get(k, True) is not True:
            raise ValueError(f"clip_score: preprocessor_config {k}={cfg.get(k)!r} is not supported (the device path always does it)")
    if cfg.get("resample", 3) != 3:
        raise ValueError(f"clip_score: preprocessor_config resample={cfg.get('resample')!r}: only 3 (PIL BICUBIC) is built")
    if abs(cfg.get("rescale_factor", 1 / 255) - 1 / 255) > 1e-12:
        raise ValueError(f"clip_score: preprocessor_config rescale_factor={cfg.get('rescale_factor')!r}: only 1/255 is built")
    size, crop = cfg.get("size", {"shortest_edge": image_size}), cfg.get("crop_size", {"height": image_size, "width": image_size})
    short = size.get("shortest_edge") if isinstance(size, dict) else size
    ch, cw = (crop.get("height"), crop.get("width")) if isinstance(crop, dict) else (crop, crop)
    if not short or ch != cw or ch != image_size or short < ch:
        raise ValueError(f"clip_score: preprocessor size={size!r} crop_size={crop!r}: needs a shortest_edge resize of at least the square crop, "
                         f"and a crop equal to the tower's image size {image_size}")
    mean, std = tuple(cfg.get("image_mean") or DEFAULT_MEAN), tuple(cfg.get("image_std") or DEFAULT_STD)
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("clip_score: image_mean / image_std must have three entries")
    return dict(short=int(short), crop=int(ch), mean=mean, std=std)


def truncate_ids(ids, max_positions, eos):
    """Token ids [n, T] cut to the tower's max_position_embeddings, the last position an EOS where the prompt was cut (CLIPTokenizer's truncation)."""
    if ids.shape[1] <= max_positions:
        return ids
    ids = ids[:, :max_positions].clone()
    cut = ~(ids == eos).any(dim=1)
    ids[cut, -1] = eos
    return ids


class ClipScorer:
    """Both towers of one CLIPModel on one context, plus the processor and the scorer op.  Every method queues work on torch's current stream
    and returns device tensors; nothing here synchronises."""

    def __init__(self, ctx, vision, text, tokenizer, pre):
        self.ctx, self.vision, self.text, self.tok, self.pre = ctx, vision, text, tokenizer, pre
        self._text_cache = {}

    def token_ids(self, prompts):
        cfg = self.text.cfg
        return truncate_ids(self.tok(list(prompts)), cfg["max_positions"], self.tok.eos)

    def text_embeddings(self, prompts):
        """[n, P]: all prompts in ONE pass of the text tower."""
        return self.text(self.token_ids(prompts))[1]

    def text_embedding(self, prompt):
        """[1, P], cached per prompt string."""
        e = self._text_cache.get(prompt)
        if e is None:
            if len(self._text_cache) >= 256:
                self._text_cache.clear()
            e = self._text_cache[prompt] = self.text_embeddings([prompt])
        return e

    def image_embeddings(self, images, masks=None):
        """images: u8 [h, w, 3] device tensors of ONE size (or a u8 [n, h, w, 3] tensor); masks: None, or per image None / a u8 [mh, mw] mode-L
        device tensor (L >= 128 = edited; any size).  Returns [n, P]: image i zeroed outside its mask (where it has one), BICUBIC-resized,
        cropped, normalised and sent through the tower -- one batched pass."""
        ctx, pre = self.ctx, self.pre
        n = len(images)
        h, w = images[0].shape[:2]
        rh, rw = resized_size(h, w, pre["short"])
        buf = torch.empty((n, rh, rw, 3), device=ctx.device, dtype=torch.uint8)
        for i in range(n):
            im = images[i].contiguous()
            if tuple(im.shape) != (h, w, 3) or im.dtype != torch.uint8:
                raise ValueError(f"clip_score: image {i} is {tuple(im.shape)} {im.dtype}, expected u8 {(h, w, 3)}")
            if masks is not None and masks[i] is not None:
                im = ctx.clip_mask(im, masks[i].contiguous())
            ctx.resize_bicubic(im, rh, rw, out=buf[i])
        top, left = crop_origin(rh, rw, pre["crop"])
        patches = ctx.clip_patches(buf, top, left, pre["crop"], self.vision.cfg["patch_size"], pre["mean"], pre["std"])
        return self.vision(patches, n)

    def score_rows(self, img_emb, txt_emb, out=None):
        """f32 [n, 2] on the device: (100 cos, max(100 cos, 0)) per pair."""
        return self.ctx.clip_score(img_emb, txt_emb, out=out)


def load(clip_dir, ctx):
    """A transformers `CLIPModel` directory -> ClipScorer on `ctx`: config.json, model.safetensors, preprocessor_config.json when present
    (else CLIPImageProcessor's defaults) and vocab.json + merges.txt for the BPE tokenizer.  Uses safetensors only."""
    from safetensors.torch import load_file
    from . import config as hconfig
    from .clip import ClipText, ClipVision
    from .tokenizer import BpeTokenizer
    need = ("config.json", "model.safetensors", "vocab.json", "merges.txt")
    missing = [f for f in need if not os.path.exists(os.path.join(clip_dir, f))]
    if missing:
        raise FileNotFoundError(f"clip_score: {clip_dir} lacks {missing} (a CLIPModel directory with its tokenizer files is needed)")
    with open(os.path.join(clip_dir, "config.json"), encoding="utf-8") as f:
        c = json.load(f)
    vcfg, tcfg = hconfig.clip_vision_cfg(c), hconfig.clip_score_text_cfg(c)
    pre_path, pre_cfg = os.path.join(clip_dir, "preprocessor_config.json"), None
    if os.path.exists(pre_path):
        with open(pre_path, encoding="utf-8") as f:
            pre_cfg = json.load(f)
    pre = preprocessor(pre_cfg, vcfg["image_size"])
    sd = load_file(os.path.join(clip_dir, "model.safetensors"))
    tok = BpeTokenizer(os.path.join(clip_dir, "vocab.json"), os.path.join(clip_dir, "merges.txt"), tcfg["pad_token_id"])
    tcfg = dict(tcfg, pad_token_id=tok.eos)               # CLIPTokenizer pads with <|endoftext|>; causal attention: padding never reaches the EOS state
    tok.pad_id = tok.eos
    if tcfg["eos_token_id"] != 2 and tcfg["eos_token_id"] != tok.eos:
        raise ValueError(f"clip_score: config eos_token_id {tcfg['eos_token_id']} but the vocabulary's <|endoftext|> is {tok.eos}")
    with torch.cuda.device(ctx.device):
        ctx.sync_stream()
        return ClipScorer(ctx, ClipVision(ctx, vcfg, sd), ClipText(ctx, tcfg, sd), tok, pre)
