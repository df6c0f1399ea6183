"""`MetricsCalculator` -- evaluation metrics with the reference's interface (/root/reference/src/metrics.py:150-386).

Evaluation only (not part of the denoising hot path): plain torch ops, as the reference's
torchmetrics are.  Restated here: SSIM (torchmetrics defaults: 11x11 Gaussian, sigma 1.5, k1/k2 0.01/0.03,
data_range 1), PSNR and MSE, all on 512x512 LANCZOS-resized RGB in [0,1] (reference :227-239, :291-347).
LPIPS(squeeze) (reference :179-183, :241-269) runs on the device when a local weight directory is given (`lpips_dir=`, else FIE_LPIPS_DIR, else
<FIE_WEIGHTS_DIR>/lpips): fie_amd/lpips.py; without one, and on the CPU, it returns None rather than a made-up number.
The DINO ViT-B/8 structure distance (reference :24-147) runs on the device when a local transformers `ViTModel` directory is given
(`dino_dir=`, else FIE_DINO_DIR, else <FIE_WEIGHTS_DIR>/dino): fie_amd/dino.py; without one, and on the CPU, it returns None.  CLIPScore(ViT-B/16) (reference :184-186, :271-289) runs on the device when a local
`CLIPModel` directory is given (`clip_dir=`, else FIE_CLIP_SCORE_DIR, else <FIE_WEIGHTS_DIR>/clip_score): fie_amd/clip_score.py,
DESIGN.md section 11; without one, and on the CPU, it returns None as well.

On a GPU (`device="cuda..."`) the arithmetic is one HIP op (csrc/metrics.hip through `ctx.metrics_pairs`): each image is
uploaded once, LANCZOS-resized on the device when it is not 512x512, and SSIM / PSNR / MSE of any number of pairs come from one launch and
one synchronisation.  `device="cpu"` is the torch restatement above.  Additive: `calculate_all_metrics(..., mask=)` adds the background
preservation scores `bg_ssim / bg_psnr / bg_mse` (both images zeroed inside the edited region, PIE-Bench's convention), and
`calculate_pairs(sources, editeds, masks=None)` scores a list at once; with a CLIP directory `mask=` also adds `clip_score_edited` (the score of
the image zeroed OUTSIDE the edited region) and `calculate_clip_scores(images, texts, masks=None)` scores a list."""
import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

import fie_amd  # noqa: F401  (alias loader for the hyphenated package directory)
from fie_amd import clip_score as hclip
from fie_amd import dino as hdino
from fie_amd import lpips as hlpips
from fie_amd import mask as hmask
from fie_amd import metrics as hmetrics

TARGET = hmetrics.TARGET


class MetricsCalculator:
    def __init__(self, device="cuda", clip_dir=None, dino_dir=None, dino_layer=hdino.DEFAULT_LAYER, lpips_dir=None):
        self.device = device
        print(f"[MetricsCalculator] Initializing on {device}...")
        d = torch.arange(-5.0, 6.0)
        g = torch.exp(-(d / 1.5) ** 2 / 2)
        g = (g / g.sum())[None]
        self._win = g.T @ g                             # the torch restatement's window (device="cpu")
        self._ctx = None
        if str(device).startswith("cuda"):              # no fallback: a missing library or GPU raises here
            from fie_amd import hip
            index = torch.device(device).index
            self._ctx = hip.context(torch.cuda.current_device() if index is None else index)
        self._clip = None                               # fie_amd.clip_score.ClipScorer: only on a GPU and only from a local CLIPModel directory
        clip_dir = hclip.resolve_dir(clip_dir) if self._ctx is not None else None
        if clip_dir:
            print(f"[MetricsCalculator] Loading the CLIP score model from {clip_dir}")
            self._clip = hclip.load(clip_dir, self._ctx)
        self._dino = None                               # fie_amd.dino.DinoScorer: only on a GPU and only from a local ViTModel directory
        dino_dir = hdino.resolve_dir(dino_dir) if self._ctx is not None else None
        if dino_dir:
            print(f"[MetricsCalculator] Loading the DINO structure distance model from {dino_dir}")
            self._dino = hdino.load(dino_dir, self._ctx, layer=dino_layer)
        self._lpips = None                              # fie_amd.lpips.LpipsScorer: only on a GPU and only from a local weight directory
        lpips_dir = hlpips.resolve_dir(lpips_dir) if self._ctx is not None else None
        if lpips_dir:
            print(f"[MetricsCalculator] Loading the LPIPS model from {lpips_dir}")
            self._lpips = hlpips.load(lpips_dir, self._ctx)
        missing = [what for what, have in (("LPIPS: no weight directory", self._lpips), ("CLIP score: no model directory", self._clip),
                                           ("DINO distance: no model directory", self._dino)) if not have]
        print("[MetricsCalculator] Initialization complete!" + (f" ({'; '.join(missing)})" if missing else ""))

    def _pil_to_tensor(self, img):
        a = np.array(img).astype(np.float32) / 255.0
        return torch.from_numpy(a).permute(2, 0, 1).unsqueeze(0).to(self.device)

    def _pair(self, img1, img2):
        if img1.size != TARGET:
            img1 = img1.resize(TARGET, Image.LANCZOS)
        if img2.size != TARGET:
            img2 = img2.resize(TARGET, Image.LANCZOS)
        return self._pil_to_tensor(img1), self._pil_to_tensor(img2)

    def _upload(self, img):
        """PIL -> u8 [512, 512, 3] on the device: one upload, the LANCZOS resize (when needed) in fie_resize_rgb_u8, bit-exact with Pillow."""
        t = torch.from_numpy(np.ascontiguousarray(np.array(img)[..., :3])).to(self._ctx.device)
        if (t.shape[1], t.shape[0]) != TARGET:
            t = self._ctx.resize_lanczos(t, TARGET[1], TARGET[0])
        return t

    def calculate_pairs(self, sources, editeds, masks=None):
        """[additive] {ssim, psnr, mse} of every (source, edited) pair of two lists of PIL images; `masks` (None, or one mask or None per
        pair: a PIL image or a uint8 / bool [H, W] array of any size, white = edited) adds {bg_ssim, bg_psnr, bg_mse} where a mask is given.
        On a GPU: one upload per image, one launch and one synchronisation for the whole list."""
        if len(sources) != len(editeds) or (masks is not None and len(masks) != len(sources)):
            raise ValueError("sources, editeds and masks must be lists of one length")
        masks = list(masks) if masks is not None else [None] * len(sources)
        bins = [None if m is None else hmetrics.binary_mask(m) for m in masks]
        if not sources:
            return []
        if self._ctx is None:
            return [self._pair_cpu(a, b, m) for a, b, m in zip(sources, editeds, bins)]
        ctx = self._ctx
        with torch.cuda.device(ctx.device):
            a = torch.stack([self._upload(im) for im in sources])
            b = torch.stack([self._upload(im) for im in editeds])
            mk = None
            if any(m is not None for m in bins):
                zero = np.zeros(TARGET[::-1], np.uint8)
                mk = torch.from_numpy(np.stack([zero if m is None else m for m in bins])).to(ctx.device)
            rows = ctx.metrics_pairs(a, b, mk).cpu()
        return hmetrics.rows_to_dicts(rows.numpy(), TARGET[1], TARGET[0], [m is not None for m in bins])

    def _pair_cpu(self, img1, img2, mask01=None):
        out = {"ssim": self._ssim_cpu(img1, img2), "psnr": self._psnr_cpu(img1, img2), "mse": self._mse_cpu(img1, img2)}
        if mask01 is not None:
            keep = torch.from_numpy(1.0 - mask01.astype(np.float32))[None, None].to(self.device)
            out.update(bg_ssim=self._ssim_cpu(img1, img2, keep), bg_psnr=self._psnr_cpu(img1, img2, keep), bg_mse=self._mse_cpu(img1, img2, keep))
        return out

    def calculate_ssim(self, img1, img2):
        if self._ctx is not None:
            return self.calculate_pairs([img1], [img2])[0]["ssim"]
        return self._ssim_cpu(img1, img2)

    def _ssim_cpu(self, img1, img2, keep=None):
        x, y = self._pair(img1, img2)
        if keep is not None:
            x, y = x * keep, y * keep
        c = x.shape[1]
        win = self._win.expand(c, 1, 11, 11)
        xp, yp = F.pad(x, (5,) * 4, mode="reflect"), F.pad(y, (5,) * 4, mode="reflect")
        mu_x, mu_y, e_xx, e_yy, e_xy = F.conv2d(torch.cat([xp, yp, xp * xp, yp * yp, xp * yp]), win, groups=c).split(1)
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        sxx, syy, sxy = e_xx - mu_x ** 2, e_yy - mu_y ** 2, e_xy - mu_x * mu_y
        m = ((2 * mu_x * mu_y + c1) * (2 * sxy + c2)) / ((mu_x ** 2 + mu_y ** 2 + c1) * (sxx + syy + c2))
        return m[..., 5:-5, 5:-5].mean().item()

    def calculate_mse(self, img1, img2):
        if self._ctx is not None:
            return self.calculate_pairs([img1], [img2])[0]["mse"]
        return self._mse_cpu(img1, img2)

    def _mse_cpu(self, img1, img2, keep=None):
        x, y = self._pair(img1, img2)
        if keep is not None:
            x, y = x * keep, y * keep
        return ((x - y) ** 2).mean().item()

    def calculate_psnr(self, img1, img2):
        if self._ctx is not None:
            return self.calculate_pairs([img1], [img2])[0]["psnr"]
        return self._psnr_cpu(img1, img2)

    def _psnr_cpu(self, img1, img2, keep=None):
        m = self._mse_cpu(img1, img2, keep)
        return float("inf") if m == 0 else float(10.0 * np.log10(1.0 / m))

    def calculate_lpips(self, img1, img2):
        """The reference's LPIPS (SqueezeNet, both images LANCZOS-resized to 512 x 512), or None without a weight directory / on the CPU."""
        if self._lpips is None or img1 is None or img2 is None:
            return None
        return self.calculate_lpipses([img1], [img2])[0]["lpips"]

    def calculate_lpipses(self, sources, editeds, masks=None):
        """[additive] {"lpips": float} per (source, edited) pair of two lists of PIL images; `masks` (None, or per pair None / a mask as
        calculate_pairs takes it) adds "bg_lpips" where a mask is given: the same number with both images' bytes set to 0 inside the binarised
        512 x 512 mask, as bg_ssim treats them.  One upload per image, all images through the tower in batched passes, one synchronisation.
        Without a weight directory every entry is None."""
        if len(sources) != len(editeds) or (masks is not None and len(masks) != len(sources)):
            raise ValueError("sources, editeds and masks must be lists of one length")
        if self._lpips is None:
            return [None] * len(sources)
        if not sources:
            return []
        ctx = self._ctx
        bins = None if masks is None else [None if m is None else hmetrics.binary_mask(m) for m in masks]
        with torch.cuda.device(ctx.device):
            a = [self._upload(im) for im in sources]
            b = [self._upload(im) for im in editeds]
            mk = None if bins is None else [None if m is None else torch.from_numpy(m).to(ctx.device) for m in bins]
            rows = self._lpips.scores(a, b, mk).cpu().numpy()
        out = []
        for i, row in enumerate(rows):
            out.append({"lpips": hlpips.total(row[:7])})
            if bins is not None and bins[i] is not None:
                out[-1]["bg_lpips"] = hlpips.total(row[7:])
        return out

    def calculate_clip_score(self, img, text):
        """max(100 cos(image embedding, text embedding), 0) of the reference's CLIPScore, or None without a model directory / on the CPU."""
        if self._clip is None or img is None:
            return None
        return self.calculate_clip_scores([img], [text])[0]["clip_score"]

    def calculate_clip_scores(self, images, texts, masks=None, unclamped=False):
        """[additive] {"clip_score": float} per (image, text) pair of two lists; `masks` (None, or per pair None / a mask as calculate_pairs takes
        it, NEAREST-resized to the image's size, L >= 128 = edited) adds "clip_score_edited": the score of the image with every pixel outside the
        edited region set to 0.  One upload per image, one batched pass of the image tower per image size, all prompts in one pass of the text
        tower, one synchronisation.  `unclamped`: 100 cos itself (may be negative) instead of the clamped score.  Without a model directory
        every entry is None."""
        if len(images) != len(texts) or (masks is not None and len(masks) != len(images)):
            raise ValueError("images, texts and masks must be lists of one length")
        if self._clip is None:
            return [None] * len(images)
        if not images:
            return []
        clip, ctx = self._clip, self._ctx
        masks = list(masks) if masks is not None else [None] * len(images)
        with torch.cuda.device(ctx.device):
            devs = [torch.from_numpy(np.ascontiguousarray(np.array(im.convert("RGB") if im.mode != "RGB" else im))).to(ctx.device) for im in images]
            mdevs = [None if m is None else torch.from_numpy(hmask.to_l_array(m)).to(ctx.device) for m in masks]
            # items = (image, masked?) sorted into size groups: a group's rows are contiguous in the text pass and in the result
            groups = {}
            for i, d in enumerate(devs):
                g = groups.setdefault(tuple(d.shape[:2]), [])
                g.append((i, False))
                if mdevs[i] is not None:
                    g.append((i, True))
            order = [it for g in groups.values() for it in g]
            txt = clip.text_embeddings([texts[i] for i, _ in order])
            rows = torch.empty((len(order), 2), device=ctx.device, dtype=torch.float32)
            r0 = 0
            for g in groups.values():
                emb = clip.image_embeddings([devs[i] for i, _ in g], [mdevs[i] if masked else None for i, masked in g])
                clip.score_rows(emb, txt[r0:r0 + len(g)], out=rows[r0:r0 + len(g)])
                r0 += len(g)
            host = rows.cpu().numpy()
        out = [{} for _ in images]
        for (i, masked), row in zip(order, host):
            out[i]["clip_score_edited" if masked else "clip_score"] = float(row[0 if unclamped else 1])
        return out

    def calculate_dino_distance(self, source_img, edited_img):
        """The reference's DinoDistanceMetric.calculate_distance (MSE between the self-similarity matrices of the layer-11 keys), or None without a
        model directory / on the CPU.  Both images must be square (ValueError naming the sizes otherwise)."""
        if self._dino is None or source_img is None or edited_img is None:
            return None
        return self.calculate_dino_distances([source_img], [edited_img])[0]

    def calculate_dino_distances(self, sources, editeds):
        """[additive] The structure distance of every (source, edited) pair of two lists of PIL images: one upload per image, one batched pass of the
        tower per (source size, edited size), one synchronisation.  Without a model directory every entry is None."""
        if len(sources) != len(editeds):
            raise ValueError("sources and editeds must be lists of one length")
        if self._dino is None:
            return [None] * len(sources)
        if not sources:
            return []
        dino, ctx = self._dino, self._ctx
        rgb = lambda im: np.ascontiguousarray(np.array(im.convert("RGB") if im.mode != "RGB" else im))
        for im in list(sources) + list(editeds):
            dino.check_size(im.size[1], im.size[0])
        with torch.cuda.device(ctx.device):
            a = [torch.from_numpy(rgb(im)).to(ctx.device) for im in sources]
            b = [torch.from_numpy(rgb(im)).to(ctx.device) for im in editeds]
            groups = {}
            for i in range(len(a)):
                groups.setdefault((tuple(a[i].shape[:2]), tuple(b[i].shape[:2])), []).append(i)
            rows = torch.empty(len(a), device=ctx.device, dtype=torch.float64)
            r0, order = 0, []
            for idx in groups.values():
                dino.distances([a[i] for i in idx], [b[i] for i in idx], out=rows[r0:r0 + len(idx)])
                r0 += len(idx)
                order += idx
            host = rows.cpu().numpy()
        out = [None] * len(a)
        for i, v in zip(order, host):
            out[i] = float(v)
        return out

    def _dino_or_none(self, source_img, edited_img):
        """calculate_dino_distance, with None for a pair the tower cannot take (not square) -- as a column of a table wants it."""
        if self._dino is None or source_img is None or edited_img is None:
            return None
        if not (hdino.supported_size(source_img.size[1], source_img.size[0]) and hdino.supported_size(edited_img.size[1], edited_img.size[0])):
            return None
        return self.calculate_dino_distance(source_img, edited_img)

    def calculate_all_metrics(self, source_img, edited_img, prompt, mask=None):
        m = self.calculate_pairs([source_img], [edited_img], None if mask is None else [mask])[0]
        return self.with_unavailable(m, source_img, edited_img, prompt, mask=mask)

    def with_unavailable(self, m, source_img=None, edited_img=None, prompt="", mask=None):
        """A calculate_pairs() dict in calculate_all_metrics()'s key order, with the metrics that need hub checkpoints as None.  `clip_score`
        is filled when the calculator has a CLIP model (and `clip_score_edited`, behind the bg_* keys, when a mask comes with it),
        `dino_distance` when it has a DINO model and both images are square, `lpips` when it has the LPIPS weights (and `bg_lpips`, directly
        behind `bg_mse`, when a mask comes with it)."""
        clip = {"clip_score": None}
        if self._clip is not None and edited_img is not None:
            clip = self.calculate_clip_scores([edited_img], [prompt], None if mask is None else [mask])[0]
        lp = {"lpips": None}
        if self._lpips is not None and source_img is not None and edited_img is not None:
            lp = self.calculate_lpipses([source_img], [edited_img], None if mask is None else [mask])[0]
        out = {"ssim": m["ssim"], "lpips": lp["lpips"], "clip_score": clip["clip_score"],
               "psnr": m["psnr"], "mse": m["mse"], "dino_distance": self._dino_or_none(source_img, edited_img)}
        out.update({k: m[k] for k in hmetrics.BG_KEYS if k in m})
        if "bg_lpips" in lp:
            out["bg_lpips"] = lp["bg_lpips"]
        if "clip_score_edited" in clip:
            out["clip_score_edited"] = clip["clip_score_edited"]
        return out

    def clear_memory(self):
        if str(self.device).startswith("cuda"):
            torch.cuda.empty_cache()
