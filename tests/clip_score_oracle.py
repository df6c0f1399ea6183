"""CPU oracle of the CLIP score tests (tests/test_clip_score_cpu.py, tests/test_clip_score_gpu.py): a seeded `transformers.CLIPModel` in fp32,
written into a directory the product loads (`save_pretrained` + the committed synthetic BPE files), and the score restated from
`CLIPImageProcessorPil` + `get_image_features` / `get_text_features`.

Weights are RE-DRAWN, not transformers' initialisation: with the default init (std 0.02 and smaller) the image barely moves the embedding --
scores of different images against one text differ by 0.1-0.6 -- and parity could not tell a broken tower from a working one.  Here every
matrix is N(0, GAIN^2 / fan_in), LayerNorm gains 1 + 0.2 N, biases 0.1 N, embeddings 0.5 N, all rounded to fp16 so that the fp16 context loads
exactly the oracle's weights.  `control()` measures what that buys: how far apart two images' embeddings and a pair's / its swapped pair's
scores are; the tests assert it is at least 10 x the parity bound."""
import math
import os
import shutil

import numpy as np
import torch
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOCAB, MERGES = os.path.join(GOLDEN, "bpe_vocab.json"), os.path.join(GOLDEN, "bpe_merges.txt")
VOCAB_SIZE, BOS, EOS = 1414, 1412, 1413

CONFIGS = {
    # 2 layers, hidden 128 (2 heads of 64), projection 64, patch 16 / image 224: still 197 tokens
    "tiny": dict(text=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2),
                 vision=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=224, patch_size=16),
                 projection_dim=64),
    # the shape of openai/clip-vit-base-patch16
    "b16": dict(text=dict(hidden_size=512, intermediate_size=2048, num_hidden_layers=12, num_attention_heads=8),
                vision=dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=224, patch_size=16),
                projection_dim=512),
}
GAIN = 2.0
SEED = {"tiny": 7, "b16": 11}

PROMPTS = ["a red kite", "a photo of a green door in a stone wall", "two toy boats on a lake at night", "an orange cat"]
LONG_PROMPT = " ".join(["a very long prompt about a small red kite over the green hills and the blue sea"] * 8)       # > 77 tokens: truncated


def rel_err(a, b):
    """The project's parity measure: max |a - b| / max |b|."""
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def image(seed, h, w):
    """u8 [h, w, 3]: smooth colour fields of a seeded tint and contrast, a few rectangles and noise -- content at every scale the resize and
    the patches see, and a global look that differs from seed to seed (the towers' CLS state follows it)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.zeros((h, w, 3))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.5, 6.0), rng.uniform(0.5, 6.0), rng.uniform(0, 6.28)
        a[..., c] = rng.uniform(30, 225) + rng.uniform(20, 100) * np.sin(2 * math.pi * (fx * xx / w + fy * yy / h) + ph)
    for _ in range(6):
        y0, x0 = rng.integers(0, h - 8), rng.integers(0, w - 8)
        y1, x1 = y0 + rng.integers(8, max(9, h // 2)), x0 + rng.integers(8, max(9, w // 2))
        a[y0:y1, x0:x1] = rng.integers(0, 256, 3)
    a += rng.normal(0, 12, a.shape)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def build_model(kind):
    """The seeded fp32 CLIPModel of CONFIGS[kind] with re-drawn, fp16-rounded weights."""
    from transformers import CLIPConfig, CLIPModel
    c = CONFIGS[kind]
    text = dict(c["text"], vocab_size=VOCAB_SIZE, max_position_embeddings=77, eos_token_id=EOS, bos_token_id=BOS, pad_token_id=EOS)
    model = CLIPModel(CLIPConfig(text_config=text, vision_config=dict(c["vision"]), projection_dim=c["projection_dim"])).eval().float()
    g = torch.Generator().manual_seed(SEED[kind])
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name == "logit_scale":
                continue
            n = lambda: torch.randn(p.shape, generator=g)
            if "embedding" in name and "patch" not in name:
                w = 0.5 * n()
            elif "norm" in name:
                w = 1.0 + 0.2 * n() if name.endswith("weight") else 0.1 * n()
            elif name.endswith("bias"):
                w = 0.1 * n()
            else:
                w = n() * GAIN / math.sqrt(math.prod(p.shape[1:]))
            p.copy_(w.half().float())
    return model


def save(model, path):
    """A directory fie_amd.clip_score.load reads: save_pretrained (safetensors) + the synthetic BPE files.  No preprocessor_config.json: defaults."""
    model.save_pretrained(str(path))
    shutil.copyfile(VOCAB, os.path.join(str(path), "vocab.json"))
    shutil.copyfile(MERGES, os.path.join(str(path), "merges.txt"))
    return str(path)


def tokenizer():
    import fie_amd  # noqa: F401
    from fie_amd.tokenizer import BpeTokenizer
    return BpeTokenizer(VOCAB, MERGES, EOS)


def processor_restated(arr, short=224, crop=224):
    """The processor in plain PIL / numpy, as the issue defines it: BICUBIC resize of the u8 image (shortest edge -> 224, the other
    int(224 * long / short)), centre crop at ((h - 224) // 2, (w - 224) // 2), /255, (x - mean) / std in fp32.  -> (resized u8 [h, w, 3],
    (top, left), pixel_values f32 [3, 224, 224])."""
    from fie_amd import clip_score as hclip
    h, w = arr.shape[:2]
    rh, rw = (int(short * h / w), short) if w <= h else (short, int(short * w / h))
    r = np.asarray(Image.fromarray(arr).resize((rw, rh), Image.BICUBIC))
    top, left = (rh - crop) // 2, (rw - crop) // 2
    x = r[top:top + crop, left:left + crop].astype(np.float32) / np.float32(255)
    x = (x - np.asarray(hclip.DEFAULT_MEAN, np.float32)) / np.asarray(hclip.DEFAULT_STD, np.float32)
    return r, (top, left), np.ascontiguousarray(x.transpose(2, 0, 1))


def processor_hf(arr):
    from transformers import CLIPImageProcessorPil
    return CLIPImageProcessorPil()(images=Image.fromarray(arr), return_tensors="pt")["pixel_values"][0].numpy()


def patch_rows(pixel_values, ps=16):
    """f32 [3, S, S] -> [P, 3 ps ps]: the patch rows in the K order of the patch-embedding weight viewed as [C, 3 ps ps]."""
    c, s, _ = pixel_values.shape
    g = s // ps
    return np.ascontiguousarray(pixel_values.reshape(c, g, ps, g, ps).transpose(1, 3, 0, 2, 4).reshape(g * g, c * ps * ps))


def image_features(model, arrs):
    """fp32 image embeddings [n, P] of u8 arrays through CLIPImageProcessorPil + get_image_features."""
    px = torch.from_numpy(np.stack([processor_hf(a) for a in arrs]))
    with torch.no_grad():
        out = model.get_image_features(pixel_values=px)
    return (out if torch.is_tensor(out) else out.pooler_output).float()


def text_features(model, prompts):
    ids = tokenizer()(list(prompts))
    with torch.no_grad():
        out = model.get_text_features(input_ids=ids)
    return (out if torch.is_tensor(out) else out.pooler_output).float()


def raw_scores(img, txt):
    """100 cos per pair, unclamped, in float64 from the fp32 embeddings."""
    a, b = img.double(), txt.double()
    return (100.0 * (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).numpy()


def masked(arr, mask):
    """PIE-Bench's edited variant: pixels outside the mask (any size; NEAREST-resized to the image, L >= 128 = edited) set to 0."""
    m = np.asarray(mask)
    if m.dtype == np.bool_:
        m = m.astype(np.uint8) * 255
    if m.shape != arr.shape[:2]:
        m = np.asarray(Image.fromarray(m, "L").resize((arr.shape[1], arr.shape[0]), Image.NEAREST))
    return arr * (m >= 128)[..., None].astype(np.uint8)


def kappa(emb):
    """sqrt(P) max |e| / ||e||_2 per row: turns a relative max-abs bound on an embedding into one on its direction (see score_bound)."""
    e = emb.double()
    return (math.sqrt(e.shape[1]) * e.abs().max(dim=1).values / e.norm(dim=1)).numpy()


def score_bound(img, txt, e_img, e_txt):
    """The score-level equivalent of embedding bounds e_img / e_txt (relative max-abs): an error d on embedding a with |d|_inf <= e max |a| has
    |d|_2 <= sqrt(P) e max |a|, and moves cos(a, b) by at most |d|_2 / |a|_2 to first order (the component along a does not count), i.e. by
    kappa(a) e.  Both sides, times 100, with 5 % for the second-order terms.  Per pair, from the ORACLE's embeddings only."""
    return 100.0 * 1.05 * (kappa(img) * e_img + kappa(txt) * e_txt)


def control(model, arrs, prompts):
    """What parity can see: (smallest relative max-abs difference between the oracle embeddings of two different images, smallest
    |score(pair) - score(swapped pair)| over the distinct (i, j))."""
    img, txt = image_features(model, arrs), text_features(model, prompts)
    emb = min(rel_err(img[i], img[j]) for i in range(len(arrs)) for j in range(len(arrs)) if i != j)
    s = np.array([[raw_scores(img[i:i + 1], txt[j:j + 1])[0] for j in range(len(prompts))] for i in range(len(arrs))])
    swap = min(abs(s[i, i] - s[j, i]) for i in range(len(arrs)) for j in range(len(arrs)) if i != j)
    return emb, swap, s
