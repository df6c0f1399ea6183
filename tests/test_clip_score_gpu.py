"""CLIP score on the MI355X (csrc/clip_score.hip, fie_amd/clip.py::ClipVision, fie_amd/clip_score.py, MetricsCalculator, FastEditor) against the
fp32 CPU oracle of tests/clip_score_oracle.py (a seeded transformers.CLIPModel + CLIPImageProcessorPil).

Parity bounds (relative max-abs error of the embedding, the project's usual measure): BOUND below = 3 x the error measured on the MI355X,
rounded up to one significant digit (DESIGN.md section 11 records the measured values).  The score-level bound of the end-to-end tests is
derived from them and from the oracle's own embeddings (clip_score_oracle.score_bound).  The model tests compare UNCLAMPED scores, the clamp
has its own test on hand-made embeddings."""
import numpy as np
import pytest
import torch
from PIL import Image

import clip_score_oracle as co

pytestmark = pytest.mark.gpu

# (config, context) -> bound on the image embedding; "text" / "text_tiny": on the text embedding of the hidden-512 / 8-head tower and of the tiny one.
# Measured on the MI355X (largest over the cases of each test): tiny 1.63e-6 / 1.53e-3, b16 2.58e-6 / 1.35e-3, text 4.18e-6 / 3.31e-3,
# text_tiny 1.63e-6 / 1.85e-3 (fp32 / fp16 context); x 3, rounded up to one significant digit
BOUND = {("tiny", "f32"): 5e-6, ("tiny", "f16"): 5e-3, ("b16", "f32"): 8e-6, ("b16", "f16"): 5e-3, ("text", "f32"): 2e-5, ("text", "f16"): 1e-2,
         ("text_tiny", "f32"): 5e-6, ("text_tiny", "f16"): 6e-3}

SIZES = [((512, 512), (224, 224)), ((1024, 1024), (224, 224)), ((333, 201), (371, 224)), ((100, 160), (224, 358))]     # (w, h) -> (w, h)


@pytest.fixture(scope="module")
def ctxs(fie):
    from fie_amd import hip
    return {"f16": fie, "f32": hip.context(0, torch.float32)}


@pytest.fixture(scope="module")
def models():
    return {}


def _model(models, kind):
    if kind not in models:
        models[kind] = co.build_model(kind)
    return models[kind]


@pytest.fixture(scope="module")
def dirs(tmp_path_factory, models):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = co.save(_model(models, kind), tmp_path_factory.mktemp(f"clip_{kind}"))
        return made[kind]
    return get


@pytest.fixture(scope="module")
def scorers(ctxs, dirs):
    from fie_amd import clip_score as hclip
    made = {}

    def get(kind, prec):
        if (kind, prec) not in made:
            made[(kind, prec)] = hclip.load(dirs(kind), ctxs[prec])
        return made[(kind, prec)]
    return get


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(ctx.device)


@pytest.mark.parametrize("src,dst", SIZES)
def test_resize_bicubic_is_pillows(fie, src, dst):
    a = co.image(5, src[1], src[0])
    ref = np.asarray(Image.fromarray(a).resize(dst, Image.BICUBIC))
    got = fie.resize_bicubic(_dev(fie, a), dst[1], dst[0]).cpu().numpy()
    assert np.array_equal(got, ref)
    lan = fie.resize_lanczos(_dev(fie, a), dst[1], dst[0]).cpu().numpy()               # the LANCZOS tables keep their bits beside the new ones
    assert np.array_equal(lan, np.asarray(Image.fromarray(a).resize(dst, Image.LANCZOS)))


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("shape", [(371, 224), (320, 513)])                # source (h, w): resized to 371 x 224 (top 73) and 224 x 359 (left 67)
def test_clip_patches_against_the_processor(ctxs, prec, shape):
    from fie_amd import clip_score as hclip
    ctx = ctxs[prec]
    arrs = [co.image(20 + i, *shape) for i in range(3)]
    want, res = [], []
    for a in arrs:
        r, (top, left), px = co.processor_restated(a)
        res.append(r)
        want.append(co.patch_rows(px))
    assert (top, left) in ((73, 0), (0, 67)) and np.array_equal(co.processor_hf(arrs[0]), co.processor_restated(arrs[0])[2])
    batch = _dev(ctx, np.stack(res))
    got = ctx.clip_patches(batch, top, left, 224, 16, hclip.DEFAULT_MEAN, hclip.DEFAULT_STD).cpu()
    assert got.shape == (3 * 196, 768)
    ref = torch.from_numpy(np.concatenate(want))
    if prec == "f32":
        # one fp32 rounding: the device divides by 255 and by std as the restatement does; allow one ulp of the value (or of 1 near zero)
        ulp = torch.maximum(ref.abs(), torch.ones(())) * 2.0 ** -23
        err = ((got - ref).abs() / ulp).max().item()
        print(f"[clip] patches f32 {shape}: max error {err:.2f} ulp")
        assert err <= 1.0
    else:
        # exactly the f16 rounding of the f32 value (of either neighbour where the f32 value itself is one rounding away)
        lo, hi = (ref - ref.abs() * 2.0 ** -23).half(), (ref + ref.abs() * 2.0 ** -23).half()
        ok = (got == ref.half()) | (got == lo) | (got == hi)
        print(f"[clip] patches f16 {shape}: {int((got != ref.half()).sum())} of {got.numel()} values differ from half(f32 oracle)")
        assert bool(ok.all())
    for i in range(3):                                                    # image i alone and at every batch position: the same bits
        alone = ctx.clip_patches(batch[i:i + 1].contiguous(), top, left, 224, 16, hclip.DEFAULT_MEAN, hclip.DEFAULT_STD).cpu()
        assert torch.equal(alone, got[i * 196:(i + 1) * 196])
        for pos in range(3):
            order = [(i + k - pos) % 3 for k in range(3)]
            moved = ctx.clip_patches(batch[order].contiguous(), top, left, 224, 16, hclip.DEFAULT_MEAN, hclip.DEFAULT_STD).cpu()
            assert order[pos] == i and torch.equal(moved[pos * 196:(pos + 1) * 196], alone)
    from fie_amd import hip
    with pytest.raises(hip.FieError):                                     # a crop that would leave the image is refused, not read
        ctx.clip_patches(batch, res[0].shape[0] - 223, 0, 224, 16, hclip.DEFAULT_MEAN, hclip.DEFAULT_STD)


def _tower(scorers, models, kind, prec, arrs):
    sc = scorers(kind, prec)
    got = sc.image_embeddings([_dev(sc.ctx, a) for a in arrs]).float().cpu()
    ref = co.image_features(_model(models, kind), arrs)
    errs = [co.rel_err(got[i], ref[i]) for i in range(len(arrs))]
    print(f"[clip] tower {kind} {prec} n={len(arrs)}: relative max-abs error of the image embedding {max(errs):.3e} (bound {BOUND[(kind, prec)]:.0e})")
    return got, ref, max(errs)


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("n", [1, 3])
def test_image_tower_parity_tiny(scorers, models, prec, n):
    """M = 197 and 591: ragged attention tiles in Tq and Tk, a GEMM M tail."""
    arrs = [co.image(s, 512, 512) for s in (1, 3, 7)[:n]]
    got, ref, err = _tower(scorers, models, "tiny", prec, arrs)
    assert got.shape == ref.shape == (n, 64) and err <= BOUND[("tiny", prec)]
    if n == 3:
        apart = min(co.rel_err(ref[i], ref[j]) for i in range(3) for j in range(3) if i != j)
        assert apart >= 10 * BOUND[("tiny", "f16")]                     # the control: parity at this bound tells the images apart


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_image_tower_parity_vit_b16_shape(scorers, models, prec):
    arrs = [co.image(1, 512, 512), co.image(3, 512, 512)]
    got, ref, err = _tower(scorers, models, "b16", prec, arrs)
    assert got.shape == (2, 512) and err <= BOUND[("b16", prec)]
    assert co.rel_err(ref[0], ref[1]) >= 10 * BOUND[("b16", "f16")]


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_text_tower_parity_hidden_512(scorers, models, prec):
    """ClipText at hidden 512 / 8 heads through the scorer's loader; a 3-token prompt and one beyond 77 tokens (truncated, EOS kept)."""
    sc = scorers("b16", prec)
    prompts = ["a", co.LONG_PROMPT, co.PROMPTS[1]]                   # "a" is one token of the synthetic vocabulary: BOS a EOS
    ids = sc.token_ids(prompts)
    assert ids.shape == (3, 77) and int((ids[0] != co.EOS).sum()) == 2 and int(ids[0, 2]) == co.EOS and int(ids[1, -1]) == co.EOS and int((ids[1] == co.EOS).sum()) == 1
    got = sc.text_embeddings(prompts).float().cpu()
    ref = co.text_features(_model(models, "b16"), prompts)
    err = max(co.rel_err(got[i], ref[i]) for i in range(3))
    print(f"[clip] text tower hidden 512 {prec}: relative max-abs error {err:.3e} (bound {BOUND[('text', prec)]:.0e})")
    assert err <= BOUND[("text", prec)]
    assert torch.equal(sc.text_embedding(prompts[2]).float().cpu()[0], sc.text_embeddings([prompts[2]]).float().cpu()[0])


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_text_tower_parity_tiny(scorers, models, prec):
    """The tiny config's text tower (the one the end-to-end tests score with): all test prompts in one pass."""
    sc = scorers("tiny", prec)
    prompts = co.PROMPTS + [co.LONG_PROMPT]
    got = sc.text_embeddings(prompts).float().cpu()
    ref = co.text_features(_model(models, "tiny"), prompts)
    err = max(co.rel_err(got[i], ref[i]) for i in range(len(prompts)))
    print(f"[clip] text tower tiny {prec}: relative max-abs error {err:.3e} (bound {BOUND[('text_tiny', prec)]:.0e})")
    assert err <= BOUND[("text_tiny", prec)]


@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_scorer_op(ctxs, prec):
    ctx = ctxs[prec]
    g = torch.Generator().manual_seed(3)
    p = 512
    a = torch.randn(5, p, generator=g)
    b = torch.randn(5, p, generator=g)
    b[0] = 2.5 * a[0]                                  # parallel
    b[1] = b[1] - (b[1] @ a[1]) / (a[1] @ a[1]) * a[1]  # orthogonal (up to rounding)
    b[2] = -0.5 * a[2]                                 # anti-parallel
    b[3] = 0.0                                         # a zero vector
    a, b = a.to(ctx.dtype), b.to(ctx.dtype)
    rows = ctx.clip_score(a.to(ctx.device), b.to(ctx.device)).cpu()
    a64, b64 = a.double().numpy(), b.double().numpy()
    den = np.linalg.norm(a64, axis=1) * np.linalg.norm(b64, axis=1)
    want = np.where(den > 0, 100.0 * (a64 * b64).sum(1) / np.where(den > 0, den, 1), 0.0)
    print(f"[clip] scorer {prec}: {rows[:, 0].tolist()} want {want.tolist()}")
    assert rows.shape == (5, 2) and bool(torch.isfinite(rows).all())
    assert np.allclose(rows[:, 0].numpy(), want, rtol=1e-5, atol=1e-5 * 100)
    assert abs(rows[0, 0] - 100) <= 1e-3 and abs(rows[1, 0]) <= 1e-3 and abs(rows[2, 0] + 100) <= 1e-3 and rows[3, 0] == 0 and rows[3, 1] == 0
    assert torch.equal(rows[:, 1], rows[:, 0].clamp_min(0)) and rows[2, 1] == 0 and rows[4, 0] != 0
    for i in range(5):                                 # bit-identical rows whatever n and position
        da, db = a.to(ctx.device), b.to(ctx.device)
        assert torch.equal(ctx.clip_score(da[i:i + 1], db[i:i + 1]).cpu()[0], rows[i])
        perm = [(i + k) % 5 for k in range(3)]
        assert torch.equal(ctx.clip_score(da[perm].contiguous(), db[perm].contiguous()).cpu()[0], rows[i])
    with pytest.raises(ValueError):
        ctx.clip_score(a.to(ctx.device), b[:, :8].to(ctx.device))


PAIRS = [(89, (512, 512), 0), (60, (200, 300), 1)]        # (image seed, (h, w), prompt index): a 512 x 512 and a 300 x 200 image


def _oracle_pairs(models):
    model = _model(models, "tiny")
    arrs = [co.image(s, *hw) for s, hw, _ in PAIRS]
    prompts = [co.PROMPTS[t] for _, _, t in PAIRS]
    img, txt = co.image_features(model, arrs), co.text_features(model, prompts)
    return model, arrs, prompts, img, txt


def test_calculator_end_to_end(fie, dirs, models, monkeypatch):
    from src.metrics import MetricsCalculator
    monkeypatch.delenv("FIE_CLIP_SCORE_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    model, arrs, prompts, img, txt = _oracle_pairs(models)
    want = co.raw_scores(img, txt)
    bound = co.score_bound(img, txt, BOUND[("tiny", "f16")], BOUND[("text_tiny", "f16")])
    swapped = co.raw_scores(img[[1, 0]], txt)
    print(f"[clip] end to end: oracle {want}, swapped images {swapped}, score bound {bound}")
    assert all(abs(want[i] - swapped[i]) >= 10 * bound[i] for i in range(2))          # the control at score level
    calc = MetricsCalculator("cuda", clip_dir=dirs("tiny"))
    pils = [Image.fromarray(a) for a in arrs]
    raw = calc.calculate_clip_scores(pils, prompts, unclamped=True)
    got = calc.calculate_clip_scores(pils, prompts)
    for i in range(2):
        one = calc.calculate_clip_score(pils[i], prompts[i])
        print(f"[clip] pair {i}: device {raw[i]['clip_score']:.4f} oracle {want[i]:.4f} (bound {bound[i]:.3f}); clamped {got[i]['clip_score']:.4f} single {one:.4f}")
        assert abs(raw[i]["clip_score"] - want[i]) <= bound[i]
        assert got[i]["clip_score"] == max(raw[i]["clip_score"], 0.0) and abs(one - got[i]["clip_score"]) <= bound[i] and one >= 0
    # the masked variant: a mask of another size than the image, against the oracle on the masked image
    mask = np.zeros((512, 512), np.uint8)
    mask[100:400, 60:330] = 255
    for i in range(2):
        za = co.masked(arrs[i], mask)
        zi = co.image_features(model, [za])
        zwant, zbound = co.raw_scores(zi, txt[i:i + 1])[0], co.score_bound(zi, txt[i:i + 1], BOUND[("tiny", "f16")], BOUND[("text_tiny", "f16")])[0]
        r = calc.calculate_clip_scores([pils[i]], [prompts[i]], [mask], unclamped=True)[0]
        print(f"[clip] pair {i} edited: device {r['clip_score_edited']:.4f} oracle {zwant:.4f} (bound {zbound:.3f})")
        assert set(r) == {"clip_score", "clip_score_edited"} and abs(r["clip_score_edited"] - zwant) <= zbound and abs(r["clip_score"] - want[i]) <= bound[i]
        allm = calc.calculate_all_metrics(pils[i], pils[i], prompts[i], mask=mask)
        assert list(allm)[:6] == ["ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance"] and list(allm)[-1] == "clip_score_edited"
        assert abs(allm["clip_score"] - max(want[i], 0)) <= bound[i] and abs(allm["clip_score_edited"] - max(zwant, 0)) <= zbound
    plain = calc.calculate_all_metrics(pils[0], pils[0], prompts[0])
    assert "clip_score_edited" not in plain and abs(plain["clip_score"] - got[0]["clip_score"]) <= bound[0]
    none = MetricsCalculator("cuda")
    assert none.calculate_clip_score(pils[0], prompts[0]) is None and none.calculate_clip_scores(pils, prompts) == [None, None]


@pytest.fixture(scope="module")
def editors(fie, dirs):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False), FastEditor(model_name="tiny", enable_cpu_offload=False, clip_score_dir=dirs("tiny"))


def test_edit_with_inline_clip_score(editors, dirs, models):
    from src.metrics import MetricsCalculator
    plain_ed, ed = editors
    calc = MetricsCalculator("cuda", clip_dir=dirs("tiny"))
    img = Image.fromarray(co.image(31, 384, 640))
    prompt = co.PROMPTS[0]
    base, base_m = plain_ed.edit(img, prompt, seed=42, metrics=True)
    out, m = ed.edit(img, prompt, seed=42, metrics=True)
    assert set(base_m) == {"ssim", "psnr", "mse"} and set(m) == {"ssim", "psnr", "mse", "clip_score"}
    assert np.array_equal(np.asarray(out), np.asarray(base)) and all(m[k] == base_m[k] for k in base_m)
    assert isinstance(ed.edit(img, prompt, seed=42), Image.Image) and np.array_equal(np.asarray(ed.edit(img, prompt, seed=42)), np.asarray(base))
    raw = float(ed._clip_rows[(0, 1)][0, 0])                      # the unclamped value beside the score: a clamped 0 == 0 must not pass for parity
    want = calc.calculate_clip_scores([out], [prompt], unclamped=True)[0]["clip_score"]
    print(f"[clip] inline: {raw:.5f} vs calculator on the returned image {want:.5f}; clip_score {m['clip_score']:.5f}")
    assert abs(raw - want) <= 1e-5 * max(1.0, abs(want)) and m["clip_score"] == max(raw, 0.0)
    # ... and the calculator itself is within the score bound of the oracle on that image
    model = _model(models, "tiny")
    oi, ot = co.image_features(model, [np.asarray(out)]), co.text_features(model, [prompt])
    assert abs(want - co.raw_scores(oi, ot)[0]) <= co.score_bound(oi, ot, BOUND[("tiny", "f16")], BOUND[("text_tiny", "f16")])[0]
    mask = np.zeros((384, 640), np.uint8)
    mask[90:300, 200:520] = 255
    out2, m2 = ed.edit(img, prompt, seed=42, metrics=True, mask=mask)
    assert set(m2) == {"ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse", "clip_score", "clip_score_edited"}
    r2 = calc.calculate_clip_scores([out2], [prompt], [mask], unclamped=True)[0]
    rows = ed._clip_rows[(0, 2)]
    print(f"[clip] inline masked: {rows[:, 0].tolist()} vs calculator {r2}")
    assert abs(float(rows[0, 0]) - r2["clip_score"]) <= 1e-5 * max(1.0, abs(r2["clip_score"]))
    assert abs(float(rows[1, 0]) - r2["clip_score_edited"]) <= 1e-5 * max(1.0, abs(r2["clip_score_edited"]))


def test_edit_batch_clip_scores_in_input_order(editors, dirs, models):
    from src.metrics import MetricsCalculator
    _, ed = editors
    calc = MetricsCalculator("cuda", clip_dir=dirs("tiny"))
    imgs = [Image.fromarray(co.image(40 + i, 256, 256)) for i in range(3)]
    prompts = [co.PROMPTS[i] for i in (2, 0, 3)]
    outs, ms = ed.edit_batch(imgs, prompts, seed=7, strength=0.5, metrics=True)
    rows = ed._clip_rows[(0, 3)].clone()
    model = _model(models, "tiny")
    for i in range(3):
        oi, ot = co.image_features(model, [np.asarray(outs[i])]), co.text_features(model, [prompts[i]])
        want, bound = co.raw_scores(oi, ot)[0], co.score_bound(oi, ot, BOUND[("tiny", "f16")], BOUND[("text_tiny", "f16")])[0]
        one = calc.calculate_clip_scores([outs[i]], [prompts[i]], unclamped=True)[0]["clip_score"]
        print(f"[clip] batch image {i}: inline {float(rows[i, 0]):.4f} calculator {one:.4f} oracle {want:.4f} (bound {bound:.3f})")
        assert abs(float(rows[i, 0]) - want) <= bound and abs(one - want) <= bound and ms[i]["clip_score"] == max(float(rows[i, 0]), 0.0)
