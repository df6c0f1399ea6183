"""CPU side of the CLIP score: the BICUBIC / NEAREST tables against Pillow, the processor restatement against
CLIPImageProcessorPil, the config builder's refusals, the calculators that must keep returning None, evaluate.py's unchanged header, and the
control that decides whether the GPU parity tests can see a broken tower (tests/clip_score_oracle.py)."""
import csv
import json

import numpy as np
import pytest
from PIL import Image

import clip_score_oracle as co


@pytest.mark.parametrize("src,dst", [((512, 512), (224, 224)), ((1024, 1024), (224, 224)), ((333, 201), (371, 224)), ((100, 160), (224, 358))])
def test_bicubic_tables_are_pillows(src, dst):
    from fie_amd import resize
    a = co.image(5, src[1], src[0])
    assert np.array_equal(resize.resample_numpy(a, dst[1], dst[0], filter="bicubic"), np.asarray(Image.fromarray(a).resize(dst, Image.BICUBIC)))
    assert np.array_equal(resize.resample_numpy(a, dst[1], dst[0]), np.asarray(Image.fromarray(a).resize(dst, Image.LANCZOS)))
    with pytest.raises(ValueError):
        resize.coefficients(8, 4, filter="box")


@pytest.mark.parametrize("n_in,n_out", [(512, 1024), (300, 513), (1024, 300), (77, 200), (200, 77), (333, 1024)])
def test_nearest_indices_are_pillows(n_in, n_out):
    from fie_amd import resize
    m = np.random.default_rng(1).integers(0, 256, (n_in, n_in), dtype=np.uint8)
    t = resize.nearest_indices(n_in, n_out)
    assert np.array_equal(np.asarray(Image.fromarray(m, "L").resize((n_out, n_out), Image.NEAREST)), m[t][:, t])


@pytest.mark.parametrize("size", [(300, 200), (201, 333), (512, 512), (513, 320)])
def test_processor_restatement_is_the_processor(size):
    from fie_amd import clip_score as hclip
    a = co.image(3, size[1], size[0])
    r, (top, left), px = co.processor_restated(a)
    assert np.array_equal(px, co.processor_hf(a))
    assert hclip.resized_size(size[1], size[0], 224) == r.shape[:2] and hclip.crop_origin(*r.shape[:2], 224) == (top, left)
    rows = co.patch_rows(px)
    assert rows.shape == (196, 768) and rows[15, 256 + 16 * 3 + 5] == px[1, 16 + 3, 16 + 5]


def test_config_builder_refusals():
    from fie_amd import config as hconfig
    base = dict(text_config=dict(vocab_size=1414), projection_dim=512,
                vision_config=dict(hidden_size=768, num_attention_heads=12, image_size=224, patch_size=16, num_hidden_layers=12, intermediate_size=3072))
    cfg = hconfig.clip_vision_cfg(base)
    assert cfg["tokens"] == 197 and cfg["projection_dim"] == 512 and cfg["act"] == "quick_gelu"
    assert hconfig.clip_vision_cfg(dict(base, vision_config=dict(base["vision_config"], patch_size=32)))["tokens"] == 50
    for change, word in ((dict(num_attention_heads=8), "head dim"), (dict(image_size=230), "divisible"), (dict(hidden_act="relu"), "hidden_act"),
                         (dict(patch_size=14, image_size=224), "patch size")):
        with pytest.raises(ValueError, match=word):
            hconfig.clip_vision_cfg(dict(base, vision_config=dict(base["vision_config"], **change)))
    with pytest.raises(ValueError, match="vision_config"):
        hconfig.clip_vision_cfg({"hidden_size": 768})
    t = hconfig.clip_score_text_cfg(base)
    assert t["projection_dim"] == 512 and t["hidden"] == 512 and t["heads"] == 8
    with pytest.raises(ValueError, match="head dim"):
        hconfig.clip_score_text_cfg(dict(base, text_config=dict(hidden_size=512, num_attention_heads=4)))


def test_preprocessor_settings_and_truncation():
    import torch
    from fie_amd import clip_score as hclip
    pre = hclip.preprocessor(None)
    assert pre == dict(short=224, crop=224, mean=hclip.DEFAULT_MEAN, std=hclip.DEFAULT_STD)
    from transformers import CLIPImageProcessorPil
    d = json.loads(json.dumps(CLIPImageProcessorPil().to_dict(), default=int))
    assert hclip.preprocessor(d)["mean"] == pytest.approx(hclip.DEFAULT_MEAN)
    for bad in (dict(resample=2), dict(do_center_crop=False), dict(crop_size={"height": 256, "width": 256}), dict(rescale_factor=1.0)):
        with pytest.raises(ValueError):
            hclip.preprocessor(dict(d, **bad))
    ids = torch.arange(20).view(2, 10)
    ids[0, 3] = 99
    cut = hclip.truncate_ids(ids, 6, 99)
    assert cut.shape == (2, 6) and cut[0].tolist() == [0, 1, 2, 99, 4, 5] and cut[1].tolist() == [10, 11, 12, 13, 14, 99]
    assert hclip.truncate_ids(ids, 77, 99) is ids


def test_no_directory_means_no_number(monkeypatch, tmp_path):
    from fie_amd import clip_score as hclip
    from src.metrics import MetricsCalculator
    monkeypatch.delenv("FIE_CLIP_SCORE_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    assert hclip.resolve_dir(None) is None and hclip.resolve_dir("x") == "x"
    monkeypatch.setenv("FIE_WEIGHTS_DIR", str(tmp_path))
    assert hclip.resolve_dir(None) is None
    (tmp_path / "clip_score").mkdir()
    assert hclip.resolve_dir(None) == str(tmp_path / "clip_score")
    monkeypatch.setenv("FIE_CLIP_SCORE_DIR", "/somewhere")
    assert hclip.resolve_dir(None) == "/somewhere"
    calc = MetricsCalculator("cpu", clip_dir=str(tmp_path / "clip_score"))           # the CPU calculator never loads one
    a, b = Image.fromarray(co.image(1, 64, 64)), Image.fromarray(co.image(2, 64, 64))
    assert calc.calculate_clip_score(b, "p") is None and calc.calculate_clip_scores([a, b], ["p", "q"]) == [None, None]
    m = calc.calculate_all_metrics(a, b, "p", mask=np.ones((64, 64), np.uint8) * 255)
    assert m["clip_score"] is None and "clip_score_edited" not in m and list(m)[:6] == ["ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance"]
    with pytest.raises(FileNotFoundError):
        hclip.load(str(tmp_path / "clip_score"), None)


def test_evaluate_header_and_flags(tmp_path, monkeypatch):
    import evaluate
    import run_batch
    import run_single_image
    monkeypatch.delenv("FIE_CLIP_SCORE_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    flags = lambda p: {s for a in p._actions for s in a.option_strings}
    assert flags(evaluate.add_clip_args(evaluate.build_parser())) - flags(evaluate.build_parser()) == {"--clip_score_dir"}
    assert flags(run_batch.add_clip_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == {"--clip_score_dir"}
    assert "--clip_score_dir" in flags(run_single_image.build_parser())
    (tmp_path / "src" / "0_x").mkdir(parents=True)
    (tmp_path / "out" / "0_x").mkdir(parents=True)
    Image.fromarray(co.image(1, 64, 64)).save(tmp_path / "src" / "0_x" / "a.png")
    Image.fromarray(co.image(2, 64, 64)).save(tmp_path / "out" / "0_x" / "a.png")
    json.dump({"000": {"image_path": "0_x/a.png", "editing_prompt": "p", "editing_type_id": "0"}}, open(tmp_path / "map.json", "w"))
    evaluate.main(["--mapping_file", str(tmp_path / "map.json"), "--source_dir", str(tmp_path / "src"), "--outputs_dir", str(tmp_path / "out"),
                   "--results_file", str(tmp_path / "m.csv"), "--summary_file", str(tmp_path / "s.json"), "--device", "cpu"])
    rows = list(csv.reader(open(tmp_path / "m.csv")))
    assert rows[0] == ["image_id", "image_path", "editing_type_id", "editing_prompt", "ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance"]
    assert rows[1][6] == "" and json.load(open(tmp_path / "s.json"))["overall"]["clip_score"]["mean"] is None


def test_control_parity_can_tell_images_apart():
    """The oracle alone: embeddings of different test images, and the scores of a pair and of its swapped pair, differ by at least 10 x the
    bounds the GPU tests assert (tests/test_clip_score_gpu.py: BOUND, PAIRS)."""
    import test_clip_score_gpu as g
    model = co.build_model("tiny")
    arrs = [co.image(s, 512, 512) for s in (1, 3, 7)]
    img = co.image_features(model, arrs)
    apart = min(co.rel_err(img[i], img[j]) for i in range(3) for j in range(3) if i != j)
    print(f"[clip control] tiny: embeddings of different images differ by {apart:.3f} (relative max-abs); bound {g.BOUND[('tiny', 'f16')]}")
    assert apart >= 10 * g.BOUND[("tiny", "f16")]
    pa = [co.image(s, *hw) for s, hw, _ in g.PAIRS]
    prompts = [co.PROMPTS[t] for _, _, t in g.PAIRS]
    pi, pt = co.image_features(model, pa), co.text_features(model, prompts)
    s, swapped = co.raw_scores(pi, pt), co.raw_scores(pi[[1, 0]], pt)
    bound = co.score_bound(pi, pt, g.BOUND[("tiny", "f16")], g.BOUND[("text_tiny", "f16")])
    print(f"[clip control] scores {s}, with the images swapped {swapped}, score bound {bound}")
    assert all(abs(s[i] - swapped[i]) >= 10 * bound[i] for i in range(2))
