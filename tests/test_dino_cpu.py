"""DINO structure distance, the device-free half: the antialias tap tables of fie_amd/resize.py against torch, the config
checks, the directory lookup, the loader's key mapping, the command-line plumbing, and the oracle's own controls (tests/dino_oracle.py)."""
import csv
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import dino_oracle as do

import fie_amd  # noqa: F401,E402


def _interp(x, out, dtype):
    t = torch.from_numpy(x).permute(2, 0, 1)[None].to(dtype)
    return F.interpolate(t, size=(out, out), mode="bilinear", antialias=True, align_corners=False)[0].permute(1, 2, 0)


@pytest.mark.parametrize("n_in,n_out", [(512, 224), (203, 64), (40, 64), (64, 64)])
def test_aa_tables_match_torch(n_in, n_out):
    """The tables, applied in numpy fp32 in ATen's order, against F.interpolate(antialias=True): within 4 d0 of the float64 result, d0 torch's own
    fp32 error against float64 on the same input.  Down-scaling, up-scaling and the identity (exact) from one formula."""
    from fie_amd import resize
    x = np.random.default_rng(n_in).random((n_in, n_in, 3)).astype(np.float32)
    r64 = _interp(x, n_out, torch.float64)
    d0 = (_interp(x, n_out, torch.float32).double() - r64).abs().max().item()
    got = torch.from_numpy(resize.aa_resample_numpy(x, n_out, n_out)).double()
    err = (got - r64).abs().max().item()
    ww, bounds, ks = resize.aa_coefficients(n_in, n_out)
    print(f"[dino] aa tables {n_in} -> {n_out}: {ks} taps, error {err:.3e} against float64, d0 {d0:.3e}")
    assert ww.dtype == np.float32 and ww.shape == (n_out, ks) and bounds.shape == (n_out, 2)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all() and (bounds[:, 1] >= 1).all() and (bounds[:, 1] <= ks).all()
    assert np.allclose(ww.sum(1), 1.0, atol=1e-6)
    assert err <= 4 * d0
    if n_in == n_out:
        assert d0 == 0.0 and np.array_equal(resize.aa_resample_numpy(x, n_out, n_out), x)
    if n_in < n_out:
        assert ks == 3                                                     # up-scaling: support 1


def test_dino_vit_cfg_accepts_and_refuses():
    from fie_amd import config as hconfig
    for kind, tokens in (("tiny", 65), ("b8", 785)):
        cfg = hconfig.dino_vit_cfg(dict(do.CONFIGS[kind], hidden_act="gelu", layer_norm_eps=1e-12), layer=do.LAYER[kind])
        assert cfg["tokens"] == tokens and cfg["layer"] == do.LAYER[kind] and cfg["eps"] == 1e-12 and cfg["patch_size"] == 8
    assert hconfig.dino_vit_cfg({}, layer=11)["tokens"] == 197                 # ViTConfig's defaults: B/16
    base = dict(do.CONFIGS["b8"])
    for bad, word in ((dict(num_attention_heads=8), "head dim"), (dict(patch_size=12), "patch_size 12"), (dict(image_size=220), "image_size 220"),
                      (dict(hidden_act="quick_gelu"), "hidden_act 'quick_gelu'"), (dict(hidden_act="gelu_new"), "hidden_act 'gelu_new'")):
        with pytest.raises(ValueError, match=word):
            hconfig.dino_vit_cfg(dict(base, **bad))
    for layer in (12, -1, 99):
        with pytest.raises(ValueError, match=f"layer {layer}"):
            hconfig.dino_vit_cfg(base, layer=layer)
    with pytest.raises(ValueError, match="layer 11"):                          # the default layer against the two-layer config
        hconfig.dino_vit_cfg(do.CONFIGS["tiny"])


def test_resolve_dir_precedence(monkeypatch, tmp_path):
    from fie_amd import dino as hdino
    monkeypatch.delenv("FIE_DINO_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    assert hdino.resolve_dir(None) is None and hdino.resolve_dir("x") == "x"
    monkeypatch.setenv("FIE_WEIGHTS_DIR", str(tmp_path))
    assert hdino.resolve_dir(None) is None
    (tmp_path / "dino").mkdir()
    assert hdino.resolve_dir(None) == str(tmp_path / "dino")
    monkeypatch.setenv("FIE_DINO_DIR", "/somewhere")
    assert hdino.resolve_dir(None) == "/somewhere" and hdino.resolve_dir("x") == "x"
    with pytest.raises(FileNotFoundError):
        hdino.load(str(tmp_path / "dino"), None)
    assert hdino.resized_size(512, 512, 224) == (224, 224) and hdino.resized_size(300, 200, 224) == (336, 224) and hdino.resized_size(100, 160, 224) == (224, 358)
    assert hdino.supported_size(203, 203) and not hdino.supported_size(200, 300)


def test_loader_key_mapping(tmp_path):
    """The names of a save_pretrained directory (the hub file's) and the module names of the local transformers both reach the same tensors."""
    from safetensors.torch import load_file
    from fie_amd import config as hconfig
    from fie_amd import dino as hdino
    model = do.build_model("tiny")
    path = do.save(model, tmp_path / "vit")
    cfg = hconfig.dino_vit_cfg(json.load(open(tmp_path / "vit" / "config.json")), layer=1)
    sd = load_file(str(tmp_path / "vit" / "model.safetensors"))
    assert path and "encoder.layer.0.attention.attention.key.weight" in sd
    t = hdino.tower_tensors(sd, cfg)
    blk0, q0, k0 = do.block(model, 0)
    blk1, _, k1 = do.block(model, 1)
    assert torch.equal(t["0.q.weight"], q0.weight) and torch.equal(t["0.k.bias"], k0.bias) and torch.equal(t["1.k.weight"], k1.weight)
    assert torch.equal(t["1.ln1.bias"], blk1.layernorm_before.bias) and torch.equal(t["0.ln2.weight"], blk0.layernorm_after.weight)
    assert torch.equal(t["patch.bias"], model.embeddings.patch_embeddings.projection.bias) and t["patch.weight"].shape == (128, 3, 8, 8)
    assert t["cls"].shape == (128,) and t["pos"].shape == (65, 128) and torch.equal(t["pos"], model.embeddings.position_embeddings[0])
    fc1 = {n: p for n, p in model.named_parameters() if n.endswith("0.mlp.fc1.weight") or n.endswith("0.intermediate.dense.weight")}
    assert len(fc1) == 1 and torch.equal(t["0.fc1.weight"], next(iter(fc1.values()))) and t["0.fc2.weight"].shape == (128, 256)
    assert "1.q.weight" not in t and "1.fc1.weight" not in t and not any(k.startswith("2.") for k in t)       # the walk stops at block `layer`'s keys
    by_module = hdino.tower_tensors(dict(model.state_dict()), cfg)                                             # the new-style names
    assert set(by_module) == set(t) and all(torch.equal(by_module[k].reshape(t[k].shape), t[k]) for k in t)
    with pytest.raises(KeyError, match="layernorm_before"):
        hdino.tower_tensors({k: v for k, v in sd.items() if "layer.1.layernorm_before" not in k}, cfg)


def test_cpu_calculator_gives_none(monkeypatch, tmp_path):
    from src.metrics import MetricsCalculator
    monkeypatch.delenv("FIE_DINO_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    calc = MetricsCalculator("cpu", dino_dir=str(tmp_path))                      # the CPU calculator never loads one
    ims = do.images(64)
    a, b = Image.fromarray(ims["a"]), Image.fromarray(ims["b"])
    assert calc.calculate_dino_distance(a, b) is None and calc.calculate_dino_distances([a, b], [b, a]) == [None, None]
    m = calc.calculate_all_metrics(a, b, "p")
    assert m["dino_distance"] is None and list(m) == ["ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance"]
    with pytest.raises(ValueError):
        calc.calculate_dino_distances([a], [a, b])


class _StubDino:
    """Stands in for a DinoScorer on the CPU calculator: evaluate.py only asks the calculator."""


def test_evaluate_fills_the_column(tmp_path, monkeypatch):
    import evaluate
    import run_batch
    import run_single_image
    from src.metrics import MetricsCalculator
    monkeypatch.delenv("FIE_DINO_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    flags = lambda p: {s for a in p._actions for s in a.option_strings}
    assert flags(evaluate.add_dino_args(evaluate.build_parser())) - flags(evaluate.build_parser()) == {"--dino_dir"}
    assert flags(run_batch.add_dino_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == {"--dino_dir"}
    assert "--dino_dir" in flags(run_single_image.build_parser())
    (tmp_path / "src" / "0_x").mkdir(parents=True)
    (tmp_path / "out" / "0_x").mkdir(parents=True)
    ims = do.images(64)
    for name, arr in (("a.png", ims["a"]), ("b.png", ims["c"]), ("c.png", ims["a"][:48])):      # c.png: 64 x 48, not square
        Image.fromarray(arr).save(tmp_path / "src" / "0_x" / name)
        Image.fromarray(arr[::-1].copy()).save(tmp_path / "out" / "0_x" / name)
    json.dump({f"00{i}": {"image_path": f"0_x/{n}", "editing_prompt": "p", "editing_type_id": "0"} for i, n in enumerate(("a.png", "b.png", "c.png"))},
              open(tmp_path / "map.json", "w"))
    seen = []

    def fake_distances(self, sources, editeds):
        seen.append([im.size for im in sources])
        return [0.25 + 0.5 * i for i in range(len(sources))]

    real_init = MetricsCalculator.__init__

    def init(self, device="cuda", clip_dir=None, dino_dir=None, **kw):
        real_init(self, device, clip_dir=clip_dir, dino_dir=dino_dir, **kw)
        seen.append(dino_dir)
        self._dino = _StubDino()

    monkeypatch.setattr(MetricsCalculator, "__init__", init)
    monkeypatch.setattr(MetricsCalculator, "calculate_dino_distances", fake_distances)
    evaluate.main(["--mapping_file", str(tmp_path / "map.json"), "--source_dir", str(tmp_path / "src"), "--outputs_dir", str(tmp_path / "out"),
                   "--results_file", str(tmp_path / "m.csv"), "--summary_file", str(tmp_path / "s.json"), "--device", "cpu", "--dino_dir", "/some/dir"])
    rows = list(csv.reader(open(tmp_path / "m.csv")))
    assert rows[0] == ["image_id", "image_path", "editing_type_id", "editing_prompt", "ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance"]
    assert seen == ["/some/dir", [(64, 64), (64, 64)]]                     # the flag reached the calculator; only the square pairs were asked for
    assert [r[9] for r in rows[1:]] == ["0.25", "0.75", ""]
    assert json.load(open(tmp_path / "s.json"))["overall"]["dino_distance"]["mean"] == pytest.approx(0.5)


@pytest.mark.parametrize("kind", ["tiny", "b8"])
def test_oracle_controls(kind):
    """What parity can see, from the oracle alone.  With bound(pair) = 4 e_16 d_64(pair), the widest bound the GPU tests assert:
      * the three distances a-b / a-c / a-d lie more than 10 bounds apart from each other, so a swapped or repeated pair cannot pass;
      * a tower that stops one block early (keys of block layer - 1) or hands over the QUERIES of block `layer` misses the a-b distance -- the pair
        the bound is tightest on in absolute terms -- by more than 10 bounds, and misses at least that much on the worst pair.
    (The GPU tests assert every pair, so one pair that sees the fault is enough; a-b is asserted by name so that the control cannot pass on the
    pair of random bytes alone.)"""
    d64 = do.distances_of(kind, "f64")
    e32, e16 = do.distance_errors(kind, "f32"), do.distance_errors(kind, "f16")
    bound = {p: 4 * e16 * d64[p] for p in ("ab", "ac", "ad")}
    print(f"[dino control] {kind}: d64 {d64}, e_32 {e32:.3e}, e_16 {e16:.3e}, key errors {do.key_errors(kind, 'f32'):.3e} / {do.key_errors(kind, 'f16'):.3e}")
    assert d64["aa"] == 0.0 and 0 < e32 < e16 < 0.05
    for p, q in (("ab", "ac"), ("ac", "ad"), ("ab", "ad")):
        assert abs(d64[p] - d64[q]) > 10 * max(bound[p], bound[q])
    for what, alt in (("block layer - 1", do.distances_of(kind, "f64", layer=do.LAYER[kind] - 1)), ("queries", do.distances_of(kind, "f64", which="query"))):
        miss = {p: abs(alt[p] - d64[p]) / bound[p] for p in bound}
        print(f"[dino control] {kind}: keys from {what} miss by {miss} bounds")
        assert miss["ab"] > 10 and max(miss.values()) > 10
