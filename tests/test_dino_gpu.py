"""DINO structure distance on the MI355X (csrc/dino.hip, fie_amd/dino.py, MetricsCalculator, FastEditor) against the CPU oracle of
tests/dino_oracle.py (a seeded transformers.ViTModel, F.interpolate(antialias=True), the distance as DESIGN.md section 12 defines it).

Every bound comes from the oracle alone and is computed at run time: 4 x the oracle's own error at the precision of the device context against its
float64 self (the factor allows for another summation order and tile shape; the margin of DESIGN.md section 10).  DESIGN.md section 12 records the
device errors measured beside them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import dino_oracle as do

pytestmark = pytest.mark.gpu

PAIRS = ("ab", "ac", "ad")


@pytest.fixture(scope="module")
def ctxs(fie):
    from fie_amd import hip
    return {"f16": fie, "f32": hip.context(0, torch.float32)}


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = do.save(do.model_of(kind), tmp_path_factory.mktemp(f"dino_{kind}"))
        return made[kind]
    return get


@pytest.fixture(scope="module")
def scorers(ctxs, dirs):
    from fie_amd import dino as hdino
    made = {}

    def get(kind, prec):
        if (kind, prec) not in made:
            made[(kind, prec)] = hdino.load(dirs(kind), ctxs[prec], layer=do.LAYER[kind])
        return made[(kind, prec)]
    return get


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(ctx.device)


# ---------------------------------------------------------------------------------------------------------------------- preprocess op
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("n_in,n_out", [(512, 224), (203, 64), (40, 64), (64, 64)])
def test_patches_against_torch(ctxs, n_in, n_out, n):
    """f32: every resized, normalised pixel within 4 d0 of the float64 oracle, d0 = torch's own fp32 error against float64 on the same images;
    f16: the round-to-nearest-even of the f32 output, bit for bit; the K order is `unfold`'s."""
    from fie_amd import dino as hdino
    rng = np.random.default_rng(n_in * 7 + n)
    arrs = [rng.integers(0, 256, (n_in, n_in, 3), dtype=np.uint8) for _ in range(n)]
    ref64 = torch.cat([F.unfold(do.preprocess(a, n_out, torch.float64)[None], kernel_size=8, stride=8)[0].T for a in arrs])
    ref32 = torch.cat([do.patch_rows(do.preprocess(a, n_out, torch.float32)) for a in arrs]).double()
    d0 = (ref32 - ref64).abs().max().item()
    batch = _dev(ctxs["f32"], np.stack(arrs))
    got32 = ctxs["f32"].dino_patches(batch, n_out, n_out, 8, hdino.IMAGENET_MEAN, hdino.IMAGENET_STD).cpu()
    got16 = ctxs["f16"].dino_patches(batch, n_out, n_out, 8, hdino.IMAGENET_MEAN, hdino.IMAGENET_STD).cpu()
    p = (n_out // 8) ** 2
    assert got32.shape == ref64.shape == (n * p, 192) and got32.dtype == torch.float32 and got16.dtype == torch.float16
    err = (got32.double() - ref64).abs().max().item()
    print(f"[dino] patches {n_in} -> {n_out} n={n}: device error {err:.3e} against float64, d0 {d0:.3e} (bound 4 d0 = {4 * d0:.3e})")
    assert err <= 4 * d0
    assert torch.equal(got16, got32.half())
    if n > 1:                                                             # image i alone: the same bits as at position i of the batch
        for i in range(n):
            alone = ctxs["f32"].dino_patches(batch[i:i + 1].contiguous(), n_out, n_out, 8, hdino.IMAGENET_MEAN, hdino.IMAGENET_STD).cpu()
            assert torch.equal(alone, got32[i * p:(i + 1) * p])


# ---------------------------------------------------------------------------------------------------------------------- scorer op
def _ref_distance(ka, kb, dtype):
    return do.distance(ka.to(dtype), kb.to(dtype))


@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("t,c", [(17, 128), (65, 128), (785, 768)])
def test_selfsim_op(ctxs, prec, t, c):
    """The fused self-similarity MSE on given key matrices against float64 torch on the same (already rounded) keys.  Bound: 4 x the error of the
    fp32 torch restatement, relative to the float64 value."""
    ctx = ctxs[prec]
    g = torch.Generator().manual_seed(t * 1000 + c)
    base = torch.randn(t, c, generator=g) + 0.5 * torch.randn(1, c, generator=g)           # a common component: S is not near 0 off the diagonal
    mk = lambda s: (base + s * torch.randn(t, c, generator=g)).to(ctx.dtype)
    ka = [base.to(ctx.dtype), mk(0.1), mk(1.0)]
    kb = [mk(0.05), mk(0.5), mk(2.0)]
    kb[1][3] = 0                                                         # one zero key row: S = 0 in its row and column, never NaN
    want = [_ref_distance(a, b, torch.float64) for a, b in zip(ka, kb)]
    tol = [4 * abs(_ref_distance(a, b, torch.float32) - w) for a, b, w in zip(ka, kb, want)]
    da, db = torch.stack(ka).to(ctx.device), torch.stack(kb).to(ctx.device)              # [3, T, C]
    got = ctx.selfsim_mse(da.view(3 * t, c), db.view(3 * t, c), 3).cpu()
    assert got.dtype == torch.float64 and got.shape == (3,) and bool(torch.isfinite(got).all())
    for i in range(3):
        print(f"[dino] selfsim {prec} T={t} C={c} pair {i}: device {got[i].item():.9e} float64 {want[i]:.9e} error {abs(got[i].item() - want[i]) / want[i]:.3e} "
              f"(bound {tol[i] / want[i]:.3e} relative)")
    assert all(abs(got[i].item() - want[i]) <= tol[i] for i in range(3))
    again = ctx.selfsim_mse(da.view(3 * t, c), db.view(3 * t, c), 3).cpu()
    assert torch.equal(again, got)                                       # two runs: equal bits
    # ld = 3 C: the keys as the middle column range of a fused q/k/v output; n = 1 and another position: equal bits
    qkv_a = torch.randn(3 * t, 3 * c, generator=g).to(ctx.dtype).to(ctx.device)
    qkv_b = torch.randn(3 * t, 3 * c, generator=g).to(ctx.dtype).to(ctx.device)
    qkv_a[:, c:2 * c], qkv_b[:, c:2 * c] = da.view(3 * t, c), db.view(3 * t, c)
    wide = ctx.selfsim_mse(qkv_a[:, c:2 * c], qkv_b[:, c:2 * c], 3).cpu()
    assert torch.equal(wide, got)
    for i in range(3):
        one = ctx.selfsim_mse(da[i], db[i], 1).cpu()
        assert torch.equal(one[0], got[i])
        order = [(i + 1) % 3, (i + 2) % 3, i]
        moved = ctx.selfsim_mse(da[order].reshape(3 * t, c), db[order].reshape(3 * t, c), 3).cpu()
        assert torch.equal(moved[2], got[i])
    same = ctx.selfsim_mse(db.view(3 * t, c), db.view(3 * t, c).clone(), 3).cpu()
    assert same.tolist() == [0.0, 0.0, 0.0]                              # an identical pair (zero row included): exactly 0
    with pytest.raises(ValueError):
        ctx.selfsim_mse(da.view(3 * t, c), db.view(3 * t, c)[:, :c // 2], 3)


# ---------------------------------------------------------------------------------------------------------------------- tower
@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("kind", ["tiny", "b8"])
def test_tower_keys_against_oracle(scorers, kind, prec):
    """Keys of block `layer` for n = 2 (images a and d as sources, b and c as edits: four images in one pass): relative max-abs error against the
    float64 oracle within 4 x the oracle's own error at that precision."""
    sc = scorers(kind, prec)
    ims = do.images(do.SOURCE[kind])
    order = ("a", "d", "b", "c")
    k = sc.keys([_dev(sc.ctx, ims["a"]), _dev(sc.ctx, ims["d"])], [_dev(sc.ctx, ims["b"]), _dev(sc.ctx, ims["c"])]).cpu()
    t, c = sc.vit.cfg["tokens"], sc.vit.cfg["hidden"]
    assert k.shape == (4 * t, c) and k.dtype == sc.ctx.dtype
    k64 = do.keys_of(kind, "f64")
    bound = 4 * do.key_errors(kind, prec)
    errs = [do.rel_err(k[i * t:(i + 1) * t], k64[n]) for i, n in enumerate(order)]
    print(f"[dino] tower keys {kind} {prec}: relative max-abs error {max(errs):.3e} (oracle's own {bound / 4:.3e}, bound {bound:.3e})")
    assert max(errs) <= bound
    assert do.rel_err(k64["a"], k64["b"]) >= 10 * 4 * do.key_errors(kind, "f16")            # the control: the keys tell a from b at that bound


# ---------------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("prec", ["f32", "f16"])
@pytest.mark.parametrize("kind", ["tiny", "b8"])
def test_scorer_distances_against_oracle(scorers, kind, prec):
    """DinoScorer.distances in both contexts: a-b, a-c, a-d within 4 e_p d_64, a-a exactly 0."""
    sc = scorers(kind, prec)
    ims = {n: _dev(sc.ctx, v) for n, v in do.images(do.SOURCE[kind]).items()}
    got = sc.distances([ims["a"]] * 4, [ims["b"], ims["c"], ims["d"], ims["a"]]).cpu().tolist()
    d64, e = do.distances_of(kind, "f64"), do.distance_errors(kind, prec)
    for p, v in zip(PAIRS, got):
        print(f"[dino] distance {kind} {prec} {p}: device {v:.9e} float64 {d64[p]:.9e} error {abs(v - d64[p]) / d64[p]:.3e} (e_p {e:.3e}, bound {4 * e:.3e})")
    assert all(abs(v - d64[p]) <= 4 * e * d64[p] for p, v in zip(PAIRS, got))
    assert got[3] == 0.0


def test_calculator_end_to_end(fie, dirs, monkeypatch):
    from src.metrics import MetricsCalculator
    monkeypatch.delenv("FIE_DINO_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    calc = MetricsCalculator("cuda", dino_dir=dirs("tiny"), dino_layer=do.LAYER["tiny"])
    pil = {n: Image.fromarray(v) for n, v in do.images(do.SOURCE["tiny"]).items()}
    d64, e = do.distances_of("tiny", "f64"), do.distance_errors("tiny", "f16")
    single = {p: calc.calculate_dino_distance(pil["a"], pil[p[1]]) for p in PAIRS + ("aa",)}
    print(f"[dino] calculator: {single} oracle {d64} (e_16 {e:.3e})")
    assert all(abs(single[p] - d64[p]) <= 4 * e * d64[p] for p in PAIRS) and single["aa"] == 0.0
    small = pil["c"].resize((96, 96), Image.BILINEAR)                                  # another edited size: its own group, the order kept
    many = calc.calculate_dino_distances([pil["a"]] * 5, [pil["b"], small, pil["c"], pil["d"], pil["a"]])
    assert [many[0], many[2], many[3], many[4]] == [single["ab"], single["ac"], single["ad"], 0.0]          # bit for bit the single calls
    assert many[1] == calc.calculate_dino_distance(pil["a"], small) and many[1] > 0
    wide = Image.fromarray(do.images(203)["a"][:150])
    with pytest.raises(ValueError, match="203 x 150"):
        calc.calculate_dino_distance(pil["a"], wide)
    allm = calc.calculate_all_metrics(pil["a"], pil["c"], "p")
    assert list(allm) == ["ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance"] and allm["dino_distance"] == single["ac"]
    assert calc.calculate_all_metrics(pil["a"], wide, "p")["dino_distance"] is None
    none = MetricsCalculator("cuda")
    assert none.calculate_dino_distance(pil["a"], pil["b"]) is None and none.calculate_dino_distances([pil["a"]], [pil["b"]]) == [None]
    assert none.calculate_all_metrics(pil["a"], pil["c"], "p")["dino_distance"] is None


# ---------------------------------------------------------------------------------------------------------------------- in the edit
@pytest.fixture(scope="module")
def editors(fie, dirs):
    from src.pipeline import FastEditor
    return (FastEditor(model_name="tiny", enable_cpu_offload=False),
            FastEditor(model_name="tiny", enable_cpu_offload=False, dino_dir=dirs("tiny"), dino_layer=do.LAYER["tiny"]))


def test_edit_with_inline_dino_distance(editors, dirs):
    from src.metrics import MetricsCalculator
    plain_ed, ed = editors
    calc = MetricsCalculator("cuda", dino_dir=dirs("tiny"), dino_layer=do.LAYER["tiny"])
    img = Image.fromarray(do.images(256)["c"])
    base, base_m = plain_ed.edit(img, "a red kite", seed=42, metrics=True)
    out, m = ed.edit(img, "a red kite", seed=42, metrics=True)
    assert list(base_m) == ["ssim", "psnr", "mse"] and list(m) == ["ssim", "psnr", "mse", "dino_distance"]
    assert np.array_equal(np.asarray(out), np.asarray(base)) and all(m[k] == base_m[k] for k in base_m)
    plain = ed.edit(img, "a red kite", seed=42)
    assert isinstance(plain, Image.Image) and np.array_equal(np.asarray(plain), np.asarray(base))
    want = calc.calculate_dino_distance(img, out)                        # the ORIGINAL 256 x 256 source against the 1024 x 1024 result
    print(f"[dino] inline: {m['dino_distance']!r} vs calculator on the returned image {want!r}")
    assert m["dino_distance"] == want and want > 0
    wide = Image.fromarray(do.images(256)["c"][:192])                    # 256 x 192: not square
    _, m2 = ed.edit(wide, "a red kite", seed=42, metrics=True)
    assert list(m2) == ["ssim", "psnr", "mse", "dino_distance"] and m2["dino_distance"] is None


def test_edit_batch_dino_distances(editors, dirs):
    from src.metrics import MetricsCalculator
    _, ed = editors
    calc = MetricsCalculator("cuda", dino_dir=dirs("tiny"), dino_layer=do.LAYER["tiny"])
    ims = do.images(256)
    imgs = [Image.fromarray(ims["a"]), Image.fromarray(ims["c"][:192]), Image.fromarray(ims["d"])]
    prompts = ["a red kite", "an orange cat", "two toy boats"]
    outs, ms = ed.edit_batch(imgs, prompts, seed=7, strength=0.5, metrics=True)
    assert ms[1]["dino_distance"] is None and all(list(m) == ["ssim", "psnr", "mse", "dino_distance"] for m in ms)
    # the two square pairs were scored in one pass: bit for bit what the calculator gives for the same two pairs on the returned images
    want = calc.calculate_dino_distances([imgs[0], imgs[2]], [outs[0], outs[2]])
    print(f"[dino] batch: inline {[ms[0]['dino_distance'], ms[2]['dino_distance']]!r}, calculator {want!r}")
    assert [ms[0]["dino_distance"], ms[2]["dino_distance"]] == want and all(w > 0 for w in want)
    # ... and the single edit of an image, whose result equals the batch's (edit_batch's contract: up to fp16 tiling effects), gives the same distance
    for i in (0, 2):
        one_out, one = ed.edit(imgs[i], prompts[i], seed=7, strength=0.5, metrics=True)
        print(f"[dino] batch image {i}: single edit {one['dino_distance']!r}, same image: {np.array_equal(np.asarray(one_out), np.asarray(outs[i]))}")
        if np.array_equal(np.asarray(one_out), np.asarray(outs[i])):
            assert one["dino_distance"] == ms[i]["dino_distance"]
