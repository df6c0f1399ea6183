"""Aspect-ratio edits on the SDXL resolution buckets: the halo-resident conv with edge patches (tile code 78), the rest of
the hot path at bucket shapes, and FastEditor.edit / edit_batch(resolution=...) on the tiny and the SSD-1B stacks."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from test_pipeline_gpu import synth_image

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def synth_rect(seed, w, h):
    return synth_image(seed, max(w, h)).resize((w, h), Image.LANCZOS)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# tile code 78

# (batch, OH, OW, Cin, Cout, epilogue): the UNet maps of 1152x896 (72x56), 1216x832 (76x52, 38x26), the VAE's 152x104 / 168x96, a map with only one
# side off 16 (48 x 40), 320 channels (a column tile half past N), one tile per block and -- 2 x 152x104 x 320: 420 tiles -- several per block, so the
# half-empty column tile's stores are deferred into the next tile; 168x96 x 512 and 104x152 x 640 x 2 have more tiles than CUs as well
_SHAPES78 = [(2, 56, 72, 640, 640, "bias,res"), (2, 52, 76, 320, 320, "bias,rowbias"), (2, 26, 38, 1280, 1280, "bias,res"),
             (1, 104, 152, 512, 512, "bias"), (1, 96, 168, 512, 512, "bias,res"), (1, 48, 40, 128, 256, "bias,res"), (1, 40, 48, 256, 128, ""),
             (2, 104, 152, 320, 640, "bias,rowbias"), (2, 104, 152, 320, 320, "bias,res"), (2, 96, 168, 320, 320, "bias,rowbias")]


@pytest.mark.parametrize("b,h,w,cin,cout,opts", _SHAPES78)
def test_code78_conv_vs_torch(fie, b, h, w, cin, cout, opts):
    from fie_amd import hip
    g = torch.Generator().manual_seed(h * w + cin)
    x = torch.randn(b, h, w, cin, generator=g).half().to(DEV)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half()
    bias = torch.randn(cout, generator=g).half().to(DEV) if "bias" in opts else None
    res = torch.randn(b, h, w, cout, generator=g).half().to(DEV) if "res" in opts else None
    rb = torch.randn(b, cout, generator=g).half().to(DEV) if "rowbias" in opts else None
    wp = fie.pack_conv3x3(wt.to(DEV))
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float().to(DEV), bias.float() if bias is not None else None, padding=1)
    if rb is not None:
        ref = ref + rb.float()[:, :, None, None]
    if res is not None:
        ref = ref + res.float().permute(0, 3, 1, 2)
    try:
        fie.force_tile(78)
        outs = []
        for _ in range(4):
            o = torch.full((b, h, w, cout), float("nan"), dtype=torch.float16, device=DEV)     # every pixel must be written
            outs.append(fie.conv3x3(x, wp, cout, out=o, bias=bias, residual=res, rowbias=rb))
        assert "conv_halo2_kernel+edge" in hip.last_gemm_kernel(fie) and "tile code 78" in hip.last_gemm_kernel(fie)
    finally:
        fie.force_tile(0)
    y = outs[0]
    assert not torch.isnan(y).any()
    assert rel_err(y.permute(0, 3, 1, 2), ref) < 3e-3, (b, h, w, cin, cout, opts)
    assert all(torch.equal(o, y) for o in outs[1:])


def test_code78_integer_data_matches_im2col_bit_for_bit(fie):
    """Integer data: every partial sum is exact in fp32, so the chunk-major K order of 78 and the tap-major order of the im2col codes agree bit for bit."""
    g = torch.Generator().manual_seed(78)
    for b, h, w, cin, cout in [(2, 56, 72, 640, 640), (1, 104, 152, 256, 512), (2, 26, 38, 1280, 1280)]:
        x = torch.randint(-3, 4, (b, h, w, cin), generator=g).half().to(DEV)
        wp = fie.pack_conv3x3(torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).half().to(DEV))
        bias = torch.randint(-8, 9, (cout,), generator=g).half().to(DEV)
        res = torch.randint(-8, 9, (b, h, w, cout), generator=g).half().to(DEV)
        try:
            fie.force_tile(78)
            a = fie.conv3x3(x, wp, cout, bias=bias, residual=res)
            fie.force_tile(42)
            c = fie.conv3x3(x, wp, cout, bias=bias, residual=res)
        finally:
            fie.force_tile(0)
        assert torch.equal(a, c), (b, h, w, cin, cout)


def test_code78_eligibility(fie):
    """78 is refused on maps of whole 16x16 patches (codes 71-76 keep them), with GroupNorm sums armed, and with an activation; 71 / 72 still refuse a
    non-multiple-of-16 map."""
    from fie_amd import hip
    g = torch.Generator().manual_seed(7)
    wp = fie.pack_conv3x3((torch.randn(128, 128, 3, 3, generator=g) * 0.03).half().to(DEV))
    try:
        fie.force_tile(78)
        with pytest.raises(hip.FieError, match="tile code 78"):
            fie.conv3x3(torch.randn(1, 64, 64, 128, generator=g).half().to(DEV), wp, 128)
        x = torch.randn(1, 56, 72, 128, generator=g).half().to(DEV)
        with pytest.raises(hip.FieError, match="tile code 78"):
            fie.conv3x3(x, wp, 128, gn_groups=32)
        with pytest.raises(hip.FieError, match="tile code 78"):
            fie.conv3x3(x, wp, 128, act=hip.ACT_SILU)
        for code in (71, 72):
            fie.force_tile(code)
            with pytest.raises(hip.FieError, match="halo-resident conv"):
                fie.conv3x3(x, wp, 128)
    finally:
        fie.force_tile(0)


@pytest.mark.parametrize("b,h,w,cin,cout,c2,c3", [(2, 52, 76, 320, 640, 320, 0), (1, 104, 152, 256, 256, 128, 64), (2, 104, 152, 320, 320, 320, 0),
                                                 (2, 26, 38, 640, 1280, 640, 0)])
def test_code78_with_1x1_side_inputs(fie, b, h, w, cin, cout, c2, c3):
    """A resnet's conv2 + its 1x1 shortcut as one launch (fie_conv3x3_plus_nhwc_f16) on code 78 (the SIDE + EDGE instantiation) against torch fp32;
    one and several tiles per block, one and two side inputs, a column tile half past N; repeats bit-identical."""
    from fie_amd import hip
    g = torch.Generator().manual_seed(h * w + c2)
    x = torch.randn(b, h, w, cin, generator=g).half().to(DEV)
    x2 = torch.randn(b * h * w, c2, generator=g).half().to(DEV)
    x3 = torch.randn(b * h * w, c3, generator=g).half().to(DEV) if c3 else None
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half().to(DEV)
    w1 = (torch.randn(cout, c2 + c3, generator=g) * (c2 + c3) ** -0.5).half().to(DEV)
    bias = torch.randn(cout, generator=g).half().to(DEV)
    wplus = torch.cat([fie.pack_conv3x3(wt)[:, :9 * cin], fie.pack_linear(w1)[:, :c2 + c3]], 1).contiguous()
    side = x2 if x3 is None else torch.cat([x2, x3], 1)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float(), bias.float(), padding=1) \
        + (side.float() @ w1.float().T).view(b, h, w, cout).permute(0, 3, 1, 2)
    try:
        fie.force_tile(78)
        outs = [fie.conv3x3_plus(x, wplus, cout, x2, x3, bias=bias) for _ in range(4)]
        assert "tile code 78" in hip.last_gemm_kernel(fie), hip.last_gemm_kernel(fie)
    finally:
        fie.force_tile(0)
    assert rel_err(outs[0].permute(0, 3, 1, 2), ref) < 4e-3, (b, h, w, cin, cout, c2, c3)
    assert all(torch.equal(o, outs[0]) for o in outs[1:])


def test_remembered_halo_code_the_launch_cannot_take_falls_back(fie):
    """Tuner keys carry neither the map's height / width nor the epilogue (144x112 and 168x96 share M 16128).  A remembered 72 met on a map of whole
    patches, replayed for the same key on a bucket map, and a remembered 78 met without GroupNorm sums, replayed with them, run the rule's code."""
    from fie_amd import hip
    g = torch.Generator().manual_seed(16128)
    x = torch.randn(1, 96, 168, 256, generator=g).half().to(DEV)
    wp = fie.pack_conv3x3((torch.randn(320, 256, 3, 3, generator=g) * 0.02).half().to(DEV))
    fie.tune_candidates(True)
    try:
        fie.conv3x3(x, wp, 320)
        (key, _, _), = fie.tune_candidates_read()[-1:]
        x16 = torch.randn(1, 112, 144, 256, generator=g).half().to(DEV)
        fie.conv3x3(x16, wp, 320)
        (key16, _, _), = fie.tune_candidates_read()[-1:]
    finally:
        fie.tune_candidates(False)
    assert key == key16, (key, key16)
    ref = fie.conv3x3(x, wp, 320).clone()
    xa = torch.randn(1, 56, 72, 128, generator=g).half().to(DEV)
    wa = fie.pack_conv3x3((torch.randn(128, 128, 3, 3, generator=g) * 0.03).half().to(DEV))
    fie.tune_candidates(True)
    try:
        fie.conv3x3(xa, wa, 128)
        (key_a, _, _), = fie.tune_candidates_read()[-1:]
    finally:
        fie.tune_candidates(False)
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write(f"{key} -> 72\n{key_a} -> 78\n")
        path = f.name
    try:
        fie.load_tune_table(path)
        fie.autotune(2)                                            # remembered choices only
        y = fie.conv3x3(x, wp, 320)                                # 72 remembered, 168x96: the rule (78 or an im2col code)
        assert "tile code 72" not in hip.last_gemm_kernel(fie)
        assert rel_err(y, ref) < 2e-3
        ya = fie.conv3x3(xa, wa, 128, gn_groups=32)                # 78 remembered, sums armed: the rule's im2col code
        assert "tile code 78" not in hip.last_gemm_kernel(fie) and getattr(ya, "_gn_tag", None) is not None
        fie.conv3x3(xa, wa, 128)                                   # without sums the remembered 78 runs
        assert "tile code 78" in hip.last_gemm_kernel(fie)
    finally:
        fie.autotune(0)
        fie.tune_exclude("")                                       # forgets the remembered choices (the session table is reloaded below)
        fie.load_tune_table()
        os.unlink(path)


def test_code78_rule_and_tuner_candidates(fie):
    """fie_debug_tune_candidates, computed live: 78 is the built-in rule's code for the CFG-batch UNet conv at 72x56 x 640; at 152x104 x 256 -> 256 (140
    tiles: under the rule's threshold, over the tuner's) the rule takes an im2col code and the tuner lists 78; fie_debug_tune_exclude("78") takes it
    away; for the fixture's same-size convs (maps of whole 16x16 patches) neither the rule nor the tuner offers it."""
    import json
    import os
    from fie_amd import hip
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 56, 72, 640, generator=g).half().to(DEV)
    wp = fie.pack_conv3x3((torch.randn(640, 640, 3, 3, generator=g) * 0.01).half().to(DEV))
    fie.tune_candidates(True)
    try:
        fie.conv3x3(x, wp, 640)
        assert "tile code 78" in hip.last_gemm_kernel(fie)
        rows = fie.tune_candidates_read()
    finally:
        fie.tune_candidates(False)
    (key, rule, cands), = rows[-1:]
    assert rule == 78 and 78 not in cands, rows[-1]
    fie.tune_exclude("78")
    try:
        fie.conv3x3(x, wp, 640)
        assert "tile code 78" not in hip.last_gemm_kernel(fie)
    finally:
        fie.tune_exclude("")
    # 320 channels at 152x104 (the 1216x832 edit's biggest UNet map, a column tile half past N): the rule takes 78 too
    x = torch.randn(2, 104, 152, 320, generator=g).half().to(DEV)
    wp = fie.pack_conv3x3((torch.randn(320, 320, 3, 3, generator=g) * 0.01).half().to(DEV))
    fie.conv3x3(x, wp, 320)
    assert "tile code 78" in hip.last_gemm_kernel(fie)
    # under the rule's threshold, over the tuner's: 78 is a candidate
    x = torch.randn(1, 104, 152, 256, generator=g).half().to(DEV)
    wp = fie.pack_conv3x3((torch.randn(256, 256, 3, 3, generator=g) * 0.01).half().to(DEV))
    fie.tune_candidates(True)
    try:
        fie.conv3x3(x, wp, 256)
        (key, rule, cands), = fie.tune_candidates_read()[-1:]
        fie.tune_exclude("78")
        fie.conv3x3(x, wp, 256)
        (_, rule_x, cands_x), = fie.tune_candidates_read()[-1:]
    finally:
        fie.tune_exclude("")
        fie.tune_candidates(False)
    assert rule != 78 and 78 in cands, (key, rule, cands)
    assert rule_x != 78 and 78 not in cands_x
    # the fixture's same-size convs, launched live: no 78 anywhere
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_problems.json")) as f:
        probs = json.load(f)["problems"]
    shapes = sorted({(p["b"], p["H"], p["W"], p["Cin"], p["N"]) for p in probs if p["kind"] == "conv" and p["stride"] == 1 and not p["ups"]
                     and not p["C2"] and not p["parity"] and not p["w8"] and p["M"] == p["b"] * p["H"] * p["W"]})
    assert len(shapes) >= 5
    fie.tune_candidates(True)
    try:
        for b, h, w, cin, n in shapes:
            if b * h * w * max(cin, n) > (1 << 28):
                continue
            fie.conv3x3(torch.randn(b, h, w, cin, generator=g).half().to(DEV), fie.pack_conv3x3(torch.zeros(n, cin, 3, 3).half().to(DEV)), n)
            (key, rule, cands), = fie.tune_candidates_read()[-1:]
            assert rule != 78 and 78 not in cands, key
    finally:
        fie.tune_candidates(False)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the rest of the hot path at bucket shapes

@pytest.mark.parametrize("w,h", [(1216, 832), (1344, 768)])
def test_thin_conv_at_bucket_vae_conv_out(fie, w, h):
    from fie_amd import hip
    g = torch.Generator().manual_seed(w)
    x = (torch.randn(1, h, w, 128, generator=g) * 0.5).half().to(DEV)
    wt = (torch.randn(4, 128, 3, 3, generator=g) * (9 * 128) ** -0.5).half()      # the decoder's conv_out: 3 channels written as 4
    wt[3] = 0
    bias = torch.randn(4, generator=g).half().to(DEV)
    y = fie.conv3x3(x, fie.pack_conv3x3(wt.to(DEV)), 4, bias=bias)
    assert "conv_thin" in hip.last_gemm_kernel(fie), hip.last_gemm_kernel(fie)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wt.float().to(DEV), bias.float(), padding=1)
    assert rel_err(y.permute(0, 3, 1, 2), ref) < 3e-3


@pytest.mark.parametrize("rows,c", [(1008, 1280), (988, 1280), (960, 1280), (4032, 640), (3952, 640)])
def test_groupnorm_at_bucket_rows(fie, rows, c):
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(2, rows, c, generator=g) + 0.5).half()
    gamma, beta = (1 + 0.1 * torch.randn(c, generator=g)).half(), (0.1 * torch.randn(c, generator=g)).half()
    ref = F.silu(F.group_norm(x.float().transpose(1, 2), 32, gamma.float(), beta.float(), 1e-5).transpose(1, 2))
    out = fie.groupnorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), 32, 1e-5, True)
    assert rel_err(out, ref) < 3e-3


@pytest.mark.parametrize("tq,tk,hn,d", [(4032, 4032, 10, 64), (4032, 77, 10, 64), (15808, 15808, 5, 64), (16128, 16128, 1, 64),
                                        (15808, 15808, 1, 512), (16128, 16128, 1, 512)])
def test_attention_at_bucket_tokens(fie, tq, tk, hn, d):
    """UNet self / cross attention at the 72x56 level, and the VAE's single-head head-dim-512 attention at 152x104 / 168x96 latents."""
    b = 1
    g = torch.Generator().manual_seed(tq + tk)
    c = hn * d
    q, k, v = (torch.randn(b * tq, c, generator=g).half(), torch.randn(b * tk, c, generator=g).half(), torch.randn(b * tk, c, generator=g).half())
    qf, kf, vf = (t.float().to(DEV).view(b, -1, hn, d).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(b * tq, c)
    out = fie.attention(q.to(DEV), k.to(DEV), v.to(DEV), hn, d, tq, tk, b)
    assert rel_err(out, ref) < 4e-3


def test_canny_and_mask_prep_on_non_square_maps(fie):
    from oracle import canny
    import fie_amd  # noqa: F401
    from fie_amd import mask as hmask
    for w, h in [(1152, 896), (832, 1216), (1344, 768), (200, 72)]:
        a = np.asarray(synth_rect(w + h, w, h))
        assert np.array_equal(fie.canny_device(torch.from_numpy(np.array(a)).cuda()).cpu().numpy(), canny.canny_rgb(a)), (w, h)
        rng = np.random.default_rng(w)
        lm = np.zeros((h, w), np.uint8)
        lm[h // 5: h // 2, w // 3: w - 9] = 255
        lm[rng.integers(0, h, 50), rng.integers(0, w, 50)] = 200
        binary = (lm >= 128).astype(np.float32)
        for r in (0, 2.0):
            m_px, m_lat = fie.mask_prep(torch.from_numpy(lm).cuda(), r)
            torch.cuda.synchronize()
            assert np.array_equal(m_lat.cpu().numpy().reshape(h // 8, w // 8), binary[::8, ::8].astype(np.uint8)), (w, h)
            if r == 0:
                assert np.array_equal(m_px.cpu().numpy(), binary)
            else:
                assert np.abs(m_px.cpu().numpy() - hmask.feather_numpy(binary, r)).max() <= 1e-5


@pytest.mark.parametrize("src,dst", [((800, 600), (1152, 896)), ((1600, 1200), (1152, 896)), ((1920, 1080), (1344, 768)), ((640, 360), (1344, 768)),
                                     ((1080, 1920), (768, 1344)), ((1024, 1024), (1216, 832))])
def test_lanczos_resize_non_square_bit_exact(fie, src, dst):
    img = synth_rect(sum(src), *src)
    want = np.asarray(img.resize(dst, Image.LANCZOS))
    got = fie.resize_lanczos(torch.from_numpy(np.asarray(img).copy()).cuda(), dst[1], dst[0]).cpu().numpy()
    assert np.array_equal(got, want)
    lm = np.asarray(img.convert("L"))
    got_l = fie.resize_lanczos(torch.from_numpy(lm.copy()).cuda(), dst[1], dst[0]).cpu().numpy()
    assert np.array_equal(got_l, np.asarray(Image.fromarray(lm).resize(dst, Image.LANCZOS)))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# tiny stack: non-square pipeline calls

@pytest.fixture(scope="module")
def tiny(fie):
    from fie_amd import stack
    from fie_amd.pipe import HipImg2ImgPipeline
    cfgs, sds = stack.synthetic_stack("tiny", True, device="cpu", dtype=torch.float16)
    sds32 = {k: {n: v.float() for n, v in sd.items()} for k, sd in sds.items()}
    return cfgs, sds32, HipImg2ImgPipeline(fie, cfgs, sds, noise_dtype=torch.float32)


def _tiny_call(pipe, w, h, seed=42):
    from oracle import canny
    img = synth_rect(w * 7 + h, w, h)
    ctrl = Image.fromarray(canny.canny_rgb(np.asarray(img)))
    out = pipe(prompt="a [red] circle next to a square", negative_prompt="", image=img, control_image=ctrl, strength=0.8, num_inference_steps=4,
               guidance_scale=1.5, controlnet_conditioning_scale=0.5, generator=torch.Generator("cpu").manual_seed(seed)).images[0]
    return img, ctrl, out


def test_tiny_non_square_edit_vs_oracle(tiny):
    """192x128 (w x h): a swapped h / w in the time ids, the latents or the VAE would not survive the comparison."""
    from oracle import metrics, pipeline as opipe
    cfgs, sds32, pipe = tiny
    img, ctrl, out = _tiny_call(pipe, 192, 128)
    assert out.size == (192, 128) and pipe.last_stats["latent_hw"] == (16, 24)
    ids = lambda t: (pipe.tok_l([t]), pipe.tok_g([t]))
    ref = opipe.run(sds32, cfgs, img, ctrl, ids("a [red] circle next to a square"), ids(""), strength=0.8, num_inference_steps=4, guidance_scale=1.5,
                    controlnet_conditioning_scale=0.5, generator=torch.Generator("cpu").manual_seed(42))
    s = metrics.ssim(out, ref, size=None)
    print(f"192x128 tiny edit vs oracle: ssim={s:.5f}")
    assert s >= 0.99


def test_tiny_non_square_eager_equals_replay_and_sizes_alternate(tiny):
    cfgs, sds32, pipe = tiny
    use0 = pipe.use_graph
    try:
        pipe.use_graph = False
        eager = np.asarray(_tiny_call(pipe, 192, 128)[2])
        pipe.use_graph = True
        first = {}
        for w, h in [(192, 128), (128, 128), (192, 128), (128, 192), (128, 128), (192, 128)]:
            o = np.asarray(_tiny_call(pipe, w, h)[2])
            assert o.shape == (h, w, 3)
            if (w, h) in first:
                assert np.array_equal(o, first[(w, h)]), (w, h)
            first.setdefault((w, h), o)
        assert np.array_equal(first[(192, 128)], eager)
    finally:
        pipe.use_graph = use0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# full size: the SSD-1B stack

@pytest.fixture(scope="module")
def full(fie):
    from fie_amd import stack
    from fie_amd.pipe import HipImg2ImgPipeline
    cfgs, sds = stack.synthetic_stack("ssd-1b", True, device="cpu", dtype=torch.float16)
    pipe = HipImg2ImgPipeline(fie, cfgs, sds, noise_dtype=torch.float32)
    sds32 = {k: {n: v.float() for n, v in sd.items()} for k, sd in sds.items()}
    del sds
    return cfgs, sds32, pipe


def test_full_size_eval_at_1152x896_vs_oracle(full, fie):
    """One ControlNet + UNet evaluation at 144x112 latents (1152x896), batch 1, t = 499: the bound of test_full_size_unet_controlnet_eval_vs_oracle."""
    from oracle import nets
    cfgs, sds32, pipe = full
    g = torch.Generator().manual_seed(9)
    lh, lw, t = 112, 144, 499
    lat = torch.randn(1, 4, lh, lw, generator=g).half().float()
    cond = (torch.rand(1, 3, lh * 8, lw * 8, generator=g) > 0.9).float()
    xd = cfgs["unet"]["cross_attention_dim"]
    text = torch.randn(1, 77, xd, generator=g).half().float()
    pooled = torch.randn(1, 1280, generator=g).half().float()
    tid = torch.tensor([[896., 1152., 0, 0, 896., 1152.]])
    with torch.no_grad():
        down, mid = nets.controlnet_forward(sds32["controlnet"], cfgs["controlnet"], lat, t, text, cond, 0.5, pooled, tid)
        ref = nets.unet_forward(sds32["unet"], cfgs["unet"], lat, t, text, pooled, tid, down, mid)
    dev = fie.device
    model_in = torch.zeros(1, lh, lw, 8, dtype=torch.float16, device=dev)
    model_in[..., :4] = lat.permute(0, 2, 3, 1).half().to(dev)
    cond8 = torch.zeros(1, lh * 8, lw * 8, 8, dtype=torch.float16, device=dev)
    cond8[..., :3] = cond.permute(0, 2, 3, 1).half().to(dev)
    text_d = text.reshape(77, xd).half().to(dev)
    pipe.unet.begin_image(pooled.half().to(dev), tid.to(dev))
    pipe.controlnet.begin_image(pooled.half().to(dev), tid.to(dev))
    cemb = pipe.controlnet.cond_embedding(cond8)
    t_dev = torch.full((1, 1), float(t), device=dev)
    tb_u, tb_c = pipe.unet.time_rowbias(t_dev), pipe.controlnet.time_rowbias(t_dev)
    skips, m = pipe.unet.encode(pipe.unet.conv_in(fie, model_in), tb_u, text_d, 77)
    c_skips, c_mid = pipe.controlnet.encode_cond(model_in, cemb, tb_c, text_d, 77)
    zero = [torch.zeros_like(s) for s in skips]
    r_skips, r_mid = pipe.controlnet.add_residuals(c_skips, c_mid, 0.5, zero, torch.zeros_like(m))
    worst = max(rel_err(a.permute(0, 3, 1, 2), b) for a, b in zip(r_skips + [r_mid], list(down) + [mid]))
    skips2, m2 = pipe.controlnet.add_residuals(c_skips, c_mid, 0.5, skips, m)
    eps = pipe.unet.decode(m2, skips2, tb_u, text_d, 77)
    e = rel_err(eps.permute(0, 3, 1, 2), ref)
    print(f"1152x896 eval vs oracle: eps rel_err={e:.2e}, worst ControlNet residual rel_err={worst:.2e}")
    assert worst < 2e-2 and e < 2e-2


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    ed = FastEditor(model_name="ssd-1b", enable_cpu_offload=False)
    ed.pipe.set_progress_bar_config(disable=True)
    return ed


_KW = dict(seed=7, strength=0.5, num_inference_steps=4, guidance_scale=1.5)


def test_editor_auto_bucket_and_square(editor):
    img43 = synth_rect(1, 800, 600)
    out = editor.edit(img43, "a [red] house", resolution="auto", **_KW)
    assert out.size == (1152, 896) and out.mode == "RGB"
    again = editor.edit(img43, "a [red] house", resolution=(1152, 896), **_KW)
    assert np.array_equal(np.asarray(out), np.asarray(again))
    sq = synth_rect(2, 640, 640)
    base = editor.edit(sq, "a [blue] car", **_KW)
    auto = editor.edit(sq, "a [blue] car", resolution="auto", **_KW)
    assert base.size == (1024, 1024) and np.array_equal(np.asarray(base), np.asarray(auto))
    with pytest.raises(ValueError, match="multiples of 64"):
        editor.edit(img43, "x", resolution=(1000, 800))


def test_editor_masked_bucket_edit_keeps_the_outside(editor):
    img = synth_rect(3, 1920, 1080)
    m = np.zeros((1080, 1920), np.uint8)
    m[200:700, 500:1400] = 255
    out = np.asarray(editor.edit(img, "a [golden] statue", mask=m, resolution="auto", **_KW))
    assert out.shape == (768, 1344, 3)
    src = np.asarray(img.resize((1344, 768), Image.LANCZOS))
    ml = np.asarray(Image.fromarray(m).resize((1344, 768), Image.LANCZOS))
    outside = ml < 128
    assert np.array_equal(out[outside], src[outside])
    assert not np.array_equal(out[~outside], src[~outside])


def test_editor_batch_with_mixed_aspect_ratios_matches_serial(editor):
    imgs = [synth_rect(4, 800, 600), synth_rect(5, 600, 600), synth_rect(6, 1000, 750), synth_rect(7, 1500, 1000)]
    prompts = [f"a [toy] number {i}" for i in range(len(imgs))]
    serial = [np.asarray(editor.edit(im, p, resolution="auto", **_KW)) for im, p in zip(imgs, prompts)]
    batch = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, resolution="auto", **_KW)]
    assert [b.shape for b in batch] == [(896, 1152, 3), (1024, 1024, 3), (896, 1152, 3), (832, 1216, 3)]
    for a, b in zip(batch, serial):
        assert a.shape == b.shape and np.abs(a.astype(int) - b.astype(int)).max() <= 2
