"""Mask-restricted edits, host side (no GPU): the masked oracle reduces to the unmasked one under an all-ones mask, the PIE-Bench
run-length decoder, mask conversion and argument errors, and the synthetic set's --with_masks field."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import fie_amd  # noqa: F401
from fie_amd import mask as hmask, presets as P, tokenizer, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny():
    st = P.STACKS["tiny"]
    cfgs = dict(unet=st["unet"], controlnet=st["controlnet_full"], vae=st["vae"], clip_l=st["clip_l"], clip_g=st["clip_g"])
    sds = {k: weights.synth_state_dict(cfgs[k], seed=10 + i) for i, k in enumerate(cfgs)}
    return cfgs, sds


@pytest.mark.parametrize("paste_back", [False, True])
def test_masked_oracle_all_ones_equals_unmasked_oracle(paste_back):
    import masked_oracle
    from oracle import canny, pipeline as opipe
    cfgs, sds = _tiny()
    img = Image.fromarray(np.random.default_rng(1).integers(0, 255, (64, 64, 3), dtype=np.uint8))
    ctrl = Image.fromarray(canny.canny_rgb(np.asarray(img)))
    ids = (tokenizer.StandInTokenizer(49407)(["a cat"]), tokenizer.StandInTokenizer(0)(["a cat"]))
    neg = (tokenizer.StandInTokenizer(49407)([""]), tokenizer.StandInTokenizer(0)([""]))
    kw = dict(strength=0.8, num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5)
    ref = opipe.run(sds, cfgs, img, ctrl, ids, neg, generator=torch.Generator().manual_seed(3), **kw)
    got = masked_oracle.run_masked(sds, cfgs, img, ctrl, ids, neg, np.full((64, 64), 255, np.uint8), paste_back=paste_back,
                                   generator=torch.Generator().manual_seed(3), **kw)
    assert np.array_equal(got, ref)
    # an all-zeros mask keeps the source outside: with the paste-back that is every pixel
    zero = masked_oracle.run_masked(sds, cfgs, img, ctrl, ids, neg, np.zeros((64, 64), np.uint8), paste_back=True,
                                    generator=torch.Generator().manual_seed(3), **kw)
    assert np.array_equal(zero, np.asarray(img))


def test_rle_decode_hand_written_fixture():
    # 6 x 5 array, runs (7, 3) and (20, 12): the second is clipped at the end (30 elements); then the border is set
    got = hmask.rle_decode([7, 3, 20, 12], (6, 5))
    want = np.array([[1, 1, 1, 1, 1],
                     [1, 0, 1, 1, 1],
                     [1, 0, 0, 0, 1],
                     [1, 0, 0, 0, 1],
                     [1, 1, 1, 1, 1],
                     [1, 1, 1, 1, 1]], np.uint8) * 255
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # an interior run on the PIE-Bench 512 x 512 grid: row 100, columns 200..259
    m = hmask.rle_decode([100 * 512 + 200, 60], (512, 512))
    assert m.shape == (512, 512) and m[100, 200:260].min() == 255 and m[100, 199] == 0 and m[100, 260] == 0
    assert m[0].min() == m[-1].min() == m[:, 0].min() == m[:, -1].min() == 255
    assert (m[1:-1, 1:-1] > 0).sum() == 60
    with pytest.raises(ValueError):
        hmask.rle_decode([1, 2, 3])
    with pytest.raises(ValueError):
        hmask.rle_decode([40, 1], (6, 5))


def test_rle_encode_round_trip():
    rng = np.random.default_rng(0)
    m = np.zeros((32, 32), np.uint8)
    m[1:-1, 1:-1] = rng.integers(0, 2, (30, 30))
    m[0] = m[-1] = m[:, 0] = m[:, -1] = 1
    assert np.array_equal(hmask.rle_decode(hmask.rle_encode(m), (32, 32)), m * 255)


def test_mask_conversion():
    a = np.zeros((16, 24), np.uint8)
    a[4:8, 4:12] = 200
    assert np.array_equal(hmask.to_l_array(a, (24, 16)), a)
    assert np.array_equal(hmask.to_l_array(a > 0), (a > 0).astype(np.uint8) * 255)
    rgb = Image.fromarray(np.stack([a] * 3, 2))
    assert np.array_equal(hmask.to_l_array(rgb), np.asarray(rgb.convert("L")))
    one_bit = Image.fromarray(a > 0).convert("1")
    assert np.array_equal(hmask.to_l_array(one_bit), np.asarray(one_bit.convert("L")))
    with pytest.raises(ValueError, match="differs from the image size"):
        hmask.to_l_array(a, (16, 24))
    with pytest.raises(ValueError):
        hmask.to_l_array(np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(TypeError):
        hmask.to_l_array(a.astype(np.float32))
    with pytest.raises(TypeError):
        hmask.to_l_array([[0, 1]])


def test_mask_argument_errors():
    assert hmask.check_args(0, True) == 0.0 and hmask.check_args(2, True) == 2.0 and hmask.check_args(0, False) == 0.0
    with pytest.raises(ValueError, match="paste_back"):
        hmask.check_args(1.5, False)
    with pytest.raises(ValueError, match="needs a mask"):
        hmask.check_args(1.0, True, have_mask=False)
    for bad in (-1, hmask.MAX_BLUR + 1, "x"):
        with pytest.raises(ValueError):
            hmask.check_args(bad, True)


def test_editor_mask_errors_before_any_device_work():
    """FastEditor.edit / edit_batch check their mask arguments on the host, before they touch the device (no GPU needed here)."""
    from src.pipeline import FastEditor
    ed = FastEditor.__new__(FastEditor)            # argument checks only: no context, no weights
    img = Image.new("RGB", (64, 48))
    with pytest.raises(ValueError, match="differs from the image size"):
        ed.edit(img, "x", mask=np.zeros((64, 64), np.uint8))
    with pytest.raises(ValueError, match="paste_back"):
        ed.edit(img, "x", mask=np.zeros((48, 64), np.uint8), mask_blur=2, paste_back=False)
    with pytest.raises(ValueError, match="needs a mask"):
        ed.edit(img, "x", mask_blur=2)
    with pytest.raises(ValueError, match="one mask"):
        ed.edit_batch([img, img], ["a", "b"], masks=[None])
    with pytest.raises(ValueError, match="differs from the image size"):
        ed.edit_batch([img, img], ["a", "b"], masks=[None, np.zeros((8, 8), np.uint8)])


def test_gaussian_taps_and_feather():
    t = hmask.gaussian_taps(2.0)
    assert t.dtype == np.float32 and len(t) == 2 * 6 + 1 and abs(float(t.sum()) - 1) < 1e-6 and np.allclose(t, t[::-1])
    assert np.array_equal(hmask.gaussian_taps(0), np.ones(1, np.float32))
    m = np.zeros((40, 40), np.float32)
    m[10:30, 10:30] = 1
    f = hmask.feather_numpy(m, 2.0)
    assert f.dtype == np.float32 and f.min() >= 0 and f.max() <= 1 + 1e-6
    assert f[0, 0] == 0 and abs(f[20, 20] - 1) < 1e-6 and 0.4 < f[20, 10] < 0.6
    assert np.array_equal(hmask.feather_numpy(m, 0), m)
    assert np.allclose(hmask.feather_numpy(np.ones((9, 9), np.float32), 3.0), 1, atol=1e-6)     # clamp-to-edge keeps a constant


def test_synthetic_piebench_with_masks(tmp_path):
    out = tmp_path / "pie"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_piebench.py"), "--out", str(out), "--num", "3",
                        "--with_masks"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    mapping = json.load(open(out / "mapping_file.json"))
    assert len(mapping) == 3
    for i, (k, e) in enumerate(mapping.items()):
        img = Image.open(out / "annotation_images" / e["image_path"])
        m = hmask.rle_decode(e["mask"], (img.height, img.width))
        assert img.size == (512, 512) and m.shape == (512, 512)
        inner = m[1:-1, 1:-1] > 0
        assert 0 < inner.sum() < inner.size
        ys, xs = np.nonzero(inner)
        box = inner[ys.min():ys.max() + 1, xs.min():xs.max() + 1]
        assert box.all(), "the mask is one box"
