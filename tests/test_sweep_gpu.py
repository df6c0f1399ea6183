"""Strength sweeps on the MI355X: the selector op fie_sweep_select_u8 byte for byte against fie_amd/sweep.py:
select_numpy, and FastEditor.edit_sweep -- the ragged device job of fie_amd/pipe.py -- against serial edit(strength=s) calls.

Sweep against serial edits: the project's bound for edit_batch against serial edits (tests/test_pipeline_gpu.py: max |du8| <= 2 and SSIM > 0.999);
the cause is the same, fp16 tile order at another batch size.  A variant beyond it is a finding about the ragged step (per-job state that does
not cover all k * nb rows), not a reason to widen the bound.

The metric dicts: a metric row is a function of the scored pair alone (include/fie.h: the same bits in every run and at every batch position), so
a sweep's dict must be, bit for bit, what the metric op gives for (source, the sweep's own image of that variant) -- that is checked exactly.
Against the serial dict that leaves the image difference itself: with rms the root of mse and d = max |du8| / 255, the triangle inequality gives
|rms_sweep - rms_serial| <= d, so |mse_sweep - mse_serial| <= d (rms_sweep + rms_serial); psnr follows from mse."""
import collections
import math

import numpy as np
import pytest
import torch
from PIL import Image

import isolation
import mask_grow_oracle as mgo
from sweep_cases import TABLE, _clip, _rows
from test_pipeline_gpu import synth_image

pytestmark = pytest.mark.gpu

RES = (512, 512)
PROMPT = "a [red] kite"
KW = dict(num_inference_steps=4, seed=11, resolution=RES)
ALL = [1.0, 0.875, 0.625, 0.375]                 # sweep.variants(4, "all"): 4, 3, 2, 1 steps


def _ssim(a, b):
    from oracle import metrics
    return metrics.ssim(Image.fromarray(np.asarray(a)), np.asarray(b), size=None)


def _close(got, want, what=""):
    """The project's bound for one device job against serial edits."""
    a, b = np.asarray(got), np.asarray(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    d = int(np.abs(a.astype(int) - b.astype(int)).max())
    s = _ssim(a, b)
    print(f"[sweep] {what}: max|du8| = {d}, SSIM = {s:.6f}")
    assert d <= 2 and s > 0.999, (what, d, s)
    return d


def _dicts_agree(got, want, d, what=""):
    """got / want: the metric dicts of a sweep variant and of the serial edit whose images differ by at most d u8 levels (module docstring)."""
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for pre in ("", "bg_") if "bg_mse" in want else ("",):
        r1, r2 = math.sqrt(got[pre + "mse"]), math.sqrt(want[pre + "mse"])
        tol = (d / 255.0) * (r1 + r2) + 1e-15
        print(f"[sweep] {what}: {pre}mse {got[pre + 'mse']:.3e} vs {want[pre + 'mse']:.3e} (allowed {tol:.3e}), {pre}ssim {got[pre + 'ssim']:.6f} vs "
              f"{want[pre + 'ssim']:.6f}")
        assert abs(got[pre + "mse"] - want[pre + "mse"]) <= tol, (what, pre)
        lo, hi = max(want[pre + "mse"] - tol, 1e-300), want[pre + "mse"] + tol
        if math.isfinite(want[pre + "psnr"]) and math.isfinite(got[pre + "psnr"]):
            assert -10 * math.log10(hi) - 1e-9 <= got[pre + "psnr"] <= -10 * math.log10(lo) + 1e-9, (what, pre)


# ---------------------------------------------------------------------------------------------------------------- 1. the selector op
BYTES = (1, 15, 16, 17, 5883, 65539)


def _run_select(fie, case, nbytes, out_off, src_off, rng):
    from fie_amd import sweep as hsweep
    name, ssim, bgs, scores, rule, floor, bg, want = case
    dev = fie.device
    k = len(ssim)
    rows = _rows(ssim, bgs)
    clip = None if scores is None else np.concatenate([_clip(scores), _clip([1e9, float("nan")])])      # rows behind the first k are not read
    assert want == hsweep.select_numpy(rows, clip, rule, floor, bg)
    srcs = []
    for i in range(k):
        off = (src_off + 5 * i) % 16                       # views that start 0 .. 15 bytes into their own allocations
        base = torch.from_numpy(rng.integers(0, 256, off + nbytes + 7, dtype=np.uint8)).to(dev)
        assert base.data_ptr() % 16 == 0
        srcs.append(base[off:off + nbytes])
    view, guard = isolation.guarded((out_off + nbytes,), dtype=torch.uint8, device=dev, rows=1, flat=True)
    view.fill_(0x5a)
    idx_view, idx_guard = isolation.guarded((1,), dtype=torch.int32, device=dev, flat=True)
    idx_view.fill_(-7)
    out, idx = fie.sweep_select(srcs, torch.from_numpy(rows).to(dev), None if clip is None else torch.from_numpy(clip).to(dev), rule, floor, bg,
                                out=view[out_off:], out_idx=idx_view)
    torch.cuda.synchronize()
    guard.check(f"{name}: image, {nbytes} bytes at +{out_off}")
    idx_guard.check(f"{name}: index")
    what = (name, k, nbytes, out_off, src_off)
    assert int(idx.cpu()[0]) == want, what
    assert torch.equal(out.cpu(), srcs[want].cpu()), what
    assert bool((view[:out_off] == 0x5a).all()), what       # the bytes in front of an output that starts off a 16-byte boundary


@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_selector_op_matches_select_numpy(fie, case):
    """Every branch of the CPU table (k = 1, 2, 3, 16; both rules; floors nobody passes; ties; NaN sums and scores; bg), each at every byte count, with
    the sources 0 .. 15 bytes into their allocations and the output inside a guard band at a varying offset."""
    rng = np.random.default_rng(len(case[0]))
    for j, nbytes in enumerate(BYTES):
        _run_select(fie, case, nbytes, out_off=(3 * j + len(case[1])) % 16, src_off=(7 * j) % 16, rng=rng)


def test_selector_op_at_every_relative_alignment(fie):
    """One case of three images: every output offset 0 .. 15 against every source offset 0 .. 15 at a size with a head, a body and a tail -- the
    congruent (16-byte loads) and the incongruent (aligned dwords) path and the bytes at both ends of each."""
    case = next(c for c in TABLE if c[0] == "floor, clip among the passing")
    rng = np.random.default_rng(5)
    for out_off in range(16):
        for src_off in range(16):
            _run_select(fie, case, 5883 if (out_off + src_off) % 2 else 77, out_off, src_off, rng)


def test_selector_op_refuses_bad_arguments(fie):
    from fie_amd import hip
    dev = fie.device
    img = [torch.zeros(64, device=dev, dtype=torch.uint8) for _ in range(17)]
    rows = torch.zeros((2, 4), device=dev, dtype=torch.int64)
    for bad in (lambda: fie.sweep_select([], rows), lambda: fie.sweep_select(img, torch.zeros((17, 4), device=dev, dtype=torch.int64)),
                lambda: fie.sweep_select(img[:2], rows, rule="clip_score"), lambda: fie.sweep_select(img[:2], rows, rule="best"),
                lambda: fie.sweep_select(img[:2], rows[:1]), lambda: fie.sweep_select([img[0], img[1][:32]], rows),
                lambda: fie.sweep_select(img[:2], rows.int()), lambda: fie.sweep_select(img[:2], rows, out=torch.zeros(63, device=dev, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="sweep_select"):
            bad()
    with pytest.raises(hip.FieError, match="bad argument"):
        fie.sweep_select(img[:2], rows, out=img[1])                          # the output overlaps an image


# ---------------------------------------------------------------------------------------------------------------- the product surface
@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


@pytest.fixture(scope="module")
def source():
    return synth_image(11, 640)


@pytest.fixture(scope="module")
def serial(editor, source):
    """Four serial edits, one per step count: [(u8 array, metrics dict)] strongest first.  Computed once, shared, never written to."""
    out = []
    for s in ALL:
        img, m = editor.edit(source, PROMPT, strength=s, metrics=True, **KW)
        out.append((np.asarray(img), m))
    return out


@pytest.fixture(scope="module")
def swept(editor, source, serial):
    """edit_sweep(strengths="all", select=None) on the same editor (behind the serial edits: its graph is the fifth)."""
    imgs, variants = editor.edit_sweep(source, PROMPT, strengths="all", **KW)
    return [np.asarray(i) for i in imgs], variants


def test_sweep_all_matches_four_serial_edits(editor, fie, source, serial, swept):
    from fie_amd import metrics as hmetrics
    from fie_amd import sweep as hsweep
    imgs, variants = swept
    assert len(imgs) == len(variants) == 4
    assert [v["steps"] for v in variants] == [4, 3, 2, 1] and [v["strength"] for v in variants] == [[s] for s in ALL]
    assert [v["strength"][0] for v in variants] == [v[1][0] for v in hsweep.variants(4, "all")]
    assert editor.pipe.last_stats["images"] == 4 and editor.pipe.last_stats["sweep"] == (4, 3, 2, 1) and editor.pipe.last_stats["unet_evals"] == 4
    src512 = fie.resize_lanczos(torch.from_numpy(np.asarray(source)).to(fie.device), 512, 512)
    for i, ((want, wdict), got, v) in enumerate(zip(serial, imgs, variants)):
        d = _close(got, want, f"variant {i} ({v['steps']} steps)")
        gdict = {k: v[k] for k in v if k not in ("strength", "steps")}
        _dicts_agree(gdict, wdict, d, f"variant {i}")
        rows = fie.metrics_pairs(src512, torch.from_numpy(got).to(fie.device)).cpu().numpy()
        assert gdict == hmetrics.rows_to_dicts(rows, 512, 512)[0]                 # exactly the metrics of the sweep's own image
    assert len({im.tobytes() for im in imgs}) == 4                                 # four different edits, not one four times


def test_one_variant_sweep_is_the_single_edit(editor, source, serial):
    want, wdict = editor.edit(source, PROMPT, strength=0.5, metrics=True, **KW)     # 2 steps: the graph the serial edits captured
    graphs = len(editor.pipe._graphs)
    imgs, variants = editor.edit_sweep(source, PROMPT, strengths=[0.5], **KW)
    assert len(imgs) == 1 and np.array_equal(np.asarray(imgs[0]), np.asarray(want))
    assert variants == [dict(strength=[0.5], steps=2, **wdict)]
    imgs2, variants2 = editor.edit_sweep(source, PROMPT, strengths=[0.5, 0.6], **KW)    # two strengths, one step count: still the single edit
    assert len(imgs2) == 1 and np.array_equal(np.asarray(imgs2[0]), np.asarray(want)) and variants2[0]["strength"] == [0.5, 0.6]
    assert len(editor.pipe._graphs) == graphs and editor.pipe.eager_overflow == 0


def test_eager_and_replayed_sweeps_are_bit_identical(editor, source, swept):
    imgs, variants = swept                                                        # a replay (the fixture's call captured the graph and replayed it)
    run = lambda seed: editor.edit_sweep(source, PROMPT, strengths="all", **dict(KW, seed=seed))
    editor.pipe.use_graph = False
    try:
        eager = run(11)
        eager12 = run(12)
    finally:
        editor.pipe.use_graph = True
    graphs = len(editor.pipe._graphs)
    replay12 = run(12)
    replay = run(11)
    assert len(editor.pipe._graphs) == graphs and editor.pipe.eager_overflow == 0
    for a, b, c in zip(eager[0], replay[0], imgs):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.array_equal(np.asarray(a), c)
    assert eager[1] == replay[1] == variants
    for a, b in zip(eager12[0], replay12[0]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert eager12[1] == replay12[1]
    assert not np.array_equal(np.asarray(eager12[0][0]), imgs[0])


def test_masked_sweep_with_the_full_keyword_set(fie):
    """The masked sweep against serial edits with the same keywords, twice.
    (1) At the edit size (the keyword set without output_size): the project's bound, as it stands -- max |du8| <= 2, SSIM > 0.999.
    (2) The full set with output_size="source" on the 700 x 560 source.  Here the 512 x 512 result goes through Pillow's two-pass 8-bit LANCZOS resize
    (an UPSCALE: 512 -> 700, 512 -> 560) before it is compared, and that filter has negative lobes: the absolute sum of an output pixel's
    coefficients is up to L1 = 1.5435 per axis (computed below from the tables the device uses).  Two inputs that differ by at most d0 levels leave
    the horizontal pass at most L1 d0 + 1 apart (each side is rounded to u8: half a level each), the vertical pass at most L1 (L1 d0 + 1) + 1, and the
    rounded composite adds at most one more: D(d0) = floor(L1^2 d0 + L1 + 2), 5 levels for d0 = 1 and 8 for d0 = 2, with d0 the difference measured
    in (1) for that variant.  SSIM > 0.999 holds at either size.  Outside the grown, feathered mask nothing is allowed at all: the source's bytes.
    Measured on the MI355X: (1) max |du8| 1 .. 2, (2) 2 .. 3 in two sessions, SSIM 0.99998."""
    from fie_amd import mask as hmask
    from fie_amd import resize as hresize
    from src.pipeline import FastEditor
    ed = FastEditor(model_name="tiny", enable_cpu_offload=False)
    img = synth_image(11, 700).crop((0, 0, 700, 560))                     # 700 x 560
    mask = np.zeros((560, 700), np.uint8)
    mask[150:380, 220:500] = 255
    mask[380:420, 300:340] = 255
    kw = dict(KW, mask=mask, mask_grow=8, masked_content="fill", blend="multiband", mask_blur=2)
    d0 = []
    small = ed.edit_sweep(img, PROMPT, strengths="all", **kw)[0]
    for i, (s, got) in enumerate(zip(ALL, small)):
        d0.append(_close(got, ed.edit(img, PROMPT, strength=s, **kw), f"masked variant {i}, edit size"))
    l1 = max(float((np.abs(hresize.coefficients(512, n)[0].astype(np.int64)).sum(1) / float(1 << 22)).max()) for n in (700, 560))
    assert 1.5 < l1 < 1.6
    kw["output_size"] = "source"
    serial = [ed.edit(img, PROMPT, strength=s, metrics=True, **kw) for s in ALL]
    imgs, variants = ed.edit_sweep(img, PROMPT, strengths="all", **kw)
    assert len(imgs) == 4 and all(i.size == (700, 560) for i in imgs)
    grown = mgo.grow(mask, 8) > 0
    R = hmask.blur_radius(2)
    reach = grown.copy()                                                    # where the feather of the grown mask can be non-zero: a (2R + 1)^2 box
    for axis in (0, 1):
        acc = reach.copy()
        for s in range(1, R + 1):
            lo, hi = np.zeros_like(reach), np.zeros_like(reach)
            if axis == 0:
                lo[s:], hi[:-s] = reach[:-s], reach[s:]
            else:
                lo[:, s:], hi[:, :-s] = reach[:, :-s], reach[:, s:]
            acc |= lo | hi
        reach = acc
    src = np.asarray(img)
    assert (~reach).sum() > 100000 and grown.sum() > 50000
    for i, ((want, wdict), got, v) in enumerate(zip(serial, imgs, variants)):
        got, want = np.asarray(got), np.asarray(want)
        d = int(np.abs(got.astype(int) - want.astype(int)).max())
        allowed = int(math.floor(l1 * l1 * d0[i] + l1 + 2))
        ssim = _ssim(got, want)
        print(f"[sweep] masked variant {i}, source size: max|du8| = {d} (allowed {allowed} from d0 = {d0[i]}), SSIM = {ssim:.6f}")
        assert d <= allowed and ssim > 0.999, (i, d, allowed, ssim)
        assert np.array_equal(got[~reach], src[~reach]), f"variant {i}: a byte outside the grown, feathered mask is not the source's"
        assert not np.array_equal(got[grown], src[grown])
        assert {"bg_ssim", "bg_psnr", "bg_mse"} <= set(v)
        _dicts_agree({k: v[k] for k in v if k not in ("strength", "steps")}, wdict, d, f"masked variant {i}")
    assert len({np.asarray(i).tobytes() for i in imgs}) == 4


def test_select_strongest_returns_the_variant_the_rule_names(editor, source, swept):
    from fie_amd import sweep as hsweep
    imgs, variants = swept
    ssims = sorted({v["ssim"] for v in variants})
    assert len(ssims) >= 2
    floor = (ssims[len(ssims) // 2 - 1] + ssims[len(ssims) // 2]) / 2                # the midpoint between two variants' SSIM
    passing = [v["ssim"] >= floor for v in variants]
    assert any(passing) and not all(passing)
    img, info = editor.edit_sweep(source, PROMPT, strengths="all", select="strongest", min_ssim=floor, **KW)
    want = hsweep.select_numpy(info["rows"], None, "strongest", hsweep.ssim_floor(floor), False)
    assert info["index"] == want == passing.index(True)
    assert np.array_equal(np.asarray(img), imgs[want])
    assert info["variants"] == variants and info["steps"] == variants[want]["steps"] and info["strength"] == variants[want]["strength"]
    assert info["ssim"] == variants[want]["ssim"] and info["clip_rows"] is None
    img2, info2 = editor.edit_sweep(source, PROMPT, strengths="all", select="strongest", min_ssim=1.0, **KW)      # nobody passes: the highest SSIM
    assert info2["index"] == int(np.argmax([v["ssim"] for v in variants])) == hsweep.select_numpy(info2["rows"], None, "strongest", hsweep.ssim_floor(1.0), False)
    assert np.array_equal(np.asarray(img2), imgs[info2["index"]])
    with pytest.raises(ValueError, match="clip_score_dir"):
        editor.edit_sweep(source, PROMPT, select="clip_score", **KW)


def test_select_clip_score_with_a_synthetic_clip_model(fie, source, tmp_path_factory):
    import clip_score_oracle as co
    from fie_amd import sweep as hsweep
    from src.pipeline import FastEditor
    ed = FastEditor(model_name="tiny", enable_cpu_offload=False, clip_score_dir=co.save(co.build_model("tiny"), tmp_path_factory.mktemp("clip_tiny")))
    imgs, variants = ed.edit_sweep(source, PROMPT, strengths="all", **KW)
    assert all("clip_score" in v for v in variants)
    img, info = ed.edit_sweep(source, PROMPT, strengths="all", select="clip_score", **KW)
    want = hsweep.select_numpy(info["rows"], info["clip_rows"], "clip_score", -math.inf, False)
    assert info["index"] == want and info["variants"] == variants
    assert [float(r[1]) for r in info["clip_rows"]] == [v["clip_score"] for v in variants]
    assert np.array_equal(np.asarray(img), np.asarray(imgs[want]))
    ssims = sorted(v["ssim"] for v in variants)
    floor = (ssims[1] + ssims[2]) / 2                                              # two variants pass: the better CLIP score among them
    img2, info2 = ed.edit_sweep(source, PROMPT, strengths="all", select="clip_score", min_ssim=floor, **KW)
    want2 = hsweep.select_numpy(info2["rows"], info2["clip_rows"], "clip_score", hsweep.ssim_floor(floor), False)
    assert info2["index"] == want2 and variants[want2]["ssim"] >= floor
    assert np.array_equal(np.asarray(img2), np.asarray(imgs[want2]))


def _launches(ctx, fn):
    """fn() with the launch log on -> the log's lines (marks start with '#')."""
    ctx.oplog(True)
    try:
        fn()
        return ctx.oplog_read()
    finally:
        ctx.oplog(False)


def _between(lines, start, stop):
    """The launch lines of every stretch from a `start` mark to the next `stop` mark, one list per stretch."""
    out, cur = [], None
    for l in lines:
        if l == "#" + start:
            cur = []
        elif l == "#" + stop and cur is not None:
            out.append(cur)
            cur = None
        elif cur is not None and not l.startswith("#"):
            cur.append(l)
    return out


def test_shared_work_in_the_launch_log(editor, fie, source, swept):
    """What a sweep shares: up to the `clip+vae_encode` mark it launches what ONE edit launches plus one latent_prep per extra variant (one text
    encoding, one VAE encode, one edge-map embedding); then four UNet passes, over 1, 2, 3 and 4 variants' rows."""
    editor.pipe.use_graph = False
    try:
        one = _launches(fie, lambda: editor.edit(source, PROMPT, strength=1.0, **KW))
        four = _launches(fie, lambda: editor.edit_sweep(source, PROMPT, strengths="all", **KW))
    finally:
        editor.pipe.use_graph = True
    head1, head4 = _between(one, "start", "clip+vae_encode"), _between(four, "start", "clip+vae_encode")
    assert len(head1) == len(head4) == 1 and len(head1[0]) > 20
    c1, c4 = collections.Counter(head1[0]), collections.Counter(head4[0])
    extra = c4 - c1
    assert not (c1 - c4), c1 - c4
    assert sum(extra.values()) == 3 and all("latent_prep" in l for l in extra), extra
    dec1, dec4 = _between(one, "unet_enc+controlnet", "unet_dec"), _between(four, "unet_enc+controlnet", "unet_dec")
    assert len(dec1) == len(dec4) == 4
    batch = lambda ls: {int(l.split("|", 4)[4].split("B=")[1].split()[0]) for l in ls if l.split("|", 4)[4].startswith("groupnorm")}
    nb = 2
    assert [batch(p) for p in dec1] == [{nb}] * 4
    assert [batch(p) for p in dec4] == [{nb}, {2 * nb}, {3 * nb}, {4 * nb}]
    attn = lambda ls: {int(l.split("|", 4)[4].split("B=")[1].split()[0]) for l in ls if l.split("|", 4)[4].startswith("attn ")}
    assert all(attn(p) <= {(i + 1) * nb} for i, p in enumerate(dec4))             # the attention launches of a step (if the stack has any there) too
