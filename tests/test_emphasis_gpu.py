"""Prompt emphasis on the device: fie_kv_emphasis against its numpy restatement to the bit, inside guard bands; the text K | V
caches of the UNet and the ControlNet with and without weights, grouped and per block; one ControlNet + UNet evaluation in the fp32 context against
the oracle with weighted `attn2.to_v` rows; the weights of edit / edit_batch / edit_sweep / a graph replay / a call without CFG as they arrive in
the caches; and the two identities of the setting, byte for byte on a whole edit."""
import contextlib

import numpy as np
import pytest
import torch
from PIL import Image

import emphasis_oracle as eo
import isolation as iso

pytestmark = pytest.mark.gpu
T = 77
WEIGHTS = np.array([0.0, 0.5, 0.75, 1.0, 1.3, 2.0, 8.0], np.float32)


@pytest.fixture(scope="module")
def f32():
    import fie_amd  # noqa: F401
    from fie_amd import hip
    return hip.context(0, torch.float32)


def _np_dtype(dtype):
    return np.float16 if dtype == torch.float16 else np.float32


def _operand(rows, ncols, vcols, weighted_rows, dtype, seed):
    """Normal values with the edge cases in V columns of weighted rows: f16 subnormals (the smallest and the largest), the largest finite f16 of
    both signs (8 * 65504 rounds to an f16 infinity: the restatement says so too), zeros of both signs."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, ncols)).astype(np.float16)
    specials = np.array([6e-8, -6e-8, 6.0976e-5, -6.0976e-5, 65504.0, -65504.0, 0.0, -0.0, 3.0e-5], np.float16)
    for r in weighted_rows:
        cols = rng.choice(vcols, size=len(specials), replace=False)
        x[r, cols] = specials
    x[rng.integers(0, rows), rng.choice(np.setdiff1d(np.arange(ncols), vcols), 4)] = specials[:4]       # and some where nothing may change
    return x.astype(_np_dtype(dtype))


def _run_op(ctx, x, w, flags, moat_rows=iso.ROWS, ld=None):
    """fie_kv_emphasis on a copy of x inside a guarded arena -> the view's values behind the launch; the arena around and between the rows is checked."""
    from fie_amd import emphasis
    dtype = torch.float16 if x.dtype == np.float16 else torch.float32
    view, guard = iso.guarded(x.shape, ld=ld, dtype=dtype, device=ctx.device, rows=moat_rows)
    view.copy_(torch.from_numpy(x))
    w_dev, f_dev = torch.from_numpy(w).to(ctx.device), torch.from_numpy(flags).to(ctx.device)
    assert ctx.kv_emphasis(view, w_dev, f_dev) is view
    torch.cuda.synchronize()
    guard.check("kv_emphasis")                                                         # the padding beyond ncols and the rows around X keep their bytes
    got = view.cpu().numpy()
    assert eo.same_bits(got, emphasis.kv_emphasis_numpy(x, w, flags))
    keep = np.flatnonzero(w == 1.0)
    kcols = np.flatnonzero(np.repeat(flags == 0, 8))
    assert eo.same_bits(got[keep], x[keep]) and eo.same_bits(got[:, kcols], x[:, kcols])      # said once more: rows of weight 1 and unflagged columns
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. the op
@pytest.mark.parametrize("rows", [1, 77, 154, 308])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_op_is_the_restatement(fie, f32, dtype, rows):
    """Two blocks, c = 64 and 128: [K 64 | V 64 | K 128 | V 128] = 384 columns in rows of 392."""
    from fie_amd import emphasis
    ctx = fie if dtype == torch.float16 else f32
    flags = emphasis.v_flags([64, 128])
    vcols = np.flatnonzero(np.repeat(flags != 0, 8))
    rng = np.random.default_rng(rows)
    w = rng.choice(WEIGHTS, size=rows).astype(np.float32)
    if rows == 1:
        w[:] = 8.0
    else:
        w[rng.permutation(rows)[:len(WEIGHTS)]] = WEIGHTS                              # every weight at least once, 1 included
    x = _operand(rows, 384, vcols, np.flatnonzero(w != 1.0), dtype, seed=rows + 1)
    got = _run_op(ctx, x, w, flags, ld=392)
    if dtype == torch.float16:
        assert np.isinf(got[w == 8.0]).any() and not np.isnan(got).any()               # 8 * 65504 is an infinity in f16
    else:
        assert np.isfinite(got).all()


def test_op_all_ones_touches_nothing(fie):
    from fie_amd import emphasis
    flags = emphasis.v_flags([64, 128])
    x = _operand(77, 384, np.flatnonzero(np.repeat(flags != 0, 8)), [3], torch.float16, seed=2)
    assert eo.same_bits(_run_op(fie, x, np.ones(77, np.float32), flags, ld=392), x)


def test_op_at_sdxl_width(fie):
    """154 text rows x 166 400 columns: the grouped K | V result of SDXL's UNet (10 blocks of 640 and 60 of 1280), three weighted rows."""
    from fie_amd import emphasis
    flags = emphasis.v_flags([640] * 10 + [1280] * 60)
    assert flags.size * 8 == 166400
    vcols = np.flatnonzero(np.repeat(flags != 0, 8))
    w = np.ones(154, np.float32)
    w[[79, 80, 153]] = [1.3, 2.0, 0.5]
    x = _operand(154, 166400, vcols, [79, 80, 153], torch.float16, seed=3)
    _run_op(fie, x, w, flags, moat_rows=8)


def test_wrapper_refuses_bad_operands(fie):
    dev = fie.device
    x = torch.zeros(4, 16, dtype=torch.float16, device=dev)
    w, fl = torch.ones(4, device=dev), torch.ones(2, dtype=torch.uint8, device=dev)
    for bad in (lambda: fie.kv_emphasis(x.float(), w, fl), lambda: fie.kv_emphasis(x, w[:3], fl), lambda: fie.kv_emphasis(x, w.half(), fl),
                lambda: fie.kv_emphasis(x, w, fl[:1]), lambda: fie.kv_emphasis(x.t(), w, fl), lambda: fie.kv_emphasis(x, w.cpu(), fl)):
        with pytest.raises(ValueError, match="kv_emphasis"):
            bad()
    from fie_amd import hip
    with pytest.raises(hip.FieError, match="fie_kv_emphasis"):
        fie.kv_emphasis(torch.zeros(4, 20, dtype=torch.float16, device=dev)[:, :16], w, fl)       # a row stride of 20: no multiple of 8


# ---------------------------------------------------------------------------------------------------------------- 2. the nets' caches
@pytest.fixture(scope="module")
def pipe16(fie):
    from fie_amd import stack
    from fie_amd.pipe import HipImg2ImgPipeline
    cfgs, sds = stack.synthetic_stack("tiny", True, device="cpu", dtype=torch.float16)
    return cfgs, HipImg2ImgPipeline(fie, cfgs, sds, noise_dtype=torch.float32)


def _fill_caches(pipe, ctx, x, emph):
    dev, dt = ctx.device, ctx.dtype
    text = x["text"].reshape(2 * T, x["xd"]).to(dev, dt)
    for net in (pipe.unet, pipe.controlnet):
        net.begin_image(x["pooled"].to(dev, dt), x["tid"].to(dev), emph=emph)
        for b in eo.blocks(net):
            assert b.kv_cache is None                                                  # begin_image dropped it
            b._text_kv(ctx, text)
    torch.cuda.synchronize()
    return eo.caches(pipe)


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "per-block"])
def test_caches_hold_the_weighted_v(fie, pipe16, grouped):
    cfgs, pipe = pipe16
    x = eo.eval_inputs(cfgs)
    w = eo.eval_weights()
    w[0, 76], w[1, 0] = 8.0, 1.3                                                       # the last row of an image and the first of the next
    assert pipe.unet.kv_all is not None and pipe.controlnet.kv_all is not None and fie.kv_group
    before = fie.kv_group
    fie.kv_group = grouped
    try:
        plain = _fill_caches(pipe, fie, x, None)
        got = _fill_caches(pipe, fie, x, torch.from_numpy(w.reshape(-1)).to(fie.device))
        for net in (pipe.unet, pipe.controlnet):
            shared = [b.kv_cache.untyped_storage().data_ptr() == net._kv_out.untyped_storage().data_ptr() if net._kv_out is not None else False
                      for b in eo.blocks(net)]
            assert all(shared) if grouped else not any(shared)
        again = _fill_caches(pipe, fie, x, None)                                       # begin_image without weights forgets them
    finally:
        fie.kv_group = before
    want = eo.expected_caches(plain, w)
    assert len(got) == len(plain) == len(eo.blocks(pipe.unet)) + len(eo.blocks(pipe.controlnet)) > 4
    for (c, g), (_, e), (_, p), (_, a) in zip(got, want, plain, again):
        assert g.shape == (2 * T, 2 * c) and eo.same_bits(g[:, :c], p[:, :c])          # K: bit-identical
        assert eo.same_bits(g, e) and not eo.same_bits(g[:, c:], p[:, c:])             # V: the restatement of the plain cache
        assert eo.same_bits(a, p)


# ---------------------------------------------------------------------------------------------------------------- 3. one evaluation, fp32
@pytest.mark.parametrize("stack_name", ["tiny", "tiny-nomid"])
def test_eval_fp32_against_the_weighted_oracle(f32, stack_name):
    """One ControlNet + UNet evaluation in the fp32 context (the per-block path) on the inputs of test_unet_controlnet_eval_parity with the weights
    w[1, 2:5] = 4, w[1, 7] = 0, w[0, 3] = 0.5, against the unchanged oracle whose `attn2.to_v` outputs are multiplied by them.  Bound: twice the
    plain evaluation's error against the plain oracle, measured here (the parent's path).  V rows grow by up to 4, in a term that is a small
    share of the output.  The two oracles differ by 1.0e-2 (tests/test_emphasis_cpu.py), far above it: code that ignores the weights fails.
    Measured on an MI355X: see DESIGN.md section 23."""
    from fie_amd import stack
    from fie_amd.pipe import HipImg2ImgPipeline
    cfgs, sds = stack.synthetic_stack(stack_name, True, device="cpu", dtype=torch.float32)
    pipe = HipImg2ImgPipeline(f32, cfgs, sds)
    x, w = eo.eval_inputs(cfgs), eo.eval_weights()
    ref_plain, ref_w = eo.oracle_eval(sds, cfgs, x), eo.oracle_eval(sds, cfgs, x, w)
    plain = eo.hip_eval(pipe, f32, x)
    got = eo.hip_eval(pipe, f32, x, emph=torch.from_numpy(w.reshape(-1)).to(f32.device))
    e_plain, e_w, apart = eo.rel_err(plain, ref_plain), eo.rel_err(got, ref_w), eo.rel_err(ref_w, ref_plain)
    print(f"{stack_name}: rel_err plain {e_plain:.3e}, emphasised {e_w:.3e} (bound {2 * e_plain:.3e}); the two oracles are {apart:.3e} apart; "
          f"the emphasised evaluation against the PLAIN oracle {eo.rel_err(got, ref_plain):.3e}")
    assert apart > 1e-3
    assert e_w <= 2 * e_plain


# ---------------------------------------------------------------------------------------------------------------- 4. the public calls
SIZE = dict(resolution=(512, 512))
NEG = "blurry [low] quality"


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    ed = FastEditor(model_name="tiny", enable_cpu_offload=False, prompt_emphasis=2.0)
    assert ed.prompt_emphasis == 2.0 and ed.pipe.prompt_emphasis == 2.0
    return ed


@pytest.fixture(scope="module")
def picture():
    from test_pipeline_gpu import synth_image
    return synth_image(7, 512)


@contextlib.contextmanager
def setting(ed, w, graph):
    before, g = ed.set_prompt_emphasis(w), ed.pipe.use_graph
    ed.pipe.use_graph = graph
    try:
        yield
    finally:
        ed.set_prompt_emphasis(before)
        ed.pipe.use_graph = g


def _strip(ed, prompt):
    from fie_amd import emphasis
    return emphasis.parse(prompt, 2.0)[0]


def _weights(ed, rows):
    """The token weights of the text rows of a job, [len(rows), 77], from the tokenizer's own entry."""
    return ed.pipe.tok_l.weighted(rows, 2.0)[1]


def _check(ed, plain, w):
    torch.cuda.synchronize()
    got, want = eo.caches(ed.pipe), eo.expected_caches(plain, w)
    assert (np.asarray(w) != 1.0).any() and len(got) == len(want)
    for (c, g), (_, e), (_, p) in zip(got, want, plain):
        assert g.shape[0] == np.asarray(w).size and eo.same_bits(g, e) and not eo.same_bits(g, p)


def test_edit_carries_the_weights(editor, picture):
    prompt = "a [red] kite over a (calm:0.5) sea"
    with setting(editor, None, False):
        editor.edit(picture, _strip(editor, prompt), negative_prompt=_strip(editor, NEG), seed=3, strength=0.5, **SIZE)
        plain = eo.caches(editor.pipe)
    with setting(editor, 2.0, False):
        editor.edit(picture, prompt, negative_prompt=NEG, seed=3, strength=0.5, **SIZE)
        w = _weights(editor, [NEG, prompt])                                            # CFG rows: [negative, positive]
        assert w[0, 2] == 2.0 and w[1, 2] == 2.0 and w[1, 6] == 0.5 and (w != 1.0).sum() == 3
        _check(editor, plain, w)


def test_edit_batch_gives_every_image_its_own_weights(editor, picture):
    prompts = ["a [red] kite", "a kite over the [stormy grey] sea"]
    other = picture.transpose(Image.FLIP_LEFT_RIGHT)
    with setting(editor, None, False):
        editor.edit_batch([picture, other], [_strip(editor, p) for p in prompts], seed=3, strength=0.5, **SIZE)
        plain = eo.caches(editor.pipe)
    with setting(editor, 2.0, False):
        editor.edit_batch([picture, other], prompts, seed=3, strength=0.5, **SIZE)
        w = _weights(editor, ["", prompts[0], "", prompts[1]])                         # image-major: [img0 negative, img0 positive, img1 ...]
        assert (w[0] == 1).all() and (w[2] == 1).all() and w[1, 2] == 2.0 and w[3, 5] == 2.0 and w[3, 6] == 2.0
        _check(editor, plain, w)
    w2 = _weights(editor, ["", prompts[0], "", "a plain kite"])                        # one image without a weighted token: its rows are ones
    assert (w2[3] == 1).all()
    with setting(editor, None, False):
        editor.edit_batch([picture, other], [_strip(editor, prompts[0]), "a plain kite"], seed=3, strength=0.5, **SIZE)
        plain2 = eo.caches(editor.pipe)
    with setting(editor, 2.0, False):
        editor.edit_batch([picture, other], [prompts[0], "a plain kite"], seed=3, strength=0.5, **SIZE)
        _check(editor, plain2, w2)


def test_edit_sweep_repeats_the_weights_for_every_variant(editor, picture):
    prompt = "a [red] kite"
    with setting(editor, None, False):
        editor.edit_sweep(picture, _strip(editor, prompt), strengths=[0.75, 0.5], seed=3, **SIZE)
        plain = eo.caches(editor.pipe)
    with setting(editor, 2.0, False):
        editor.edit_sweep(picture, prompt, strengths=[0.75, 0.5], seed=3, **SIZE)
        w = np.tile(_weights(editor, ["", prompt]), (2, 1))                            # two variants, each [negative, positive]
        assert w.shape == (4, T)
        _check(editor, plain, w)


def test_without_cfg_only_the_positive_rows_exist(editor, picture):
    prompt = "a [red] kite"
    with setting(editor, None, False):
        editor.edit(picture, _strip(editor, prompt), negative_prompt=NEG, guidance_scale=1.0, seed=3, strength=0.5, **SIZE)
        plain = eo.caches(editor.pipe)
    with setting(editor, 2.0, False):
        editor.edit(picture, prompt, negative_prompt=NEG, guidance_scale=1.0, seed=3, strength=0.5, **SIZE)
        w = _weights(editor, [prompt])
        assert plain[0][1].shape[0] == T
        _check(editor, plain, w)


def test_a_graph_replay_reads_the_next_prompts_weights(editor, picture):
    """The weights are device memory of the graph's static job: a replay with another prompt scales other rows by other weights."""
    first, second = "a [red] kite", "a red (kite:1.5) in the [evening sky]"
    kw = dict(seed=3, strength=0.5, guidance_scale=1.7, **SIZE)                        # a guidance no other test of this editor uses: a key of its own
    with setting(editor, None, False):                                                  # the plain caches of the SECOND prompt, eagerly, in front
        editor.edit(picture, _strip(editor, second), **kw)
        plain = eo.caches(editor.pipe)
    with setting(editor, 2.0, True):
        n = len(editor.pipe._graphs)
        editor.edit(picture, first, **kw)                                               # captures; the blocks' caches are the graph's from here on
        assert len(editor.pipe._graphs) == n + 1 and any("emph" in key[0] for key in editor.pipe._graphs)
        editor.edit(picture, second, **kw)                                              # replays
        assert len(editor.pipe._graphs) == n + 1
        w = _weights(editor, ["", second])
        assert w[1, 3] == 1.5 and w[1, 6] == 2.0 and w[1, 7] == 2.0 and w[1, 2] == 1.0
        _check(editor, plain, w)


# ---------------------------------------------------------------------------------------------------------------- 5. the identities
def _edit128(pipe, prompt, w):
    from oracle import canny
    from test_pipeline_gpu import synth_image
    img = synth_image(11, 128)
    ctrl = Image.fromarray(canny.canny_rgb(np.asarray(img)))
    pipe.prompt_emphasis = w
    try:
        kw = dict(prompt=prompt, negative_prompt="", image=img, control_image=ctrl, strength=0.8, num_inference_steps=4, guidance_scale=1.5,
                  controlnet_conditioning_scale=0.5)
        job = pipe.prepare(generator=torch.Generator("cpu").manual_seed(42), **kw)
        out = np.asarray(pipe(generator=torch.Generator("cpu").manual_seed(42), **kw).images[0])
    finally:
        pipe.prompt_emphasis = None
    return out, job


def test_identities_byte_for_byte(fie, pipe16, monkeypatch):
    from fie_amd import emphasis
    from fie_amd.tokenizer import StandInTokenizer
    _, pipe = pipe16
    marked, stripped = "a [red] circle next to a [blue] square", "a red circle next to a blue square"
    stripped_out, stripped_job = _edit128(pipe, stripped, None)
    n_graphs = len(pipe._graphs)
    # (b) setting 1.0: the stripped prompt under None -- the same job, graph key and bytes
    one_out, one_job = _edit128(pipe, marked, 1.0)
    assert np.array_equal(one_out, stripped_out) and len(pipe._graphs) == n_graphs
    assert set(one_job) == set(stripped_job) and "emph" not in one_job and pipe._graph_base(one_job, 0) == pipe._graph_base(stripped_job, 0)
    assert torch.equal(one_job["ids_l"], stripped_job["ids_l"]) and torch.equal(one_job["ids_g"], stripped_job["ids_g"])
    # (c) a weight that is not 1: a key of its own, the stripped ids, weights among the job's tensors
    two_out, two_job = _edit128(pipe, marked, 2.0)
    assert pipe._graph_base(two_job, 0) == pipe._graph_base(stripped_job, 0) + ("emph",) and len(pipe._graphs) == n_graphs + 1
    assert torch.equal(two_job["ids_l"], stripped_job["ids_l"]) and "emph" in pipe._tensor_keys(two_job) and "emph" not in pipe._tensor_keys(one_job)
    assert two_job["emph"].dtype == torch.float32 and two_job["emph"].cpu().numpy().tolist() == pipe.tok_l.weighted(["", marked], 2.0)[1].reshape(-1).tolist()
    assert two_out.shape == stripped_out.shape
    d = np.abs(two_out.astype(int) - stripped_out.astype(int))
    print(f"weight 2 on two tokens, tiny stack, 128 px: {int((d > 0).sum())} of {d.size} bytes differ, by at most {int(d.max())}")      # synthetic weights barely react
    # (a) setting None: nothing is parsed or launched, the brackets are tokenised as they are, the key is what it was
    def boom(*a, **k):
        raise AssertionError("prompt_emphasis=None must not reach the new code")
    monkeypatch.setattr(emphasis, "parse", boom)
    monkeypatch.setattr(StandInTokenizer, "weighted", boom)
    monkeypatch.setattr(type(fie), "kv_emphasis", boom)
    none_out, none_job = _edit128(pipe, marked, None)
    verbatim = pipe.tok_l(["", marked]).to(torch.int32)
    assert torch.equal(none_job["ids_l"].cpu(), verbatim) and not torch.equal(none_job["ids_l"], stripped_job["ids_l"])
    assert set(none_job) == set(stripped_job) and pipe._graph_base(none_job, 0) == pipe._graph_base(stripped_job, 0) and len(pipe._graph_base(none_job, 0)) == 7
    again, _ = _edit128(pipe, marked, None)
    assert np.array_equal(none_out, again) and len(pipe._graphs) == n_graphs + 1
