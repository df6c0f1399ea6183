"""Control weights on the device: fie_control_pyramid_u8 and fie_control_add against their numpy restatements to the bit,
inside guard bands; one ControlNet + UNet evaluation in the fp32 context against the oracle with its residuals weighed on the host; the scalar
path against the map path where they must agree; the steps window in the launch log; the weights of edit / edit_batch / edit_sweep / a graph
replay as they arrive in the job; and the identities of the setting, byte for byte on a whole edit."""
import contextlib

import numpy as np
import pytest
import torch
from PIL import Image

import control_oracle as co
import emphasis_oracle as eo
import isolation as iso

pytestmark = pytest.mark.gpu
A_VALUES = (0, 1, 128, 255)


@pytest.fixture(scope="module")
def f32():
    import fie_amd  # noqa: F401
    from fie_amd import hip
    return hip.context(0, torch.float32)


# ---------------------------------------------------------------------------------------------------------------- 1. the pyramid op
@pytest.mark.parametrize("size", [(8, 8), (24, 40), (128, 128), (512, 320)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_is_the_restatement(fie, size):
    """Byte-exact against weights_numpy(pyramid_numpy(...)) for a in {0, 1, 128, 255}: a random binary map and a grey map read as L masks, the grey
    map read as a level map, all 0, all 255 -- written inside guard bands."""
    from fie_amd import control
    h, w = size
    dims = control.level_dims(h, w)
    p_tot = sum(a * b for a, b in dims)
    maps = co.maps(h, w)
    cases = [("binary", True), ("grey", True), ("grey", False), ("zeros", True), ("full", False), ("full", True)]
    for name, binary in cases:
        e = maps[name]
        e_dev = torch.from_numpy(e).to(fie.device)
        pyr = control.pyramid_numpy(control.edit_ness(e) if binary else e, dims)
        for a in A_VALUES:
            view, guard = iso.guarded((p_tot,), dtype=torch.float32, device=fie.device, flat=True)
            assert fie.control_pyramid(e_dev, a, binary, out=view) is view
            torch.cuda.synchronize()
            guard.check(f"control_pyramid {name} a={a}")
            got = view.cpu().numpy()
            assert got.tobytes() == control.weights_numpy(pyr, a).tobytes(), (name, binary, a)
            if name == "zeros":
                assert (got == 1.0).all()
            if name == "full" and a == 0:
                assert (got == 0.0).all()
    fresh = fie.control_pyramid(torch.from_numpy(maps["grey"]).to(fie.device), 64, False, levels=2)       # two levels, an output of its own
    assert fresh.cpu().numpy().tobytes() == control.weights_numpy(control.pyramid_numpy(maps["grey"], dims[:2]), 64).tobytes()


# ---------------------------------------------------------------------------------------------------------------- 2. the add op
P_LEVELS = (256, 15, 1)                    # three levels; 15 makes an odd tail
W_OFF = (0, 256, 271)
SPECIALS = np.array([6e-8, -6e-8, 6.0976e-5, -6.0976e-5, 65504.0, -65504.0, 0.0, -0.0, 3.0e-5], np.float16)


def _weights(images, seed):
    """f32 [images, 272]: zeros, ones and fractions at every level, every image different."""
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array([0.0, 1.0, 0.5, 0.25, 0.75, 1.0 / 3.0, 0.99609375], np.float32), size=(images, sum(P_LEVELS))).astype(np.float32)
    w[:, 0], w[:, 1], w[:, 256], w[:, 257], w[0, 271], w[1:, 271] = 0.0, 1.0, 0.0, 0.5, 0.0, 0.75
    return w


def _operands(rows, c, dtype, seed):
    """u and t with the edge cases of test_emphasis_gpu.py::_operand: f16 subnormals, the largest finite f16 of both signs, zeros of both signs."""
    rng = np.random.default_rng(seed)
    u, t = (rng.standard_normal((rows, c)).astype(np.float16) for _ in range(2))
    for x in (u, t):
        for r in rng.choice(rows, size=min(rows, 3), replace=False):
            x[r, rng.choice(c, size=min(c, len(SPECIALS)), replace=False)] = SPECIALS[:min(c, len(SPECIALS))]
    return u.astype(dtype), t.astype(dtype)


def _run_add(ctx, specs, w, dtype):
    """One launch on the segments `specs` = [(B, level, C, s)] -> asserts every output against add_numpy, to the bit, inside guard bands."""
    from fie_amd import control
    tdt = torch.float16 if dtype == np.float16 else torch.float32
    w_dev = torch.from_numpy(w).to(ctx.device)
    segs, outs, guards, want = [], [], [], []
    for i, (b, lvl, c, s) in enumerate(specs):
        p, woff = P_LEVELS[lvl], W_OFF[lvl]
        u, t = _operands(b * p, c, dtype, seed=100 * len(specs) + i)
        zero_rows = [r for r in range(b * p) if np.float32(s) * w[(r // p) // 2, woff + r % p] == 0]
        assert zero_rows
        t[zero_rows[0]] = np.nan                                                       # under c == 0: t is not read, u's bits come out
        if len(zero_rows) > 1:
            t[zero_rows[-1], 0] = np.inf
        view, guard = iso.guarded((b * p, c), dtype=tdt, device=ctx.device, flat=True)
        segs.append((torch.from_numpy(u).to(ctx.device), torch.from_numpy(t).to(ctx.device), p, woff, s))
        outs.append(view)
        guards.append(guard)
        want.append((control.add_numpy(u, t, s, w[:, woff:woff + p], 2), u, zero_rows))
    made = ctx.control_add(segs, w_dev, 2, outs=outs)
    torch.cuda.synchronize()
    assert all(m is o for m, o in zip(made, outs))
    for i, (g, o, (exp, u, zero_rows)) in enumerate(zip(guards, outs, want)):
        g.check(f"control_add segment {i} {specs[i]}")
        got = o.cpu().numpy()
        assert eo.same_bits(got, exp), (i, specs[i], int((got.view(np.uint8) != exp.view(np.uint8)).sum()))
        assert eo.same_bits(got[zero_rows], u[zero_rows])                              # said once more: c == 0 keeps u, NaN and infinity in t or not
    fresh = ctx.control_add(segs[:1], w_dev, 2)                                        # and into an output of the wrapper's own
    torch.cuda.synchronize()
    assert fresh[0].shape == segs[0][0].shape and eo.same_bits(fresh[0].cpu().numpy(), want[0][0])


@pytest.mark.parametrize("dtype", [np.float16, np.float32], ids=["f16", "f32"])
def test_add_is_the_restatement(fie, f32, dtype):
    """One launch with the maximum of 16 segments -- C in {8, 64, 320, 1280} x P in {256, 15, 1}, 2 rows (one image x CFG) and 8 (four images x
    CFG), s in {0.5, 2, 1e-42: products that are f32 subnormals} -- and one launch with a single segment."""
    ctx = fie if dtype == np.float16 else f32
    w = _weights(4, seed=7)
    scales = (0.5, 2.0, 1e-42)
    specs = []
    for i, (c, lvl) in enumerate([(c, lvl) for c in (8, 64, 320, 1280) for lvl in (0, 1, 2)] + [(8, 1), (320, 2), (64, 0), (1280, 1)]):
        specs.append((2 if i % 2 else 8, lvl, c, scales[i % 3]))
    assert len(specs) == 16 and {s[0] for s in specs} == {2, 8}
    _run_add(ctx, specs, w, dtype)
    _run_add(ctx, [(8, 1, 320, 2.0)], w, dtype)
    if dtype == np.float16:                                                            # 65504 + 2 * 65504 is an f16 infinity, as the restatement says
        u = np.full((2, 8), 65504.0, np.float16)
        out = ctx.control_add([(torch.from_numpy(u).to(ctx.device), torch.from_numpy(u).to(ctx.device), 1, 257, 2.0)], torch.from_numpy(w).to(ctx.device), 2)
        assert w[0, 257] == 0.5 and np.isinf(out[0].cpu().numpy()).all()


def test_wrappers_refuse_bad_tensors(fie):
    dev = fie.device
    e = torch.zeros(16, 24, dtype=torch.uint8, device=dev)
    for bad in (lambda: fie.control_pyramid(e.float(), 0, True), lambda: fie.control_pyramid(e[:, :8], 0, True), lambda: fie.control_pyramid(e, 256, True),
                lambda: fie.control_pyramid(e, 0.5, True), lambda: fie.control_pyramid(e[:12], 0, True), lambda: fie.control_pyramid(e, 0, True, levels=4),
                lambda: fie.control_pyramid(e, 0, True, out=torch.zeros(5, device=dev)), lambda: fie.control_pyramid(e[None], 0, True),
                lambda: fie.control_pyramid(torch.zeros(8, 2056, dtype=torch.uint8, device=dev), 0, True)):
        with pytest.raises(ValueError, match="control"):
            bad()
    u = torch.zeros(4, 16, dtype=torch.float16, device=dev)
    w = torch.ones(1, 2, device=dev)
    seg = (u, u.clone(), 2, 0, 0.5)
    for bad in (lambda: fie.control_add([], w, 2), lambda: fie.control_add([seg] * 17, w, 2), lambda: fie.control_add([seg], w.half(), 2),
                lambda: fie.control_add([seg], w[0], 2), lambda: fie.control_add([seg], w, 0), lambda: fie.control_add([seg], w, 1),
                lambda: fie.control_add([(u.float(), u.float(), 2, 0, 0.5)], w, 2), lambda: fie.control_add([(u, u[:2], 2, 0, 0.5)], w, 2),
                lambda: fie.control_add([(u.t(), u.t(), 2, 0, 0.5)], w, 2), lambda: fie.control_add([(u, u, 3, 0, 0.5)], w, 2),
                lambda: fie.control_add([(u, u, 2, 1, 0.5)], w, 2), lambda: fie.control_add([(u[:, :12], u[:, :12], 2, 0, 0.5)], w, 2),
                lambda: fie.control_add([(u, u.cpu(), 2, 0, 0.5)], w, 2), lambda: fie.control_add([seg], w, 2, outs=[u]),
                lambda: fie.control_add([seg], w, 2, outs=[]), lambda: fie.control_add([(u, u, 2, 0, float("nan"))], w, 2)):
        with pytest.raises(ValueError, match="control_add"):
            bad()


# ---------------------------------------------------------------------------------------------------------------- 3. one evaluation, fp32
@pytest.fixture(scope="module", params=["tiny", "tiny-nomid"])
def rig32(request, f32):
    from fie_amd import stack
    from fie_amd.pipe import HipImg2ImgPipeline
    cfgs, sds = stack.synthetic_stack(request.param, True, device="cpu", dtype=torch.float32)
    pipe = HipImg2ImgPipeline(f32, cfgs, sds)
    x = eo.eval_inputs(cfgs)
    ref_plain = eo.oracle_eval(sds, cfgs, x)                                           # computed once, shared, left unchanged
    plain = eo.hip_eval(pipe, f32, x)                                                  # the parent's own path
    return request.param, cfgs, sds, pipe, x, ref_plain, plain


def test_eval_fp32_against_the_weighted_oracle(f32, rig32):
    """One ControlNet + UNet evaluation in the fp32 context on the inputs of test_unet_controlnet_eval_parity under (a) layers="prompt" -- the scalar
    path --, (b) in_mask=0 with the hole rows 20..99 x columns 36..127 of the 128 x 128 edit -- the map path, the weights made by
    fie_control_pyramid_u8 --, (c) both, against the unchanged oracle whose ControlNet residuals, taken at scale 1, are multiplied on the host by
    0.5 * layer_i * w.  Bound: twice the plain evaluation's error against the plain oracle, measured here on the parent's path.  The weighted
    oracles are 4.6e-2 .. 7.6e-2 from the plain one (tests/test_control_cpu.py): code that ignores the weights fails.  Measured on an MI355X: see
    DESIGN.md section 25."""
    from fie_amd import control
    name, cfgs, sds, pipe, x, ref_plain, plain = rig32
    assert pipe.controlnet.n_out == 10 and pipe.controlnet.residual_levels() == co.LEVELS
    e_plain = eo.rel_err(plain, ref_plain)
    w_host = co.eval_weights(0.0)
    w_dev = f32.control_pyramid(torch.from_numpy(co.hole_map()).to(f32.device), control.mask_a(0.0), True)[None]
    torch.cuda.synchronize()
    assert w_dev.cpu().numpy().tobytes() == w_host[None].tobytes()
    prompt = control.presets(10)["prompt"]
    cases = {"(a) prompt": (prompt, None), "(b) in_mask=0": ((1.0,) * 10, w_host), "(c) both": (prompt, w_host)}
    for case, (layers, w) in cases.items():
        ref = co.oracle_eval(sds, cfgs, x, [0.5 * v for v in layers], w)
        got = co.hip_eval(pipe, f32, x, control.layer_scales(0.5, layers), None if w is None else w_dev)
        e_w, apart = eo.rel_err(got, ref), eo.rel_err(ref, ref_plain)
        print(f"{name} {case}: rel_err plain {e_plain:.3e}, weighted {e_w:.3e} (bound {2 * e_plain:.3e}, ratio {e_w / e_plain:.2f}); the two oracles are "
              f"{apart:.3e} apart; the weighted evaluation against the PLAIN oracle {eo.rel_err(got, ref_plain):.3e}")
        assert apart > 1e-2
        assert e_w <= 2 * e_plain, case


def test_scalar_path_equals_map_path_under_a_map_of_ones(f32, rig32):
    """A mask of all 0 at a = 0 weighs every position 1: the map path -- bare residuals, then one fie_control_add -- must give what the scalar path
    gives, up to the f32 ulps by which u + s * t in two roundings differs from the GEMM epilogue's form.  Bound: the plain evaluation's own error
    against its oracle (some 1e-5), three orders below the 4.6e-2 .. 7.7e-2 by which the weighted oracles stand apart.  Measured: DESIGN.md 25."""
    from fie_amd import control
    name, cfgs, sds, pipe, x, ref_plain, plain = rig32
    ones = f32.control_pyramid(torch.zeros(128, 128, dtype=torch.uint8, device=f32.device), 0, True)[None]
    assert bool((ones == 1.0).all())
    for layers in ((1.0,) * 10, control.presets(10)["guess"]):
        scales = control.layer_scales(0.5, layers)
        scalar, mapped = co.hip_eval(pipe, f32, x, scales, None), co.hip_eval(pipe, f32, x, scales, ones)
        d = eo.rel_err(mapped, scalar)
        print(f"{name}: max relative difference map path vs scalar path {d:.3e} (layers[0] = {layers[0]:.3g}); plain error {eo.rel_err(plain, ref_plain):.3e}")
        assert d <= eo.rel_err(plain, ref_plain)
    assert eo.rel_err(co.hip_eval(pipe, f32, x, control.layer_scales(0.5, None, 10), None), plain) == 0.0      # all layers 1, scalar: the parent's kernels and bits
    skipped = co.hip_eval(pipe, f32, x, (0.0,) * 10, None)                             # every s_i == 0: the UNet alone
    assert eo.rel_err(skipped, co.oracle_eval(sds, cfgs, x, [0.0] * 10)) <= 2 * eo.rel_err(plain, ref_plain)


# ---------------------------------------------------------------------------------------------------------------- 4. the steps window
SIZE = dict(resolution=(512, 512))
PROMPT = "a red kite over a calm sea"


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    ed = FastEditor(model_name="tiny", enable_cpu_offload=False, control_weights=dict(in_mask=0.5))
    assert ed.control_weights == dict(layers=None, steps=None, in_mask=0.5) and ed.pipe.control_weights.in_mask == 0.5
    assert ed.set_control_weights() == dict(layers=None, steps=None, in_mask=0.5) and ed.pipe.control_weights is None
    return ed


@pytest.fixture(scope="module")
def picture():
    from test_pipeline_gpu import synth_image
    return synth_image(7, 512)


@contextlib.contextmanager
def setting(ed, graph=False, **kw):
    before, g = ed.set_control_weights(**kw), ed.pipe.use_graph
    ed.pipe.use_graph = graph
    try:
        yield
    finally:
        ed.set_control_weights(**(before or {}))
        ed.pipe.use_graph = g


def _logged(ctx, fn):
    ctx.oplog(True)
    try:
        out = fn()
        return out, ctx.oplog_read()
    finally:
        ctx.oplog(False)


def _desc(line):
    """The op's own description of a launch line; "" for a mark."""
    return "" if line.startswith("#") else line.split("|", 4)[4]


def _trunk(line):
    """The ControlNet's conv_in: the one conv on the 8-channel latents that adds a residual (the edge-map embedding)."""
    d = _desc(line)
    return d.startswith("conv ") and " in=64x64x8 " in d and " res=1 " in d


def _embedding(line):
    """The edge-map embedding's stride-2 convs: the only stride-2 convs with an activation."""
    d = _desc(line)
    return d.startswith("conv ") and " s2 " in d and " act=1 " in d


def _per_step(lines):
    """The launch lines of every loop step: from an `embed` mark to the step's `lcm_step` mark."""
    out, cur = [], None
    for l in lines:
        if l == "#embed":
            cur = []
        elif l == "#lcm_step" and cur is not None:
            out.append(cur)
            cur = None
        elif cur is not None and not l.startswith("#"):
            cur.append(l)
    return out


def test_steps_window_in_the_launch_log(editor, fie, picture):
    kw = dict(seed=3, strength=1.0, num_inference_steps=4, **SIZE)
    with setting(editor):
        _, plain = _logged(fie, lambda: editor.edit(picture, PROMPT, **kw))
    steps = _per_step(plain)
    convs = [_desc(l) for l in plain if _desc(l).startswith("conv ")]
    assert len(steps) == 4 and [sum(map(_trunk, s)) for s in steps] == [1] * 4 and sum(map(_embedding, plain)) >= 2, convs[:40]
    with setting(editor, steps=(0, 0.5)):
        (_, met), half = _logged(fie, lambda: editor.edit(picture, PROMPT, metrics=True, **kw))
    assert met["control_steps_kept"] == 2 and editor.pipe.last_stats["control_steps_kept"] == 2
    steps2 = _per_step(half)
    assert [sum(map(_trunk, s)) for s in steps2] == [1, 1, 0, 0] and sum(map(_embedding, half)) == sum(map(_embedding, plain))
    assert [len(s) for s in steps2[:2]] == [len(s) for s in steps[:2]] and all(len(a) < len(b) for a, b in zip(steps2[2:], steps[2:]))
    # (0, 0): no launch of the ControlNet at all, and the bytes and latents of conditioning scale 0 under the setting None (x + 0 * y leaves a finite x)
    with setting(editor, steps=(0, 0)):
        (img0, met0), none = _logged(fie, lambda: editor.edit(picture, PROMPT, metrics=True, **kw))
        lat0 = editor.pipe._latents.clone()
    assert met0["control_steps_kept"] == 0 and not any(map(_trunk, none)) and not any(map(_embedding, none))
    assert len([l for l in none if not l.startswith("#")]) < len([l for l in plain if not l.startswith("#")])
    with setting(editor):
        img_ref, ref = _logged(fie, lambda: editor.edit(picture, PROMPT, controlnet_conditioning_scale=0.0, **kw))
        lat_ref = editor.pipe._latents.clone()
    assert any(map(_trunk, ref)) and torch.isfinite(lat_ref).all()
    assert torch.equal(lat0, lat_ref) and np.array_equal(np.asarray(img0), np.asarray(img_ref))


# ---------------------------------------------------------------------------------------------------------------- 5. the public calls
def _mask(box, size=512):
    m = np.zeros((size, size), np.uint8)
    m[box[0]:box[1], box[2]:box[3]] = 255
    return m


@contextlib.contextmanager
def jobs_of(pipe):
    """Inside: every job run_device() sees is appended to the list."""
    seen, plain = [], pipe.run_device

    def run(job):
        seen.append(job)
        return plain(job)
    pipe.run_device = run
    try:
        yield seen
    finally:
        del pipe.run_device


def _expected(mask_l, in_mask, binary=True):
    from fie_amd import control
    e = control.edit_ness(mask_l) if binary else mask_l
    return control.weights_numpy(control.pyramid_numpy(e, control.level_dims(*mask_l.shape)), control.mask_a(in_mask))


def test_edit_weighs_by_the_grown_mask(editor, picture):
    import mask_grow_oracle as mgo
    from fie_amd import control
    m = _mask((100, 301, 141, 400))
    with setting(editor, in_mask=0.25), jobs_of(editor.pipe) as jobs:
        editor.edit(picture, PROMPT, mask=Image.fromarray(m), mask_grow=8, seed=3, strength=0.5, **SIZE)
    assert len(jobs) == 1 and jobs[0]["ctl_w"].shape == (1, 64 * 64 + 32 * 32 + 16 * 16) and jobs[0]["ctl_w"].dtype == torch.float32
    got = jobs[0]["ctl_w"][0].cpu().numpy()
    assert got.tobytes() == _expected(mgo.grow(m, 8), 0.25).tobytes() and got.tobytes() != _expected(m, 0.25).tobytes()
    assert got.min() == 0.25 and got.max() == 1.0 and jobs[0]["ctl_layers"] == control.layer_scales(jobs[0]["cn_scale"], None, 10)
    assert jobs[0]["ctl_keep"] == (True,) * len(jobs[0]["steps"])
    with setting(editor, in_mask=0.25), jobs_of(editor.pipe) as jobs:                  # no mask: nothing to weigh, the scalar job, no error
        editor.edit(picture, PROMPT, seed=3, strength=0.5, **SIZE)
    assert "ctl_w" not in jobs[0] and jobs[0]["ctl_layers"] == control.layer_scales(jobs[0]["cn_scale"], None, 10)


def test_edit_batch_gives_an_unmasked_image_ones(editor, picture):
    m = _mask((64, 200, 64, 333))
    other = picture.transpose(Image.FLIP_LEFT_RIGHT)
    with setting(editor, in_mask=0.0), jobs_of(editor.pipe) as jobs:
        editor.edit_batch([picture, other], [PROMPT, "a plain kite"], masks=[Image.fromarray(m), None], seed=3, strength=0.5, **SIZE)
    w = jobs[0]["ctl_w"].cpu().numpy()
    assert w.shape[0] == 2 and w[0].tobytes() == _expected(m, 0.0).tobytes() and (w[1] == 1.0).all() and w[0].min() == 0.0


def test_levels_mode_weighs_by_the_greys(editor, picture):
    yy, xx = np.mgrid[0:512, 0:512]
    v = np.clip(xx - 100, 0, 255).astype(np.uint8)                                     # a ramp of greys: 0 on the left, 255 on the right
    with setting(editor, in_mask=0.0), jobs_of(editor.pipe) as jobs:
        editor.edit(picture, PROMPT, mask=Image.fromarray(v), mask_mode="levels", seed=3, strength=0.5, **SIZE)
    got = jobs[0]["ctl_w"][0].cpu().numpy()
    assert got.tobytes() == _expected(v, 0.0, binary=False).tobytes() and got.tobytes() != _expected(v, 0.0, binary=True).tobytes()
    assert len(np.unique(got)) > 20


def test_edit_sweep_shares_one_weight_vector_and_refuses_a_window(editor, picture):
    from fie_amd import control
    m = _mask((100, 301, 141, 400))
    with setting(editor, layers="prompt", in_mask=0.0), jobs_of(editor.pipe) as jobs:
        imgs, variants = editor.edit_sweep(picture, PROMPT, strengths=[0.75, 0.5], mask=Image.fromarray(m), seed=3, **SIZE)
    assert len(imgs) == 2 and jobs[0]["sweep"] and jobs[0]["ctl_w"].shape[0] == 1
    assert jobs[0]["ctl_w"][0].cpu().numpy().tobytes() == _expected(m, 0.0).tobytes()
    assert jobs[0]["ctl_layers"] == control.layer_scales(jobs[0]["cn_scale"], control.presets(10)["prompt"]) and jobs[0]["ctl_layers"][0] < jobs[0]["ctl_layers"][9]
    assert [v["control_steps_kept"] for v in variants] == [v["steps"] for v in variants]
    with setting(editor):
        plain, _ = editor.edit_sweep(picture, PROMPT, strengths=[0.75, 0.5], mask=Image.fromarray(m), seed=3, **SIZE)
    assert any(not np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(imgs, plain))
    with setting(editor, steps=(0, 0.5)):
        with pytest.raises(ValueError, match="steps"):
            editor.edit_sweep(picture, PROMPT, strengths=[0.75, 0.5], seed=3, **SIZE)


def test_a_graph_replay_reads_the_next_masks_weights(editor, picture):
    """The weights are device memory of the graph's static job: a replay with another mask weighs other positions."""
    first, second = _mask((100, 301, 141, 400)), _mask((10, 500, 200, 260))
    kw = dict(seed=3, strength=0.5, guidance_scale=1.9, **SIZE)                        # a guidance no other test of this editor uses: a key of its own
    with setting(editor, graph=True, in_mask=0.0):
        before = set(editor.pipe._graphs)
        a = editor.edit(picture, PROMPT, mask=Image.fromarray(first), **kw)            # captures
        new = set(editor.pipe._graphs) - before
        assert len(new) == 1
        key = next(iter(new))
        static = editor.pipe._graphs[key][1]
        assert [part for part in key[0] if isinstance(part, tuple) and part and part[0] == "ctl"] == [("ctl", static["ctl_layers"], static["ctl_keep"], True)]
        assert all(static["ctl_keep"]) and len(set(static["ctl_layers"])) == 1
        assert static["ctl_w"][0].cpu().numpy().tobytes() == _expected(first, 0.0).tobytes()
        b = editor.edit(picture, PROMPT, mask=Image.fromarray(second), **kw)           # replays
        assert set(editor.pipe._graphs) - before == new
        torch.cuda.synchronize()
        assert static["ctl_w"][0].cpu().numpy().tobytes() == _expected(second, 0.0).tobytes()
        assert not np.array_equal(np.asarray(a), np.asarray(b))
        again = editor.edit(picture, PROMPT, mask=Image.fromarray(first), **kw)
        assert np.array_equal(np.asarray(a), np.asarray(again))


# ---------------------------------------------------------------------------------------------------------------- 6. the identities
@pytest.fixture(scope="module")
def pipe16(fie):
    from fie_amd import stack
    from fie_amd.pipe import HipImg2ImgPipeline
    cfgs, sds = stack.synthetic_stack("tiny", True, device="cpu", dtype=torch.float16)
    return HipImg2ImgPipeline(fie, cfgs, sds, noise_dtype=torch.float32)


def _edit128(pipe, ctl):
    from oracle import canny
    from test_pipeline_gpu import synth_image
    img = synth_image(11, 128)
    ctrl = Image.fromarray(canny.canny_rgb(np.asarray(img)))
    pipe.control_weights = ctl
    try:
        kw = dict(prompt="a red circle next to a blue square", negative_prompt="", image=img, control_image=ctrl, strength=0.8, num_inference_steps=4,
                  guidance_scale=1.5, controlnet_conditioning_scale=0.5)
        job = pipe.prepare(generator=torch.Generator("cpu").manual_seed(42), **kw)
        out = np.asarray(pipe(generator=torch.Generator("cpu").manual_seed(42), **kw).images[0])
    finally:
        pipe.control_weights = None
    return out, job


def test_identities_byte_for_byte(fie, pipe16, monkeypatch):
    from fie_amd import control
    from fie_amd.nn import ControlNet
    pipe = pipe16
    base_out, base_job = _edit128(pipe, None)
    n_graphs = len(pipe._graphs)
    assert len(pipe._graph_base(base_job, 0)) == 7 and not any(k in base_job for k in ("ctl_layers", "ctl_keep", "ctl_w"))
    # (b) the neutral setting is None: the same job, graph key and bytes, and no new graph
    neutral = control.check([1.0] * 10, (0, 1), 1.0, 10)
    assert neutral is None
    one_out, one_job = _edit128(pipe, neutral)
    assert np.array_equal(one_out, base_out) and len(pipe._graphs) == n_graphs
    assert set(one_job) == set(base_job) and pipe._graph_base(one_job, 0) == pipe._graph_base(base_job, 0)
    # (c) layers="prompt": a key of its own, other bytes
    p_out, p_job = _edit128(pipe, control.check("prompt", None, None, 10))
    key = pipe._graph_base(p_job, 0)
    assert key[:7] == pipe._graph_base(base_job, 0) and key[7] == ("ctl", control.layer_scales(0.5, control.presets(10)["prompt"]), (True,) * len(p_job["steps"]), False)
    assert len(pipe._graphs) == n_graphs + 1 and set(p_job) == set(base_job) | {"ctl_layers", "ctl_keep"} and "ctl_w" not in pipe._tensor_keys(p_job)
    d = np.abs(p_out.astype(int) - base_out.astype(int))
    print(f"layers='prompt', tiny stack, 128 px: {int((d > 0).sum())} of {d.size} bytes differ, by at most {int(d.max())}")
    assert (d > 0).any()
    # (a) setting None: nothing new is parsed, allocated or launched
    def boom(*a, **k):
        raise AssertionError("control_weights=None must not reach the new code")
    for owner, name in ((type(fie), "control_pyramid"), (type(fie), "control_add"), (ControlNet, "add_residuals_weighted"), (control, "layer_scales"),
                        (control, "keep"), (control, "mask_a"), (control, "check")):
        monkeypatch.setattr(owner, name, boom)
    none_out, none_job = _edit128(pipe, None)
    assert set(none_job) == set(base_job) and pipe._graph_base(none_job, 0) == pipe._graph_base(base_job, 0) and len(pipe._graph_base(none_job, 0)) == 7
    assert np.array_equal(none_out, base_out) and len(pipe._graphs) == n_graphs + 1
