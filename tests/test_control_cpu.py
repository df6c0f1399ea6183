"""Control weights, host side (no GPU): the setting and its presets, the keep rule against a table written out by hand, the
weight pyramid against a plain Python loop, the add's restatement, the interface (pinned signatures, the environment's format, the command line,
the C entries' argument checks) -- and the condition of the GPU evaluation test: the oracle with weighed ControlNet residuals differs from the plain
one by far more than any fp32 bound."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import fie_amd  # noqa: F401
from fie_amd import control, hip

import control_oracle as co
import emphasis_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    hip.build()
    return hip.lib()


# ---------------------------------------------------------------------------------------------------------------- 1. the setting
def test_presets_and_neutral_forms():
    s = control.check("prompt", None, None, 10)
    assert s.steps is None and s.in_mask is None and len(s.layers) == 10
    assert s.layers[9] == 1.0 and s.layers[8] == 0.825 and s.layers[0] == 0.825 ** 9 and all(a < b for a, b in zip(s.layers, s.layers[1:]))
    g = control.check("guess", None, None, 10).layers
    assert g[0] == pytest.approx(0.1, rel=1e-15) and g[9] == 1.0 and g[3] == pytest.approx(10 ** (-1 + 3 / 9), rel=1e-15)
    assert g == tuple(float(v) for v in np.logspace(-1, 0, 10))
    for neutral in ((None, None, None), ("balanced", None, None), ([1.0] * 10, (0, 1), 1.0), ((1,) * 10, [0.0, 1.0], 1), (None, (0, 1), None)):
        assert control.check(*neutral, 10) is None
    s = control.check([1.0] * 10, (0, 0.5), 1.0, 10)
    assert s == control.Setting(None, (0.0, 0.5), None)
    s = control.check(np.linspace(0, 2, 10), None, 0, 10)
    assert s.layers[0] == 0.0 and s.layers[9] == 2.0 and s.in_mask == 0.0 and isinstance(s.in_mask, float)
    assert control.check(None, (0, 0), None, 10).steps == (0.0, 0.0) and control.check(None, (0.3, 0.3), None, 10).steps == (0.3, 0.3)
    assert len(control.check("prompt", None, None, 4).layers) == 4


def test_every_bad_argument_raises():
    for bad in ("strong", [1.0] * 9, [1.0] * 11, [1.0] * 9 + [2.01], [1.0] * 9 + [-0.1], [1.0] * 9 + [float("nan")], [1.0] * 9 + ["1"], [True] * 10, 1.0):
        with pytest.raises(ValueError, match="layers"):
            control.check(bad, None, None, 10)
    for bad in ((0.5, 0.25), (-0.1, 1), (0, 1.1), (0, 0.5, 1), (0,), 0.5, "0:1", (0, float("nan")), (False, True)):
        with pytest.raises(ValueError, match="steps"):
            control.check(None, bad, None, 10)
    for bad in (-0.01, 1.01, float("nan"), "0", True, [0.5]):
        with pytest.raises(ValueError, match="in_mask"):
            control.check(None, None, bad, 10)
    for bad in (1, 17, 10.0, True):
        with pytest.raises(ValueError, match="n_out"):
            control.check(None, None, None, bad)


def test_layer_scales():
    for c in (0.5, 0.3, 1.0, 0.0, 1.7):
        s = control.layer_scales(c, (1.0,) * 10)
        assert s == control.layer_scales(c, None, 10) and all(np.float32(v).tobytes() == np.float32(c).tobytes() for v in s)      # c itself, bit for bit
    lay = control.presets(10)["prompt"]
    s = control.layer_scales(0.3, lay)
    assert [np.float32(v) for v in s] == [np.float32(np.float64(0.3) * np.float64(v)) for v in lay] and all(isinstance(v, float) for v in s)
    assert control.layer_scales(0.5, (0.0, 2.0)) == (0.0, 1.0)


KEEP = {  # (start, end) -> the kept steps of K = 1, 2, 3, 4, written out by hand from: drop k iff k / K < start or (k + 1) / K > end
    (0, 1): ["1", "11", "111", "1111"],
    (0, 0.5): ["0", "10", "100", "1100"],
    (0.5, 1): ["0", "01", "001", "0011"],
    (0, 0): ["0", "00", "000", "0000"],
    (0.25, 0.75): ["0", "00", "010", "0110"],
}


def test_keep_rule_against_the_table():
    for window, rows in KEEP.items():
        for n, row in enumerate(rows, 1):
            assert control.keep(n, window) == tuple(c == "1" for c in row), (window, n)
            assert control.keep(n, None) == (True,) * n
    assert control.keep(4, control.check(None, (0, 1), None, 10) and (0, 1)) == (True,) * 4


# ---------------------------------------------------------------------------------------------------------------- 2. the weight pyramid
@pytest.mark.parametrize("size", co.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pyramid_against_a_plain_loop(size):
    h, w = size
    dims = control.level_dims(h, w)
    assert dims[0] == (h // 8, w // 8) and all(b == ((a[0] + 1) // 2, (a[1] + 1) // 2) for a, b in zip(dims, dims[1:])) and len(dims) == 3
    if size == (8, 8):
        assert dims == [(1, 1)] * 3
    if size == (24, 40):
        assert dims == [(3, 5), (2, 3), (1, 2)]                                        # odd latent sizes: the last block of every level is clipped
    names = ("binary", "grey", "zeros", "full") if h * w <= 128 * 128 else ("grey",)    # the loop is slow: one map at the largest size
    for name in names:
        e = co.maps(h, w)[name]
        pyr, ref = control.pyramid_numpy(e, dims), co.pyramid_loop(e)
        for (big_e, cnt), (re_, rc) in zip(pyr, ref):
            assert big_e.dtype == np.int32 and cnt.dtype == np.int32 and big_e.tolist() == re_ and cnt.tolist() == rc
        for a in (0, 1, 128, 255):
            got = control.weights_numpy(pyr, a)
            assert got.dtype == np.float32 and got.shape == (sum(x * y for x, y in dims),)
            assert got.tobytes() == co.weights_loop(ref, a).tobytes(), (name, a)
        if name == "zeros":
            assert (control.weights_numpy(pyr, 0) == 1.0).all()
        if name == "full":
            assert (control.weights_numpy(pyr, 0) == 0.0).all() and (control.weights_numpy(pyr, 128) == 0.5).all()
    with pytest.raises(ValueError):
        control.pyramid_numpy(co.maps(h, w)["grey"], dims[::-1] if dims[0] != dims[-1] else [(2, 2)])


def test_weights_are_monotone_and_fractional_at_the_rim_only():
    cnt = np.full((1, 5), 64, np.int32)
    big_e = np.array([[0, 255, 255 * 32, 255 * 63, 255 * 64]], np.int32)
    for a in (0, 1, 128, 255):
        w = control.weights_numpy([(big_e, cnt)], a)
        assert w[0] == 1.0 and (np.diff(w) < 0).all() and w[-1] == np.float32(a / 256)
    # the hole of the evaluation test: rows 20 .. 99 and columns 36 .. 127 -- cut through 8-px blocks above, below and on the left
    e = co.hole_map()
    w0 = control.weights_numpy(control.pyramid_numpy(e, control.level_dims(128, 128)), 0)[:256].reshape(16, 16)
    inside = np.zeros((16, 16), bool)
    inside[3:12, 5:16] = True                                                          # blocks wholly inside: rows 24 .. 95, columns 40 .. 127
    rim = np.zeros((16, 16), bool)
    rim[2:13, 4:16] = True
    rim &= ~inside
    assert (w0[inside] == 0.0).all() and (w0[~inside & ~rim] == 1.0).all() and ((w0[rim] > 0) & (w0[rim] < 1)).all()
    assert w0[2, 8] == np.float32(0.5) and w0[12, 8] == np.float32(0.5) and w0[5, 4] == np.float32(0.5) and w0[2, 4] == np.float32(0.75)
    assert control.mask_a(0) == 0 and control.mask_a(0.25) == 64 and control.mask_a(0.5) == 128 and control.mask_a(0.999) == 255
    assert control.edit_ness(np.array([[0, 127, 128, 255]], np.uint8)).tolist() == [[0, 0, 255, 255]]


# ---------------------------------------------------------------------------------------------------------------- 3. the add
def test_add_restatement():
    rng = np.random.default_rng(1)
    p, c, nb = 3, 8, 2
    w = np.array([[1.0, 0.0, 0.25], [0.5, 1.0, 0.0]], np.float32)                      # two images
    u = rng.standard_normal((2 * nb * p, c)).astype(np.float16)
    t = rng.standard_normal((2 * nb * p, c)).astype(np.float16)
    t[1] = np.nan                                                                      # image 0, row 0, position 1: weight 0
    t[4, 0] = np.inf                                                                   # image 0, row 1, position 1
    t[11] = -np.inf                                                                    # image 1, row 1, position 2: weight 0
    t[0, 0], u[0, 0] = 65504.0, 65504.0                                                # weight 1, s = 2: beyond f16
    out = control.add_numpy(u, t, 2.0, w, nb)
    assert out.dtype == np.float16 and eo.same_bits(out[[1, 4, 11]], u[[1, 4, 11]]) and np.isinf(out[0, 0]) and np.isfinite(np.delete(out, 0, 0)).all()
    for r in range(12):
        wr = w[r // (nb * p), r % p]
        with np.errstate(over="ignore"):
            want = u[r] if wr == 0 else (u[r].astype(np.float32) + (np.float32(2.0) * wr) * t[r].astype(np.float32)).astype(np.float16)
        assert eo.same_bits(out[r], want), r
    u32, t32 = u.astype(np.float32), np.nan_to_num(t.astype(np.float32), nan=1.0, posinf=2.0, neginf=-2.0)
    out32 = control.add_numpy(u32, t32, 0.5, w, nb)
    c32 = (np.float32(0.5) * w[np.arange(12) // (nb * p), np.arange(12) % p])[:, None]
    assert out32.dtype == np.float32 and eo.same_bits(out32, np.where(c32 == 0, u32, u32 + (c32 * t32).astype(np.float32)))
    tiny = control.add_numpy(u32, t32, 1e-45, w, nb)                                    # a subnormal scale: c is subnormal or 0, never an error
    assert np.isfinite(tiny).all()
    with pytest.raises(ValueError):
        control.add_numpy(u, t.astype(np.float32), 1.0, w, nb)
    with pytest.raises(ValueError):
        control.add_numpy(u, t, 1.0, w, 1)                                             # 4 batch rows at 1 per image: more than w's two images


# ---------------------------------------------------------------------------------------------------------------- 4. the interface
def test_public_signatures_are_what_they_were():
    from fie_amd.pipe import HipImg2ImgPipeline
    from src.pipeline import FastEditor
    for fn in (FastEditor.edit, FastEditor.edit_batch, FastEditor.edit_sweep, HipImg2ImgPipeline.__call__, HipImg2ImgPipeline.prepare,
               HipImg2ImgPipeline.prepare_batch, HipImg2ImgPipeline.prepare_sweep):
        new = ("control_weights", "control_layers", "control_steps", "control_in_mask", "layers", "steps", "in_mask")
        assert not any(name.startswith("ctl") or name in new for name in inspect.signature(fn).parameters), fn.__qualname__
    par = inspect.signature(FastEditor.__init__).parameters
    assert par["control_weights"].kind is inspect.Parameter.KEYWORD_ONLY and par["control_weights"].default is None
    assert list(inspect.signature(FastEditor.set_control_weights).parameters) == ["self", "layers", "steps", "in_mask"]
    assert HipImg2ImgPipeline.control_weights is None
    from fie_amd.nn import ControlNet
    assert list(inspect.signature(ControlNet.add_residuals).parameters) == ["self", "skips", "mid", "scale", "unet_skips", "unet_mid"]


def test_editor_setting(monkeypatch):
    from src.pipeline import FastEditor
    ed = FastEditor.__new__(FastEditor)
    assert ed.control_weights is None
    assert ed.set_control_weights(layers="prompt", in_mask=0.25) is None
    assert ed.control_weights == dict(layers=control.presets(10)["prompt"], steps=None, in_mask=0.25)
    for bad, name in ((dict(layers="x"), "layers"), (dict(steps=(1, 0)), "steps"), (dict(in_mask=2), "in_mask")):
        with pytest.raises(ValueError, match=name):
            ed.set_control_weights(**bad)
        assert ed.control_weights["in_mask"] == 0.25                                   # a refused value leaves the setting alone
    before = ed.set_control_weights(steps=(0, 0.5))
    assert before["in_mask"] == 0.25 and ed.control_weights == dict(layers=None, steps=(0.0, 0.5), in_mask=None)
    assert ed.set_control_weights(**before)["steps"] == (0.0, 0.5) and ed.control_weights == before      # what it returns sets it back

    class Pipe:
        control_weights = None
    ed.pipe = Pipe()
    ed.set_control_weights(in_mask=0)
    assert ed.pipe.control_weights == control.Setting(None, None, 0.0)
    assert ed.set_control_weights(layers=[1.0] * 10, steps=(0, 1), in_mask=1.0) is not None and ed.control_weights is None and ed.pipe.control_weights is None
    with pytest.raises(ValueError, match="in_mask"):
        FastEditor(model_name="tiny", device="cpu", control_weights=dict(in_mask=1.5))
    with pytest.raises(ValueError, match="control_weights"):
        FastEditor(model_name="tiny", device="cpu", control_weights="prompt")
    monkeypatch.setenv("FIE_CONTROL_WEIGHTS", "layers=prompt;steps=0-0.5")
    with pytest.raises(ValueError, match="FIE_CONTROL_WEIGHTS"):
        FastEditor(model_name="tiny", device="cpu")
    monkeypatch.setenv("FIE_CONTROL_WEIGHTS", "steps=0.5:0.25")
    with pytest.raises(ValueError, match="steps"):
        FastEditor(model_name="tiny", device="cpu")
    monkeypatch.setenv("FIE_CONTROL_WEIGHTS", "layers=prompt;steps=0:0.5;in_mask=0")
    with pytest.raises(RuntimeError, match="device"):                                  # the setting was fine: the CPU device is what is refused
        FastEditor(model_name="tiny", device="cpu")


def test_env_format():
    assert control.parse_env("layers=prompt;steps=0:0.5;in_mask=0") == dict(layers="prompt", steps=(0.0, 0.5), in_mask=0.0)
    assert control.parse_env(" in_mask = 0.25 ; ") == dict(in_mask=0.25)
    assert control.parse_env("layers=" + ",".join(["0.5"] * 10)) == dict(layers=[0.5] * 10)
    for bad in ("", ";", "layers", "layers=", "steps=0.5", "steps=a:b", "in_mask=x", "scale=1", "in_mask=0;in_mask=1", "layers=1,x"):
        with pytest.raises(ValueError, match="control weights"):
            control.parse_env(bad)


def test_command_line():
    import run_batch
    import run_single_image
    one = ["--image", "a.png", "--prompt", "a kite"]
    args = run_single_image.full_parser().parse_args(one)
    assert (args.control_layers, args.control_steps, args.control_in_mask) == (None, None, None) and run_single_image.control_keywords(args) == {}
    args = run_single_image.full_parser().parse_args(one + ["--control_layers", "guess", "--control_steps", "0:0.5", "--control_in_mask", "0"])
    assert run_single_image.control_keywords(args) == dict(layers="guess", steps=(0.0, 0.5), in_mask=0.0)
    for flags in (["--control_steps", "0.5"], ["--control_layers", "1,2"], ["--control_in_mask", "1.5"], ["--control_steps", "0.6:0.5"]):
        with pytest.raises(ValueError):
            run_single_image.control_keywords(run_single_image.full_parser().parse_args(one + flags))
    assert "--control_layers" not in run_single_image.build_parser().format_help()
    assert not any(f in run_batch.full_parser().format_help() for f in ("--control_layers", "--control_steps", "--control_in_mask"))
    assert "FIE_CONTROL_WEIGHTS" in run_batch.__doc__


def test_header_declares_and_library_exports_the_entries(lib):
    with open(os.path.join(ROOT, "include", "fie.h")) as fh:
        text = fh.read()
    c = hip.ctypes
    for name in ("fie_control_pyramid_u8", "fie_control_add"):
        assert re.search(rf"\b{name}\s*\(", text) and name in hip.SIGNATURES and hasattr(lib, name)
    assert hip.header.FUNCTIONS["fie_control_pyramid_u8"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_void_p])
    assert hip.header.FUNCTIONS["fie_control_add"] == (c.c_int, [c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int, c.c_int])
    assert hip.header.DEFINES["CONTROL_MAX_SEGMENTS"] == control.MAX_SEGMENTS == 16 and hip.header.DEFINES["CONTROL_MAX_LEVELS"] == control.MAX_LEVELS
    assert [n for n, _ in hip.ControlTable._fields_] == ["count", "C", "P", "woff", "rows", "s", "u", "t", "out"]
    assert list(inspect.signature(hip.Context.control_pyramid).parameters) == ["self", "e", "a", "binary", "levels", "out"]
    assert list(inspect.signature(hip.Context.control_add).parameters) == ["self", "segments", "w", "rows_per_image", "outs"]


def _table(**over):
    """A valid one-segment table on fake addresses (never dereferenced: the checks run before any launch), with `over` applied to segment 0."""
    tab = hip.ControlTable()
    tab.count = 1
    seg = dict(C=8, P=4, woff=0, rows=8, s=0.5, u=4096, t=8192, out=12288)
    seg.update(over)
    for k, v in seg.items():
        getattr(tab, k)[0] = v
    return tab


def test_entries_refuse_bad_arguments(lib):
    """Argument checks run before any launch: no GPU is touched (the context pointer is only compared with NULL)."""
    einval = hip.header.DEFINES["EINVAL"]
    c = hip.ctypes
    ctx, buf = c.c_void_p(16), 4096
    for e, h, w, levels, a, binary, out in ((0, 8, 8, 3, 0, 1, buf), (buf, 8, 8, 3, 0, 1, 0), (buf, 0, 8, 3, 0, 1, buf), (buf, 12, 8, 3, 0, 1, buf),
                                            (buf, 8, 20, 3, 0, 1, buf), (buf, 2056, 8, 3, 0, 1, buf), (buf, 8, 8, 0, 0, 1, buf), (buf, 8, 8, 4, 0, 1, buf),
                                            (buf, 8, 8, 3, -1, 1, buf), (buf, 8, 8, 3, 256, 1, buf), (buf, 8, 8, 3, 0, 2, buf), (buf + 4, 8, 8, 3, 0, 1, buf),
                                            (buf, 8, 8, 3, 0, 1, buf + 2)):
        assert lib.fie_control_pyramid_u8(ctx, e, h, w, levels, a, binary, out) == einval, (e, h, w, levels, a, binary, out)
        assert b"fie_control_pyramid_u8" in lib.fie_last_error()
    assert lib.fie_control_pyramid_u8(None, buf, 8, 8, 3, 0, 1, buf) == einval
    call = lambda tab, w=buf, p_tot=4, rpi=2, f32=0: lib.fie_control_add(ctx, c.byref(tab) if tab is not None else None, w, p_tot, rpi, f32)
    bad = [_table(u=0), _table(t=0), _table(out=0), _table(u=4104), _table(out=4096), _table(out=8192), _table(C=12), _table(C=0), _table(P=0),
           _table(rows=6), _table(rows=0), _table(woff=1), _table(woff=-1), _table(s=float("nan"))]
    none, many = _table(), _table()
    none.count, many.count = 0, 17
    for tab in bad + [none, many]:
        assert call(tab) == einval
        assert b"fie_control_add" in lib.fie_last_error()
    for kw in (dict(w=0), dict(w=buf + 2), dict(p_tot=0), dict(p_tot=3), dict(rpi=0), dict(f32=2)):
        assert call(_table(), **kw) == einval, kw
        assert b"fie_control_add" in lib.fie_last_error()
    assert call(None) == einval and lib.fie_control_add(None, c.byref(_table()), buf, 4, 2, 0) == einval


# ---------------------------------------------------------------------------------------------------------------- 5. the evaluation test's condition
@pytest.mark.parametrize("stack_name", ["tiny", "tiny-nomid"])
def test_weighted_oracle_differs_from_the_plain_one(stack_name):
    """tests/test_control_gpu.py bounds the fp32 context's weighted evaluation by 2x its plain error against the oracle (some 1e-5).  That test can
    only fail code which ignores the weights if the weighted oracle -- the ControlNet's residuals at scale 1 times 0.5 * layer_i * w on the host --
    is far from the plain scale-0.5 oracle: required > 1e-2 for in_mask = 0 with the hole, for "prompt", for "guess" and for no ControlNet at all.
    Measured here: tiny 7.6e-2 / 5.9e-2 / 6.7e-2 / 9.2e-2, tiny-nomid 6.7e-2 / 4.6e-2 / 5.2e-2 / 7.7e-2."""
    from fie_amd import stack
    cfgs, sds = stack.synthetic_stack(stack_name, True, device="cpu", dtype=torch.float32)
    x = eo.eval_inputs(cfgs)
    plain = eo.oracle_eval(sds, cfgs, x)
    assert eo.rel_err(co.oracle_eval(sds, cfgs, x), plain) < 1e-6                      # scale 1 times 0.5 on the host is the scale-0.5 oracle
    pre = control.presets(10)
    cases = {"in_mask=0": (None, co.eval_weights(0.0)), "prompt": ([0.5 * v for v in pre["prompt"]], None),
             "guess": ([0.5 * v for v in pre["guess"]], None), "no ControlNet": ([0.0] * 10, None)}
    for name, (scales, w) in cases.items():
        d = eo.rel_err(co.oracle_eval(sds, cfgs, x, scales, w), plain)
        print(f"{stack_name}: rel_err({name} oracle, plain oracle) = {d:.3e}")
        assert d > 1e-2, name
    assert eo.rel_err(co.oracle_eval(sds, cfgs, x, None, np.ones(336, np.float32)), plain) < 1e-6       # weights of 1 change nothing
