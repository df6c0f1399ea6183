"""Prompt emphasis, host side (no GPU): the grammar on the 700 PIE-Bench prompts and on the cases that matter, the two tokenizers'
weighted entries, the range of the setting, identity (b) on the host, the numpy restatement, the C ABI's declaration, the public signatures -- and the
condition of the GPU evaluation test: the oracle with weighted `attn2.to_v` rows differs from the plain one by far more than any fp32 bound."""
import csv
import inspect
import os
import re

import numpy as np
import pytest
import torch

import fie_amd  # noqa: F401
from fie_amd import emphasis, hip
from fie_amd.tokenizer import BOS, EOS, MAXLEN, BpeTokenizer, StandInTokenizer

import emphasis_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
W = 1.5


@pytest.fixture(scope="module")
def prompts():
    with open(os.path.join(GOLD, "pie_bench_items.csv"), newline="") as fh:
        out = [row["editing_prompt"] for row in csv.DictReader(fh)]
    assert len(out) == 700
    return out


@pytest.fixture(scope="module")
def bpe():
    return BpeTokenizer(os.path.join(GOLD, "bpe_vocab.json"), os.path.join(GOLD, "bpe_merges.txt"), 0)


@pytest.fixture(scope="module")
def lib():
    hip.build()
    return hip.lib()


# ---------------------------------------------------------------------------------------------------------------- 1. the benchmark's prompts
def test_every_pie_bench_prompt_parses(prompts, bpe):
    stand = StandInTokenizer(0)
    marked = 0
    for p in prompts:
        stripped, cw = emphasis.parse(p, W)
        assert "[" not in stripped and "]" not in stripped and len(cw) == len(stripped) and cw.dtype == np.float32
        marks = re.findall(r"\[([^\[\]]*)\]", p)
        assert stripped == re.sub(r"\[([^\[\]]*)\]", r"\1", p) and "(" not in p
        marked += bool(marks)
        ids, w = stand.weighted([p], W)
        assert torch.equal(ids, stand([stripped])) and w.shape == (1, MAXLEN) and w.dtype == np.float32
        assert int((w == W).sum()) == sum(len(m.split()) for m in marks), p           # the words inside the marks, and only they
        assert set(np.unique(w)) <= {1.0, W} and w[0, 0] == 1.0
        ids_b, w_b = bpe.weighted([p], W)
        assert torch.equal(ids_b, bpe([stripped])), p                                  # the ids of the stripped text
        assert bool(marks) == bool((w_b != 1.0).any()) and w_b[0, 0] == 1.0
        n = int((ids_b[0] == bpe.eos).nonzero()[0, 0]) if bpe.eos != bpe.pad_id else None
        if n is not None:
            assert (w_b[0, n:] == 1.0).all()                                           # EOS and padding carry 1
    assert marked == 615


# ---------------------------------------------------------------------------------------------------------------- 2. the grammar
def test_grammar_cases():
    s, w = emphasis.parse("a [silver] cat [sculpture] sitting", 2.0)
    assert s == "a silver cat sculpture sitting"
    assert w.tolist() == [1, 1] + [2] * 6 + [1] * 5 + [2] * 9 + [1] * 8
    s, w = emphasis.parse("a (red hat:1.4) and (x:.5) and (y:2)", 3.0)
    assert s == "a red hat and x and y" and w.tolist() == [1, 1] + [np.float32(1.4)] * 7 + [1] * 5 + [0.5] + [1] * 5 + [2]
    for literal in ("a (x) b", "a (x:) b", "a (x:1.) b", "f(x): 1.4", "a (x:1.4", "(a (b):1.2)", "(x:-1)"):
        s, w = emphasis.parse(literal, 2.0)
        assert s == literal and (w == 1).all(), literal                               # parentheses in any other form are text
    assert emphasis.parse("(x:8)", 2.0)[1].tolist() == [8.0] and emphasis.parse("(x:8.0)", 0.0)[1].tolist() == [8.0]
    for bad in ("(x:9)", "a (dog:8.01) b", "(x:100)"):
        with pytest.raises(ValueError, match="above 8"):
            emphasis.parse(bad, 2.0)
    for bad in ("a dog] b", "a [dog b", "[[a]]", "[a [b] c]", "]a[", "([a:1.2)"):
        with pytest.raises(ValueError) as e:
            emphasis.parse(bad, 2.0)
        assert repr(bad) in str(e.value), bad                                          # the error quotes the prompt
    assert emphasis.parse("a [] b", 2.0)[0] == "a  b" and (emphasis.parse("a [] b", 2.0)[1] == 1).all()      # an empty mark: stripped, nothing weighted
    assert emphasis.parse("a (:1.3) b", 2.0)[0] == "a  b"
    s, w = emphasis.parse("([a]:1.2)", 2.0)                                            # brackets inside parentheses: the bracket is the mark
    assert s == "(a:1.2)" and w.tolist() == [1, 2, 1, 1, 1, 1, 1]
    assert emphasis.parse("", 2.0)[0] == "" and emphasis.parse("", 2.0)[1].shape == (0,)
    with pytest.raises(ValueError, match="None"):
        emphasis.parse("a [b]", None)


def test_a_mark_next_to_punctuation(bpe):
    stand = StandInTokenizer(0)
    ids, w = stand.weighted(["a [dog], running"], 2.0)
    assert torch.equal(ids, stand(["a dog, running"])) and w[0, :5].tolist() == [1, 1, 2, 1, 1]        # the word "dog," starts inside the mark
    ids, w = bpe.weighted(["a [dog], running"], 2.0)
    assert torch.equal(ids, bpe(["a dog, running"]))
    pieces = [m.group(0) for m in bpe.pat.finditer("a dog, running")]
    assert pieces == ["a", "dog", ",", "running"]
    counts = [len(bpe._bpe("".join(bpe.b2u[b] for b in p.encode()))) for p in pieces]
    want = [1.0] + [1.0] * counts[0] + [2.0] * counts[1] + [1.0] * counts[2] + [1.0] * counts[3] + [1.0]
    assert w[0, :len(want)].tolist() == want and (w[0, len(want):] == 1).all()       # the comma is its own piece and starts outside the mark


def test_normalisation_comes_first(bpe):
    """Lower-casing can change a string's length: the marks are found in the normalised text, so the offsets fit."""
    stand = StandInTokenizer(0)
    p = "İstanbul   [Big\tDOG]  (Cat:1.5)"                                        # U+0130 lower-cases to two code points
    for tok in (stand, bpe):
        ids, w = tok.weighted([p], 2.0)
        assert torch.equal(ids, tok(["İstanbul big dog cat"]))
    ids, w = stand.weighted([p], 2.0)
    assert w[0, :6].tolist() == [1, 1, 2, 2, 1.5, 1]
    assert torch.equal(stand.weighted("a [b]", 2.0)[0], stand("a b"))                  # a bare string, as __call__ takes it


def test_truncation_past_77(bpe):
    stand = StandInTokenizer(0)
    p = " ".join(f"w{i}" for i in range(70)) + " [" + " ".join(f"m{i}" for i in range(20)) + "]"
    ids, w = stand.weighted([p], 2.0)
    assert torch.equal(ids, stand([p.replace("[", "").replace("]", "")])) and ids[0, -1] == EOS and ids[0, 0] == BOS
    assert w[0].tolist() == [1.0] * 71 + [2.0] * 5 + [1.0]                             # 75 words survive; EOS carries 1
    ids, w = bpe.weighted([p], 2.0)
    assert torch.equal(ids, bpe([p.replace("[", "").replace("]", "")])) and ids[0, -1] == bpe.eos and w[0, -1] == 1.0 and w.shape == (1, MAXLEN)


def test_call_does_not_read_marks(bpe):
    stand = StandInTokenizer(0)
    assert not torch.equal(stand(["a [b] c"]), stand(["a b c"])) and not torch.equal(bpe(["a [b] c"]), bpe(["a b c"]))


# ---------------------------------------------------------------------------------------------------------------- 3. the setting
def test_range_of_the_setting():
    assert emphasis.check(None) is None and emphasis.check(0) == 0.0 and emphasis.check(8) == 8.0 and emphasis.check(1.3) == 1.3
    assert isinstance(emphasis.check(2), float)
    for bad in (-0.01, 8.01, float("nan"), float("inf"), True, "2", [2.0]):
        with pytest.raises(ValueError, match="prompt_emphasis"):
            emphasis.check(bad)
        with pytest.raises(ValueError, match="prompt_emphasis"):
            emphasis.parse("a [b]", bad)


def test_editor_setting(monkeypatch):
    from src.pipeline import FastEditor
    ed = FastEditor.__new__(FastEditor)
    assert ed.prompt_emphasis is None
    assert ed.set_prompt_emphasis(1.3) is None and ed.prompt_emphasis == 1.3
    for bad in (9, -1, "x", True):
        with pytest.raises(ValueError, match="prompt_emphasis"):
            ed.set_prompt_emphasis(bad)
        assert ed.prompt_emphasis == 1.3                                               # a refused value leaves the setting alone
    assert ed.set_prompt_emphasis(None) == 1.3 and ed.prompt_emphasis is None

    class Pipe:
        prompt_emphasis = None
    ed.pipe = Pipe()
    ed.set_prompt_emphasis(2)
    assert ed.pipe.prompt_emphasis == 2.0 and isinstance(ed.pipe.prompt_emphasis, float)        # the pipeline object carries the same attribute
    ed.set_prompt_emphasis(None)
    assert ed.pipe.prompt_emphasis is None
    with pytest.raises(ValueError, match="prompt_emphasis"):
        FastEditor(model_name="tiny", device="cpu", prompt_emphasis=8.5)
    monkeypatch.setenv("FIE_PROMPT_EMPHASIS", "strong")
    with pytest.raises(ValueError, match="FIE_PROMPT_EMPHASIS"):
        FastEditor(model_name="tiny", device="cpu")
    monkeypatch.setenv("FIE_PROMPT_EMPHASIS", "9")
    with pytest.raises(ValueError, match="prompt_emphasis"):
        FastEditor(model_name="tiny", device="cpu")
    monkeypatch.setenv("FIE_PROMPT_EMPHASIS", "1.5")
    with pytest.raises(RuntimeError, match="device"):                                  # the setting was fine: the CPU device is what is refused
        FastEditor(model_name="tiny", device="cpu")
    from fie_amd.pipe import HipImg2ImgPipeline
    assert HipImg2ImgPipeline.prompt_emphasis is None


def test_command_line():
    import run_batch
    import run_single_image
    one = ["--image", "a.png", "--prompt", "a [red] kite"]
    assert run_single_image.full_parser().parse_args(one).prompt_emphasis is None
    assert run_single_image.full_parser().parse_args(one + ["--prompt_emphasis", "1.3"]).prompt_emphasis == 1.3
    assert "--prompt_emphasis" not in run_single_image.build_parser().format_help()
    assert "--prompt_emphasis" not in run_batch.full_parser().format_help() and "FIE_PROMPT_EMPHASIS" in run_batch.__doc__


# ---------------------------------------------------------------------------------------------------------------- 4. identity (b), host side
def test_weight_one_is_the_stripped_prompt(bpe):
    for tok in (StandInTokenizer(0), bpe):
        ids, w = tok.weighted(["a [silver] cat", "[x] (y:1.0) (z:1)"], 1.0)
        assert torch.equal(ids, tok(["a silver cat", "x y z"])) and (w == 1.0).all()
        assert emphasis.row_weights(w) is None                                         # no `emph`: the job is the stripped prompt's
        ids, w = tok.weighted(["a silver cat"], 2.0)                                  # no marks
        assert torch.equal(ids, tok(["a silver cat"])) and emphasis.row_weights(w) is None
        ids, w = tok.weighted(["a [silver] cat", ""], 2.0)
        e = emphasis.row_weights(w)
        assert e.shape == (2 * MAXLEN,) and e.dtype == np.float32 and e[2] == 2.0 and (np.delete(e, 2) == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------- 5. the restatement
def test_restatement():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 48)).astype(np.float16)
    x[1, 24] = np.float16(65504.0)
    x[1, 25] = np.float16(6e-8)                                                        # the smallest f16 subnormal
    x[3, 30] = np.float16(-65504.0)
    flags = emphasis.v_flags([16, 8])                                                  # [K 16 | V 16 | K 8 | V 8]
    assert flags.tolist() == [0, 0, 1, 1, 0, 1] and flags.dtype == np.uint8
    w = np.array([1.0, 8.0, 0.5, 0.0, 1.3], np.float32)
    y = emphasis.kv_emphasis_numpy(x, w, flags)
    vcols = np.r_[16:32, 40:48]
    kcols = np.r_[0:16, 32:40]
    assert y.dtype == np.float16 and eo.same_bits(y[:, kcols], x[:, kcols]) and eo.same_bits(y[0], x[0])
    assert np.isinf(y[1, 24]) and y[1, 25] == np.float16(8 * float(np.float16(6e-8)))
    with np.errstate(over="ignore"):
        for r in range(1, 5):
            for c in vcols:
                assert y[r, c] == np.float16(np.float32(x[r, c]) * w[r]) or (np.isinf(y[r, c]) and r == 1)
    assert (y[3, vcols] == 0).all() and np.signbit(y[3, 30])                          # 0 * -65504 is -0
    x32 = x.astype(np.float32)
    y32 = emphasis.kv_emphasis_numpy(x32, w, flags)
    assert y32.dtype == np.float32 and eo.same_bits(y32[:, vcols], x32[:, vcols] * w[:, None]) and eo.same_bits(y32[:, kcols], x32[:, kcols])
    with pytest.raises(ValueError):
        emphasis.v_flags([12])
    with pytest.raises(ValueError):
        emphasis.kv_emphasis_numpy(x, w[:4], flags)


# ---------------------------------------------------------------------------------------------------------------- 6. the ABI
def test_header_declares_and_library_exports_the_entry(lib):
    with open(os.path.join(ROOT, "include", "fie.h")) as fh:
        text = fh.read()
    assert re.search(r"\bfie_kv_emphasis\s*\(", text)
    assert "fie_kv_emphasis" in hip.SIGNATURES and hasattr(lib, "fie_kv_emphasis")
    ret, args = hip.header.FUNCTIONS["fie_kv_emphasis"]
    c = hip.ctypes
    assert ret is c.c_int and args == [c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p, c.c_int]
    assert list(inspect.signature(hip.Context.kv_emphasis).parameters) == ["self", "x", "w", "vflags"]


def test_entry_refuses_bad_arguments(lib):
    """Argument checks run before any launch: no GPU is touched (the context pointer is only compared with NULL)."""
    einval = hip.header.DEFINES["EINVAL"]
    ctx = hip.ctypes.c_void_p(16)
    buf = 4096                                                                         # 16-byte aligned fake addresses: never dereferenced
    for x, ld, rows, ncols, w, fl, f32 in ((0, 8, 1, 8, buf, buf, 0), (buf, 8, 1, 8, 0, buf, 0), (buf, 8, 1, 8, buf, 0, 0), (buf, 8, 0, 8, buf, buf, 0),
                                           (buf, 12, 1, 8, buf, buf, 0), (buf, 16, 1, 12, buf, buf, 0), (buf, 8, 1, 16, buf, buf, 0),
                                           (buf + 8, 8, 1, 8, buf, buf, 0), (buf, 8, 1, 8, buf, buf, 2), (buf, 8, 1, 0, buf, buf, 1)):
        assert lib.fie_kv_emphasis(ctx, x, ld, rows, ncols, w, fl, f32) == einval, (x, ld, rows, ncols, w, fl, f32)
        assert b"fie_kv_emphasis" in lib.fie_last_error()
    assert lib.fie_kv_emphasis(None, buf, 8, 1, 8, buf, buf, 0) == einval


def test_public_signatures_are_what_they_were():
    """The prompt carries the marks and a setting switches the reading on: no call gained a keyword (tests/test_mask_spec_cpu.py pins them all)."""
    from fie_amd.pipe import HipImg2ImgPipeline
    from src.pipeline import FastEditor
    for fn in (FastEditor.edit, FastEditor.edit_batch, FastEditor.edit_sweep, HipImg2ImgPipeline.__call__, HipImg2ImgPipeline.prepare,
               HipImg2ImgPipeline.prepare_batch, HipImg2ImgPipeline.prepare_sweep):
        assert not any("emph" in name for name in inspect.signature(fn).parameters), fn.__qualname__
    assert "prompt_emphasis" in inspect.signature(FastEditor.__init__).parameters
    assert inspect.signature(FastEditor.__init__).parameters["prompt_emphasis"].kind is inspect.Parameter.KEYWORD_ONLY


# ---------------------------------------------------------------------------------------------------------------- 7. the evaluation test's condition
@pytest.mark.parametrize("stack_name", ["tiny", "tiny-nomid"])
def test_weighted_oracle_differs_from_the_plain_one(stack_name):
    """tests/test_emphasis_gpu.py bounds the fp32 context's emphasised evaluation by 2x its plain error against the oracle (some 1e-5).  That
    test can only fail code which ignores the weights if the two oracles are far apart: measured here 1e-2 on both stacks; required 1e-3, a
    hundred times any fp32 bound."""
    from fie_amd import stack
    cfgs, sds = stack.synthetic_stack(stack_name, True, device="cpu", dtype=torch.float32)
    x = eo.eval_inputs(cfgs)
    plain = eo.oracle_eval(sds, cfgs, x)
    weighted = eo.oracle_eval(sds, cfgs, x, eo.eval_weights())
    d = eo.rel_err(weighted, plain)
    print(f"{stack_name}: rel_err(weighted oracle, plain oracle) = {d:.3e}")
    assert d > 1e-3
    assert eo.rel_err(eo.oracle_eval(sds, cfgs, x, np.ones((2, 77), np.float32)), plain) == 0.0       # the wrap itself changes nothing
