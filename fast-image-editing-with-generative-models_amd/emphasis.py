"""Prompt emphasis, host side: the marks of a prompt, the weight of every character, and the numpy restatement of the device op.

A mark gives its text a weight: `[text]` the editor's setting w (PIE-Bench writes its changed words this way), `(text:1.3)` the written number.
The tokenizers (fie_amd/tokenizer.py) turn the character weights into one weight per token; fie_kv_emphasis multiplies the V row of every
cross-attention by it -- Prompt-to-Prompt's re-weighting behind the softmax."""
import re

import numpy as np

W_MIN, W_MAX = 0.0, 8.0
MARK = re.compile(r"\[([^\[\]]*)\]|\(([^()\[\]]*):(\d+(?:\.\d+)?|\.\d+)\)")


def check(w):
    """The setting `prompt_emphasis`: None (off), or a number in [0, 8], returned as a float.  Anything else is a ValueError."""
    if w is None:
        return None
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not W_MIN <= float(w) <= W_MAX:
        raise ValueError(f"prompt_emphasis={w!r}: None, or a number in [{W_MIN:g}, {W_MAX:g}] (the weight of the words a prompt marks with [...])")
    return float(w)


def parse(prompt, w):
    """(stripped, weights): the prompt with every mark replaced by its text and nothing else changed, and the weight of each of its characters as
    f32 [len(stripped)].  Marks are the matches of MARK, left to right: `[text]` weighs `w`, `(text:number)` the number (above 8: a ValueError).
    A `[` or `]` left over behind the matches is a ValueError that quotes the prompt; parentheses in any other form are text."""
    w = check(w)
    if w is None:
        raise ValueError("parse: prompt_emphasis=None reads no marks")
    parts, weights, pos = [], [], 0
    for m in MARK.finditer(prompt):
        plain = prompt[pos:m.start()]
        if m.group(1) is not None:
            text, weight = m.group(1), w
        else:
            text, weight = m.group(2), float(m.group(3))
            if weight > W_MAX:
                raise ValueError(f"prompt emphasis: the weight {m.group(3)} of {m.group(0)!r} is above {W_MAX:g} in the prompt {prompt!r}")
        parts += [plain, text]
        weights += [1.0] * len(plain) + [weight] * len(text)
        pos = m.end()
    parts.append(prompt[pos:])
    weights += [1.0] * (len(prompt) - pos)
    stripped = "".join(parts)
    if "[" in stripped or "]" in stripped:
        raise ValueError(f"prompt emphasis: a '[' or ']' that belongs to no [...] mark (unbalanced, or nested) in the prompt {prompt!r}")
    return stripped, np.asarray(weights, np.float32)


def row_weights(weights):
    """Token weights f32 [rows, 77] of a job -> its `emph`, f32 [rows * 77], or None when every weight is 1: that job is the un-emphasised one."""
    weights = np.ascontiguousarray(weights, np.float32)
    return None if bool((weights == 1.0).all()) else weights.reshape(-1)


def v_flags(cs):
    """The per-8-column flag table of a K | V result whose blocks are c_0, c_1, ... wide: [K_0 | V_0 | K_1 | V_1 | ...], 1 over the V columns."""
    out = []
    for c in cs:
        if c % 8:
            raise ValueError(f"prompt emphasis: a cross-attention width of {c} is no multiple of 8")
        out += [0] * (c // 8) + [1] * (c // 8)
    return np.asarray(out, np.uint8)


def kv_emphasis_numpy(x, w, vflags):
    """fie_kv_emphasis restated: x [rows, ncols] float16 or float32, w float32 [rows], vflags u8 [ncols / 8] -> a copy of x with the flagged columns
    of every row with w != 1 replaced by dtype(f32(x) * w): one fp32 multiply and, for float16, numpy's round-to-nearest-even conversion."""
    x, w = np.asarray(x), np.asarray(w, np.float32)
    rows, ncols = x.shape
    if x.dtype not in (np.float16, np.float32) or w.shape != (rows,) or np.asarray(vflags).shape != (ncols // 8,) or ncols % 8:
        raise ValueError("kv_emphasis_numpy: x [rows, ncols] f16 / f32, w f32 [rows], vflags u8 [ncols / 8]")
    out = x.copy()
    r = np.flatnonzero(w != 1.0)
    c = np.flatnonzero(np.repeat(np.asarray(vflags) != 0, 8))
    if r.size and c.size:
        with np.errstate(over="ignore", invalid="ignore"):
            out[np.ix_(r, c)] = (x[np.ix_(r, c)].astype(np.float32) * w[r, None]).astype(x.dtype)
    return out
