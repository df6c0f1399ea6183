"""Guard bands and NaN moats: does an op stay inside its operands?

The hot path addresses memory through raw buffer descriptors: rows past M, K tails, im2col padding and halo pixels are not masked but sent
out of range, so an extent that is a few bytes too long reads a neighbour (and multiplies it by a zero weight) or writes into allocator
slack, and no test on contiguous, exact-size tensors can tell.  The helpers here put every operand INSIDE one larger allocation:

  moat(t)            a view equal to t with `rows` rows of moat before and after it and (2-D tensors) `gap` columns between its rows,
                     every element outside the view set to `fill`
  guarded(shape)     an output view in an arena of a fixed byte pattern + a Guard whose check() compares the bytes outside the view
  isolated(fn, ...)  runs fn twice on the same operand values -- input moats NaN, then large and finite; the output prefilled differently -- and
                     asserts that the two outputs are bit-equal and finite and both guards intact

Bit-equality under different moats: no value from outside an operand reached the result (NaN * 0 is NaN: a stray read that zero padding would
hide shows).  Bit-equality under different prefills: every output element was written.  Device-agnostic (CPU and CUDA tensors); everything
stays inside torch allocations, a miss of up to `rows` rows or `gap` columns lands in a moat.
"""
import math

import torch

E4M3 = torch.float8_e4m3fn           # e4m3 operands travel as this dtype (their moat NaN is the byte 0x7f; plain uint8 = image bytes, 0xff)
ROWS, GAP = 256, 64                   # a whole tile of rows / a whole K-step of columns


def _bytes(t):
    """The storage of a CONTIGUOUS tensor as uint8."""
    return t.view(torch.uint8) if t.dtype != torch.uint8 else t


def _bits(t):
    """A tensor as integers of its element size: equality of these is equality of bits (NaN == NaN, -0 != 0)."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _align(dtype):
    """Elements per 16 bytes: the row-stride granule the ops demand (f16: 8 elements, e4m3 / u8: 16 bytes, f32: 4)."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def nan_fill(dtype):
    return {torch.float16: float("nan"), torch.float32: float("nan"), E4M3: 0x7f, torch.uint8: 0xff}[dtype]


def finite_fill(dtype):
    return {torch.float16: 1000.0, torch.float32: 1000.0, E4M3: 0x00, torch.uint8: 0x00}[dtype]


def _fill(arena, fill):
    """Every element of the 1-D arena = fill.  Float NaN is written as the canonical quiet NaN (f16 0x7e00, f32 0x7fc00000); e4m3 as a byte."""
    if arena.dtype == E4M3 or arena.dtype == torch.uint8:
        _bytes(arena).fill_(int(fill))
    elif isinstance(fill, float) and math.isnan(fill):
        if arena.dtype == torch.float16:
            arena.view(torch.int16).fill_(0x7e00)
        else:
            arena.view(torch.int32).fill_(0x7fc00000)
    else:
        arena.fill_(fill)


def _layout(shape, dtype, rows, gap, ld, flat):
    """(ld, lead, total) in elements of the arena around a view of `shape`: 2-D views (or any with `ld`) get `rows` rows of `ld` elements before
    and after and ld - cols between their rows; flat ones (`flat`, or not 2-D without ld) `rows` rows of their last dimension, rounded to 16 bytes."""
    al = _align(dtype)
    cols = shape[-1] if len(shape) else 1
    nrows = math.prod(shape[:-1]) if len(shape) > 1 else 1
    if flat or (len(shape) != 2 and ld is None):
        lead = (rows * max(cols, 1) + al - 1) // al * al
        return None, lead, 2 * lead + max(math.prod(shape), 1)
    if ld is None:
        ld = (cols + gap + al - 1) // al * al
    assert ld >= cols and (rows * ld) % al == 0, f"ld={ld}: rows overlap, or the view would not start on a 16-byte boundary"      # an explicit ld is the caller's (the ABI takes ldc % 4)
    return ld, rows * ld, (2 * rows + nrows) * ld


def _view(arena, shape, ld, lead):
    if ld is None:
        return arena[lead:lead + max(math.prod(shape), 1)].view(shape)
    strides, s = [], ld
    for n in reversed(shape[:-1]):
        strides.insert(0, s)
        s *= n
    return torch.as_strided(arena, tuple(shape), tuple(strides) + (1,), lead)


def moat(t, rows=ROWS, gap=GAP, fill=None, flat=False):
    """A view equal to t (shape, values, last dimension contiguous) inside one larger allocation, everything outside it = `fill` (default: the
    dtype's NaN).  2-D: row stride cols + gap (gap rounded up to keep 16-byte rows) and `rows` full rows before and after.  `flat`, or not 2-D:
    the tensor stays contiguous (what the ABI demands of NHWC conv and GroupNorm inputs) with the leading and trailing moat only."""
    fill = nan_fill(t.dtype) if fill is None else fill
    ld, lead, total = _layout(tuple(t.shape), t.dtype, rows, gap, None, flat)
    arena = torch.empty(total, dtype=t.dtype, device=t.device)
    _fill(arena, fill)
    v = _view(arena, tuple(t.shape), ld, lead)
    if t.dtype == E4M3:
        v.view(torch.uint8).copy_(t.view(torch.uint8))
    else:
        v.copy_(t)
    return v


class GuardError(AssertionError):
    pass


class Guard:
    """The arena around a guarded() view: check() raises GuardError naming the first byte outside the view that no longer holds the pattern,
    as (row, col) relative to the view (row < 0 / >= rows: the moat before / after; col >= cols: the gap behind a row)."""

    def __init__(self, arena, expected, outside, shape, ld, lead):
        self.arena, self.expected, self.outside, self.shape, self.ld, self.lead = arena, expected, outside, shape, ld, lead

    def position(self, elem):
        """Arena element index -> (row, col) relative to the view."""
        cols = self.shape[-1] if len(self.shape) else 1
        ld = self.ld or max(cols, 1)
        rel = elem - self.lead
        return rel // ld, rel % ld

    def check(self, what="output"):
        touched = (_bytes(self.arena) != self.expected) & self.outside
        if bool(touched.any()):
            esz = self.arena.element_size()
            first = int(touched.nonzero()[0, 0])
            n = int(touched.sum())
            row, col = self.position(first // esz)
            raise GuardError(f"{what}: {n} byte(s) outside the view were written, the first at (row {row}, col {col}) of a view of shape "
                             f"{tuple(self.shape)}, row stride {self.ld}")


def guarded(shape, ld=None, dtype=torch.float16, device="cpu", rows=ROWS, gap=GAP, flat=False):
    """(view, guard): an uninitialised output view of `shape` (row stride `ld` elements between its rows, all leading dimensions folded into rows; flat: contiguous)
    in an arena that holds a fixed non-NaN byte pattern around and between the view's rows.  dtype E4M3: the view is uint8 (what the ops take)."""
    shape = tuple(shape)
    store = torch.uint8 if dtype == E4M3 else dtype
    ld, lead, total = _layout(shape, store, rows, gap, ld, flat)
    arena = torch.empty(total, dtype=store, device=device)
    nbytes = total * arena.element_size()
    # bytes 0x40 .. 0x6f by position: no f16 / f32 / e4m3 built from them is a NaN or an Inf, and neighbours differ
    pattern = (torch.arange(nbytes, device=device, dtype=torch.int64) % 0x30 + 0x40).to(torch.uint8)
    _bytes(arena).copy_(pattern)
    view = _view(arena, shape, ld, lead)
    outside = torch.ones(total, dtype=torch.bool, device=device)
    _view(outside, shape, ld, lead).fill_(False)
    outside = outside.repeat_interleave(arena.element_size()) if arena.element_size() > 1 else outside
    return view, Guard(arena, pattern, outside, shape, ld, lead)


class keep:
    """Marks an input isolated() hands to fn as it is (packed weights, workspaces: formats with no row stride to widen)."""

    def __init__(self, value):
        self.value = value


class flat:
    """Marks an input the ABI wants contiguous: leading and trailing moat only."""

    def __init__(self, value):
        self.value = value


class wide:
    """Marks a 2-D input whose rows get `gap` columns of moat (instead of the default) -- independent strides for q, k, v."""

    def __init__(self, value, gap):
        self.value, self.gap = value, gap


_PREFILL = {torch.float16: (1234.0, -4321.0), torch.float32: (1234.0, -4321.0), torch.uint8: (0x11, 0x26)}


def _finite(t, dtype):
    if dtype == E4M3:
        return (t & 0x7f) != 0x7f
    if dtype == torch.uint8:
        return torch.ones_like(t, dtype=torch.bool)
    return torch.isfinite(t)


def _first(mask, shape):
    """(row, col) of the first set element of a mask of `shape` (leading dimensions folded into the row)."""
    cols = shape[-1] if len(shape) else 1
    i = int(mask.reshape(-1).nonzero()[0, 0])
    return i // max(cols, 1), i % max(cols, 1)


def isolated(fn, inputs, out_spec, device=None):
    """Runs fn(inputs, out) twice and returns the output (a contiguous copy; a list for a list of specs).

    inputs: dict name -> tensor (moated: 2-D strided, others flat), flat(t), wide(t, gap), keep(x) or a non-tensor (passed through).
    out_spec: dict(shape=, ld=None, dtype=torch.float16, flat=False), or a list of them (fn then gets a list).  The same operand values both
    times; run 1: every input moat NaN (f16 0x7e00, f32 NaN, e4m3 0x7f, u8 0xff), run 2: 1000.0 / 0x00; the output view prefilled with a
    different pattern each time.  Asserts: outputs bit-equal, both finite, both guards intact -- each failure names the (row, col)."""
    specs = out_spec if isinstance(out_spec, (list, tuple)) else [out_spec]
    if device is None:
        device = next((v.value if isinstance(v, (flat, wide, keep)) else v).device for v in inputs.values()
                      if torch.is_tensor(v.value if isinstance(v, (flat, wide, keep)) else v))
    results = []
    for run, fill_of in enumerate((nan_fill, finite_fill)):
        ins = {}
        for name, v in inputs.items():
            if isinstance(v, keep):
                ins[name] = v.value
            elif isinstance(v, flat):
                ins[name] = moat(v.value, fill=fill_of(v.value.dtype), flat=True)
            elif isinstance(v, wide):
                ins[name] = moat(v.value, gap=v.gap, fill=fill_of(v.value.dtype))
            elif torch.is_tensor(v):
                ins[name] = moat(v, fill=fill_of(v.dtype)) if v.dtype in (torch.float16, torch.float32, torch.uint8, E4M3) else v
            else:
                ins[name] = v
        outs, guards = [], []
        for s in specs:
            dtype = s.get("dtype", torch.float16)
            view, guard = guarded(s["shape"], ld=s.get("ld"), dtype=dtype, device=device, flat=s.get("flat", False))
            view.fill_(_PREFILL[view.dtype][run])
            outs.append(view)
            guards.append(guard)
        fn(ins, outs if isinstance(out_spec, (list, tuple)) else outs[0])
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        for i, g in enumerate(guards):
            g.check(f"output {i}, run {run + 1} ({'NaN' if run == 0 else 'finite'} moats)")
        results.append([o.clone().contiguous() for o in outs])
    for i, s in enumerate(specs):
        a, b = results[0][i], results[1][i]
        dtype = s.get("dtype", torch.float16)
        shape = tuple(s["shape"])
        differ = _bits(a).ne(_bits(b))
        if bool(differ.any()):
            r, c = _first(differ, shape)
            raise AssertionError(f"output {i}: the runs with NaN and with finite moats differ in {int(differ.sum())} element(s), the first at (row {r}, col {c}): "
                                 f"{a.reshape(-1, shape[-1])[r, c].item()} vs {b.reshape(-1, shape[-1])[r, c].item()} -- a value from outside the operands "
                                 f"reached it, or it was never written (prefills {_PREFILL[a.dtype]})")
        bad = ~_finite(a, dtype)
        if bool(bad.any()):
            r, c = _first(bad, shape)
            raise AssertionError(f"output {i}: {int(bad.sum())} non-finite element(s), the first at (row {r}, col {c})")
    first = results[0]
    return first if isinstance(out_spec, (list, tuple)) else first[0]
