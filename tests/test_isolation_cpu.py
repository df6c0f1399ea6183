"""The isolation harness (tests/isolation.py) proved on fake ops written in torch: a correct strided matmul passes, and every planted
defect -- a stray store, a stray load that zero weights would hide, an element never written -- fails with the position in the message."""
import re

import pytest
import torch

import isolation as iso
from isolation import isolated, guarded, moat

M, N, K = 37, 24, 40


def operands(seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    return a, w


def beyond(t, rows=0, cols=0, row0=0):
    """The view t widened over its own storage: `rows` more rows behind it, `cols` more columns per row, starting `row0` rows earlier -- the
    addressing slip of a kernel whose extent is too long (legal here: the moat is part of the same allocation)."""
    ld = t.stride(0)
    return torch.as_strided(t, (t.shape[0] + rows - row0, t.shape[1] + cols), (ld, 1), t.storage_offset() + row0 * ld)


def matmul(ins, out):
    out.copy_((ins["a"].float() @ ins["w"].float().T).half())


SPEC = dict(shape=(M, N), ld=N + 8)


def run(fn, spec=SPEC):
    a, w = operands()
    return isolated(fn, {"a": a, "w": w}, spec)


def test_moat_is_a_view_equal_to_its_tensor_inside_one_allocation():
    a, _ = operands()
    v = moat(a)
    assert torch.equal(v, a) and v.stride() == (K + 64, 1) and v.storage_offset() == 256 * (K + 64)
    arena = torch.as_strided(v, (M + 512, K + 64), (K + 64, 1), 0)
    assert arena.isnan().sum() == arena.numel() - M * K                    # everything outside the view is the fill
    assert (arena.view(torch.int16)[0, 0] & 0xffff) == 0x7e00
    assert moat(a, gap=3).stride(0) == 48                                   # rounded up to 8 f16 elements
    b = moat(a.view(torch.uint8).view(iso.E4M3), fill=0x7f)
    assert b.stride(0) % 16 == 0 and b.stride(0) >= 2 * K + 64 and torch.equal(b.view(torch.uint8), a.view(torch.uint8))
    x = torch.arange(2 * 3 * 5 * 8, dtype=torch.float32).view(2, 3, 5, 8)
    f = moat(x, fill=1000.0)
    assert f.is_contiguous() and torch.equal(f, x) and f.storage_offset() == 256 * 8
    flat2d = moat(a, flat=True)
    assert flat2d.is_contiguous() and torch.equal(flat2d, a)
    assert moat(x.to(torch.uint8)).is_contiguous()


def test_guard_reports_the_first_touched_position():
    view, guard = guarded((5, 16), ld=24, dtype=torch.float16)
    guard.check()
    view.fill_(3.0)
    guard.check()                                                           # the view itself is the op's to write
    beyond(view, cols=1)[2, 16] = 1.0
    beyond(view, cols=8)[4, 20] = 1.0
    with pytest.raises(iso.GuardError, match=r"first at \(row 2, col 16\)"):
        guard.check()
    view, guard = guarded((2, 3, 8), ld=16, dtype=iso.E4M3)                 # leading dimensions fold into rows; e4m3 views are bytes
    assert view.dtype == torch.uint8 and view.stride() == (48, 16, 1)
    torch.as_strided(view, (7, 8), (16, 1), view.storage_offset())[6, 0] = 1
    with pytest.raises(iso.GuardError, match=r"\(row 6, col 0\)"):
        guard.check()
    view, guard = guarded((4, 4), dtype=torch.float32, flat=True)
    assert view.is_contiguous()
    torch.as_strided(view, (1,), (1,), view.storage_offset() - 1)[0] = 0.0
    with pytest.raises(iso.GuardError, match=r"\(row -1, col 3\)"):
        guard.check()


def test_a_correct_strided_matmul_passes():
    a, w = operands()
    out = run(matmul)
    assert out.is_contiguous() and torch.equal(out, (a.float() @ w.float().T).half())
    # several outputs, a contiguous input, a pass-through one and a byte output
    def two(ins, outs):
        assert ins["a"].is_contiguous() and ins["w"] is w and ins["n"] == 3
        outs[0].copy_((ins["a"].float() @ ins["w"].float().T).half())
        outs[1].copy_(ins["a"][:, :16].abs().clamp(0, 100).to(torch.uint8))
    o = isolated(two, {"a": iso.flat(a), "w": iso.keep(w), "n": 3}, [SPEC, dict(shape=(M, 16), ld=32, dtype=torch.uint8)])
    assert torch.equal(o[0], out) and o[1].dtype == torch.uint8


def fails_at(fn, row, col, spec=SPEC):
    with pytest.raises(AssertionError) as e:
        run(fn, spec)
    assert re.search(rf"\(row {row}, col {col}\)", str(e.value)), str(e.value)
    return str(e.value)


def test_a_write_one_element_past_a_rows_end_is_caught():
    def op(ins, out):
        matmul(ins, out)
        beyond(out, cols=1)[11, N] = 0.5
    assert "outside the view" in fails_at(op, 11, N)


def test_a_write_of_row_m_is_caught():
    def op(ins, out):
        matmul(ins, out)
        beyond(out, rows=1)[M, :4] = 0.5
    assert "outside the view" in fails_at(op, M, 0)


def test_a_write_before_row_0_is_caught():
    def op(ins, out):
        matmul(ins, out)
        beyond(out, row0=-1)[0, 5] = 0.5
    assert "outside the view" in fails_at(op, -1, 5)


def test_a_sum_that_includes_column_k_of_the_gap_is_caught():
    """The stray column meets a ZERO weight: the value is right with any finite neighbour, and only the NaN moat shows the read."""
    def op(ins, out):
        a = beyond(ins["a"], cols=1).float()                                            # columns 0 .. K of every row
        w = torch.cat([ins["w"].float(), torch.zeros(N, 1)], 1)                         # the packed weight's zero padding
        out.copy_((a @ w.T).half())
    assert "differ" in fails_at(op, 0, 0)


def test_a_reduction_that_includes_row_m_is_caught():
    def op(ins, out):
        out.copy_(beyond(ins["a"], rows=1).float().abs().amax(0, keepdim=True).half())
    assert "differ" in fails_at(op, 0, 0, dict(shape=(1, K), ld=K + 8))
    def good(ins, out):
        out.copy_(ins["a"].float().abs().amax(0, keepdim=True).half())
    run(good, dict(shape=(1, K), ld=K + 8))


def test_one_output_element_left_unwritten_is_caught():
    def op(ins, out):
        ref = (ins["a"].float() @ ins["w"].float().T).half()
        hole = torch.zeros(M, N, dtype=torch.bool)
        hole[M - 1, N - 1] = True
        out.copy_(torch.where(hole, out, ref))
    assert "never written" in fails_at(op, M - 1, N - 1)


def test_a_nan_the_op_makes_itself_is_caught():
    def op(ins, out):
        matmul(ins, out)
        out[3, 7] = float("inf")
    assert "non-finite" in fails_at(op, 3, 7)
