"""Host side of strength sweeps without a GPU: fie_amd/sweep.py (the variants of a list of strengths, the ragged
schedule, the selector's rule restated), the argument errors of FastEditor.edit_sweep in front of any device work, the command-line flags and
run_batch's --auto_strength loop through a stub editor."""
import itertools
import math
import threading

import numpy as np
import pytest
from PIL import Image

import fie_amd  # noqa: F401
from fie_amd import sweep
from fie_amd.lcm import LCMSchedule
from sweep_cases import INF, NAN, TABLE, _clip, _rows


# ---------------------------------------------------------------------------------------------------------------- variants
def test_variants_merge_strengths_with_one_step_count():
    vs = sweep.variants(4, [0.5, 0.6, 0.8, 1.0])
    assert [m for m, _ in vs] == [4, 3, 2]
    assert vs == [(4, [1.0]), (3, [0.8]), (2, [0.5, 0.6])]
    assert sweep.variants(4, (0.6, 1.0, 0.5)) == [(4, [1.0]), (2, [0.6, 0.5])]          # the requested order is kept inside a variant
    assert sweep.variants(4, [0.25]) == [(1, [0.25])]


@pytest.mark.parametrize("n", range(1, 17))
def test_variants_all_is_every_step_count_and_its_strengths_plan_that_many_steps(n):
    sched = LCMSchedule()
    vs = sweep.variants(n, "all")
    assert [m for m, _ in vs] == list(range(n, 0, -1))
    for m, (s,) in vs:
        assert 0.0 < s <= 1.0 and int(n * s) == m and len(sched.plan(n, s)) == m
    assert vs[0][1] == [1.0]


def test_variants_errors():
    with pytest.raises(ValueError, match="number of pipeline steps is 0"):
        sweep.variants(4, [0.8, 0.2])                        # int(4 * 0.2) == 0: the message edit() raises
    with pytest.raises(ValueError, match="at most 16"):
        sweep.variants(17, "all")
    with pytest.raises(ValueError, match="at most 16"):
        sweep.variants(40, [(m + 0.5) / 40 for m in range(1, 18)])
    with pytest.raises(ValueError, match="empty"):
        sweep.variants(4, [])
    for bad in ([1.5], [-0.1], [NAN], "some", 0.5):
        with pytest.raises(ValueError):
            sweep.variants(4, bad)
    assert len(sweep.variants(16, "all")) == 16


# ---------------------------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("n", [4, 8])
def test_schedule_gives_every_variant_its_own_plan_in_order(n):
    sched = LCMSchedule()
    rep = lambda m: 1.0 if m == n else (m + 0.5) / n
    for size in (1, 2, 3):
        for ms in itertools.combinations(range(n, 0, -1), size):              # descending, as variants() orders them
            plans = [sched.plan(n, rep(m)) for m in ms]
            assert [len(p) for p in plans] == list(ms)
            rows = sweep.schedule(plans)
            big = ms[0]
            assert len(rows) == big and sweep.noise_count(plans) == 2 + (big - 1)
            act = [len(r) for r in rows]
            assert act == sorted(act) and act[-1] == len(ms) and act[0] >= 1
            seen = {i: [] for i in range(len(ms))}
            for k, row in enumerate(rows):
                assert [i for i, _, _ in row] == list(range(len(row)))        # the active variants are a prefix
                assert len(row) == sum(1 for m in ms if m >= big - k)
                assert len({st["t"] for _, st, _ in row}) == 1                # one timestep for every active variant
                for i, st, z in row:
                    seen[i].append((st, z))
            for i, m in enumerate(ms):
                assert [st for st, _ in seen[i]] == plans[i]                  # its own records, in order
                assert [z for _, z in seen[i]] == list(range(2, 2 + m - 1)) + [None]
                assert seen[i][-1][0]["last"] and not any(st["last"] for st, _ in seen[i][:-1])


def test_schedule_refuses_plans_out_of_order():
    sched = LCMSchedule()
    with pytest.raises(ValueError):
        sweep.schedule([sched.plan(4, 0.5), sched.plan(4, 1.0)])
    with pytest.raises(ValueError):
        sweep.schedule([])


# ---------------------------------------------------------------------------------------------------------------- the selector's rule
@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_select_numpy_table(case):
    _, ssim, bgs, scores, rule, floor, bg, want = case
    clip = None if scores is None else _clip(scores)
    assert sweep.select_numpy(_rows(ssim, bgs), clip, rule, floor, bg) == want
    if clip is not None:                                       # rows the scorer appends for masked variants lie behind the first k and are not read
        more = np.concatenate([clip, _clip([1e9] * 3)])
        assert sweep.select_numpy(_rows(ssim, bgs), more, rule, floor, bg) == want


def test_select_numpy_errors_and_floor():
    with pytest.raises(ValueError):
        sweep.select_numpy(_rows([1., 2.]), None, "clip_score", -INF, False)
    with pytest.raises(ValueError):
        sweep.select_numpy(_rows([1., 2.]), None, "best", -INF, False)
    with pytest.raises(ValueError):
        sweep.select_numpy(_rows(list(range(17))), None, "strongest", -INF, False)
    assert sweep.ssim_floor(None) == -INF
    assert sweep.ssim_floor(0.5) == 0.5 * 3 * 502 * 502 and isinstance(sweep.ssim_floor(0.5), float)
    assert sweep.RULES == {"strongest": 0, "clip_score": 1} and sweep.MAX_VARIANTS == 16
    # the floor is in the units metrics.from_sums divides away: a reported SSIM maps back onto its raw sum to the last few bits
    from fie_amd import metrics as hmetrics
    raw = 123456.789
    assert math.isclose(sweep.ssim_floor(hmetrics.from_sums(0, raw, 512, 512)["ssim"]), raw, rel_tol=4e-16)


# ---------------------------------------------------------------------------------------------------------------- edit_sweep's argument checks
@pytest.fixture
def bare_editor():
    """A FastEditor without a device behind it: edit_sweep checks its arguments before it touches one."""
    from src.pipeline import FastEditor
    ed = FastEditor.__new__(FastEditor)
    ed.clip_scorer = None
    return ed


def test_edit_sweep_argument_errors(bare_editor):
    img = Image.new("RGB", (64, 64))
    call = lambda **kw: bare_editor.edit_sweep(img, "a [toy]", **kw)
    with pytest.raises(ValueError, match="region"):
        call(region="mask", mask=np.ones((64, 64), np.uint8))
    with pytest.raises(ValueError, match="region"):
        call(region=(0, 0, 32, 32))
    with pytest.raises(ValueError, match="tiles"):
        call(tiles="auto")
    with pytest.raises(ValueError, match="select"):
        call(select="best")
    with pytest.raises(ValueError, match="clip_score_dir"):
        call(select="clip_score")
    with pytest.raises(ValueError, match="min_ssim"):
        call(select="strongest")
    with pytest.raises(ValueError, match="min_ssim"):
        call(min_ssim=0.5)
    for bad in (2.0, NAN, "0.5", True):
        with pytest.raises(ValueError, match="min_ssim"):
            call(select="strongest", min_ssim=bad)
    with pytest.raises(ValueError, match="number of pipeline steps is 0"):
        call(strengths=[0.1])
    with pytest.raises(ValueError, match="empty"):
        call(strengths=[])
    with pytest.raises(ValueError, match="at most 16"):
        call(strengths="all", num_inference_steps=17)
    with pytest.raises(ValueError):
        call(output_size="huge")
    with pytest.raises(ValueError):
        call(mask_blur=3)                                      # a mask keyword without a mask, as in edit()
    with pytest.raises(ValueError):
        call(masked_content="fill")
    with pytest.raises(TypeError):
        call(strength=0.5)                                     # the keyword a sweep replaces
    with pytest.raises(TypeError):
        call(metrics=True)


# ---------------------------------------------------------------------------------------------------------------- command lines
def _flags(parser):
    return {a.option_strings[0] for a in parser._actions if a.option_strings}


def test_sweep_flags_live_on_mains_parser_only():
    import run_batch
    import run_single_image
    single = {"--sweep", "--strengths", "--select", "--min_ssim"}
    batch = {"--auto_strength", "--min_ssim", "--strengths"}
    assert single <= _flags(run_single_image.full_parser()) and not single & _flags(run_single_image.build_parser())
    assert batch <= _flags(run_batch.full_parser()) and not batch & _flags(run_batch.build_parser())
    a = run_single_image.full_parser().parse_args(["--image", "x.jpg", "--prompt", "p", "--sweep", "--strengths", "0.5,0.8,1", "--select", "strongest",
                                                   "--min_ssim", "0.6"])
    assert a.sweep and a.strengths == [0.5, 0.8, 1.0] and a.select == "strongest" and a.min_ssim == 0.6
    d = run_single_image.full_parser().parse_args(["--image", "x.jpg", "--prompt", "p"])
    assert not d.sweep and d.strengths == "all" and d.select == "none" and d.min_ssim is None
    b = run_batch.full_parser().parse_args(["--auto_strength", "clip_score", "--strengths", "all"])
    assert b.auto_strength == "clip_score" and b.strengths == "all" and b.min_ssim is None
    assert run_batch.sweep_kwargs(b) == dict(select="clip_score", strengths="all")
    assert run_batch.sweep_kwargs(run_batch.full_parser().parse_args([])) == {}
    assert run_batch.sweep_kwargs(run_batch.build_parser().parse_args([])) == {}           # a parser without the group: no sweep
    for bad in ("0.5,x", "1.5", ""):
        with pytest.raises(SystemExit):
            run_single_image.full_parser().parse_args(["--image", "x.jpg", "--prompt", "p", "--strengths", bad])
        with pytest.raises(SystemExit):
            run_batch.full_parser().parse_args(["--strengths", bad])


@pytest.mark.parametrize("argv", [["--auto_strength", "strongest", "--min_ssim", "0.5", "--batch_size", "2"],
                                  ["--auto_strength", "strongest", "--min_ssim", "0.5", "--tiles", "auto"],
                                  ["--auto_strength", "clip_score", "--use_mask", "--region", "mask"],
                                  ["--auto_strength", "strongest"],
                                  ["--auto_strength", "strongest", "--min_ssim", "1.5"],
                                  ["--min_ssim", "0.5"]])
def test_run_batch_refuses_what_a_sweep_cannot_do(argv, capsys):
    import run_batch
    with pytest.raises(ValueError):
        run_batch.sweep_kwargs(run_batch.full_parser().parse_args(argv))
    with pytest.raises(SystemExit) as e:                        # main() turns it into a parser error before anything is loaded
        run_batch.main(argv)
    assert e.value.code == 2


class SweepStub:
    """The slice of FastEditor that run_batch's --auto_strength loop touches."""

    def __init__(self):
        self.calls, self.plain = [], []
        self.in_flight = 1
        self._tls = threading.local()

    def edit(self, image, prompt, **kw):
        self.plain.append(prompt)
        return Image.new("RGB", (8, 8))

    def edit_sweep(self, image, prompt, **kw):
        self.calls.append(kw)
        steps = 1 + len(prompt) % 3
        v = [dict(strength=[1.0], steps=4, ssim=0.5), dict(strength=[steps / 4 + 0.1], steps=steps, ssim=0.9, psnr=20.0, mse=0.01)]
        return Image.new("RGB", (8, 8), (steps, 0, 0)), dict(v[1], index=1, variants=v, rows=None, clip_rows=None)

    def clear_memory(self):
        pass


def test_run_batch_auto_strength_rows_and_summary(tmp_path, capsys):
    import run_batch
    src = tmp_path / "src"
    entries = []
    for i in range(5):
        rel = f"0_cat/{i:04d}.png"
        (src / "0_cat").mkdir(parents=True, exist_ok=True)
        Image.new("RGB", (16, 16), (i, i, i)).save(src / rel)
        entries.append((i, f"{i:04d}", {"image_path": rel, "editing_prompt": "p" * (i + 1), "editing_type_id": "0"}))
    out = tmp_path / "o"
    argv = ["--source_dir", str(src), "--output_dir", str(out), "--seed", "3", "--strength", "0.5", "--auto_strength", "strongest", "--min_ssim",
            "0.8", "--strengths", "0.5,1.0", "--metrics"]
    args = run_batch.full_parser().parse_args(argv)
    ed = SweepStub()
    r = run_batch.process_shard(ed, entries, args, str(out / "e"), str(out / "c"))
    assert (r["processed"], r["failed"]) == (5, 0) and not ed.plain and len(ed.calls) == 5
    for kw in ed.calls:
        assert kw["select"] == "strongest" and kw["min_ssim"] == 0.8 and kw["strengths"] == [0.5, 1.0] and kw["seed"] == 3
        assert "strength" not in kw and "metrics" not in kw
    for row, (_, _, e) in zip(r["rows"], entries):
        steps = 1 + len(e["editing_prompt"]) % 3
        assert row["chosen_steps"] == steps and row["chosen_strength"] == steps / 4 + 0.1 and row["ssim"] == 0.9
        assert Image.open(out / "e" / e["image_path"]).getpixel((0, 0))[0] == steps
    run_batch.print_summary(dict(r, rows=r["rows"]), args, str(out / "e"), str(out / "c"), 1, 1.0)
    text = capsys.readouterr().out
    assert "Chosen step counts" in text and "3 steps: 2 images" in text and "2 steps: 2 images" in text and "1 steps: 1 images" in text
    # without --metrics the rows carry the choice alone
    args2 = run_batch.full_parser().parse_args(argv[:-1])
    r2 = run_batch.process_shard(SweepStub(), entries, args2, str(out / "e2"), str(out / "c2"))
    assert all("ssim" not in row and "chosen_steps" in row for row in r2["rows"])


def test_selector_entry_refuses_bad_arguments_without_a_device():
    """fie_sweep_select_u8 checks its arguments before it launches: the ABI's "bad argument" error, no GPU needed."""
    import ctypes
    from fie_amd import hip
    hip.build()
    lib = hip.lib()
    assert hip.SIGNATURES["fie_sweep_select_u8"] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    with pytest.raises(hip.FieError, match="bad argument"):
        hip._chk(lib.fie_sweep_select_u8(None, None, 1, 16, None, None, 0, 0.0, 0, None, None))
