"""The hand-written table of the sweep selector's rule (fie_amd/sweep.py: select_numpy; include/fie.h: fie_sweep_select_u8): tests/test_sweep_cpu.py
runs the numpy restatement over it, tests/test_sweep_gpu.py the device op."""
import numpy as np

NAN, INF = float("nan"), float("inf")


def _rows(ssim, bg=None):
    """int64 [k, 4] metric rows whose ssim_sum / bg_ssim_sum fields hold the given doubles; the integer fields hold decoys."""
    k = len(ssim)
    r = np.zeros((k, 4), np.float64)
    r[:, 1] = ssim
    r[:, 3] = bg if bg is not None else [-5.0] * k
    out = r.view(np.int64).copy()
    out[:, 0] = np.arange(k) * 1000 + 7                        # sse fields: integers, never read by the rule
    out[:, 2] = 1 << 40
    return out


def _clip(scores):
    return np.stack([np.full(len(scores), -99.0, np.float32), np.asarray(scores, np.float32)], 1)


# (name, ssim sums, bg sums or None, clip scores or None, rule, floor, bg, winner): the hand-written table; tests/test_sweep_gpu.py runs the
# device op over the same rows
TABLE = [
    ("no floor, strongest",            [10., 20., 30.], None, None, "strongest", -INF, False, 0),
    ("no floor, clip",                 [10., 20., 30.], None, [1., 3., 2.], "clip_score", -INF, False, 1),
    ("floor, strongest",               [10., 20., 30.], None, None, "strongest", 15., False, 1),
    ("floor met exactly",              [10., 20., 30.], None, None, "strongest", 20., False, 1),
    ("floor, clip among the passing",  [10., 20., 30.], None, [9., 1., 2.], "clip_score", 15., False, 2),
    ("nobody passes",                  [10., 25., 20.], None, None, "strongest", 99., False, 1),
    ("nobody passes, clip rule",       [10., 25., 20.], None, [9., 1., 2.], "clip_score", 99., False, 1),
    ("nobody passes, tie",             [25., 10., 25.], None, None, "strongest", 99., False, 2),
    ("tie, strongest",                 [20., 20., 20.], None, None, "strongest", 20., False, 0),
    ("tie, clip: the weaker edit",     [20., 20., 20.], None, [5., 7., 7.], "clip_score", -INF, False, 2),
    ("tie, clip, passing only",        [20., 20., 5.], None, [7., 7., 7.], "clip_score", 10., False, 1),
    ("NaN sum never passes",           [NAN, 20., 30.], None, None, "strongest", -INF, False, 1),
    ("NaN sums, nobody passes",        [NAN, 20., NAN], None, None, "strongest", 99., False, 1),
    ("all sums NaN",                   [NAN, NAN, NAN], None, [1., 2., 3.], "clip_score", -INF, False, 2),
    ("all sums NaN, strongest",        [NAN, NAN], None, None, "strongest", 0., False, 1),
    ("NaN score never wins",           [10., 20., 30.], None, [NAN, 1., NAN], "clip_score", -INF, False, 1),
    ("all scores NaN",                 [10., 20., 30.], None, [NAN, NAN, NAN], "clip_score", 15., False, 2),
    ("all scores NaN, one passes",     [30., 20., 10.], None, [NAN, NAN, NAN], "clip_score", 25., False, 0),
    ("NaN floor: nobody passes",       [10., 30., 20.], None, None, "strongest", NAN, False, 1),
    ("-inf sum passes no floor",       [-INF, 5.], None, None, "strongest", -INF, False, 0),
    ("bg reads field 3",               [10., 20., 30.], [30., 20., 10.], None, "strongest", 15., True, 0),
    ("bg reads field 3, clip",         [10., 20., 30.], [5., 20., 30.], [9., 1., 2.], "clip_score", 15., True, 2),
    ("bg, nobody passes",              [10., 20., 30.], [3., 2., 1.], None, "strongest", 15., True, 0),
    ("k = 1",                          [10.], None, None, "strongest", 99., False, 0),
    ("k = 1, clip, NaN everywhere",    [NAN], None, [NAN], "clip_score", -INF, False, 0),
    ("k = 16",                         list(range(16)), None, [float(i % 5) for i in range(16)], "clip_score", 7., False, 14),
    ("k = 16, strongest",              list(range(16)), None, None, "strongest", 7.5, False, 8),
]
