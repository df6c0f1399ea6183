"""Host side of a strength sweep (the device side is csrc/sweep.hip and the ragged job of pipe.py).  Device-free, so
all of it runs (and is tested) on the CPU.

`strength` only decides how many leading LCM timesteps an edit drops (lcm.py: plan -- m = min(int(N * strength), N) steps remain), so N steps
allow at most N different edits.  All of them end on the same trailing timesteps: with M the largest step count, the variant with m steps joins
the loop at step M - m and from there on runs the timestep every other active variant runs.  Variants are ordered by DESCENDING m, so the active
ones are a leading slice of every tensor of the job.  With one seed they also share every noise draw: a generator's stream for m steps is a
prefix of its stream for M steps.

    variants()      the distinct step counts of a list of strengths
    schedule()      per loop step: who is active, with which step record and which noise tensor
    select_numpy()  the rule the device selector (fie_sweep_select_u8) evaluates, restated
"""
import math

import numpy as np

MAX_VARIANTS = 16                                  # what fie_sweep_select_u8 takes as kernel arguments
RULES = {"strongest": 0, "clip_score": 1}          # the `rule` argument of fie_sweep_select_u8


def variants(num_inference_steps, strengths):
    """The variants of a sweep over `strengths` ("all", or a non-empty list of floats in [0, 1]) at N = `num_inference_steps`:
    [(m, [the requested strengths with m = min(int(N * s), N) steps])] by descending m -- index 0 is the strongest edit.  "all": one variant per
    m = 1 .. N, represented by (m + 0.5) / N (1.0 for m = N).  ValueError: an empty list, a strength outside [0, 1] or with m == 0, more than
    MAX_VARIANTS variants."""
    n = int(num_inference_steps)
    if n < 1:
        raise ValueError(f"num_inference_steps={num_inference_steps!r}: at least 1")
    if isinstance(strengths, str):
        if strengths != "all":
            raise ValueError(f"strengths={strengths!r}: 'all' or a list of floats in [0, 1]")
        out = [(m, [1.0 if m == n else (m + 0.5) / n]) for m in range(n, 0, -1)]
    else:
        try:
            given = [float(s) for s in strengths]
        except TypeError:
            raise ValueError(f"strengths={strengths!r}: 'all' or a list of floats in [0, 1]") from None
        if not given:
            raise ValueError("strengths is empty: 'all' or a non-empty list of floats in [0, 1]")
        by_m = {}
        for s in given:
            if not 0.0 <= s <= 1.0:               # a NaN fails both comparisons
                raise ValueError(f"The value of strength should in [0.0, 1.0] but is {s}")
            m = min(int(n * s), n)
            if m == 0:
                raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {s}, the number of "
                                 f"pipeline steps is 0 which is < 1 and not appropriate for this pipeline.")
            by_m.setdefault(m, []).append(s)
        out = [(m, by_m[m]) for m in sorted(by_m, reverse=True)]
    if len(out) > MAX_VARIANTS:
        raise ValueError(f"{len(out)} variants: a sweep takes at most {MAX_VARIANTS}")
    return out


def noise_count(plans):
    """Noise tensors one sweep draws, shared by all variants: the posterior sample, the init noise, one per non-final step of the longest plan."""
    return 2 + (max(len(p) for p in plans) - 1)


def schedule(plans):
    """plans[i] = LCMSchedule.plan(N, s_i), by descending length (variants()' order).  -> one list per loop step k = 0 .. M - 1 (M the longest
    plan) with one entry (i, step record, noise index or None) per ACTIVE variant: those with m_i >= M - k, a prefix i = 0 .. act_k - 1.  The
    record is plans[i][k - (M - m_i)], the noise index 2 + k - (M - m_i) into the sweep's noise_count(plans) tensors, None on the variant's last
    step (which draws nothing)."""
    ms = [len(p) for p in plans]
    if not ms or min(ms) < 1 or any(a < b for a, b in zip(ms, ms[1:])):
        raise ValueError(f"schedule: step counts {ms}: non-empty plans by descending length")
    big = ms[0]
    out = []
    for k in range(big):
        row = []
        for i, (p, m) in enumerate(zip(plans, ms)):
            j = k - (big - m)
            if j < 0:
                break                              # descending m: everyone behind i is inactive too
            row.append((i, p[j], None if p[j]["last"] else 2 + j))
        out.append(row)
    return out


def ssim_floor(min_ssim, h=512, w=512):
    """`min_ssim` in the raw units of a metric row's ssim_sum (fie_amd/metrics.py: from_sums) for an h x w pair, in float64; -inf for None."""
    return -math.inf if min_ssim is None else float(min_ssim) * 3 * (int(h) - 10) * (int(w) - 10)


def select_numpy(rows, clip, rule, floor, bg):
    """The winner of a sweep, exactly as fie_sweep_select_u8 picks it (float64 and float32 compares only).  rows: int64 [k, 4] metric rows of
    fie_metrics_pairs_u8 in variants() order; clip: float32 [>= k, 2] CLIP rows (score in column 1) or None; rule: "strongest" / "clip_score";
    floor: float64 in raw ssim_sum units (ssim_floor()); bg: read bg_ssim_sum (field 3: a masked edit) instead of ssim_sum (field 1).
    ok[i] = sums[i] >= floor (a NaN never passes).  Nobody passes: the largest non-NaN sum, ties to the larger index; all NaN: k - 1.
    "strongest": the smallest passing index.  "clip_score": the largest clip[i, 1] among the passing, ties to the larger index, a NaN score
    never wins; all NaN: the largest passing index."""
    if rule not in RULES:
        raise ValueError(f"rule={rule!r}: one of {sorted(RULES)}")
    r = np.ascontiguousarray(np.asarray(rows), dtype=np.int64).reshape(-1, 4)
    k = r.shape[0]
    if not 1 <= k <= MAX_VARIANTS:
        raise ValueError(f"{k} rows: 1 .. {MAX_VARIANTS}")
    sums = r.view(np.float64)[:, 3 if bg else 1]
    floor = np.float64(floor)
    ok = [bool(sums[i] >= floor) for i in range(k)]
    if not any(ok):
        best = -1
        for i in range(k):
            if not np.isnan(sums[i]) and (best < 0 or sums[i] >= sums[best]):
                best = i
        return best if best >= 0 else k - 1
    if rule == "strongest":
        return ok.index(True)
    if clip is None:
        raise ValueError("rule 'clip_score' needs the CLIP rows")
    score = np.asarray(clip, dtype=np.float32).reshape(-1, 2)[:, 1]
    best = last = -1
    for i in range(k):
        if ok[i]:
            last = i
            if not np.isnan(score[i]) and (best < 0 or score[i] >= score[best]):
                best = i
    return best if best >= 0 else last
