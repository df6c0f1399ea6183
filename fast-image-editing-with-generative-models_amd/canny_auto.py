"""Edge-budget Canny: the host side of `canny_density`.

The thresholds of an edit's Canny are picked per image so that about a fraction d of the pixels are strong edge seeds.  The device picks them
(csrc/canny_device.hip); what the host owns is the keyword's range, the integer budget the device is handed, and the caller's pair (lo, hi),
which gives only the ratio low / high.  Everything here is Python integers: the product, the tests' restatement and the command-line tools call
these functions, nothing restates them.
"""
DENSITY_MIN, DENSITY_MAX = 0.001, 0.25
FLOOR, MAX_MAGNITUDE = 16, 2040      # high never falls below 16 (grey levels +-1 apart give |dx|, |dy| <= 8); |dx| + |dy| <= 2 * 4 * 255


def check_density(canny_density):
    """None, or the density as a float in [0.001, 0.25]; anything else is a ValueError."""
    if canny_density is None:
        return None
    if isinstance(canny_density, bool) or not isinstance(canny_density, (int, float)) or not DENSITY_MIN <= float(canny_density) <= DENSITY_MAX:
        raise ValueError(f"canny_density={canny_density!r}: None, or a number in [{DENSITY_MIN}, {DENSITY_MAX}] (the fraction of the pixels that may be "
                         "strong edge seeds)")
    return float(canny_density)


def check_ratio(canny_low_threshold, canny_high_threshold):
    """(lo, hi) with lo <= hi: the caller's thresholds as the ratio low / high of an edge-budget Canny.  Integers >= 0, hi > 0."""
    pair = (canny_low_threshold, canny_high_threshold)
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in pair):
        raise ValueError(f"canny_density with canny_low_threshold={pair[0]!r}, canny_high_threshold={pair[1]!r}: the pair gives the ratio low / high "
                         "and must be integers >= 0")
    lo, hi = min(pair), max(pair)
    if hi == 0:
        raise ValueError("canny_density with canny_low_threshold = canny_high_threshold = 0: the pair gives the ratio low / high, and 0 / 0 is none")
    return lo, hi


def budget(pixels, canny_density):
    """The number of strong seeds an image of `pixels` pixels may have at density d: max(1, pixels * round(d * 10^6) // 10^6)."""
    ppm = int(round(check_density(canny_density) * 10 ** 6))
    return max(1, int(pixels) * ppm // 10 ** 6)


def low_of(high, lo, hi):
    """Rule 4: the low threshold that goes with `high` under the caller's ratio lo / hi (lo <= hi, hi > 0)."""
    return int(high) * int(lo) // int(hi)


def check(canny_density, canny_low_threshold, canny_high_threshold):
    """The argument check of every entry that takes the keyword: the density (or None), and with one the ratio."""
    d = check_density(canny_density)
    if d is not None:
        check_ratio(canny_low_threshold, canny_high_threshold)
    return d
