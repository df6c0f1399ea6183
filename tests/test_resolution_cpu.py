"""Aspect-ratio edits, host side (fie_amd/buckets.py): bucket choice, the tie rule, "WxH" parsing and size validation,
and the CLIs' --resolution flag.  No GPU needed."""
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import fie_amd  # noqa: E402,F401
from fie_amd import buckets  # noqa: E402


@pytest.mark.parametrize("src,want", [((1000, 1000), (1024, 1024)), ((800, 600), (1152, 896)), ((600, 800), (896, 1152)),
                                      ((1500, 1000), (1216, 832)), ((1920, 1080), (1344, 768)), ((2000, 1000), (1344, 768)),
                                      ((4000, 1000), (1536, 640)), ((1000, 4000), (640, 1536)), ((1080, 1920), (768, 1344)),
                                      ((512, 512), (1024, 1024)), ((1, 1), (1024, 1024))])
def test_nearest_bucket_known_answers(src, want):
    assert buckets.nearest_bucket(src) == want
    assert buckets.target_size("auto", src) == want


def test_bucket_table():
    assert len(buckets.BUCKETS) == 9 and len(set(buckets.BUCKETS)) == 9
    for w, h in buckets.BUCKETS:
        assert w % 64 == 0 and h % 64 == 0 and w * h <= 1024 * 1024
        assert (h, w) in buckets.BUCKETS                               # transposed buckets mirror each other


def test_tie_takes_the_larger_area(monkeypatch):
    # two buckets of one aspect ratio: the larger wins whichever comes first
    monkeypatch.setattr(buckets, "BUCKETS", ((512, 512), (1024, 1024), (768, 768)))
    assert buckets.nearest_bucket((300, 300)) == (1024, 1024)
    # equal log distance on both sides of the source's ratio: the larger area wins
    monkeypatch.setattr(buckets, "BUCKETS", ((1024, 512), (512, 1024), (640, 1280)))
    assert buckets.nearest_bucket((700, 700)) == (640, 1280)
    monkeypatch.setattr(buckets, "BUCKETS", ((640, 1280), (1024, 512)))
    assert buckets.nearest_bucket((700, 700)) == (640, 1280)


def test_distance_is_the_log_ratio():
    # 1.4 lies between 1216/832 (1.4615) and 1152/896 (1.2857): the log distance picks 1216x832
    r = math.log(1.4)
    d = {b: abs(r - math.log(b[0] / b[1])) for b in buckets.BUCKETS}
    assert min(d, key=d.get) == (1216, 832) == buckets.nearest_bucket((1400, 1000))


def test_square_and_default():
    for r in (None, "square", "SQUARE", " square "):
        assert buckets.target_size(r, (1920, 1080)) == (1024, 1024)


@pytest.mark.parametrize("spec,want", [("1152x896", (1152, 896)), ("896X1152", (896, 1152)), ("512x512", (512, 512)),
                                       ("2048x512", (2048, 512)), ("1024x1024", (1024, 1024)), ("auto", "auto"), ("square", "square")])
def test_parse(spec, want):
    assert buckets.parse(spec) == want


@pytest.mark.parametrize("spec", ["1000x1000", "1152x900", "448x512", "512x2112", "2048x1024", "1088x1024", "1024", "x", "axb", "1024x1024x3",
                                  "-512x512", "", "wide"])
def test_parse_rejects(spec):
    with pytest.raises(ValueError, match="multiples of 64|square|auto"):
        buckets.parse(spec)


@pytest.mark.parametrize("size", [(1000, 1000), (1024, 1000), (448, 512), (512, 2112), (2048, 1024), (1088, 1024), (1024.5, 1024), (True, 1024),
                                  (1024,), "x", 7])
def test_check_size_rejects(size):
    with pytest.raises(ValueError):
        buckets.target_size(size, (100, 100))


def test_check_size_message_names_the_rule():
    with pytest.raises(ValueError, match=r"multiples of 64, each in 512\.\.2048.*1048576"):
        buckets.check_size((1088, 1024))


@pytest.mark.parametrize("size", [(1152, 896), (512, 512), (2048, 512), (512, 2048), (1024, 1024), (640, 1536), (1088, 960)])
def test_check_size_accepts(size):
    assert buckets.target_size(size, (1, 1)) == size
    assert buckets.target_size(list(size), (1, 1)) == size


def test_editor_signature_is_keyword_only():
    import inspect
    from src.pipeline import FastEditor
    for fn in (FastEditor.edit, FastEditor.edit_batch):
        p = inspect.signature(fn).parameters["resolution"]
        assert p.kind == p.KEYWORD_ONLY and p.default is None


def test_cli_resolution_flags():
    import run_batch
    import run_single_image
    a = run_single_image.build_parser().parse_args(["--image", "x.jpg", "--prompt", "p"])
    assert a.resolution == "square"
    a = run_single_image.build_parser().parse_args(["--image", "x.jpg", "--prompt", "p", "--resolution", "1344x768"])
    assert buckets.parse(a.resolution) == (1344, 768)
    p = run_batch.add_resolution_args(run_batch.add_mask_args(run_batch.build_parser()))
    assert p.parse_args([]).resolution == "square"
    assert p.parse_args(["--resolution", "auto"]).resolution == "auto"
    assert not hasattr(run_batch.build_parser().parse_args([]), "resolution")      # build_parser's flag set stays the reference's + earlier additions
