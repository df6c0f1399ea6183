"""The hipGraph capture of an edit keeps Python's cycle collector out (fie_amd/pipe.py: _capture): dead cycles are collected in front of the capture,
no collector pass can start inside it, and the collector is back on behind it."""
import gc

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu


class _Cycle:
    """A dead reference cycle whose finaliser notes whether it ran on a capturing stream."""

    def __init__(self, seen):
        self.me, self.seen = self, seen

    def __del__(self):
        self.seen.append(bool(torch.cuda.is_current_stream_capturing()))


def test_no_collector_pass_inside_the_capture(fie):
    from fie_amd import stack
    from fie_amd.pipe import HipImg2ImgPipeline
    from oracle import canny
    from test_pipeline_gpu import synth_image
    cfgs, sds = stack.synthetic_stack("tiny", True, device="cpu", dtype=torch.float16)
    pipe = HipImg2ImgPipeline(fie, cfgs, sds, noise_dtype=torch.float32)
    img = synth_image(11, 128)
    ctrl = Image.fromarray(canny.canny_rgb(np.asarray(img)))
    passes, plain = [], pipe.run_device

    def run(job):
        passes.append((bool(torch.cuda.is_current_stream_capturing()), gc.isenabled()))
        return plain(job)
    pipe.run_device = run
    seen = []
    assert gc.isenabled()
    gc.collect()
    gc.disable()                       # so that the cycle below is still there when the call begins, whatever the collector's counters say
    try:
        _Cycle(seen)
        assert seen == []
        gc.enable()
        pipe(prompt="a red circle", negative_prompt="", image=img, control_image=ctrl, strength=0.8, num_inference_steps=4,
             generator=torch.Generator("cpu").manual_seed(42))
    finally:
        gc.enable()
        del pipe.run_device
    assert passes == [(False, True), (True, False)]                   # the eager warm-up, then the captured pass with the collector off
    assert seen == [False]                                             # the dead cycle went in front of the capture, not inside it
    assert gc.isenabled() and len(pipe._graphs) == 1
