"""The context's GroupNorm scratch buffers are cached per (stream, graph slot) and replaced by a larger one when a larger batch arrives.  A
hipGraph captured before that has the OLD address in its launches (an edit of one image, then a batch of three, then the first edit's graph
again: the ControlNet's GroupNorm scratch on the pipeline's side stream), so the replaced buffer must stay allocated: hip.Context._scratch
keeps it.  Checked on the bookkeeping, without replaying anything into freed memory."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_a_grown_groupnorm_scratch_keeps_the_buffer_it_replaces(fie):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(6, 4096, 256, generator=g) + 0.5).half().to(fie.device)
    gamma, beta = torch.randn(256, generator=g).half().to(fie.device), torch.randn(256, generator=g).half().to(fie.device)
    st = torch.cuda.Stream(device=fie.device)
    with torch.cuda.stream(st):
        fie.sync_stream()
        for cache in (fie._gn_ws, fie._gn_stats):                           # a handle the runtime hands out again may have been met before:
            old = cache.pop((fie._stream, fie.ws_tag), None)                # start from an empty slot, keeping what was there allocated
            if old is not None:
                fie._ws_retired.append(old)
        one = fie.groupnorm(x[:2].contiguous(), gamma, beta, 32, 1e-5, True)
        key = (fie._stream, fie.ws_tag)
        assert key[0] == st.cuda_stream
        small = fie._gn_ws[key]
        ptr, kept = small.data_ptr(), len(fie._ws_retired)
        fie.groupnorm(x[:2].contiguous(), gamma, beta, 32, 1e-5, True)
        assert fie._gn_ws[key] is small and len(fie._ws_retired) == kept    # the same need: the same buffer, nothing retired
        six = fie.groupnorm(x, gamma, beta, 32, 1e-5, True)                   # three times the batch: a larger scratch
        large = fie._gn_ws[key]
        assert large is not small and large.numel() > small.numel()
        assert any(t is small for t in fie._ws_retired[kept:]) and small.data_ptr() == ptr      # still allocated, where a captured launch expects it
        again = fie.groupnorm(x[:2].contiguous(), gamma, beta, 32, 1e-5, True)
        assert fie._gn_ws[key] is large                                     # no shrinking back
    st.synchronize()
    assert torch.equal(one, again) and torch.equal(one, six[:2])          # and the results do not depend on which scratch served them
    # the sums a producer's epilogue leaves (hip.Context._gn_stats_arm) follow the same rule
    with torch.cuda.stream(st):
        fie.sync_stream()
        key = (fie._stream, fie.ws_tag)
        a = fie._scratch(fie._gn_stats, key, 1024)
        kept = len(fie._ws_retired)
        b = fie._scratch(fie._gn_stats, key, 4096)
        assert b is not a and fie._gn_stats[key] is b and fie._ws_retired[kept:] == [a] and fie._scratch(fie._gn_stats, key, 2048) is b
