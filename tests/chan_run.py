"""The channelizer's driver of the GPU tests (tests/test_chan_gpu.py): one sdr_chan over a list of raw pieces, one call each,
through capi.Chan.  A plain helper module, not a test file: pytest does not rewrite its asserts, so each carries its own
message."""
import numpy as np


def run_gpu(capi, fmt, m, d, taps, pieces, channels=None, first_sample=None, host=False, gap=4):
    """One channelizer over the raw pieces, one call each, every call with device tensors of its own (a call's pointers are
    16-byte aligned whatever the pieces' lengths).  Returns float32 [streams, outputs, 2].  The words behind a stream's
    outputs, up to the band stride (the outputs rounded up to 4, and gap more), must be left alone: the tensors are filled
    with NaN.  host: True, False, or one of them per call; a host call is given an array of its own, which is overwritten
    with garbage as soon as sdr_chan_process_host has returned."""
    import torch

    host = [bool(host)] * len(pieces) if isinstance(host, (bool, int)) else [bool(h) for h in host]
    assert len(host) == len(pieces), "one entry point per call"
    chan = capi.Chan(m, d, taps, channels, in_format=fmt, max_in_samples=max(len(p) for p in pieces))
    n_out = len(chan.channels)
    chan.set_stream(torch.cuda.current_stream().cuda_stream)
    if first_sample is not None:
        chan.set_first_sample(first_sample)
    start = chan.total_samples
    outs, keep = [], []
    for i, raw in enumerate(pieces):
        k = len(raw) // d
        stride = (k + 3) // 4 * 4 + gap
        out = torch.full((n_out, stride, 2), float("nan"), dtype=torch.float32, device="cuda")
        if host[i]:
            mine = np.array(raw, copy=True, order="C")
            chan.process_host(mine, out.data_ptr(), stride)
            mine.view(np.uint8)[...] = 0xA5
        else:
            dev = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
            chan.process_device(dev.data_ptr(), len(raw), out.data_ptr(), stride)
            keep.append(dev)
        outs.append((out, k))
    chan.sync()
    assert chan.total_samples == start + sum(len(p) for p in pieces), "sdr_chan_total_samples"
    chan.close()
    got = [o.cpu().numpy() for o, _ in outs]
    for g, (_, k) in zip(got, outs):
        assert np.isnan(g[:, k:]).all(), "the kernel wrote behind a stream's outputs"
    return np.concatenate([g[:, :k] for g, (_, k) in zip(got, outs)], axis=1)
