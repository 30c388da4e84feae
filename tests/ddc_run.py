"""The DDC driver of the GPU tests (tests/test_ddc_gpu.py, tests/test_ddc_fuzz_gpu.py): one sdr_ddc over a list of raw
pieces, one call each, through capi.Ddc.  A plain helper module, not a test file: pytest does not rewrite its asserts, so
each carries its own message."""
import numpy as np


def run_gpu(capi, fmt, d, taps, steps, pieces, first_sample=None, between=None, host=False, switch_at=None):
    """One DDC over the raw pieces, one call each, every call with device tensors of its own (a call's pointers are 16-byte
    aligned whatever the pieces' lengths); between(ddc, i) runs in front of call i.  Returns float32 [bands, outputs, 2].
    The words behind a band's outputs, up to the band stride, must be left alone (the tensors are filled with NaN).

    host: True, False, or one of them per call.  A host call is given an array of its own, which is overwritten with
    garbage as soon as sdr_ddc_process_host has returned: the library has copied what it needs by then.
    switch_at: in front of that call the DDC moves to a second stream (sdr_ddc_set_stream).  The outputs of the calls before
    it are read, with all the others, only after the final sdr_ddc_sync."""
    import torch

    host = [bool(host)] * len(pieces) if isinstance(host, (bool, int)) else [bool(h) for h in host]
    assert len(host) == len(pieces), "one entry point per call"
    ddc = capi.Ddc(d, taps, steps, in_format=fmt, max_in_samples=max(len(p) for p in pieces))
    first = torch.cuda.current_stream()
    second = torch.cuda.Stream() if switch_at is not None else None
    ddc.set_stream(first.cuda_stream)
    if first_sample is not None:
        ddc.set_first_sample(first_sample)
    start = ddc.total_samples
    outs, keep = [], []
    for i, raw in enumerate(pieces):
        if between:
            between(ddc, i)
        if i == switch_at:
            ddc.set_stream(second.cuda_stream)
        m = len(raw) // d
        stride = (m + 3) // 4 * 4 + 4
        out = torch.full((len(steps), stride, 2), float("nan"), dtype=torch.float32, device="cuda")
        dev = None if host[i] else torch.from_numpy(np.ascontiguousarray(raw)).cuda()
        if second is not None and i >= switch_at:
            second.wait_stream(first)  # (the tensors of this call were filled on the first stream)
        if host[i]:
            mine = np.array(raw, copy=True, order="C")
            ddc.process_host(mine, out.data_ptr(), stride)
            mine.view(np.uint8)[...] = 0xA5
        else:
            ddc.process_device(dev.data_ptr(), len(raw), out.data_ptr(), stride)
            keep.append(dev)
        outs.append((out, m))
    ddc.sync()
    assert ddc.total_samples == start + sum(len(p) for p in pieces), "sdr_ddc_total_samples"
    ddc.close()
    got = [o.cpu().numpy() for o, _ in outs]
    for g, (_, m) in zip(got, outs):
        assert np.isnan(g[:, m:]).all(), "the kernel wrote behind a band's outputs"
    return np.concatenate([g[:, :m] for g, (_, m) in zip(got, outs)], axis=1)
