"""The drivers of tests/test_iqc_gpu.py: one sdr_ddc or sdr_chan over a list of raw pieces, one call each, with an IQ
correction per call and the raw stream's sums, in the manner of tests/ddc_run.py and tests/chan_run.py.  A plain helper
module, not a test file: pytest does not rewrite its asserts, so each carries its own message."""
import numpy as np

KEEP = "keep"  # a call's entry in `corrs` that sets nothing in front of it


def _run(obj, d, n_streams, pieces, corrs, host, sums, first_sample, reads):
    import torch

    host = [bool(host)] * len(pieces) if isinstance(host, (bool, int)) else [bool(h) for h in host]
    corrs = [KEEP] * len(pieces) if corrs is None else list(corrs)
    assert len(host) == len(pieces) == len(corrs), "one entry point and one correction per call"
    obj.set_stream(torch.cuda.current_stream().cuda_stream)
    if first_sample is not None:
        obj.set_first_sample(first_sample)
    if sums:
        obj.enable_iq_sums(True)
    outs, keep, read = [], [], []
    for i, raw in enumerate(pieces):
        if not isinstance(corrs[i], str):
            obj.set_iq_correction(corrs[i])
        m = len(raw) // d
        stride = (m + 3) // 4 * 4 + 4
        out = torch.full((n_streams, stride, 2), float("nan"), dtype=torch.float32, device="cuda")
        if host[i]:
            mine = np.array(raw, copy=True, order="C")
            obj.process_host(mine, out.data_ptr(), stride)
            mine.view(np.uint8)[...] = 0xA5
        else:
            dev = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
            obj.process_device(dev.data_ptr(), len(raw), out.data_ptr(), stride)
            keep.append(dev)
        outs.append((out, m))
        if sums and i in reads:
            read.append(obj.read_iq_sums())
    obj.sync()
    if sums:
        read.append(obj.read_iq_sums())
        again = obj.read_iq_sums()
        assert not any(again.values()), "a second read returns zeros"
    obj.close()
    got = [o.cpu().numpy() for o, _ in outs]
    for g, (_, m) in zip(got, outs):
        assert np.isnan(g[:, m:]).all(), "the kernel wrote behind a stream's outputs"
    return np.concatenate([g[:, :m] for g, (_, m) in zip(got, outs)], axis=1), read


def run_ddc(capi, fmt, d, taps, steps, pieces, corrs=None, host=False, sums=False, first_sample=None, reads=()):
    """corrs: per call None (sdr_iq_ddc_set_correction(NULL)), four values, or KEEP.  sums: switched on in front of the
    first call, read behind the calls listed in `reads` and behind the last one, where a second read must give zeros.
    Returns (float32 [bands, outputs, 2], the reads)."""
    ddc = capi.Ddc(d, taps, steps, in_format=fmt, max_in_samples=max(len(p) for p in pieces))
    return _run(ddc, d, len(steps), pieces, corrs, host, sums, first_sample, reads)


def run_chan(capi, fmt, m, d, taps, pieces, channels=None, corrs=None, host=False, sums=False, first_sample=None, reads=()):
    chan = capi.Chan(m, d, taps, channels, in_format=fmt, max_in_samples=max(len(p) for p in pieces))
    return _run(chan, d, len(chan.channels), pieces, corrs, host, sums, first_sample, reads)
