"""The driver of tests/test_nb_gpu.py: one sdr_nb over a list of raw pieces, one call each, in the manner of
tests/iqc_run.py.  A plain helper module, not a test file: pytest does not rewrite its asserts, so each carries its own
message."""
import numpy as np

GUARD = 64  # bytes behind every call's output that the kernel must leave alone


def run_nb(capi, fmt, block, window, ratio_q4, hold, pieces, host=False, thresholds=None, first_sample=None, reads=()):
    """thresholds: per call None (keep) or (ratio_q4, hold), set in front of that call.  host: per call or for all, True
    takes sdr_nb_process_host.  reads: the calls behind which the statistics are read, besides the read behind the last one,
    where a second read must give zeros.  Returns (the calls' outputs, each shaped and typed as its piece, and the reads)."""
    import torch

    host = [bool(host)] * len(pieces) if isinstance(host, (bool, int)) else [bool(h) for h in host]
    thresholds = [None] * len(pieces) if thresholds is None else list(thresholds)
    assert len(host) == len(pieces) == len(thresholds), "one entry point and one threshold per call"
    nb = capi.Nb(fmt, block, window, ratio_q4, hold, max_in_samples=max(len(p) for p in pieces))
    nb.set_stream(torch.cuda.current_stream().cuda_stream)
    if first_sample is not None:
        nb.set_first_sample(first_sample)
    total = 0 if first_sample is None else first_sample
    outs, keep, read = [], [], []
    for i, raw in enumerate(pieces):
        raw = np.ascontiguousarray(raw)
        if thresholds[i] is not None:
            nb.set_threshold(*thresholds[i])
        out = torch.full((raw.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        if host[i]:
            mine = np.array(raw, copy=True, order="C")
            nb.process_host(mine, out.data_ptr())
            mine.view(np.uint8)[...] = 0x5A
        else:
            dev = torch.from_numpy(raw).cuda()
            nb.process_device(dev.data_ptr(), len(raw), out.data_ptr())
            keep.append(dev)
        total += len(raw)
        assert nb.total_samples == total, "sdr_nb_total_samples counts the accepted samples"
        outs.append((out, raw))
        if i in reads:
            read.append(nb.read_stats())
    nb.sync()
    read.append(nb.read_stats())
    again = nb.read_stats()
    assert not any(again.values()), "a second read returns zeros"
    nb.close()
    got = []
    for out, raw in outs:
        b = out.cpu().numpy()
        assert (b[raw.nbytes:] == 0xA5).all(), "the kernel wrote behind a call's output"
        got.append(b[:raw.nbytes].view(raw.dtype).reshape(raw.shape))
    return got, read
