"""The fine converter's driver of the GPU tests (tests/test_fine_gpu.py): one sdr_fine over a list of pieces, one call each,
through capi.Fine.  A plain helper module, not a test file: pytest does not rewrite its asserts, so each carries its own
message."""
import numpy as np


def run_gpu(capi, d, taps, steps, inputs, pieces, first_sample=None, between=None, switch_at=None, in_gap=4, out_gap=4):
    """pieces: float32 [n_inputs, n, 2] each, one call each, every call with device tensors of its own; between(fine, i) runs
    in front of call i.  Returns float32 [bands, outputs, 2].

    The inputs of a call lie in_stride = n rounded up to 4, plus in_gap, samples apart and a band's outputs out_gap behind
    the outputs rounded up to 4; the samples between two inputs and the words behind a band's outputs are filled with NaN
    and must be NaN afterwards (a kernel that read an input gap would also turn its outputs into NaN).
    switch_at: in front of that call the object moves to a second stream (sdr_fine_set_stream).  The outputs of the calls
    before it are read, with all the others, only after the final sdr_fine_sync."""
    import torch

    n_inputs = pieces[0].shape[0]
    fine = capi.Fine(n_inputs, d, taps, steps, inputs=inputs, max_in_samples=max(p.shape[1] for p in pieces))
    first = torch.cuda.current_stream()
    second = torch.cuda.Stream() if switch_at is not None else None
    fine.set_stream(first.cuda_stream)
    if first_sample is not None:
        fine.set_first_sample(first_sample)
    start = fine.total_samples
    calls = []
    for i, x in enumerate(pieces):
        if between:
            between(fine, i)
        if i == switch_at:
            fine.set_stream(second.cuda_stream)
        n = x.shape[1]
        m = n // d
        in_stride = (n + 3) // 4 * 4 + in_gap
        stride = (m + 3) // 4 * 4 + out_gap
        host = np.full((n_inputs, in_stride, 2), np.nan, np.float32)
        host[:, :n] = x
        dev = torch.from_numpy(host).cuda()
        out = torch.full((len(steps), stride, 2), float("nan"), dtype=torch.float32, device="cuda")
        if second is not None and i >= switch_at:
            second.wait_stream(first)  # (the tensors of this call were filled on the first stream)
        fine.process_device(dev.data_ptr(), in_stride, n, out.data_ptr(), stride)
        calls.append((dev, out, n, m))
    fine.sync()
    assert fine.total_samples == start + sum(p.shape[1] for p in pieces), "sdr_fine_total_samples"
    fine.close()
    got = []
    for (dev, out, n, m), x in zip(calls, pieces):
        back = dev.cpu().numpy()
        assert np.array_equal(back[:, :n].view(np.uint32), np.ascontiguousarray(x, np.float32).view(np.uint32)), "the inputs were written"
        assert np.isnan(back[:, n:]).all(), "the samples between two inputs were written"
        g = out.cpu().numpy()
        assert np.isnan(g[:, m:]).all(), "the kernel wrote behind a band's outputs"
        got.append(g[:, :m])
    return np.concatenate(got, axis=1)
