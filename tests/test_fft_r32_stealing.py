"""k_fft_r32's frame claiming (k_fft_r32.hip): about one workgroup per CU, each taking its next frame from a per-band
counter that the launch's last workgroup puts back to zero.  Every frame's psd row must be written, by the right frame's
input, bit-equal to the CPU oracle - at batch sizes that are and are not multiples of the grid, over consecutive batches
on one bank (the counter's reset), with two bands (a counter per band), with two banks at once on one device (counters
per bank) and over graph replays (the reset under replay).

The input is cheap to check: frame f of a batch is frame f % P of a pool of P random frames (P prime, a fresh pool per
batch, so that a row left from an earlier batch or taken from another frame cannot pass), and the oracle computes the
pool only.  Every row is read back with sdr_read_spectrum.
"""
import pytest

from parity_tools import capi, check_pool_rows, pool_bank, pool_batch, pool_frames  # noqa: F401 (capi: the fixture)

pytestmark = pytest.mark.gpu


def test_batch_sizes_and_consecutive_batches(capi):
    """1024, 1031 (not a multiple of the grid), 3000 and 8192 frames, one after the other on one bank: each batch's
    launch finds the counter its predecessor left at zero."""
    import torch
    bank = pool_bank(capi, 1, 8192)
    for i, frames in enumerate([1024, 1031, 3000, 8192, 1031]):
        iq, want = pool_frames(7000 + i)
        dev = pool_batch(torch.from_numpy(iq).cuda(), frames)
        torch.cuda.synchronize()
        bank.process_device(dev.data_ptr(), frames)
        bank.sync()
        check_pool_rows(bank, 0, frames, want)
    bank.close()


def test_two_bands(capi):
    """Two bands in one launch: each band claims from a counter of its own."""
    import torch
    frames = 2048
    bank = pool_bank(capi, 2, frames)
    for rep in range(2):
        pools = [pool_frames(7100 + 2 * rep + b) for b in range(2)]
        dev = torch.stack([pool_batch(torch.from_numpy(p[0]).cuda(), frames) for p in pools]).contiguous()
        torch.cuda.synchronize()
        bank.process_device(dev.data_ptr(), frames)
        bank.sync()
        for b in range(2):
            check_pool_rows(bank, b, frames, pools[b][1])
    bank.close()


def test_two_banks_at_once(capi):
    """Two banks on device 0, their FFTs in flight together on streams of their own: counters per bank."""
    import torch
    banks = [pool_bank(capi, 1, 4096) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in banks]
    for bank, s in zip(banks, streams):
        bank.set_stream(s.cuda_stream)
    for rep in range(2):
        pools = [pool_frames(7200 + 2 * rep + k) for k in range(2)]
        devs = [pool_batch(torch.from_numpy(p[0]).cuda(), 4096 - 5 * k) for k, p in enumerate(pools)]
        torch.cuda.synchronize()
        for k, bank in enumerate(banks):
            bank.process_device(devs[k].data_ptr(), 4096 - 5 * k)
        for bank in banks:
            bank.sync()
        for k, bank in enumerate(banks):
            check_pool_rows(bank, 0, 4096 - 5 * k, pools[k][1])
    for bank in banks:
        bank.close()


def test_graph_replays(capi):
    """Three replays of the captured steady state (1024-frame batches): the counters' reset needs no host step."""
    import torch
    per = 1024
    bank = pool_bank(capi, 1, per)
    stream = torch.cuda.Stream()
    bank.set_stream(stream.cuda_stream)
    K = bank.graph_batches
    bank.graph_capture(per)
    for rep in range(3):
        pools = [pool_frames(7300 + rep * K + k) for k in range(K)]
        devs = [pool_batch(torch.from_numpy(p[0]).cuda(), per) for p in pools]
        torch.cuda.synchronize()
        bank.graph_launch([d.data_ptr() for d in devs])
        bank.sync()
        check_pool_rows(bank, 0, per, pools[-1][1])  # (the read calls see the replay's last batch)
    bank.graph_release()
    bank.close()
